/*
 * context_refs_test.c — TEST INFRASTRUCTURE: eight threads take and drop references to ONE context at the same time, as
 * the queues, buffers and operation objects of eight host threads do (tests/test_gpu_threads.py). Afterwards the count
 * must be the creator's one reference again. Built with ThreadSanitizer by tests/test_host_sanitizers.py over
 * cl_ops_amd/csrc/clo_ccl.c and the host stub of the thin C-ABI.
 */
#include "clo_ccl.h"

#include <pthread.h>
#include <stdio.h>

#define THREADS 8
#define TRIPS 200000

static CCLContext* ctx;

static void* work(void* arg) {
	(void) arg;
	for (int i = 0; i < TRIPS; ++i) {
		ccl_context_ref(ctx);
		ccl_context_unref(ctx);
	}
	return NULL;
}

int main(void) {
	GError* err = NULL;
	ctx = ccl_context_new_offline(&err);
	if (!ctx) return 2;
	pthread_t t[THREADS];
	for (int i = 0; i < THREADS; ++i) pthread_create(&t[i], NULL, work, NULL);
	for (int i = 0; i < THREADS; ++i) pthread_join(t[i], NULL);
	const int count = *(const int*) ctx;   /* struct ccl_context begins with its count */
	printf("references after %d x %d pairs: %d\n", THREADS, TRIPS, count);
	ccl_context_destroy(ctx);
	if (count != 1) return 1;
	printf("context refs ok\n");
	return 0;
}
