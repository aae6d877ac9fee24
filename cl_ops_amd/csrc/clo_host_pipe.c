/* clo_host_pipe.c — what the pipelined host-data paths share (clo_scan_abstract.c, clo_sort_satradix.c): the helper
 * thread that copies finished items out, and the per-item runtime calls. See clo_internal.h. */
#include "clo_internal.h"

#include <string.h>

static void* drain_main(void* arg) {
	clo_drain* d = (clo_drain*) arg;
	clo_hip_set_device(d->device);
	for (size_t k = 0; k < d->count; ++k) {
		pthread_mutex_lock(&d->mtx);
		while (d->posted <= k && !d->abort) pthread_cond_wait(&d->cv, &d->mtx);
		const int stop = d->posted <= k;   /* stopped, and nothing more will come */
		pthread_mutex_unlock(&d->mtx);
		if (stop) break;
		const int st = d->copy(d->user, k);
		pthread_mutex_lock(&d->mtx);
		if (st != 0) d->status = st;
		else d->completed = k + 1;
		pthread_cond_broadcast(&d->cv);
		pthread_mutex_unlock(&d->mtx);
		if (st != 0) break;
	}
	return NULL;
}

int clo_drain_start(clo_drain* d, size_t count, int (*copy)(void* user, size_t k), void* user) {
	memset(d, 0, sizeof(*d));
	d->count = count;
	d->copy = copy;
	d->user = user;
	if (clo_hip_get_device(&d->device) != 0) d->device = 0;
	pthread_mutex_init(&d->mtx, NULL);
	pthread_cond_init(&d->cv, NULL);
	if (pthread_create(&d->thread, NULL, drain_main, d) != 0) {
		pthread_mutex_destroy(&d->mtx);
		pthread_cond_destroy(&d->cv);
		return CLO_HIP_EARGS;
	}
	d->started = 1;
	return 0;
}

void clo_drain_post(clo_drain* d, size_t k) {
	pthread_mutex_lock(&d->mtx);
	d->posted = k;
	pthread_cond_broadcast(&d->cv);
	pthread_mutex_unlock(&d->mtx);
}

int clo_drain_wait(clo_drain* d, size_t k) {
	pthread_mutex_lock(&d->mtx);
	while (d->completed < k && d->status == 0) pthread_cond_wait(&d->cv, &d->mtx);
	const int st = d->status;
	pthread_mutex_unlock(&d->mtx);
	return st;
}

void clo_drain_stop(clo_drain* d) {
	if (!d->started) return;
	pthread_mutex_lock(&d->mtx);
	d->abort = 1;
	pthread_cond_broadcast(&d->cv);
	pthread_mutex_unlock(&d->mtx);
	pthread_join(d->thread, NULL);
	pthread_mutex_destroy(&d->mtx);
	pthread_cond_destroy(&d->cv);
	d->started = 0;
}

int clo_pipe_copy_out(void* ready, void* host, const void* dev, size_t bytes, void* s_out) {
	int st = clo_hip_event_synchronize(ready);
	if (st == 0 && bytes) st = clo_hip_memcpy_d2h_async(host, dev, bytes, s_out);
	if (st == 0) st = clo_hip_stream_synchronize(s_out);
	return st;
}

void* clo_pipe_transfer_stream(CCLQueue* cq_comm, void* s_exec, void* own) {
	void* s_in = ccl_queue_get_stream(cq_comm);
	return s_in == s_exec ? own : s_in;
}

int clo_pipe_upload(void* dev, const void* host, size_t bytes, void* s_in, void* arrived, void* s_exec) {
	int st = clo_hip_memcpy_h2d_async(dev, host, bytes, s_in);
	if (st == 0) st = clo_hip_event_record(arrived, s_in);
	if (st == 0) st = clo_hip_stream_wait_event(s_exec, arrived);
	return st;
}
