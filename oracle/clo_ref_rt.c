/*
 * clo_ref_rt.c — a host runtime for OpenCL C kernels compiled to x86-64 objects.
 *
 * TEST INFRASTRUCTURE ONLY. oracle/ref_build.py compiles the upstream cl_ops
 * kernels with an OpenCL C front end that targets the host, and links each
 * configuration with this file into oracle/_ref/libclo_ref_<config>.so. What
 * runs is upstream's program text; this file supplies only what an OpenCL
 * device would: the work-item built-ins the objects leave undefined (under
 * their Itanium-mangled names) and the loop that launches an ND-range.
 *
 * Execution model: work-groups run one after another. Inside a group every
 * work-item is a fiber with a stack of its own; barrier() yields to a round-robin scheduler
 * that resumes the items in local-id order, so all items of a group reach a
 * barrier before any of them passes it. A kernel that never calls barrier()
 * needs no fibers: its items are plain calls on the caller's stack.
 *
 * SINGLE-THREADED BY CONTRACT. Kernel-scope __local arrays become module
 * statics on this target, and the state below is static too, so two groups
 * must never be in flight in one library: never call clo_ref_launch from two
 * threads, and never from inside a kernel.
 */
#define _GNU_SOURCE
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <sys/mman.h>

#if !defined(__x86_64__)
#error "the fiber switch below is x86-64 System V; the kernels are compiled for that target too"
#endif

#define CLO_REF_STACK (64 * 1024)

typedef void (*clo_ref_body)(void** args);

/* Fiber switch: push the callee-saved registers, park the stack pointer in *from, adopt `to`,
 * pop its registers and return on its stack. (swapcontext would do, at two system calls a switch:
 * a radix sort of 4096 keys is millions of switches.) The kernels never touch MXCSR or the x87
 * control word, so those are not saved. */
void clo_ref_switch(void** from, void* to);
__asm__(
	".text\n"
	".globl clo_ref_switch\n"
	".hidden clo_ref_switch\n"
	".type clo_ref_switch,@function\n"
	"clo_ref_switch:\n"
	"	pushq %rbp\n	pushq %rbx\n	pushq %r12\n	pushq %r13\n	pushq %r14\n	pushq %r15\n"
	"	movq %rsp, (%rdi)\n"
	"	movq %rsi, %rsp\n"
	"	popq %r15\n	popq %r14\n	popq %r13\n	popq %r12\n	popq %rbx\n	popq %rbp\n"
	"	ret\n"
	".size clo_ref_switch, .-clo_ref_switch\n");

/* The work-item that is running now (1-D ranges only, like every cl_ops kernel). */
static size_t cur_lid, cur_lsz, cur_grp, cur_ngrp, cur_gsz;

/* Fiber state of the group that is running now. */
static void* sched_sp;
static void** item_sp;
static unsigned char* item_done;
static char* stacks;
static size_t stacks_for;      /* number of stacks mapped */
static int in_fiber;
static clo_ref_body cur_body;
static void** cur_args;

/* ---- work-item built-ins: size_t f(uint dim); dimensions other than 0 are trivial ---- */
size_t _Z13get_global_idj(unsigned d) { return d == 0 ? cur_grp * cur_lsz + cur_lid : 0; }
size_t _Z12get_local_idj(unsigned d) { return d == 0 ? cur_lid : 0; }
size_t _Z14get_local_sizej(unsigned d) { return d == 0 ? cur_lsz : 1; }
size_t _Z12get_group_idj(unsigned d) { return d == 0 ? cur_grp : 0; }
size_t _Z14get_num_groupsj(unsigned d) { return d == 0 ? cur_ngrp : 1; }
size_t _Z15get_global_sizej(unsigned d) { return d == 0 ? cur_gsz : 1; }

/* mul_hi(uint, uint): the high word of the 64-bit product. */
unsigned _Z6mul_hijj(unsigned a, unsigned b) { return (unsigned) (((uint64_t) a * (uint64_t) b) >> 32); }

/* convert_uint(ulong), no _sat: the low word, like a cast. */
unsigned _Z12convert_uintm(unsigned long x) { return (unsigned) x; }

/* barrier(cl_mem_fence_flags): give way to the scheduler; it resumes this item once
 * every other item of the group has yielded too. Memory is coherent by construction. */
void _Z7barrierj(unsigned flags) {
	(void) flags;
	if (!in_fiber) abort(); /* a kernel with barriers was launched without fibers */
	size_t me = cur_lid;
	clo_ref_switch(&item_sp[me], sched_sp);
	cur_lid = me;
}

static void item_main(void) {
	cur_body(cur_args);
	item_done[cur_lid] = 1;
	clo_ref_switch(&item_sp[cur_lid], sched_sp);
	abort(); /* a finished item is never resumed */
}

static int reserve(size_t lws) {
	if (lws <= stacks_for) return 0;
	if (stacks) { munmap(stacks, stacks_for * CLO_REF_STACK); free(item_sp); free(item_done); }
	stacks = mmap(NULL, lws * CLO_REF_STACK, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
	item_sp = malloc(lws * sizeof(void*));
	item_done = malloc(lws);
	if (stacks == MAP_FAILED || !item_sp || !item_done) { stacks = NULL; stacks_for = 0; return -1; }
	stacks_for = lws;
	return 0;
}

/*
 * Run `body(args)` once per work-item of a 1-D range of gws items in groups of lws.
 * use_fibers: nonzero for kernels that call barrier().
 * Returns 0, -1 on bad arguments or no memory, -2 if the items of a group did not
 * all reach the same number of barriers (undefined behaviour on a device).
 */
int clo_ref_launch(clo_ref_body body, void** args, size_t gws, size_t lws, int use_fibers) {
	if (lws == 0 || gws % lws != 0) return -1;
	cur_body = body; cur_args = args;
	cur_lsz = lws; cur_gsz = gws; cur_ngrp = gws / lws;
	if (!use_fibers) {
		in_fiber = 0;
		for (cur_grp = 0; cur_grp < cur_ngrp; ++cur_grp)
			for (size_t l = 0; l < lws; ++l) { cur_lid = l; body(args); }
		return 0;
	}
	if (reserve(lws)) return -1;
	int rc = 0;
	for (cur_grp = 0; cur_grp < cur_ngrp && rc == 0; ++cur_grp) {
		for (size_t l = 0; l < lws; ++l) {
			/* a fresh stack as clo_ref_switch expects it: six zeroed registers, then the address it
			 * returns to; the slot above keeps the stack aligned as after a call */
			void** top = (void**) (stacks + (l + 1) * CLO_REF_STACK);
			top[-1] = NULL;
			top[-2] = (void*) item_main;
			for (int r = 3; r <= 8; ++r) top[-r] = NULL;
			item_sp[l] = (void*) (top - 8);
			item_done[l] = 0;
		}
		in_fiber = 1;
		for (;;) {
			size_t finished = 0;
			for (size_t l = 0; l < lws; ++l) {
				cur_lid = l;
				clo_ref_switch(&sched_sp, item_sp[l]);
				finished += item_done[l];
			}
			if (finished == lws) break;
			if (finished != 0) { rc = -2; break; }
		}
		in_fiber = 0;
	}
	return rc;
}
