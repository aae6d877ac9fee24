/*
 * clo_sort_abstract.c — the CloSort object and its name->implementation
 * dispatch. Follows the behaviour of the reference's
 * src/cl_ops/sort/clo_sort_abstract.c:91-629 (constructor, destructor,
 * device-data and host-data entry points, getters); the JIT step
 * (:144-179) is replaced by parsing `compare` / `get_key` into a CloSortKeySpec
 * that selects ahead-of-time HIP kernels.
 */
#include "clo_sort.h"
#include "clo_internal.h"

#include <ctype.h>
#include <stdlib.h>
#include <string.h>

struct clo_sort {
	CloSortImplDef impl_def;
	CCLContext* ctx;
	CCLProgram* prg;
	CloType elem_type;
	CloType key_type;
	void* data;
	CloSortKeySpec spec;
	void* jit;  /* hiprtc-specialised kernels (bitonic network / satradix key extraction), or NULL */
	int jit_is_radix;
};

/* ------------------------------------------------------------------ */
/* get_key / compare parsing                                           */
/* ------------------------------------------------------------------ */

/* f(x) = (x >> shift) & mask */
typedef struct { int shift; unsigned long long mask; int ok; } keyfn;

typedef struct { const char* p; } cursor;

static void skip_ws(cursor* c) { while (isspace((unsigned char) *c->p)) ++c->p; }

static int accept(cursor* c, const char* tok) {
	skip_ws(c);
	size_t n = strlen(tok);
	if (strncmp(c->p, tok, n) == 0) { c->p += n; return 1; }
	return 0;
}

/* A cast "(type)": returns the type size or 0 if the text is not a cast. */
static int parse_cast(cursor* c) {
	static const struct { const char* name; int size; } names[] = {
		{"unsigned long", 8}, {"unsigned int", 4}, {"unsigned short", 2}, {"unsigned char", 1},
		{"uchar", 1}, {"char", 1}, {"ushort", 2}, {"short", 2}, {"uint", 4}, {"int", 4},
		{"ulong", 8}, {"long", 8}
	};
	cursor save = *c;
	if (!accept(c, "(")) return 0;
	skip_ws(c);
	for (size_t i = 0; i < sizeof(names) / sizeof(names[0]); ++i) {
		size_t n = strlen(names[i].name);
		if (strncmp(c->p, names[i].name, n) == 0 && !isalnum((unsigned char) c->p[n]) && c->p[n] != '_') {
			cursor t = *c;
			t.p += n;
			if (accept(&t, ")")) { *c = t; return names[i].size; }
		}
	}
	*c = save;
	return 0;
}

static int parse_number(cursor* c, unsigned long long* out) {
	skip_ws(c);
	if (!isdigit((unsigned char) *c->p)) return 0;
	char* end = NULL;
	*out = strtoull(c->p, &end, 0);
	while (*end == 'u' || *end == 'U' || *end == 'l' || *end == 'L') ++end;
	c->p = end;
	return 1;
}

static keyfn parse_and(cursor* c);

/* OpenCL C reinterpretation "as_<type>(": keeps the bits, so it acts like a
 * cast to an integer of that size. Returns the size or 0. */
static int parse_as_type(cursor* c) {
	static const struct { const char* name; int size; } names[] = {
		{"as_uchar", 1}, {"as_char", 1}, {"as_ushort", 2}, {"as_short", 2}, {"as_half", 2},
		{"as_uint", 4}, {"as_int", 4}, {"as_float", 4}, {"as_ulong", 8}, {"as_long", 8}, {"as_double", 8}
	};
	skip_ws(c);
	for (size_t i = 0; i < sizeof(names) / sizeof(names[0]); ++i) {
		size_t n = strlen(names[i].name);
		if (strncmp(c->p, names[i].name, n) == 0) {
			cursor t = *c;
			t.p += n;
			skip_ws(&t);
			if (*t.p == '(') { *c = t; return names[i].size; }   /* the '(' is left for parse_primary */
		}
	}
	return 0;
}

/* primary := cast primary | as_type '(' and ')' | '(' and ')' | 'x' */
static keyfn parse_primary(cursor* c) {
	keyfn f = {0, ~0ull, 0};
	int cast = parse_cast(c);
	if (!cast) cast = parse_as_type(c);
	if (cast) {
		f = parse_primary(c);
		if (f.ok && cast < 8) f.mask &= (1ull << (8 * cast)) - 1ull;
		return f;
	}
	if (accept(c, "(")) {
		f = parse_and(c);
		if (!accept(c, ")")) f.ok = 0;
		return f;
	}
	skip_ws(c);
	if (*c->p == 'x' && !isalnum((unsigned char) c->p[1]) && c->p[1] != '_') {
		++c->p;
		f.ok = 1;
	}
	return f;
}

/* shift := primary ('>>' number)* */
static keyfn parse_shift(cursor* c) {
	keyfn f = parse_primary(c);
	unsigned long long n;
	while (f.ok && accept(c, ">>")) {
		if (!parse_number(c, &n) || n > 63) { f.ok = 0; break; }
		f.shift += (int) n;
		f.mask >>= n;
	}
	return f;
}

/* and := shift ('&' number)* */
static keyfn parse_and(cursor* c) {
	keyfn f = parse_shift(c);
	unsigned long long n;
	while (f.ok && accept(c, "&")) {
		if (!parse_number(c, &n)) { f.ok = 0; break; }
		f.mask &= n;
	}
	return f;
}

static int parse_get_key(const char* text, int elem_size, int key_size, int* shift, int* bits) {
	keyfn f = {0, ~0ull, 1};
	if (text) {
		cursor c = { text };
		f = parse_and(&c);
		skip_ws(&c);
		if (*c.p != '\0') f.ok = 0;
	}
	if (!f.ok) return 0;
	/* x has elem_size bytes; the result is converted to the key type. */
	if (elem_size < 8) {
		unsigned long long em = (1ull << (8 * elem_size)) - 1ull;
		f.mask &= f.shift >= 8 * elem_size ? 0ull : (em >> f.shift);
	} else if (f.shift > 0) {
		f.mask &= ~0ull >> f.shift;
	}
	if (key_size < 8) f.mask &= (1ull << (8 * key_size)) - 1ull;
	/* only contiguous low masks (2^k - 1) are built */
	if (f.mask == 0 || (f.mask & (f.mask + 1ull)) != 0ull) return 0;
	*shift = f.shift;
	*bits = f.mask == ~0ull ? 64 : (int) clo_ones32((unsigned int) f.mask) + (int) clo_ones32((unsigned int) (f.mask >> 32));
	return 1;
}

/* compare: "a > b" (ascending, default) or "a < b" with any parenthesisation. */
static int parse_compare(const char* text, int* descending) {
	if (!text) { *descending = 0; return 1; }
	char buf[64];
	size_t n = 0;
	for (const char* p = text; *p; ++p) {
		if (isspace((unsigned char) *p) || *p == '(' || *p == ')') continue;
		if (n + 1 >= sizeof(buf)) return 0;
		buf[n++] = *p;
	}
	buf[n] = '\0';
	if (strcmp(buf, "a>b") == 0) { *descending = 0; return 1; }
	if (strcmp(buf, "a<b") == 0) { *descending = 1; return 1; }
	return 0;
}

/* ------------------------------------------------------------------ */
/* object                                                              */
/* ------------------------------------------------------------------ */

/* Upstream builds (and thereby loads) its kernels in clo_sort_new; HIP loads a
 * code object at the first launch that needs it, which would otherwise land in
 * the first timed sort of a sweep (1.2 ms at the first multi-tile size). So the
 * first sorter of each kind in a process sorts two small dummy arrays here: the
 * one-launch path and the multi-tile path. Best effort, errors are dropped. */
static void sort_warmup(CloSort* sorter, const char* type, size_t elem_size) {
	static unsigned char done[4][4];
	static const char* const kinds[4] = { "satradix", "abitonic", "sbitonic", "gselect" };
	if (clo_env_no_warmup() || sorter->jit) return;
	int k = -1, e = elem_size == 1 ? 0 : (elem_size == 2 ? 1 : (elem_size == 4 ? 2 : 3));
	for (int i = 0; i < 4; ++i) if (strcmp(type, kinds[i]) == 0) k = i;
	if (k < 0 || __atomic_exchange_n(&done[k][e], 1, __ATOMIC_RELAXED)) return;   /* (sorters may be made on several threads at once) */
	/* satradix has three families of kernels, each in a code object of its own:
	 * the one-launch sort (<= 2^14 elements), the chain-free passes, and the
	 * single-sweep passes the library uses from 128 tiles on (4 MiB of elements) */
	if (k == 0) (void) clo_hip_radix_preload();   /* (the chain-free passes start above the dummy sorts' sizes) */
	const size_t sizes[3] = { 16, k == 0 ? 20000 : (k == 3 ? 2048 : 32768),
		k == 0 && elem_size >= 4 ? ((size_t) 4 << 20) / elem_size : 0 };
	for (int i = 0; i < 3; ++i) {
		if (sizes[i] == 0) continue;
		void* in = calloc(sizes[i], elem_size);
		void* out = malloc(sizes[i] * elem_size);
		GError* err = NULL;
		if (in && out) clo_sort_with_host_data(sorter, NULL, NULL, in, out, sizes[i], 0, &err);
		if (err) clo_gerror_free(err);
		free(in);
		free(out);
	}
}

const clo_sort_impl_ext* clo_sort_impl_ext_find(const char* name) {
	static const clo_sort_impl_ext* const table[] = { &clo_sort_satradix_ext, NULL };
	for (unsigned i = 0; name != NULL && table[i] != NULL; ++i)
		if (strcmp(table[i]->name, name) == 0) return table[i];
	return NULL;
}

/* Does `text` use, as an identifier, a name that `compiler_opts` defines or undefines (-DNAME[=value], -D NAME, -UNAME)?
 * Then the expression means what the COMPILER makes of it, not what the parser of the fixed family reads: it is
 * pasted into the kernel source and built with those options, as upstream builds everything
 * (sort/clo_sort_abstract.c:144-179). */
static int is_ident_char(int c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_'; }
static int opts_name_used(const char* compiler_opts, const char* text) {
	if (!compiler_opts || !text) return 0;
	const char* p = compiler_opts;
	while (*p) {
		while (*p == ' ' || *p == '\t' || *p == '\n') ++p;
		if (p[0] == '-' && (p[1] == 'D' || p[1] == 'U')) {
			p += 2;
			while (*p == ' ' || *p == '\t') ++p;   /* "-D NAME" */
			const char* name = p;
			while (is_ident_char((unsigned char) *p)) ++p;
			const size_t n = (size_t) (p - name);
			for (const char* t = text; n > 0 && *t; ++t) {
				if (strncmp(t, name, n) == 0 && !is_ident_char((unsigned char) t[n]) && (t == text || !is_ident_char((unsigned char) t[-1]))) return 1;
			}
		}
		while (*p && *p != ' ' && *p != '\t' && *p != '\n') ++p;
	}
	return 0;
}

CloSort* clo_sort_new(const char* type, const char* options, CCLContext* ctx,
	CloType* elem_type, CloType* key_type, const char* compare, const char* get_key,
	const char* compiler_opts, GError** err) {

	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	clo_return_val_if_fail(ctx != NULL, NULL);
	clo_return_val_if_fail(elem_type != NULL, NULL);

	/* ref: clo_sort_abstract.c:111-117 */
	const CloSortImplDef* impls[] = {
		&clo_sort_sbitonic_def, &clo_sort_abitonic_def, &clo_sort_gselect_def, &clo_sort_satradix_def, NULL
	};

	CloSort* sorter = NULL;
	GError* err_internal = NULL;
	clo_hip_env_refresh();   /* the environment switches are read when an object is made, never per call */

	for (unsigned i = 0; impls[i] != NULL; ++i) {
		if (type == NULL || strcmp(type, impls[i]->name) != 0) continue;

		sorter = (CloSort*) calloc(1, sizeof(CloSort));
		if (!sorter) break;
		sorter->impl_def = *impls[i];
		ccl_context_ref(ctx);
		sorter->ctx = ctx;
		sorter->elem_type = *elem_type;
		sorter->key_type = key_type ? *key_type : *elem_type;

		/* what upstream expresses as CLO_SORT_ELEM_TYPE / KEY_TYPE / COMPARE /
		 * KEY_GET macros (:144-168) */
		CloSortKeySpec* ks = &sorter->spec;
		ks->elem_size = (int) clo_type_sizeof(sorter->elem_type);
		ks->key_size = (int) clo_type_sizeof(sorter->key_type);
		ks->key_kind = clo_type_key_kind(sorter->key_type);
		if (ks->elem_size == 0 || ks->key_size == 0) {
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_UNKNOWN_TYPE, "Unknown element or key type");
			goto fail;
		}
		const int key_ok = parse_get_key(get_key, ks->elem_size, ks->key_size, &ks->key_shift, &ks->key_bits)
			&& !(ks->key_kind == 2 && ks->key_bits != 8 * ks->key_size)   /* a float key is the whole key type */
			&& !opts_name_used(compiler_opts, get_key);
		int cmp_ok = parse_compare(compare, &ks->descending) && !opts_name_used(compiler_opts, compare);
		const int is_satradix = strcmp(type, "satradix") == 0;
		if (is_satradix && !cmp_ok) {
			/* upstream's radix kernels never expand CLO_SORT_COMPARE (always ascending):
			 * whatever the string says is accepted and ignored */
			cmp_ok = 1;
			ks->descending = 0;
		}
		if (!key_ok || !cmp_ok) {
			/* what upstream does for every sorter: paste the macro bodies into the
			 * kernel source and build it (clo_sort_abstract.c:144-179) */
			char* log = NULL;
			int st;
			if (is_satradix) {
				st = clo_hip_radix_jit_create((int) sorter->elem_type, (int) sorter->key_type, get_key, compiler_opts, &sorter->jit, &log);
				sorter->jit_is_radix = 1;
			} else {
				st = clo_hip_bitonic_jit_create((int) sorter->elem_type, (int) sorter->key_type, compare, get_key, compiler_opts,
					&sorter->jit, &log);
			}
			if (st != 0) {
				clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS,
					"Could not build kernels for compare '%s' / get_key '%s'%s%s%s: %s%s%.600s",
					compare ? compare : "((a) > (b))", get_key ? get_key : "(x)",
					compiler_opts ? " with options '" : "", compiler_opts ? compiler_opts : "", compiler_opts ? "'" : "",
					clo_hip_error_string(st), log ? "\n" : "", log ? log : "");
				free(log);
				goto fail;
			}
			free(log);
			ks->key_shift = 0;
			ks->key_bits = 8 * ks->key_size;
			ks->descending = 0;
		}

		const char* token = sorter->impl_def.init(sorter, options, &err_internal);
		if (err_internal) { clo_gerror_propagate(err, err_internal); goto fail; }
		if (!token) {
			clo_gerror_set(err, CLO_ERROR, CLO_ERROR_LIBRARY, "Sort implementation '%s' failed to initialise", type);
			goto fail;
		}
		/* No JIT: the "program" is a token naming the ahead-of-time kernels. */
		sorter->prg = ccl_program_new_token(ctx, token, compiler_opts);
		sort_warmup(sorter, type, ks->elem_size);
		break;
	}

	if (sorter == NULL) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_IMPL_NOT_FOUND,
			"The requested sort implementation, '%s', was not found.", type ? type : "(null)");
	}
	return sorter;

fail:
	if (sorter) {
		/* finalize only what init created */
		if (sorter->jit) { if (sorter->jit_is_radix) clo_hip_radix_jit_destroy(sorter->jit); else clo_hip_bitonic_jit_destroy(sorter->jit); }
		if (sorter->data) sorter->impl_def.finalize(sorter);
		ccl_context_unref(sorter->ctx);
		ccl_program_destroy(sorter->prg);
		free(sorter);
	}
	return NULL;
}

void clo_sort_destroy(CloSort* sorter) {
	clo_return_if_fail(sorter != NULL);
	sorter->impl_def.finalize(sorter);
	if (sorter->jit) { if (sorter->jit_is_radix) clo_hip_radix_jit_destroy(sorter->jit); else clo_hip_bitonic_jit_destroy(sorter->jit); }
	if (sorter->ctx) ccl_context_unref(sorter->ctx);
	if (sorter->prg) ccl_program_destroy(sorter->prg);
	free(sorter);
}

CCLEvent* clo_sort_with_device_data(CloSort* sorter, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* data_in, CCLBuffer* data_out, size_t numel, size_t lws_max, GError** err) {
	clo_return_val_if_fail(sorter != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	return sorter->impl_def.sort_with_device_data(sorter, cq_exec, cq_comm, data_in, data_out, numel, lws_max, err);
}

/* ref: clo_sort_abstract.c:296-418 — buffers, H2D on cq_comm, sort on cq_exec, D2H of the result, on the named
 * stage of clo_internal.h: the two copies are upstream's clo_sort_write and clo_sort_read to a CCLProf consumer. */
cl_bool clo_sort_with_host_data(CloSort* sorter, CCLQueue* cq_exec, CCLQueue* cq_comm,
	void* data_in, void* data_out, size_t numel, size_t lws_max, GError** err) {

	clo_return_val_if_fail(sorter != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);

	const size_t data_size = numel * clo_type_sizeof(sorter->elem_type);
	const clo_sort_impl_ext* ext = clo_sort_impl_ext_find(sorter->impl_def.name);
	const int in_place = sorter->impl_def.in_place != 0;   /* then the input buffer is sorted and read back: no second one */
	clo_stage st;
	clo_stage_open(&st, sorter->ctx, cq_exec, cq_comm);
	st.write_name = "clo_sort_write";
	st.read_name = "clo_sort_read";

	/* Transfers overlapped with the sort where the implementation knows how (satradix on large
	 * arrays: clo_sort_satradix.c); the result is the blocking path's. */
	if (clo_stage_ok(&st) && ext && ext->host_pipeline) {
		int handled = 0;
		const cl_bool status = ext->host_pipeline(sorter, st.cq_exec, st.cq_comm, data_in, data_out, numel, &handled, &st.err);
		if (handled) return clo_stage_close(&st, err) && status;
	}

	clo_stage_in(&st, 0, data_in, data_size);
	if (!in_place) clo_stage_out(&st, 1, data_out, data_size);
	if (clo_stage_ok(&st))
		st.evt = sorter->impl_def.sort_with_device_data(sorter, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], numel, lws_max, &st.err);
	clo_stage_read(&st, in_place ? 0 : 1, data_out, data_size);
	/* A sorter whose kernels poll other work-groups may have given up a bounded
	 * spin: asked here explicitly, whatever queues the caller passed (with a
	 * separate cq_comm — upstream's own harness, benchmarks/clo_sort_bench.c:160-162 —
	 * the wait above has synchronised with the transfer queue only). */
	if (clo_stage_ok(&st) && ext && ext->check_status) ext->check_status(sorter, st.cq_exec, &st.err);
	return clo_stage_close(&st, err);
}

/* ---- sorting by key (not upstream; include/clo_sort.h) ---- */

/* Why a by-key sort refuses these arguments, or NULL: checked before any device call. */
static const char* by_key_refusal(CloSort* sorter, const void* keys_in, const void* values_out, size_t numel,
	const clo_sort_impl_ext** ext) {
	*ext = clo_sort_impl_ext_find(sorter->impl_def.name);
	if (!*ext || !(*ext)->sort_by_key) return "sorting by key is provided by the satradix sorter only";
	if (sorter->jit) return "sorting by key needs a get_key of the ahead-of-time family, not one compiled at run time";
	if (sorter->spec.elem_size > 4) return "sorting by key takes elements of 1, 2 or 4 bytes (8-byte ones would need 12-byte pairs)";
	if (!keys_in) return "keys_in is required";
	if (!values_out) return "values_out is required";
	if (numel > 0xffffffffull) return "numel must be below 2^32";
	return NULL;
}

CCLEvent* clo_sort_by_key_with_device_data(CloSort* sorter, CCLQueue* cq_exec, CCLQueue* cq_comm,
	CCLBuffer* keys_in, CCLBuffer* values_in, CCLBuffer* keys_out, CCLBuffer* values_out,
	size_t numel, size_t lws_max, GError** err) {
	clo_return_val_if_fail(sorter != NULL, NULL);
	clo_return_val_if_fail(err == NULL || *err == NULL, NULL);
	(void) cq_comm;  /* nothing is copied: the first pass reads the arrays where they are */
	(void) lws_max;
	const clo_sort_impl_ext* ext;
	const char* why = by_key_refusal(sorter, keys_in, values_out, numel, &ext);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return NULL;
	}
	clo_return_val_if_fail(cq_exec != NULL, NULL);
	return ext->sort_by_key(sorter, cq_exec, keys_in, values_in, keys_out, values_out, numel, err);
}

/* Upstream's blocking host-data path (sort/clo_sort_abstract.c:348-395) for the four arrays: copy in on cq_comm, sort on
 * cq_exec, copy out on cq_comm. */
cl_bool clo_sort_by_key_with_host_data(CloSort* sorter, CCLQueue* cq_exec, CCLQueue* cq_comm,
	const void* keys_in, const void* values_in, void* keys_out, void* values_out,
	size_t numel, size_t lws_max, GError** err) {
	clo_return_val_if_fail(sorter != NULL, CL_FALSE);
	clo_return_val_if_fail(err == NULL || *err == NULL, CL_FALSE);
	const clo_sort_impl_ext* ext;
	const char* why = by_key_refusal(sorter, keys_in, values_out, numel, &ext);
	if (why) {
		clo_gerror_set(err, CLO_ERROR, CLO_ERROR_ARGS, "%s", why);
		return CL_FALSE;
	}
	if (numel == 0) return CL_TRUE;

	/* keys in, values in, keys out, values out. The copies keep the names the buffer calls give them; the read-backs
	 * are waited for like the plain sort's, so the transfer queue's give-up watch is asked here too. */
	const size_t kbytes = numel * (size_t) sorter->spec.elem_size, vbytes = numel * sizeof(cl_uint);
	clo_stage st;
	clo_stage_open(&st, sorter->ctx, cq_exec, cq_comm);
	st.read_name = "read_buffer";
	clo_stage_in(&st, 0, keys_in, kbytes);
	clo_stage_in(&st, 1, values_in, vbytes);
	if (keys_out) clo_stage_out(&st, 2, keys_out, kbytes);
	clo_stage_out(&st, 3, values_out, vbytes);
	if (clo_stage_ok(&st))
		st.evt = clo_sort_by_key_with_device_data(sorter, st.cq_exec, st.cq_comm, st.dev[0], st.dev[1], st.dev[2], st.dev[3], numel, lws_max, &st.err);
	clo_stage_read(&st, 3, values_out, vbytes);
	clo_stage_read(&st, 2, keys_out, kbytes);
	if (clo_stage_ok(&st) && ext->check_status) ext->check_status(sorter, st.cq_exec, &st.err);
	return clo_stage_close(&st, err);
}

/* ---- getters, ref: clo_sort_abstract.c:428-629 ---- */

CCLContext* clo_sort_get_context(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, NULL);
	return sorter->ctx;
}

CCLProgram* clo_sort_get_program(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, NULL);
	return sorter->prg;
}

CloType clo_sort_get_element_type(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, (CloType) -1);
	return sorter->elem_type;
}

size_t clo_sort_get_element_size(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, 0);
	return clo_type_sizeof(sorter->elem_type);
}

CloType clo_sort_get_key_type(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, (CloType) -1);
	return sorter->key_type;
}

size_t clo_sort_get_key_size(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, 0);
	return clo_type_sizeof(sorter->key_type);
}

void* clo_sort_get_data(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, NULL);
	return sorter->data;
}

void clo_sort_set_data(CloSort* sorter, void* data) {
	clo_return_if_fail(sorter != NULL);
	sorter->data = data;
}

cl_uint clo_sort_get_num_kernels(CloSort* sorter, GError** err) {
	clo_return_val_if_fail(sorter != NULL, 0);
	return sorter->impl_def.get_num_kernels(sorter, err);
}

const char* clo_sort_get_kernel_name(CloSort* sorter, cl_uint i, GError** err) {
	clo_return_val_if_fail(sorter != NULL, NULL);
	return sorter->impl_def.get_kernel_name(sorter, i, err);
}

size_t clo_sort_get_localmem_usage(CloSort* sorter, cl_uint i, size_t lws_max, size_t numel, GError** err) {
	clo_return_val_if_fail(sorter != NULL, 0);
	return sorter->impl_def.get_localmem_usage(sorter, i, lws_max, numel, err);
}

void* clo_sort_get_jit(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, NULL);
	return sorter->jit;
}

const CloSortKeySpec* clo_sort_get_key_spec(CloSort* sorter) {
	clo_return_val_if_fail(sorter != NULL, NULL);
	return &sorter->spec;
}
