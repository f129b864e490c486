/* rqphase.c -- the RMQ chainer of a whole batch in phases, for mga_batch_chain() (batch.c); rq_chain_all() is the one entry. */
#include <stdio.h>
#include "batch_priv.h"

/* ---- MG_M_RMQ (-x asm): the RMQ chainer in phases -------------------------------------------------------------------------
 * A batch under -x asm is a handful of contigs with up to 10^7 anchors each, and one chaining pass over such a contig is seconds of
 * sequential tree work.  The forward pass restarts from empty trees wherever the target (segment, strand) changes
 * (rmq.c: mga_lchain_rmq_fwd), so runs of whole groups are independent: phase 1 sorts every read's anchors (hit order from the
 * device) and cuts them into such runs, phase 2 runs the forward pass of all runs of all reads on all threads, phase 3 backtracks
 * per read and decides about the long-join rescue (map-algo.c:407-417), phases 4-5 repeat 2-3 with bw_long for the reads that
 * need it.  chain_worker then picks the chains up. */
typedef struct { int32_t read, k; } rq_task_t;

#define RQ_RUN_MIN 16384 /* anchors per work item, at least */
#define RQ_RUN_MIN_DEV 1024 /* ... of the device pass: a wavefront per run, thousands of them */
#define RQ_RUN_MAX_DEV (1 << 20) /* a run beyond this is the host's: one wavefront walks a run anchor by anchor */

static void rq_cut(rq_read_t *r, int64_t run_min)
{
	int64_t i, last = 0;
	int32_t m = 16;
	r->cut = MGA_MALLOC(int64_t, m + 1), r->n_cut = 0;
	r->cut[0] = 0;
	for (i = 1; i < r->n; ++i)
		if (r->a[i].x >> 32 != r->a[i - 1].x >> 32 && i - last >= run_min) {
			if (r->n_cut + 1 == m) { m <<= 1; r->cut = MGA_REALLOC(int64_t, r->cut, m + 1); }
			r->cut[++r->n_cut] = i, last = i;
		}
	r->cut[++r->n_cut] = r->n;
}

static void rq_arrays(mga_batch_t *b, rq_read_t *r, int64_t i)
{
	if (b->rq_harr) { /* the device pass: slices of the chunk's pinned arrays p | f | v | t (pass 2 has fewer anchors than pass 1: the same slices) */
		const int64_t T = (b->rq_tot + 1) & ~1LL, o = b->a_off[i] - b->a_off[0];
		r->p = (int64_t*)b->rq_harr + o, r->f = (int32_t*)(b->rq_harr + 8 * T) + o, r->v = (int32_t*)(b->rq_harr + 12 * T) + o, r->t = (int32_t*)(b->rq_harr + 16 * T) + o;
		/* the pinned block is neither zeroed by its allocation nor between chunks (whose p | f | v | t cuts differ), and every HOST forward pass -- the DP of an ultra-long -x lr
		 * read, the barrier form, a run the device hands back -- wants its skip marks cleared (lchain.c:166, :270): cheap next to any of them, so always */
		memset(r->t, 0, (size_t)r->n * 4);
		return;
	}
	r->p = MGA_MALLOC(int64_t, r->n); r->f = MGA_MALLOC(int32_t, r->n); r->v = MGA_MALLOC(int32_t, r->n); r->t = MGA_CALLOC(int32_t, r->n);
}

static void rq_prepare_worker_(void *data, int64_t i, int tid)
{
	mga_batch_t *b = (mga_batch_t*)data;
	rq_read_t *r = &b->rq[i];
	int64_t tc = cpu_now();
	(void)tid;
	r->n = b->a_off[i + 1] - b->a_off[i];
	if (b->qlens[i] == 0 || (b->opt.max_qlen > 0 && b->qlens[i] > b->opt.max_qlen)) r->n = 0; /* chain_worker returns early for these */
	if (r->n <= 0) return;
	r->a = (mg128_t*)(b->a + b->a_off[i]); /* every read owns its slice of the staging buffer */
	if ((b->a_is_raw == 2 || b->a_is_raw == 3) && r->n > 1) mga_ksort_128x(r->n, r->a); /* hit order from the device: radix_sort_128x (map-algo.c:189) */
	if (b->a_is_raw == 3 || b->a_is_raw == 5) { /* (5: already sorted -- the CPU tests' oracle anchors) */ r->cut = MGA_MALLOC(int64_t, 2); r->cut[0] = 0, r->cut[1] = r->n, r->n_cut = 1; } /* an ultra-long -x lr read: its first pass is the DP, one work item */
	else rq_cut(r, b->rq_dev_fwd ? RQ_RUN_MIN_DEV : RQ_RUN_MIN);
	rq_arrays(b, r, i);
	CPU_ADD(C_LCCOPY, tc);
}

static void rq_fwd_worker(void *data, int64_t j, int tid)
{
	mga_batch_t *b = ((mga_batch_t**)data)[0];
	const rq_task_t *task = &((const rq_task_t*)((void**)data)[1])[j];
	rq_read_t *r = &b->rq[task->read];
	const mg_mapopt_t *opt = &b->opt;
	int64_t tc = cpu_now();
	(void)tid;
	if ((b->a_is_raw == 3 || b->a_is_raw == 5) && !r->pass2) { /* mg_lchain_dp (map-algo.c:393-403) on this host thread: hchain.c */
		mga_lchain_par_t par;
		mga_batch_lchain_par(b->gi, opt, 0, &par);
		if (opt->max_gap_ref <= 0 && opt->max_frag_len > 0) { const int g = opt->max_frag_len - b->qlens[task->read]; par.max_dist_x = g > opt->max_gap ? g : opt->max_gap; } /* -F: map-algo.c:383-386 */
		mga_lchain_dp_fwd(par.max_dist_x, par.max_dist_y, par.bw, par.max_skip, par.max_iter, par.chn_pen_gap, par.chn_pen_skip, r->n, r->a, r->f, r->p, r->v, r->t);
	} else
	mga_lchain_rmq_fwd(opt->max_gap, opt->max_gap_pre, r->pass2 ? opt->bw_long : opt->bw, opt->max_lc_skip, opt->rmq_size_cap, b->pen_gap, b->pen_skip,
					   r->cut[task->k], r->cut[task->k + 1], r->a, r->f, r->p, r->v, r->t);
	CPU_ADD(r->pass2 ? C_LCRESCUE : C_LCCOPY, tc);
}

/* runs of the RMQ chainer's forward pass: [0] taken by the device, [1] redone on the host because two candidates tied on the priority (the AVL shape decides: k_rmq.hip),
 * [2] ... because the inner window held more candidates than the kernel sorts, [3] kept on the host for their length, [4] device call failed */
static int64_t g_rq_dev_stat[8];
void mga_rq_dev_stats(int64_t *out, int reset) { int k; for (k = 0; k < 8; ++k) { out[k] = __atomic_load_n(&g_rq_dev_stat[k], __ATOMIC_RELAXED); if (reset) __atomic_store_n(&g_rq_dev_stat[k], 0, __ATOMIC_RELAXED); } }

typedef struct { int64_t len; int32_t k; } rq_ord_t;
static int rq_ord_cmp(const void *x, const void *y) { const rq_ord_t *p = (const rq_ord_t*)x, *q = (const rq_ord_t*)y; return p->len > q->len ? -1 : p->len < q->len ? 1 : (p->k > q->k) - (p->k < q->k); }

static int rq_use_dev(const mga_batch_t *b, const rq_read_t *r) { return b->rq_dev_fwd != 0 && !((b->a_is_raw == 3 || b->a_is_raw == 5) && !r->pass2); }

/* the forward pass of ALL runs of some reads' current pass (the same pass for all of them): on the device, a wavefront per run, ONE launch for all the reads (k_rmq.hip:
 * a launch lasts as long as its longest run, and a read's ~2 000 runs fill a quarter of the wave slots); what the device gives back -- a run with tied priorities, an inner
 * window beyond the kernel's sort -- and what is too long for one wavefront goes through the host's exact tree (rmq.c), run by run, on this thread */
static void rq_dev_worker(mga_batch_t *b, int n_reads, const int32_t *reads)
{
	const mg_mapopt_t *opt = &b->opt;
	const int pass2 = b->rq[reads[0]].pass2;
	int64_t n_runs = 0, k, q, *runs, *abs0, *rn, cnt[5] = { 0, 0, 0, 0, 0 }, tc = cpu_now();
	const mg128_t **ra; int32_t **rf, **rv; int64_t **rp;
	rq_ord_t *ord;
	int32_t *order, *status, n_dev = 0;
	int rc = 0, x;
	for (x = 0; x < n_reads; ++x) n_runs += b->rq[reads[x]].n_cut;
	runs = MGA_MALLOC(int64_t, 3 * n_runs + 3); ord = MGA_MALLOC(rq_ord_t, n_runs + 1); order = MGA_MALLOC(int32_t, n_runs + 1); status = MGA_MALLOC(int32_t, n_runs + 1);
	abs0 = MGA_MALLOC(int64_t, n_reads); rn = MGA_MALLOC(int64_t, n_reads); ra = (const mg128_t**)MGA_MALLOC(void*, n_reads); rf = (int32_t**)MGA_MALLOC(void*, n_reads);
	rv = (int32_t**)MGA_MALLOC(void*, n_reads); rp = (int64_t**)MGA_MALLOC(void*, n_reads);
	for (x = 0, q = 0; x < n_reads; ++x) {
		rq_read_t *r = &b->rq[reads[x]];
		abs0[x] = b->a_off[reads[x]] - b->a_off[0], rn[x] = r->n, ra[x] = r->a, rf[x] = r->f, rv[x] = r->v, rp[x] = r->p;
		for (k = 0; k < r->n_cut; ++k, ++q) {
			runs[3 * q] = abs0[x] + r->cut[k], runs[3 * q + 1] = abs0[x] + r->cut[k + 1], runs[3 * q + 2] = abs0[x];
			status[q] = 3;
			if (r->cut[k + 1] - r->cut[k] <= RQ_RUN_MAX_DEV) ord[n_dev].len = r->cut[k + 1] - r->cut[k], ord[n_dev++].k = (int32_t)q;
		}
	}
	qsort(ord, (size_t)n_dev, sizeof *ord, rq_ord_cmp); /* longest first: a launch lasts as long as its longest run */
	for (k = 0; k < n_dev; ++k) order[k] = ord[k].k, status[ord[k].k] = 4;
	if (n_dev > 0) {
		const double tw0 = mga_wtime();
		pthread_mutex_lock(&b->rq_dev_mtx);
		const double tw1 = mga_wtime();
		rc = b->rq_dev_fwd(b->rq_dev_ctx, n_reads, abs0, rn, ra, rf, rp, rv, (int)n_runs, runs, n_dev, order, pass2 ? opt->bw_long : opt->bw, status);
		if (rc < 0 && !b->rq_dev_err) { b->rq_dev_err = 1; snprintf(b->rq_dev_errmsg, sizeof b->rq_dev_errmsg, "%s", mga_last_error()); } /* (the message is this thread's) */
		pthread_mutex_unlock(&b->rq_dev_mtx);
		if (g_cpu_on) fprintf(stderr, "[rq] pass %d of %d reads: %d runs (longest %ld anchors) through the device in %.1f ms (+ %.1f ms waiting for it)\n", pass2 + 1, n_reads, n_dev, (long)ord[0].len, (mga_wtime() - tw1) * 1e3, (tw1 - tw0) * 1e3);
		if (rc < 0) for (k = 0; k < n_dev; ++k) status[order[k]] = 4; /* (the task graph runs to its end on the host's tree; mga_batch_chain() then FAILS the chunk with the device's message) */
	}
	for (x = 0, q = 0; x < n_reads; ++x) {
		rq_read_t *r = &b->rq[reads[x]];
		for (k = 0; k < r->n_cut; ++k, ++q) {
			if (status[q] == 0) { ++cnt[0]; continue; }
			++cnt[status[q] <= 4 ? status[q] : 4];
			memset(r->t + r->cut[k], 0, (size_t)(r->cut[k + 1] - r->cut[k]) * 4); /* the marks of a run stay inside it */
			mga_lchain_rmq_fwd(opt->max_gap, opt->max_gap_pre, pass2 ? opt->bw_long : opt->bw, opt->max_lc_skip, opt->rmq_size_cap, b->pen_gap, b->pen_skip,
							   r->cut[k], r->cut[k + 1], r->a, r->f, r->p, r->v, r->t);
		}
	}
	for (k = 0; k < 5; ++k) if (cnt[k]) __atomic_fetch_add(&g_rq_dev_stat[k], cnt[k], __ATOMIC_RELAXED);
	free(runs); free(ord); free(order); free(status); free(abs0); free(rn); free((void*)ra); free(rf); free(rv); free(rp);
	CPU_ADD(pass2 ? C_LCRESCUE : C_LCCOPY, tc);
}

static void rq_finish_worker_(void *data, int64_t i, int tid)
{
	mga_batch_t *b = (mga_batch_t*)data;
	rq_read_t *r = &b->rq[i];
	const mg_mapopt_t *opt = &b->opt;
	int64_t tc = cpu_now();
	(void)tid;
	if (r->n <= 0 || r->f == 0) return;
	if (!r->pass2) {
		r->out = mga_lchain_rmq_finish2(opt->bw, opt->min_lc_cnt, opt->min_lc_score, r->n, r->a, r->f, r->p, r->v, r->t, &r->n_lc, &r->u, b->rq_harr != 0);
		r->f = r->v = r->t = 0, r->p = 0; free(r->cut); r->cut = 0;
		if (opt->bw_long > opt->bw && (opt->flag & (MG_M_SPLICE | MG_M_SR)) == 0 && r->n_lc > 1) { /* map-algo.c:407-417 */
			const int32_t qlen = b->qlens[i], st = (int32_t)r->out[0].y, en = (int32_t)r->out[(int32_t)r->u[0] - 1].y;
			if (qlen - (en - st) > opt->rmq_rescue_size || qlen - (en - st) > qlen * opt->rmq_rescue_ratio) {
				int32_t k;
				int64_t n_a = 0;
				for (k = 0; k < r->n_lc; ++k) n_a += (int32_t)r->u[k];
				free(r->u); r->u = 0;
				mga_ksort_128x(n_a, r->out);
				r->a = r->out, r->n = n_a, r->pass2 = 1;
				if (b->rq_dev_fwd && b->a_is_raw == 2) { /* the re-chained anchors go back into the read's slice of the (pinned) staging buffer: the device pass uploads from there, and the
				                                          * chunk-level positions of the second pass are the first pass's (n_a <= the slice's length) */
					mg128_t *slice = (mg128_t*)(b->a + b->a_off[i]);
					memcpy(slice, r->out, (size_t)n_a * sizeof(mg128_t));
					free(r->out); r->out = 0, r->a = slice;
				}
				rq_cut(r, b->rq_dev_fwd ? RQ_RUN_MIN_DEV : RQ_RUN_MIN); rq_arrays(b, r, i);
			}
		}
		CPU_ADD(C_LCCOPY, tc);
	} else {
		mg128_t *a2 = mga_lchain_rmq_finish2(opt->bw_long, opt->min_lc_cnt, opt->min_lc_score, r->n, r->a, r->f, r->p, r->v, r->t, &r->n_lc, &r->u, b->rq_harr != 0);
		r->f = r->v = r->t = 0, r->p = 0; free(r->cut); r->cut = 0;
		free(r->out); r->out = a2;
		CPU_ADD(C_LCRESCUE, tc);
	}
}

/* the big sorts of a contig fan out over the pool (ksortx.c: mga_ksort_threads is per thread) for the duration of the task that sorts, and never beyond it */
static void rq_prepare_worker(void *data, int64_t i, int tid) { mga_ksort_threads = ((mga_batch_t*)data)->n_threads; rq_prepare_worker_(data, i, tid); mga_ksort_threads = 1; }
static void rq_finish_worker(void *data, int64_t i, int tid) { mga_ksort_threads = ((mga_batch_t*)data)->n_threads; rq_finish_worker_(data, i, tid); mga_ksort_threads = 1; }

static void rq_run_fwd(mga_batch_t *b, int pass2)
{
	int64_t n_task = 0, j = 0;
	int i, k;
	rq_task_t *task;
	void *arg[2];
	for (i = 0; i < b->n; ++i) if (b->rq[i].f && b->rq[i].pass2 == pass2) n_task += b->rq[i].n_cut;
	if (n_task == 0) return;
	task = MGA_MALLOC(rq_task_t, n_task);
	for (i = 0; i < b->n; ++i)
		if (b->rq[i].f && b->rq[i].pass2 == pass2)
			for (k = 0; k < b->rq[i].n_cut; ++k) task[j].read = i, task[j++].k = k;
	arg[0] = b, arg[1] = task;
	mga_parallel_for(b->n_threads, n_task, rq_fwd_worker, arg);
	free(task);
}

/* The phases as a task graph (round 4).  With barriers between the phases a batch of 8 contigs keeps 8 of 16 threads busy while it sorts and backtracks (one thread per read,
 * ~1 s per 50 Mbp contig and pass) and every read waits for the slowest: [measured, 10 x 50 Mbp contigs vs a 500 Mbp graph] 65 CPU-s of RMQ chaining in 7.9 s of wall time.
 * The dependencies are per READ -- sort(i) -> forward runs (i, k) -> backtrack(i) -> forward runs with bw_long (i, k) -> backtrack(i) -- so the threads take tasks from one queue:
 * finished forward passes hand their read's backtrack to the FRONT of the queue, a read's forward runs are queued as one block behind the others', and read i backtracks while the
 * forward runs of read i+1 are still being taken.  Same calls on the same data per read: the bytes cannot change.  MGA_RQ_BARRIERS=1: the phases with barriers (A/B). */
typedef struct {
	mga_batch_t *b;
	pthread_mutex_t mtx; pthread_cond_t cv;
	rq_task_t *lo; int64_t lo_head, lo_tail, lo_cap;  /* forward runs (FIFO) */
	int32_t *hi; int32_t n_hi;                         /* reads whose sort (>= 0: read, < 0: ~read = backtrack) is due: taken first, last in first out */
	int32_t *pending;                                  /* forward runs of a read not finished yet */
	int n_open;                                        /* reads with work left */
} rq_sched_t;

static void rq_push_fwd(rq_sched_t *S, int read) /* (locked) */
{
	const rq_read_t *r = &S->b->rq[read];
	int k;
	if (S->lo_tail + r->n_cut > S->lo_cap) { S->lo_cap = (S->lo_tail + r->n_cut) * 2; S->lo = MGA_REALLOC(rq_task_t, S->lo, S->lo_cap); }
	if (rq_use_dev(S->b, r)) { /* ONE task: all runs of the read through the device (k = -1) */
		S->lo[S->lo_tail].read = read, S->lo[S->lo_tail++].k = -1;
		S->pending[read] = 1;
		return;
	}
	for (k = 0; k < r->n_cut; ++k) S->lo[S->lo_tail].read = read, S->lo[S->lo_tail++].k = k;
	S->pending[read] = r->n_cut;
}

static void rq_sched_worker(void *data, int64_t j_, int tid)
{
	rq_sched_t *S = (rq_sched_t*)data;
	mga_batch_t *b = S->b;
	(void)j_;
	pthread_mutex_lock(&S->mtx);
	for (;;) {
		while (S->n_hi == 0 && S->lo_head == S->lo_tail && S->n_open > 0) pthread_cond_wait(&S->cv, &S->mtx);
		if (S->n_hi > 0) {
			const int32_t h = S->hi[--S->n_hi], read = h >= 0 ? h : ~h;
			rq_read_t *r = &b->rq[read];
			pthread_mutex_unlock(&S->mtx);
			if (h >= 0) rq_prepare_worker(b, read, tid); else rq_finish_worker(b, read, tid);
			pthread_mutex_lock(&S->mtx);
			if (r->n > 0 && r->f != 0) rq_push_fwd(S, read); /* sorted and cut, or a second pass with bw_long is due */
			else --S->n_open;
			pthread_cond_broadcast(&S->cv);
		} else if (S->lo_head < S->lo_tail) {
			const rq_task_t t = S->lo[S->lo_head++];
			void *arg[2];
			if (t.k < 0) { /* a device task: every other read whose forward pass of the SAME pass is waiting in the queue goes into the same launch */
				int32_t *rd = MGA_MALLOC(int32_t, S->lo_tail - S->lo_head + 1), n_rd = 0;
				int64_t j, w_ = S->lo_head;
				int x;
				rd[n_rd++] = t.read;
				for (j = S->lo_head; j < S->lo_tail; ++j) {
					if (S->lo[j].k < 0 && b->rq[S->lo[j].read].pass2 == b->rq[t.read].pass2) rd[n_rd++] = S->lo[j].read;
					else S->lo[w_++] = S->lo[j];
				}
				S->lo_tail = w_;
				pthread_mutex_unlock(&S->mtx);
				rq_dev_worker(b, n_rd, rd);
				pthread_mutex_lock(&S->mtx);
				for (x = 0; x < n_rd; ++x) if (--S->pending[rd[x]] == 0) S->hi[S->n_hi++] = ~rd[x];
				pthread_cond_broadcast(&S->cv);
				free(rd);
				continue;
			}
			pthread_mutex_unlock(&S->mtx);
			arg[0] = b, arg[1] = (void*)&t;
			rq_fwd_worker(arg, 0, tid);
			pthread_mutex_lock(&S->mtx);
			if (--S->pending[t.read] == 0) { S->hi[S->n_hi++] = ~t.read; pthread_cond_broadcast(&S->cv); }
		} else break; /* n_open == 0 */
	}
	pthread_mutex_unlock(&S->mtx);
}

void rq_chain_all(mga_batch_t *b)
{
	const int prof = getenv("MGA_DEBUG_PIPE") && atoi(getenv("MGA_DEBUG_PIPE")) > 0; /* wall time: where a -x asm job's host time goes (long queries) */
	const int64_t n_a = b->n > 0 ? b->a_off[b->n] - b->a_off[0] : 0;
	double t[6];
	b->rq = MGA_CALLOC(rq_read_t, b->n > 0 ? b->n : 1);
	t[0] = mga_wtime();
	if (getenv("MGA_RQ_BARRIERS") && atoi(getenv("MGA_RQ_BARRIERS")) > 0) {
		b->rq_dev_fwd = 0; /* (the A/B form with barriers between the phases is the host's) */
		mga_parallel_for(b->n_threads, b->n, rq_prepare_worker, b);
		t[1] = mga_wtime();
		rq_run_fwd(b, 0);
		t[2] = mga_wtime();
		mga_parallel_for(b->n_threads, b->n, rq_finish_worker, b);
		t[3] = mga_wtime();
		rq_run_fwd(b, 1);
		t[4] = mga_wtime();
		mga_parallel_for(b->n_threads, b->n, rq_finish_worker, b);
		t[5] = mga_wtime();
		if (prof) fprintf(stderr, "[rq] %d queries, %ld anchors, %d threads: sort %.3f s, forward pass %.3f, backtrack + rescue decision %.3f, forward pass (bw_long) %.3f, backtrack %.3f\n", b->n, (long)n_a,
						  b->n_threads, t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], t[5] - t[4]);
		return;
	}
	if (b->n > 0) {
		rq_sched_t S;
		int i;
		memset(&S, 0, sizeof S);
		S.b = b, S.n_open = b->n;
		pthread_mutex_init(&S.mtx, 0); pthread_cond_init(&S.cv, 0);
		S.lo_cap = 1024, S.lo = MGA_MALLOC(rq_task_t, S.lo_cap);
		S.hi = MGA_MALLOC(int32_t, b->n), S.pending = MGA_CALLOC(int32_t, b->n);
		for (i = b->n - 1; i >= 0; --i) S.hi[S.n_hi++] = i; /* (taken from the top: read 0 first) */
		mga_parallel_for(b->n_threads, b->n_threads, rq_sched_worker, &S);
		pthread_mutex_destroy(&S.mtx); pthread_cond_destroy(&S.cv);
		free(S.lo); free(S.hi); free(S.pending);
	}
	if (prof) fprintf(stderr, "[rq] %d queries, %ld anchors, %d threads: sort, forward passes and backtracks of both passes as one task graph: %.3f s\n", b->n, (long)n_a, b->n_threads, mga_wtime() - t[0]);
}
