/*
 * chunk.c -- one chunk of reads through the stage sequence: map_chunk() and its chunk_* stage functions (mapper.c has the map of the pipeline).
 * The device stages are launched from here, on the pipeline context's HIP stream; the host halves in between are mga_batch_t's (batch.c).
 */
#include <assert.h>
#include "batch_priv.h"
#include "chunk.h"

/* ------------------------------------------------------------------------------------------------
 * device orchestration
 *
 * A batch is cut into chunks of MGA_CHUNK reads (default 16384).  MGA_PIPE pipeline threads (default 6 with more than
 * four host threads, else 4), each with its own HIP stream context, device buffers and pinned staging buffers, pull chunks
 * from a shared counter and run map_chunk()'s stage functions on them; one token per GPU phase staggers them so that the GPU work of one chunk
 * overlaps the host work of the others.
 * ---------------------------------------------------------------------------------------------- */
#include <pthread.h>

double g_job_t0;
int g_dbg_pipe = -1;
static gpu_token_t g_gpu_front = { PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, 1 }, g_gpu_wfa = { PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, 1 };
static void token_acquire(gpu_token_t *t) { pthread_mutex_lock(&t->m); while (t->avail <= 0) pthread_cond_wait(&t->c, &t->m); --t->avail; pthread_mutex_unlock(&t->m); }
static void token_release(gpu_token_t *t) { pthread_mutex_lock(&t->m); ++t->avail; pthread_cond_signal(&t->c); pthread_mutex_unlock(&t->m); }

static pthread_once_t g_init_once = PTHREAD_ONCE_INIT;
static void chunk_init(void) { g_dbg_pipe = env_int("MGA_DEBUG_PIPE", 0); g_gpu_wfa.avail = env_int("MGA_WFA_SLOTS", 2); g_gpu_front.avail = env_int("MGA_FRONT_SLOTS", 1); }
void chunk_init_once(void) { pthread_once(&g_init_once, chunk_init); } /* (chunk.h says what the two defaults are about) */

/* reads of at least this many bases are "ultra-long" -x lr reads (chunks of their own, first chaining pass on host threads): read ONCE per process (the cut and
 * the chunk's placement must agree, whatever happens to the environment in between) */
int lr_long_bases(void) { static int v = -1; if (v < 0) v = env_int("MGA_LONG_READ", 262144); return v; }

#define CK(x) do { if ((x) < 0) return -1; } while (0) /* inside a stage of map_chunk(): the error is set, chunk_release() cleans up */

/* mga_batch_t's device hook: the forward pass of the RMQ chainer over the runs `order[0 .. n_order)` of one read's x-sorted anchors (k_rmq.hip), on this chunk's stream.
 * Called by ONE host thread at a time (mga_batch_t::rq_dev_mtx) while the chunk's pipeline thread waits inside mga_batch_chain(); f, p, v arrive in the caller's arrays
 * (pinned: the chunk's h_rq), status[run] says which runs the host has to redo. */
typedef struct { pipe_ctx_t *P; const mg_mapopt_t *opt; float pen_gap, pen_skip; int64_t n_total; } rq_dev_ctx_t;
static int rq_dev_fwd_hook(void *ctx_, int n_reads, const int64_t *r_abs0, const int64_t *r_n, const mg128_t *const *r_a, int32_t *const *r_f, int64_t *const *r_p, int32_t *const *r_v,
						   int n_runs, const int64_t *runs, int n_order, const int32_t *order, int bw, int32_t *status)
{
	rq_dev_ctx_t *C = (rq_dev_ctx_t*)ctx_;
	pipe_ctx_t *P = C->P;
	mga_sctx_t *sc = P->sc;
	const mg_mapopt_t *opt = C->opt;
	const int64_t n = C->n_total; /* the chunk's anchors: the device arrays are chunk-level, a read's slice sits at its offset */
	char *hs;
	int x;
	if (mga_dev_bind_thread() < 0) return -1;
	if (mga_dbuf_reserve(&P->rq_a, (size_t)n * 16 + 64) < 0 || mga_dbuf_reserve(&P->rq_f, (size_t)n * 4 + 64) < 0 || mga_dbuf_reserve(&P->rq_p, (size_t)n * 8 + 64) < 0 ||
		mga_dbuf_reserve(&P->rq_v, (size_t)n * 4 + 64) < 0 || mga_dbuf_reserve(&P->rq_t, (size_t)n * 4 + 64) < 0 || mga_dbuf_reserve(&P->rq_pri, (size_t)n * 8 + 64) < 0 ||
		mga_dbuf_reserve(&P->rq_ys, (size_t)n * 4 + 64) < 0 || mga_dbuf_reserve(&P->rq_cut, (size_t)n_runs * 24 + 64) < 0 || mga_dbuf_reserve(&P->rq_ord, (size_t)n_runs * 4 + 64) < 0 ||
		mga_dbuf_reserve(&P->rq_stat, (size_t)n_runs * 4 + 64) < 0 || mga_dbuf_reserve(&P->rq_cnt, 64) < 0 || mga_hbuf_reserve(&P->h_rqs, (size_t)n_runs * 32 + 64) < 0) return -1;
	hs = (char*)P->h_rqs.p; /* runs | order | status through pinned staging: copies from pageable memory wait inside the runtime */
	memcpy(hs, runs, (size_t)n_runs * 24); memcpy(hs + (size_t)n_runs * 24, order, (size_t)n_order * 4); memcpy(hs + (size_t)n_runs * 28, status, (size_t)n_runs * 4);
	for (x = 0; x < n_reads; ++x)
		if (mga_h2d_s(sc, (mg128_t*)P->rq_a.p + r_abs0[x], r_a[x], (size_t)r_n[x] * 16) < 0 || mga_dmemset_s(sc, (int32_t*)P->rq_t.p + r_abs0[x], 0, (size_t)r_n[x] * 4) < 0) return -1;
	if (mga_h2d_s(sc, P->rq_cut.p, hs, (size_t)n_runs * 24) < 0 || mga_h2d_s(sc, P->rq_ord.p, hs + (size_t)n_runs * 24, (size_t)n_order * 4) < 0 ||
		mga_h2d_s(sc, P->rq_stat.p, hs + (size_t)n_runs * 28, (size_t)n_runs * 4) < 0) return -1;
	if (mga_dev_rmq_fwd(sc, n, (const mg128_t*)P->rq_a.p, n_order, P->rq_cut.p, (const int32_t*)P->rq_ord.p, opt->max_gap, opt->max_gap_pre, bw, opt->max_lc_skip, opt->rmq_size_cap,
						C->pen_gap, C->pen_skip, (int32_t*)P->rq_f.p, (int64_t*)P->rq_p.p, (int32_t*)P->rq_v.p, (int32_t*)P->rq_t.p, (double*)P->rq_pri.p, (int32_t*)P->rq_ys.p,
						(int32_t*)P->rq_stat.p, (int*)P->rq_cnt.p) < 0) return -1;
	for (x = 0; x < n_reads; ++x)
		if (mga_d2h_s(sc, r_f[x], (int32_t*)P->rq_f.p + r_abs0[x], (size_t)r_n[x] * 4) < 0 || mga_d2h_s(sc, r_p[x], (int64_t*)P->rq_p.p + r_abs0[x], (size_t)r_n[x] * 8) < 0 ||
			mga_d2h_s(sc, r_v[x], (int32_t*)P->rq_v.p + r_abs0[x], (size_t)r_n[x] * 4) < 0) return -1;
	if (mga_d2h_s(sc, hs + (size_t)n_runs * 28, P->rq_stat.p, (size_t)n_runs * 4) < 0 || mga_ssync(sc) < 0) return -1;
	memcpy(status, hs + (size_t)n_runs * 28, (size_t)n_runs * 4);
	return 0;
}

/* ---- GAF lines on the device (k_gaf.hip) ----
 * One record per line the reference's writer prints for the chunk (format.c:121-250), in print order: the printed chains of every read (in text mode exactly the chains with a
 * text-kernel chain: chain_id >= 0), or the one line of an unmapped read under MG_M_SHOW_UNMAP.  Returns the number of lines; -1: a read of the chunk has chains but no plan
 * (it was not chained here) -- the host then formats the chunk as before. */
static int64_t gaf_lines_build(const mga_batch_t *b, int n, mga_gaf_line_t *line)
{
	int64_t nl = 0;
	int i, k;
	for (i = 0; i < n; ++i) {
		const mg_gchains_t *gcs = b->gcs[i];
		const read_plan_t *pl = &b->plan[i];
		if (gcs == 0 || gcs->n_gc == 0) {
			if (b->opt.flag & MG_M_SHOW_UNMAP) { mga_gaf_line_t *l = &line[nl++]; memset(l, 0, sizeof *l); l->read = i, l->chain = -1, l->qlen = b->qlens[i]; }
			continue;
		}
		if (pl->chain_id == 0) return -1;
		for (k = 0; k < gcs->n_gc; ++k) {
			const mg_gchain_t *p = &gcs->gc[k];
			mga_gaf_line_t *l;
			if (pl->chain_id[k] < 0) continue; /* not printed (format.c:135-136) */
			l = &line[nl++];
			l->read = i, l->qlen = b->qlens[i];
			l->chain = (int32_t)(pl->tid < 0 ? pl->chain_id[k] : b->dp_n_chain + b->tp_chain_base[pl->tid] + pl->chain_id[k]); /* device-planned chains first, then the pools' */
			l->qs = p->qs, l->qe = p->qe, l->plen = p->plen, l->ps = p->ps, l->pe = p->pe;
			l->mapq = (int32_t)p->mapq, l->n_anchor = p->n_anchor, l->score = p->score, l->subsc = p->subsc;
			l->primary = p->id == p->parent, l->div = p->div;
		}
	}
	return nl;
}

typedef struct { char *dst; const char *src; int64_t bytes; int T; } pcopy_t;
static void pcopy_worker(void *data, int64_t t, int tid) { pcopy_t *c = (pcopy_t*)data; const int64_t b = c->bytes * t / c->T, e = c->bytes * (t + 1) / c->T; (void)tid; if (e > b) memcpy(c->dst + b, c->src + b, (size_t)(e - b)); }

/* ---- one chunk: map_chunk() runs the stage functions below, in this order, over one chunk_t ---- */

/* The environment knobs of a chunk, listed HERE only and read once at the chunk's entry (per chunk, not per process: the tests change them between calls of one process). */
typedef struct {
	int host_text;      /* MGA_HOST_TEXT=1: cg:Z / ds:Z are stitched and printed by the host threads even where only GAF bytes are wanted */
	int no_longq;       /* MGA_NO_LONGQ=1: no long-query path for -x asm / ultra-long -x lr chunks */
	int sketch_2bit;    /* MGA_SKETCH_2BIT=1: A/B: the reads as bit planes for the sketch (k_sketch.hip; DESIGN.md has the measurement) */
	int host_rescue;    /* MGA_HOST_RESCUE=1 keeps the long-join rescue (map-algo.c:407-417) on the host (A/B testing); otherwise it runs inside k_lchain */
	int lc_order;       /* MGA_LC_ORDER=0: k_lchain takes the reads in input order instead of most anchors first */
	int dev_gchain_set, dev_gchain_has, dev_gchain; /* MGA_DEV_GCHAIN is in the environment / has a value / that value: 1 / 0 forces graph chaining onto the device / the host threads */
	int host_gchain;    /* MGA_HOST_GCHAIN=1: graph chaining on the host threads, whatever MGA_DEV_GCHAIN says */
	int dev_gchain_pct; /* MGA_DEV_GCHAIN_PCT: percentage of chunks chained on the device when MGA_DEV_GCHAIN is not set and there are more than 12 host threads (default 25) */
	int gc_prof;        /* MGA_GC_PROF=1: per-stage cycle sums of k_gchain for every chunk (profiling aid) */
	int dev_plan;       /* MGA_DEV_PLAN=0: the gap list of device-made chains is made by the host threads instead of k_plan.hip */
	int check;          /* MGA_CHECK=1: debugging aid: invariants of what the device stages handed back (host placement) */
	int dev_splice;     /* MGA_DEV_SPLICE=0: the gaps' targets are spliced on the host and uploaded as bytes (align.h: want_src) */
	int dev_rmq;        /* MGA_DEV_RMQ=0: the RMQ chainer's forward passes stay on the host threads (k_rmq.hip otherwise) */
	int txt_tight;      /* MGA_TXT_TIGHT=1: a deliberately small text pool, so that a test sees the second launch */
	int dev_gaf;        /* MGA_DEV_GAF=0: the host formats the GAF lines as in rounds 1-5 (A/B, tests) */
	int gaf_direct;     /* MGA_GAF_DIRECT=0: a chunk's lines always go through its pieces, never straight to their place in the job's output */
} chunk_knobs_t;

static void chunk_knobs_read(chunk_knobs_t *k)
{
	const char *s = getenv("MGA_DEV_GCHAIN");
	k->host_text = env_int("MGA_HOST_TEXT", 0), k->no_longq = env_int("MGA_NO_LONGQ", 0), k->sketch_2bit = env_int("MGA_SKETCH_2BIT", 0), k->host_rescue = env_int("MGA_HOST_RESCUE", 0);
	k->lc_order = env_int("MGA_LC_ORDER", 1), k->dev_gchain_set = s != 0, k->dev_gchain_has = s && *s, k->dev_gchain = k->dev_gchain_has ? atoi(s) : 0;
	k->host_gchain = env_int("MGA_HOST_GCHAIN", 0), k->dev_gchain_pct = env_int("MGA_DEV_GCHAIN_PCT", 25), k->gc_prof = env_int("MGA_GC_PROF", 0), k->dev_plan = env_int("MGA_DEV_PLAN", 1);
	k->check = env_int("MGA_CHECK", 0), k->dev_splice = env_int("MGA_DEV_SPLICE", 1), k->dev_rmq = env_int("MGA_DEV_RMQ", 1);
	k->txt_tight = env_int("MGA_TXT_TIGHT", 0), k->dev_gaf = env_int("MGA_DEV_GAF", 1), k->gaf_direct = env_int("MGA_GAF_DIRECT", 1);
}

typedef struct { /* one run of the stage sequence: a stack object of map_chunk() */
	/* inputs (map_chunk()'s arguments; `in` is a copy, so that a coverage job can override three of them) */
	pipe_ctx_t *P; chunk_args_t in;
	chunk_knobs_t k;
	/* mode flags */
	int is_rmq, chunk_long; /* -x asm; -x lr, a chunk of ultra-long reads (batch_cut): the long-query path as well, first chaining pass on host threads (hchain.c: mga_lchain_dp_fwd) */
	int long_q;     /* few, very long queries -- intra-query parallel sketch and seed expansion, anchors sorted by the host chainer */
	int want_text;  /* only GAF bytes are wanted: cg/ds come from the device */
	int dev_gc, dev_plan, dev_splice; /* graph chaining (k_gchain.hip) / its gap list (k_plan.hip) / the gaps' targets (align.h: want_src) made on the device */
	int need_a;     /* the host reads the device-made chains' anchors */
	int gaps;       /* there is something to align, or text to make: the WFA stages run */
	/* counts */
	int64_t tot, n_mz, n_a, n_mini, n_prob, n_tb;
	unsigned long long ptot[8]; /* device-made gap list: printed chains, plan items, problems, walk vertices, target bytes, query bases, overflow flag */
	unsigned long long ctl[9];  /* k_gchain's counters: [1] [2] [6] records used in the three pools, [3] reads to retry, [4] [5] GWFA / shortest-k calls, [7] arena peak, [8] GWFA calls / graph searches that ran in the LDS scratch */
	int64_t gc_cap, lc_cap, ga_cap; /* ... and the pools' capacities */
	int64_t dp_chain, dp_item, dp_prob, dp_vert, dp_tb, hp_prob, hp_tb; /* the device-made gap list (dev_plan) comes first in every array; what the host threads planned (all reads, or with dev_plan the few reads chained here) follows */
	int64_t n_item, n_chain, n_vert, n_ops, cells; unsigned long long txt_used;
	/* owned host arrays (chunk_release() frees them) */
	int64_t *q_off, *h_mzoff, *h_aoff, *h_minioff; int32_t *h_nmz, *h_rep, *h_nu, *h_nb, *h_rflag;
	/* borrowed, inside the context's pinned staging: the device-made chains' headers, the device-made gap list's first printed chain per read */
	mga_gc_hdr_t *h_gchdr_p; int64_t *h_ploff;
	/* state; rq_ctx lives HERE because its address leaves the stage that sets it (other threads use it inside mga_batch_chain()); held because one stage acquires the token and a later one releases it */
	const char *d_seq; double t0 /* start of the interval being timed */; mga_lchain_par_t par; rq_dev_ctx_t rq_ctx; mga_batch_t *b;
	gpu_token_t *held; /* GPU phase token currently owned */
} chunk_t;

static void chunk_token_acquire(chunk_t *c, gpu_token_t *t) { token_acquire(t); c->held = t; }
static void chunk_token_release(chunk_t *c) { if (c->held) { token_release(c->held); c->held = 0; } }

/* a stage is over: its interval goes to `acc` and to the MGA_DEBUG_PIPE log */
static void chunk_lap(chunk_t *c, const char *what, double *acc)
{
	double t1;
	if (g_dbg_pipe > 1) PIPE_LOG(what, c->in.n, c->t0);
	t1 = mga_wtime(); *acc += t1 - c->t0; c->t0 = t1;
}

/* ---- reads -> HBM, back to back, 64 readable bytes of padding at the end (8-byte compares in k_wfa);
 *      skipped when the caller keeps the batch resident (d_seq_res + absolute offsets q_off_res) ---- */
static int chunk_upload_reads(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; const int n = c->in.n; int64_t *q_off = c->q_off;
	gpu_token_t *front = P->tok_front ? P->tok_front : &g_gpu_front;
	int i;
	if (c->in.d_seq_res) {
		memcpy(q_off, c->in.q_off_res, (size_t)(n + 1) * 8);
		c->tot = q_off[n] - q_off[0];
		chunk_token_acquire(c, front);
		c->d_seq = c->in.d_seq_res;
	} else {
		const char *h_seq;
		int64_t tot = 0;
		for (i = 0; i < n; ++i) { q_off[i] = tot; tot += c->in.qlens[i]; }
		q_off[n] = c->tot = tot;
		if (c->in.seqs_pinned) h_seq = c->in.seqs[0]; /* the reader parsed the batch into pinned memory, reads back to back: no staging copy */
		else { /* staged before the GPU phase token is taken: the copy is host work */
			char *h;
			CK(mga_hbuf_reserve(&P->h_seq, (size_t)tot + 64));
			h = (char*)P->h_seq.p;
			for (i = 0; i < n; ++i) memcpy(h + q_off[i], c->in.seqs[i], (size_t)c->in.qlens[i]);
			memset(h + tot, 0, 64);
			h_seq = h;
		}
		chunk_token_acquire(c, front);
		CK(mga_dbuf_reserve(&P->seq, (size_t)tot + 64));
		CK(mga_h2d_s(sc, P->seq.p, h_seq, (size_t)tot + 64));
		c->d_seq = (const char*)P->seq.p;
	}
	CK(mga_dbuf_reserve(&P->qoff, (size_t)(n + 1) * 8));
	CK(mga_h2d_s(sc, P->qoff.p, q_off, (size_t)(n + 1) * 8));
	return 0;
}

/* the long_q sketch -- contigs of megabases: pieces of 64 kb are the work items (k_sketch.hip), count + scan + write, exact contiguous offsets */
static int sketch_pieces(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; const mg_idx_t *gi = c->in.gi; const int n = c->in.n; const int *qlens = c->in.qlens;
	int64_t *h_mzoff = c->h_mzoff; int32_t *h_nmz = c->h_nmz;
	const int32_t PIECE = 1 << 16;
	int64_t n_items = 0, it = 0, *h_itoff;
	int32_t *h_item;
	int rc, i;
	for (i = 0; i < n; ++i) n_items += qlens[i] > 0 ? (qlens[i] + PIECE - 1) / PIECE : 1;
	h_item = MGA_MALLOC(int32_t, n_items * 4);
	h_itoff = MGA_MALLOC(int64_t, n_items + 1);
	for (i = 0; i < n; ++i) {
		int32_t beg = 0;
		do { h_item[it * 4] = i, h_item[it * 4 + 1] = beg, h_item[it * 4 + 2] = beg + PIECE < qlens[i] ? beg + PIECE : qlens[i], h_item[it * 4 + 3] = 0; ++it, beg += PIECE; } while (beg < qlens[i]);
	}
	rc = mga_dbuf_reserve(&P->sk_item, (size_t)n_items * 16) < 0 || mga_dbuf_reserve(&P->sk_cnt, (size_t)n_items * 4 + 4) < 0 || mga_dbuf_reserve(&P->sk_off, (size_t)(n_items + 1) * 8) < 0
		|| mga_h2d_s(sc, P->sk_item.p, h_item, (size_t)n_items * 16) < 0
		|| mga_dev_sketch_items(sc, (int)n_items, (const int32_t*)P->sk_item.p, c->d_seq, (const int64_t*)P->qoff.p, 0, gi->w, gi->k, (int32_t*)P->sk_cnt.p, 0, 0) < 0
		|| mga_dev_scan_i32_to_i64(sc, (const int32_t*)P->sk_cnt.p, n_items, (int64_t*)P->sk_off.p) < 0
		|| mga_ssync(sc) < 0 || mga_d2h(h_itoff, P->sk_off.p, (size_t)(n_items + 1) * 8) < 0 ? -1 : 0; /* (h_item must stay alive until the copy has been consumed) */
	if (rc == 0) {
		for (i = 0, it = 0; i < n; ++i) { h_mzoff[i] = h_itoff[it]; it += qlens[i] > 0 ? (qlens[i] + PIECE - 1) / PIECE : 1; }
		h_mzoff[n] = c->n_mz = h_itoff[n_items];
		for (i = 0; i < n; ++i) {
			if (h_mzoff[i + 1] - h_mzoff[i] > 0x7fffffff) { mga_set_error("read %d has more than 2^31 minimizers", i); rc = -1; break; }
			h_nmz[i] = (int32_t)(h_mzoff[i + 1] - h_mzoff[i]);
		}
	}
	free(h_item); free(h_itoff);
	if (rc < 0) return -1;
	CK(mga_h2d_s(sc, P->mzoff.p, h_mzoff, (size_t)(n + 1) * 8)); CK(mga_h2d_s(sc, P->cnt.p, h_nmz, (size_t)n * 4));
	CK(mga_dbuf_reserve(&P->mz, (size_t)c->n_mz * 16 + 16));
	CK(mga_dev_sketch_items(sc, (int)n_items, (const int32_t*)P->sk_item.p, c->d_seq, (const int64_t*)P->qoff.p, 0, gi->w, gi->k, 0, (const int64_t*)P->sk_off.p, (mg128_t*)P->mz.p));
	CK(mga_ssync(sc)); /* h_mzoff / h_nmz uploads done */
	return 0;
}

/* ---- sketch: ONE pass into per-read slots of qlen/2 + 64 minimizers (the density is 2/(w+1), ~3x less); a read that would
 *      overflow its slots (never seen) sends the chunk through count + scan + write ---- */
static int chunk_sketch(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; const mg_idx_t *gi = c->in.gi; const int n = c->in.n; const int *qlens = c->in.qlens;
	int64_t *h_mzoff, n_mz = 0;
	int32_t *h_nmz;
	int i, overflow = 0;
	CK(mga_dbuf_reserve(&P->cnt, (size_t)n * 4 + 4)); CK(mga_dbuf_reserve(&P->mzoff, (size_t)(n + 1) * 8));
	h_mzoff = c->h_mzoff = MGA_MALLOC(int64_t, n + 1);
	h_nmz = c->h_nmz = MGA_MALLOC(int32_t, n);
	if (c->long_q) return sketch_pieces(c);
	for (i = 0; i < n; ++i) { h_mzoff[i] = n_mz; n_mz += qlens[i] / 2 + 64; }
	h_mzoff[n] = n_mz; /* capacity of the chunk */
	CK(mga_h2d_s(sc, P->mzoff.p, h_mzoff, (size_t)(n + 1) * 8));
	CK(mga_dbuf_reserve(&P->mz, (size_t)n_mz * 16 + 16));
	if (c->k.sketch_2bit) CK(mga_dev_pack2(sc, c->d_seq, c->q_off[n]));
	CK(mga_dev_sketch(sc, n, c->d_seq, (const int64_t*)P->qoff.p, 0, gi->w, gi->k, (int32_t*)P->cnt.p, (const int64_t*)P->mzoff.p, (mg128_t*)P->mz.p));
	CK(mga_d2h_s(sc, h_nmz, P->cnt.p, (size_t)n * 4)); CK(mga_ssync(sc));
	for (i = 0; i < n; ++i) if (h_nmz[i] > qlens[i] / 2 + 64) overflow = 1;
	if (overflow) {
		CK(mga_dev_scan_i32_to_i64(sc, (const int32_t*)P->cnt.p, n, (int64_t*)P->mzoff.p));
		CK(mga_d2h_s(sc, h_mzoff, P->mzoff.p, (size_t)(n + 1) * 8)); CK(mga_ssync(sc));
		n_mz = h_mzoff[n];
		CK(mga_dbuf_reserve(&P->mz, (size_t)n_mz * 16 + 16));
		CK(mga_dev_sketch(sc, n, c->d_seq, (const int64_t*)P->qoff.p, 0, gi->w, gi->k, 0, (const int64_t*)P->mzoff.p, (mg128_t*)P->mz.p));
	}
	c->n_mz = n_mz;
	return 0;
}

/* ---- seeds: occurrences per minimizer, anchors and kept minimizers per read, their offsets on the host ---- */
static int chunk_seed_count(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; struct mg_idx_bucket_s *B = c->in.gi->B; const mg_mapopt_t *opt = c->in.opt; const int n = c->in.n; const int64_t n_mz = c->n_mz;
	CK(mga_dbuf_reserve(&P->occ, (size_t)n_mz * 4 + 4)); CK(mga_dbuf_reserve(&P->val, (size_t)n_mz * 8 + 8));
	CK(mga_dbuf_reserve(&P->na, (size_t)n * 4 + 4)); CK(mga_dbuf_reserve(&P->nmini, (size_t)n * 4 + 4)); CK(mga_dbuf_reserve(&P->rep, (size_t)n * 4 + 4));
	CK(mga_dbuf_reserve(&P->aoff, (size_t)(n + 1) * 8)); CK(mga_dbuf_reserve(&P->minioff, (size_t)(n + 1) * 8));
	if (c->long_q) {
		CK(mga_dbuf_reserve(&P->sd_tk, (size_t)n_mz * 4 + 4)); CK(mga_dbuf_reserve(&P->sd_kf, (size_t)n_mz * 4 + 4));
		CK(mga_dbuf_reserve(&P->sd_offa, (size_t)(n_mz + 1) * 8)); CK(mga_dbuf_reserve(&P->sd_offm, (size_t)(n_mz + 1) * 8));
		CK(mga_dbuf_reserve(&P->sd_rkey, (size_t)n_mz * 8 + 8)); CK(mga_dbuf_reserve(&P->sd_rmax, (size_t)n_mz * 8 + 8));
		CK(mga_dev_seed_long_count(sc, &B->dev, n, (const mg128_t*)P->mz.p, (const int64_t*)P->mzoff.p, n_mz, opt->occ_max1, (int32_t*)P->occ.p, (uint64_t*)P->val.p,
								   (int32_t*)P->sd_tk.p, (int32_t*)P->sd_kf.p, (int64_t*)P->sd_offa.p, (int64_t*)P->sd_offm.p, (uint64_t*)P->sd_rkey.p, (uint64_t*)P->sd_rmax.p,
								   (int64_t*)P->aoff.p, (int64_t*)P->minioff.p, (int32_t*)P->rep.p));
	} else {
		CK(mga_dev_seed_count(sc, &B->dev, n, (const mg128_t*)P->mz.p, (const int64_t*)P->mzoff.p, (const int32_t*)P->cnt.p, opt->occ_max1, (int32_t*)P->occ.p, (uint64_t*)P->val.p,
						  (int32_t*)P->na.p, (int32_t*)P->nmini.p, (int32_t*)P->rep.p));
		CK(mga_dev_scan_i32_to_i64(sc, (const int32_t*)P->na.p, n, (int64_t*)P->aoff.p));
		CK(mga_dev_scan_i32_to_i64(sc, (const int32_t*)P->nmini.p, n, (int64_t*)P->minioff.p));
	}
	c->h_aoff = MGA_MALLOC(int64_t, n + 1); c->h_minioff = MGA_MALLOC(int64_t, n + 1); c->h_rep = MGA_MALLOC(int32_t, n);
	CK(mga_d2h_s(sc, c->h_aoff, P->aoff.p, (size_t)(n + 1) * 8)); CK(mga_d2h_s(sc, c->h_minioff, P->minioff.p, (size_t)(n + 1) * 8)); CK(mga_d2h_s(sc, c->h_rep, P->rep.p, (size_t)n * 4));
	CK(mga_ssync(sc));
	return 0;
}

/* ... and the anchors themselves (map_chunk() books the time up to here to the sketch, from here on to the chaining) */
static int chunk_seed_fill(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; struct mg_idx_bucket_s *B = c->in.gi->B; const mg_mapopt_t *opt = c->in.opt; const int n = c->in.n; const int64_t n_mz = c->n_mz;
	const int64_t n_a = c->n_a = c->h_aoff[n], n_mini = c->n_mini = c->h_minioff[n];
	CK(mga_dbuf_reserve(&P->a, (size_t)n_a * 16 + 64)); CK(mga_dbuf_reserve(&P->mini, (size_t)n_mini * 4 + 16));
	if (c->long_q) {
		CK(mga_dev_seed_long_fill(sc, &B->dev, n, (const mg128_t*)P->mz.p, (const int64_t*)P->mzoff.p, n_mz, opt->occ_max1, (const int32_t*)P->occ.p, (const uint64_t*)P->val.p,
								  (const int64_t*)P->sd_offa.p, (const int64_t*)P->sd_offm.p, (mg128_t*)P->a.p, (int32_t*)P->mini.p));
	} else {
		CK(mga_dbuf_reserve(&P->tmp, (size_t)n_a * 16 + 64));
		CK(mga_dev_seed_fill(sc, &B->dev, n, (const mg128_t*)P->mz.p, (const int64_t*)P->mzoff.p, (const int32_t*)P->cnt.p, opt->occ_max1, (const int32_t*)P->occ.p, (const uint64_t*)P->val.p,
							 (const int64_t*)P->aoff.p, (mg128_t*)P->a.p, (const int64_t*)P->minioff.p, (int32_t*)P->mini.p, (mg128_t*)P->tmp.p));
	}
	CK(mga_hbuf_reserve(&P->h_mini, (size_t)n_mini * 4 + 16));
	return 0;
}

/* Where a chunk's graph chaining (gc_core.h) runs.  It runs where it fits: on the device, one wavefront per read (k_gchain.hip, [measured] ~0.13 s of GPU time per 100k reads),
 * when this GPU has few host threads to itself -- a node whose CPU quota does not grow with its GPUs -- and on the host threads
 * ([measured] ~3 CPU-s per 100k reads on a 3 Gbp graph) when there are enough of them to keep up.  [measured, cores = threads] 8: 1.42 (host) vs 1.78 Gbp/s
 * (device); 10: 1.59 vs 1.83; 16: 2.00 vs 1.84.  MGA_DEV_GCHAIN=1 / 0 forces one or the other; same bytes either way.
 * Round 6: with many host threads neither side is idle -- the host threads chain the graph for 2.3-2.7 CPU-s per 125 000 reads while the GPU runs 250 ms of kernels --
 * so a SHARE of the chunks takes the device placement (k_gchain + k_plan fill the chip's idle wave slots at 2 waves per SIMD) and the rest the host's: both placements
 * give the same bytes (every e2e test runs them), a chunk is a unit.  MGA_DEV_GCHAIN_PCT = percentage of chunks on the device when MGA_DEV_GCHAIN is not set
 * (default 25: [measured, profiles/r06y_hybrid.txt] the same throughput as 0 on a box whose 16 cores keep up -- 4.40 vs 4.42 Gbp/s -- at 2.9 instead of 4.0 CPU-s per step;
 * the final bench run of this round landed on a box where they do not: 3.72 Gbp/s at 4.95 CPU-s with all chunks on the host, 4.05 with all on the device);
 * MGA_DEV_GCHAIN=0 / 1 forces one placement as before.
 * The process-wide turn counter advances on the percentage route only: the sequence of placements over a job depends on it. */
static int gchain_on_device(const chunk_t *c, int rescue_enabled)
{
	static int g_gc_turn = 0;
	int turn;
	if (!rescue_enabled || c->in.gi->B->dev.d_arc == 0 || c->k.host_gchain) return 0; /* (the kernel needs the rescue flags of k_lchain and the graph's arcs in HBM) */
	if (c->k.dev_gchain_has) return c->k.dev_gchain != 0;
	if (c->in.n_threads <= 12) return 1;
	if (c->k.dev_gchain_set) return 0; /* (set to an empty string: no percentage route) */
	turn = __sync_fetch_and_add(&g_gc_turn, 1);
	return c->k.dev_gchain_pct > 0 && ((int64_t)(turn + 1) * c->k.dev_gchain_pct) / 100 > ((int64_t)turn * c->k.dev_gchain_pct) / 100;
}

/* ---- linear chaining (k_lchain.hip), not for -x asm / ultra-long reads, whose anchors the host chainer takes as they are ---- */
static int chunk_lchain(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; const mg_mapopt_t *opt = c->in.opt; const int n = c->in.n; const int64_t n_a = c->n_a, *h_aoff = c->h_aoff;
	size_t wsb;
	mga_rescue_par_t rs;
	int i;
	CK(mga_hbuf_reserve(&P->h_b, (size_t)n_a * 16 + 16));
	if (c->is_rmq || c->chunk_long) return 0;
	wsb = mga_dev_lchain_ws_bytes(n_a);
	mga_batch_lchain_par(c->in.gi, opt, 0, &c->par);
	CK(mga_dbuf_reserve(&P->u, (size_t)n_a * 8 + 8)); CK(mga_dbuf_reserve(&P->b, (size_t)n_a * 16 + 16));
	CK(mga_dbuf_reserve(&P->nu, (size_t)n * 4 + 4)); CK(mga_dbuf_reserve(&P->nb, (size_t)n * 4 + 4)); CK(mga_dbuf_reserve(&P->ws, wsb));
	memset(&rs, 0, sizeof rs);
	rs.enabled = opt->bw_long > opt->bw && (opt->flag & (MG_M_SPLICE | MG_M_SR)) == 0 && !c->k.host_rescue;
	rs.max_dist = opt->max_gap, rs.max_dist_inner = opt->max_gap_pre, rs.bw = opt->bw_long, rs.max_skip = opt->max_lc_skip, rs.cap = opt->rmq_size_cap;
	rs.min_cnt = opt->min_lc_cnt, rs.min_sc = opt->min_lc_score, rs.chn_pen_gap = c->par.chn_pen_gap, rs.chn_pen_skip = c->par.chn_pen_skip;
	rs.rescue_size = opt->rmq_rescue_size, rs.rescue_ratio = opt->rmq_rescue_ratio;
	if (opt->max_gap_ref <= 0 && opt->max_frag_len > 0) rs.frag_len = opt->max_frag_len, rs.frag_min_gap = opt->max_gap; /* -F */
	CK(mga_dbuf_reserve(&P->rflag, (size_t)n * 4 + 4));
	if (c->k.lc_order) { /* the launch lasts as long as its longest read: the reads with the most anchors are launched first (a counting sort of the anchor counts, 16 per bin) */
		enum { NBIN = 4096 };
		/* (the order is built in the context's pinned staging and the copy is only ENQUEUED -- the stream puts it before k_lchain; two mallocs, a pageable
		 * copy and a full synchronisation per chunk stood here while the chunk held the front-phase token.  The buffer is next written by this context's next chunk.) */
		int32_t *ord, cnt_[NBIN + 1];
		CK(mga_hbuf_reserve(&P->h_lcord, (size_t)n * 4 + 16)); CK(mga_dbuf_reserve(&P->lcord, (size_t)n * 4 + 4));
		ord = (int32_t*)P->h_lcord.p;
		memset(cnt_, 0, sizeof cnt_);
		for (i = 0; i < n; ++i) { const int64_t na_ = (h_aoff[i + 1] - h_aoff[i]) >> 4; ++cnt_[NBIN - 1 - (na_ < NBIN ? na_ : NBIN - 1) + 1]; }
		for (i = 0; i < NBIN; ++i) cnt_[i + 1] += cnt_[i];
		for (i = 0; i < n; ++i) { const int64_t na_ = (h_aoff[i + 1] - h_aoff[i]) >> 4; ord[cnt_[NBIN - 1 - (na_ < NBIN ? na_ : NBIN - 1)]++] = (int32_t)i; }
		CK(mga_h2d_s(sc, P->lcord.p, ord, (size_t)n * 4));
		mga_dev_lchain_order(sc, (const int32_t*)P->lcord.p);
	}
	CK(mga_dev_lchain(sc, n, (const mg128_t*)P->a.p, (const int64_t*)P->aoff.p, &c->par, &rs, (const int64_t*)P->qoff.p, (uint64_t*)P->u.p, (mg128_t*)P->b.p,
					  (int32_t*)P->nu.p, (int32_t*)P->nb.p, (int32_t*)P->rflag.p, P->ws.p, wsb, n_a));
	c->h_nu = MGA_MALLOC(int32_t, n); c->h_nb = MGA_MALLOC(int32_t, n);
	CK(mga_hbuf_reserve(&P->h_u, (size_t)n_a * 8 + 8));
	CK(mga_d2h_s(sc, c->h_nu, P->nu.p, (size_t)n * 4)); CK(mga_d2h_s(sc, c->h_nb, P->nb.p, (size_t)n * 4));
	if (rs.enabled) { /* otherwise the host evaluates the rescue condition itself */
		c->h_rflag = MGA_MALLOC(int32_t, n);
		CK(mga_d2h_s(sc, c->h_rflag, P->rflag.p, (size_t)n * 4));
	}
	c->dev_gc = gchain_on_device(c, rs.enabled);
	return 0;
}

/* one launch of k_gchain.hip: the n reads of `list` (NULL: all of them), in the 1 MiB arenas or the large ones; reads that outgrow theirs are listed in retry_out */
static int gchain_launch(chunk_t *c, int n, const int32_t *list, int large, int32_t *retry_out)
{
	pipe_ctx_t *P = c->P;
	return mga_dev_gchain(P->sc, &c->in.gi->B->dev, c->in.opt, c->in.gi->k, c->par.chn_pen_gap, n, list, large, (const int64_t*)P->aoff.p, (const int32_t*)P->nu.p, (const int32_t*)P->nb.p, (const uint64_t*)P->u.p,
						  (const mg128_t*)P->b.p, (const int64_t*)P->minioff.p, (const int32_t*)P->mini.p, (const int64_t*)P->qoff.p, c->d_seq, (const uint32_t*)P->hash.p,
						  (const int32_t*)P->rflag.p, (mga_gc_hdr_t*)P->gchdr.p, P->gcpool.p, c->gc_cap, (mg_llchain_t*)P->lcpool.p, c->lc_cap, (mg128_t*)P->apool.p, c->ga_cap,
						  (unsigned long long*)P->gcctl.p, retry_out);
}

/* reads that outgrew the 1 MiB arena: once more with the large arenas, records appended to the same pools */
static int gchain_retry(chunk_t *c, int64_t n_retry)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; unsigned long long *ctl = c->ctl;
	unsigned long long zero2[1] = { 0 };
	long long n_again;
	CK(mga_h2d_s(sc, (char*)P->gcctl.p, zero2, 8)); CK(mga_h2d_s(sc, (char*)P->gcctl.p + 24, zero2, 8)); CK(mga_ssync(sc));
	CK(gchain_launch(c, (int)n_retry, (const int32_t*)P->gcretry.p, 1, (int32_t*)P->gcretry.p + c->in.n)); /* (its own list for what fails again: the input list is still being consumed) */
	CK(mga_d2h_s(sc, ctl, P->gcctl.p, 72)); CK(mga_ssync(sc));
	/* A read that fails again -- more scratch than the large arena, or the record pools ran out during the retry -- is left with a non-zero status
	 * and no records: the host threads chain it, like the reads whose rescue k_lchain deferred (this used to fail the whole job). */
	if ((int64_t)ctl[1] > c->gc_cap) ctl[1] = (unsigned long long)c->gc_cap; /* (the pool counters ran past the pools: only what fits was written) */
	if ((int64_t)ctl[2] > c->lc_cap) ctl[2] = (unsigned long long)c->lc_cap;
	if ((int64_t)ctl[6] > c->ga_cap) ctl[6] = (unsigned long long)c->ga_cap;
	c->in.st->n_gc_retry += n_retry;
	n_again = (long long)ctl[3]; /* reads the retry launch gave up on as well are chained by the host threads: counted, and said once */
	if (n_again > 0) {
		static int warned = 0;
		c->in.st->n_gc_host += n_again;
		if (mg_verbose >= 2 && !warned) { warned = 1; fprintf(stderr, "[W::map_chunk] graph chaining on the device: %lld of %lld retried reads go to the host threads (record pools %lld/%lld %lld/%lld %lld/%lld)\n", n_again, (long long)n_retry, (long long)ctl[1], (long long)c->gc_cap, (long long)ctl[2], (long long)c->lc_cap, (long long)ctl[6], (long long)c->ga_cap); }
	}
	return 0;
}

/* the chunk through k_gchain until the record pools hold it; leaves the counters in c->ctl */
static int gchain_run(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; unsigned long long *ctl = c->ctl;
	const size_t rec = mga_gc_rec_bytes();
	int attempt;
	for (attempt = 0;; ++attempt) {
		CK(mga_dbuf_reserve(&P->gcpool, (size_t)c->gc_cap * rec)); CK(mga_dbuf_reserve(&P->lcpool, (size_t)c->lc_cap * sizeof(mg_llchain_t))); CK(mga_dbuf_reserve(&P->apool, (size_t)c->ga_cap * 16));
		CK(mga_dmemset_s(sc, P->gcctl.p, 0, 256));
		if (c->k.gc_prof) { unsigned long long one = 1; CK(mga_h2d_s(sc, (char*)P->gcctl.p + 15 * 8, &one, 8)); CK(mga_ssync(sc)); }
		CK(gchain_launch(c, c->in.n, 0, 0, (int32_t*)P->gcretry.p));
		CK(mga_d2h_s(sc, ctl, P->gcctl.p, 72)); CK(mga_ssync(sc));
		if ((int64_t)ctl[1] <= c->gc_cap && (int64_t)ctl[2] <= c->lc_cap && (int64_t)ctl[6] <= c->ga_cap) break;
		/* a record pool was too small: size it to what the kernel asked for and run the chunk again */
		if (attempt >= 2) { mga_set_error("graph chaining: record pools keep overflowing (%lld/%lld/%lld)", (long long)ctl[1], (long long)ctl[2], (long long)ctl[6]); return -1; }
		if ((int64_t)ctl[1] > c->gc_cap) c->gc_cap = (int64_t)ctl[1] * 2;
		if ((int64_t)ctl[2] > c->lc_cap) c->lc_cap = (int64_t)ctl[2] * 2;
		if ((int64_t)ctl[6] > c->ga_cap) c->ga_cap = (int64_t)ctl[6] * 2;
	}
	if ((int64_t)ctl[3] > 0) CK(gchain_retry(c, (int64_t)ctl[3]));
	return 0;
}

/* ---- graph chaining: chain records, clean-up, DP + shortest walks, GWFA bridging, ordering, filters -- one wavefront per read ---- */
static int chunk_gchain_dev(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; struct mg_idx_bucket_s *B = c->in.gi->B; const mg_mapopt_t *opt = c->in.opt; const int n = c->in.n; unsigned long long *ctl = c->ctl;
	const size_t rec = mga_gc_rec_bytes();
	uint32_t *h_hash;
	int rc, i;
	if (!c->dev_gc) return 0;
	h_hash = MGA_MALLOC(uint32_t, n);
	for (i = 0; i < n; ++i) h_hash[i] = mga_read_hash(c->in.qnames ? c->in.qnames[i] : 0, c->in.qlens[i], opt->seed);
	c->gc_cap = c->n_a / (opt->min_lc_cnt > 0 ? opt->min_lc_cnt : 1) + n + 64, c->lc_cap = c->gc_cap * 3 + 4096, c->ga_cap = c->n_a + 64;
	rc = mga_dbuf_reserve(&P->hash, (size_t)n * 4 + 4) < 0 || mga_h2d_s(sc, P->hash.p, h_hash, (size_t)n * 4) < 0 || mga_ssync(sc) < 0 ? -1 : 0;
	free(h_hash);
	if (rc < 0) return -1;
	CK(mga_dbuf_reserve(&P->gchdr, (size_t)n * sizeof(mga_gc_hdr_t) + 64)); CK(mga_dbuf_reserve(&P->gcctl, 256)); CK(mga_dbuf_reserve(&P->gcretry, (size_t)n * 8 + 8)); /* (two lists: the first launch's retries, the retry launch's own) */
	CK(mga_hbuf_reserve(&P->h_gchdr, (size_t)n * sizeof(mga_gc_hdr_t) + 64)); /* (large read-backs go to pinned memory) */
	CK(gchain_run(c));
	c->in.st->n_gwfa += (int64_t)ctl[4], c->in.st->n_shortk += (int64_t)ctl[5];
	if (c->k.gc_prof) { /* per-stage cycle sums of this chunk (profiling aid) */
		unsigned long long tk[16];
		static const char *nm[16] = { "", "records", "cleanup", "index", "dp+shortk", "assemble(rest)", "post", "MAX-wave", "gwfa(rest)", "measure", "order", "gw:clear", "gw:runs", "gw:heads", "gw:dedup", "MAX-read" };
		int q_;
		CK(mga_d2h_s(sc, tk, (char*)P->gcctl.p + 128, 128)); CK(mga_ssync(sc));
		fprintf(stderr, "[gc-prof] %d reads, %llu GWFA calls (%llu in the LDS scratch), Mcycles:", n, ctl[4], ctl[8]);
		for (q_ = 1; q_ < 16; ++q_) if (nm[q_][0]) fprintf(stderr, " %s %.1f", nm[q_], tk[q_] * 1e-6);
		fprintf(stderr, "\n");
	}
	if ((int64_t)ctl[7] > c->in.st->gc_arena_peak) c->in.st->gc_arena_peak = (int64_t)ctl[7];
	c->dev_plan = c->want_text && c->k.dev_plan;
	if (c->dev_plan) { /* the gap list of the chains just made (k_plan.hip), pass 1: sizes; the fill pass follows the host's strand flags */
		CK(mga_dbuf_reserve(&P->plcnt, (size_t)n * 5 * 4 + 64)); CK(mga_dbuf_reserve(&P->ploff, (size_t)(n + 1) * 5 * 8 + 64)); CK(mga_dbuf_reserve(&P->pltot, 64));
		CK(mga_dev_plan_count(sc, &B->dev, n, (opt->flag & MG_M_PRINT_2ND) != 0, (const mga_gc_hdr_t*)P->gchdr.p, P->gcpool.p, (const mg_llchain_t*)P->lcpool.p,
							  (const mg128_t*)P->apool.p, (int32_t*)P->plcnt.p, (int64_t*)P->ploff.p, (unsigned long long*)P->pltot.p));
		CK(mga_hbuf_reserve(&P->h_ploff, (size_t)(n + 1) * 8 + 16));
		c->h_ploff = (int64_t*)P->h_ploff.p;
		CK(mga_d2h_s(sc, c->ptot, P->pltot.p, 64)); CK(mga_d2h_s(sc, c->h_ploff, P->ploff.p, (size_t)(n + 1) * 8));
	}
	CK(mga_hbuf_reserve(&P->h_gcpool, (size_t)ctl[1] * rec + 16)); CK(mga_hbuf_reserve(&P->h_lcpool, (size_t)ctl[2] * sizeof(mg_llchain_t) + 16)); CK(mga_hbuf_reserve(&P->h_apool, (size_t)ctl[6] * 16 + 16));
	c->h_gchdr_p = (mga_gc_hdr_t*)P->h_gchdr.p;
	CK(mga_d2h_s(sc, c->h_gchdr_p, P->gchdr.p, (size_t)n * sizeof(mga_gc_hdr_t)));
	CK(mga_d2h_s(sc, P->h_gcpool.p, P->gcpool.p, (size_t)ctl[1] * rec)); CK(mga_d2h_s(sc, P->h_lcpool.p, P->lcpool.p, (size_t)ctl[2] * sizeof(mg_llchain_t)));
	c->need_a = (!c->dev_plan && !c->in.cov) || (mg_dbg_flag & 0x8) || (opt->flag & MG_M_WRITE_LCHAIN); /* with the gap list made on the device, only the per-vertex lines (-S / --write-mz) read anchors on the host */
	if (c->need_a) CK(mga_d2h_s(sc, P->h_apool.p, P->apool.p, (size_t)ctl[6] * 16));
	CK(mga_ssync(sc)); /* (h_nu / h_nb / h_rflag arrived with the first sync) */
	for (i = 0; i < n; ++i) /* the few reads whose rescue k_lchain left to the host tree: their chains, anchors and minimizer positions come down for the host path */
		if (c->h_gchdr_p[i].status != 0) { /* (MGA_GC_HOST, or a read the device gave up on even in the large arena) */
			const int64_t ao = c->h_aoff[i], mo = c->h_minioff[i];
			CK(mga_d2h_s(sc, (uint64_t*)P->h_u.p + ao, (const uint64_t*)P->u.p + ao, (size_t)c->h_nu[i] * 8));
			CK(mga_d2h_s(sc, (mg128_t*)P->h_b.p + ao, (const mg128_t*)P->b.p + ao, (size_t)c->h_nb[i] * 16));
			CK(mga_d2h_s(sc, (int32_t*)P->h_mini.p + mo, (const int32_t*)P->mini.p + mo, (size_t)(c->h_minioff[i + 1] - mo) * 4));
			CK(mga_ssync(sc));
		}
	return 0;
}

/* ---- what the host chains from comes down (host placement: everything; -x asm / ultra-long: the raw anchors); the front phase is over ---- */
static int chunk_front_readback(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc;
	if (c->is_rmq || c->chunk_long) {
		CK(mga_d2h_s(sc, P->h_mini.p, P->mini.p, (size_t)c->n_mini * 4));
		CK(mga_d2h_s(sc, P->h_b.p, P->a.p, (size_t)c->n_a * 16));
	} else if (!c->dev_gc) {
		CK(mga_d2h_s(sc, P->h_mini.p, P->mini.p, (size_t)c->n_mini * 4));
		CK(mga_d2h_s(sc, P->h_u.p, P->u.p, (size_t)c->n_a * 8)); CK(mga_d2h_s(sc, P->h_b.p, P->b.p, (size_t)c->n_a * 16));
	}
	CK(mga_ssync(sc));
	chunk_token_release(c);
	return 0;
}

/* MGA_CHECK -- debugging aid: invariants of what the device stages handed back (host placement) */
static int chunk_check(chunk_t *c)
{
	const int n = c->in.n; const int *qlens = c->in.qlens; const int64_t *h_aoff = c->h_aoff, *h_minioff = c->h_minioff; const int32_t *h_nu = c->h_nu, *h_nb = c->h_nb, *h_mini = (const int32_t*)c->P->h_mini.p;
	int64_t bad = 0;
	int i;
	if (!c->k.check || c->is_rmq || c->chunk_long || c->dev_gc || !h_nu || !h_nb) return 0;
	for (i = 0; i < n && bad < 5; ++i) {
		const int64_t na_i = h_aoff[i + 1] - h_aoff[i], nm_i = h_minioff[i + 1] - h_minioff[i];
		int64_t k_;
		int why = 0;
		if (na_i < 0 || nm_i < 0 || nm_i > qlens[i]) why = 1;
		else if (h_nb[i] < 0 || h_nb[i] > na_i || h_nu[i] < 0 || h_nu[i] > h_nb[i]) why = 2;
		else for (k_ = 0; k_ < nm_i; ++k_) { const int32_t y = h_mini[h_minioff[i] + k_]; if (y < 0 || y >= qlens[i] || (k_ > 0 && y <= h_mini[h_minioff[i] + k_ - 1])) { why = 3; break; } }
		if (why) { fprintf(stderr, "[check] chunk of %d reads: read %ld fails check %d: aoff %ld..%ld minioff %ld..%ld nu %d nb %d nmz %d qlen %d\n", n, (long)i, why, (long)h_aoff[i], (long)h_aoff[i + 1], (long)h_minioff[i], (long)h_minioff[i + 1], h_nu[i], h_nb[i], c->h_nmz[i], qlens[i]); ++bad; }
	}
	fprintf(stderr, "[check] chunk of %d reads: %ld bad (n_a %ld n_mini %ld n_mz capacity %ld)\n", n, (long)bad, (long)c->n_a, (long)c->n_mini, (long)c->n_mz);
	return 0;
}

/* ---- host: graph chaining + gap list ---- */
static int chunk_host_chain(chunk_t *c)
{
	pipe_ctx_t *P = c->P; struct mg_idx_bucket_s *B = c->in.gi->B; const unsigned long long *ptot = c->ptot;
	mga_batch_t *b = c->b = mga_batch_init(c->in.gi, c->in.opt, c->in.n, c->in.qlens, c->in.seqs, c->in.qnames, c->q_off, c->in.n_threads);
	b->want_text = c->want_text;
	c->dev_splice = c->want_text && B->dev.d_gseq != 0 && B->dev.d_gseq_rc != 0 && c->k.dev_splice;
	if (c->dev_splice) mga_batch_set_want_src(b, 1);
	if (c->dev_plan) {
		if (ptot[6] != 0 || ptot[2] > 0x7fffffffULL) { mga_set_error("gap list: too many WFA problems or target bases in one chunk (%llu problems); lower MGA_CHUNK", ptot[2]); return -1; }
		CK(mga_hbuf_reserve(&P->h_plrev, (size_t)ptot[0] * 4 + 16));
		memset(P->h_plrev.p, 0, (size_t)ptot[0] * 4); /* (reads that chain_worker skips -- max_qlen, empty -- leave their chains' flags unwritten: defined now; their lines are never printed) */
		mga_batch_set_device_plan(b, c->h_ploff, (int32_t*)P->h_plrev.p, (int64_t)ptot[0]);
	}
	if (c->dev_gc) mga_batch_set_device_chains(b, c->h_gchdr_p, P->h_gcpool.p, (const mg_llchain_t*)P->h_lcpool.p, c->need_a ? (const mg128_t*)P->h_apool.p : 0);
	if (c->long_q && c->n_a > 0 && c->k.dev_rmq) { /* -x asm (and the rescue pass of ultra-long -x lr reads): the RMQ chainer's forward passes on the device (k_rmq.hip) */
		c->rq_ctx.P = P, c->rq_ctx.opt = c->in.opt, c->rq_ctx.pen_gap = b->pen_gap, c->rq_ctx.pen_skip = b->pen_skip, c->rq_ctx.n_total = c->n_a;
		CK(mga_hbuf_reserve(&P->h_rq, (size_t)((c->n_a + 1) & ~1LL) * 20 + 64));
		mga_batch_set_rq_device(b, rq_dev_fwd_hook, &c->rq_ctx, (char*)P->h_rq.p, c->n_a);
	}
	CK(mga_batch_chain(b, c->h_nmz, c->h_rep, (const int32_t*)P->h_mini.p, c->h_minioff, c->h_nu, c->h_nb, (const uint64_t*)P->h_u.p, (const mg128_t*)P->h_b.p, c->h_aoff, c->chunk_long ? 3 : c->long_q ? 2 : c->is_rmq, c->h_rflag));
	return 0;
}

/* the text kernel's inputs that the host threads planned -- items, printed chains, walk vertices -- behind the device-made part of each array */
static int text_inputs_upload(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc;
	const int64_t hp_item = c->n_item - c->dp_item, hp_chain = c->n_chain - c->dp_chain, hp_vert = c->n_vert - c->dp_vert;
	int64_t k;
	CK(mga_hbuf_reserve(&P->h_item, (size_t)hp_item * sizeof(mga_cigitem_t) + 16)); CK(mga_hbuf_reserve(&P->h_chain, (size_t)hp_chain * sizeof(mga_txt_chain_t) + 16));
	CK(mga_hbuf_reserve(&P->h_vert, (size_t)hp_vert * 4 + 16));
	mga_batch_text_export(c->b, (mga_cigitem_t*)P->h_item.p, (mga_txt_chain_t*)P->h_chain.p, (uint32_t*)P->h_vert.p);
	for (k = 0; c->dev_plan && k < hp_chain; ++k) { /* behind the device-made part */
		mga_txt_chain_t *tc = (mga_txt_chain_t*)P->h_chain.p + k;
		tc->item_beg += c->dp_item, tc->item_end += c->dp_item, tc->vert_beg += c->dp_vert, tc->prob_base += c->dp_prob;
	}
	CK(mga_h2d_s(sc, (mga_cigitem_t*)P->item.p + c->dp_item, P->h_item.p, (size_t)hp_item * sizeof(mga_cigitem_t)));
	CK(mga_h2d_s(sc, (mga_txt_chain_t*)P->chain.p + c->dp_chain, P->h_chain.p, (size_t)hp_chain * sizeof(mga_txt_chain_t)));
	CK(mga_h2d_s(sc, (uint32_t*)P->vert.p + c->dp_vert, P->h_vert.p, (size_t)hp_vert * 4));
	return 0;
}

/* the WFA problems of the chunk into HBM: export, k_plan's pass 2, uploads -- all of it before the WFA token is taken */
static int wfa_inputs_upload(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; struct mg_idx_bucket_s *B = c->in.gi->B; const mg_mapopt_t *opt = c->in.opt; mga_batch_t *b = c->b;
	const int64_t dp_prob = c->dp_prob, dp_tb = c->dp_tb, hp_prob = c->hp_prob, hp_tb = c->hp_tb, n_prob = c->n_prob, n_tb = c->n_tb;
	mga_wfa_prob_t *h_prob;
	int i;
	CK(mga_hbuf_reserve(&P->h_prob, (size_t)hp_prob * sizeof(mga_wfa_prob_t) + 16)); CK(mga_hbuf_reserve(&P->h_tseq, c->dev_splice ? 64 : (size_t)hp_tb + 64));
	h_prob = (mga_wfa_prob_t*)P->h_prob.p;
	if (c->dev_splice) { /* descriptors instead of bytes: 24 bytes per gap; the vertices they index follow the device-made part (dp_vert) of the walk array */
		CK(mga_hbuf_reserve(&P->h_plsrc, (size_t)hp_prob * sizeof(mga_plan_src_t) + 16));
		mga_batch_wfa_export_src(b, h_prob, 0, (mga_plan_src_t*)P->h_plsrc.p, c->dp_vert);
	} else {
		mga_batch_wfa_export(b, h_prob, (char*)P->h_tseq.p);
		memset((char*)P->h_tseq.p + hp_tb, 0, 64);
	}
	for (i = 0; dp_tb > 0 && i < hp_prob; ++i) h_prob[i].t_off += dp_tb;
	CK(mga_dbuf_reserve(&P->tseq, (size_t)n_tb + 64)); CK(mga_dbuf_reserve(&P->prob, (size_t)n_prob * sizeof(mga_wfa_prob_t) + 16)); CK(mga_dbuf_reserve(&P->res, (size_t)n_prob * sizeof(mga_wfa_res_t) + 16));
	CK(mga_dbuf_reserve(&P->used, 64));
	if (b->want_text) {
		CK(mga_dbuf_reserve(&P->item, (size_t)c->n_item * sizeof(mga_cigitem_t) + 16)); CK(mga_dbuf_reserve(&P->chain, (size_t)c->n_chain * sizeof(mga_txt_chain_t) + 16));
		CK(mga_dbuf_reserve(&P->vert, (size_t)c->n_vert * 4 + 16)); CK(mga_dbuf_reserve(&P->txtres, (size_t)c->n_chain * sizeof(mga_txt_res_t) + 16));
	}
	if (c->dev_plan || c->dev_splice) CK(mga_dbuf_reserve(&P->plsrc, (size_t)n_prob * sizeof(mga_plan_src_t) + 16));
	if (c->dev_plan) { /* pass 2 of k_plan.hip: items, problems + their targets, printed chains and walks, straight from the record pools in HBM */
		CK(mga_dbuf_reserve(&P->plrev, (size_t)c->dp_chain * 4 + 16));
		CK(mga_h2d_s(sc, P->plrev.p, P->h_plrev.p, (size_t)c->dp_chain * 4));
		CK(mga_dev_plan_fill(sc, &B->dev, c->in.n, (opt->flag & MG_M_PRINT_2ND) != 0, (const mga_gc_hdr_t*)P->gchdr.p, P->gcpool.p, (const mg_llchain_t*)P->lcpool.p, (const mg128_t*)P->apool.p,
							 (const int64_t*)P->qoff.p, (const int64_t*)P->ploff.p, (const int32_t*)P->plrev.p, dp_prob, (mga_cigitem_t*)P->item.p, (mga_wfa_prob_t*)P->prob.p,
							 (mga_plan_src_t*)P->plsrc.p, (mga_txt_chain_t*)P->chain.p, (uint32_t*)P->vert.p, (char*)P->tseq.p));
	}
	/* uploads ride the copy engine while another chunk owns the WFA phase */
	CK(mga_h2d_s(sc, (mga_wfa_prob_t*)P->prob.p + dp_prob, h_prob, (size_t)hp_prob * sizeof(mga_wfa_prob_t)));
	if (c->dev_splice) { /* walk vertices first (the text kernel's inputs travel now instead of after the ladder), then the targets are spliced where the graph's sequence lies */
		CK(text_inputs_upload(c));
		CK(mga_h2d_s(sc, (mga_plan_src_t*)P->plsrc.p + dp_prob, P->h_plsrc.p, (size_t)hp_prob * sizeof(mga_plan_src_t)));
		CK(mga_dmemset_s(sc, (char*)P->tseq.p + n_tb, 0, 64));
		CK(mga_dev_plan_target_verts(sc, &B->dev, hp_prob, (const mga_wfa_prob_t*)P->prob.p + dp_prob, (const mga_plan_src_t*)P->plsrc.p + dp_prob, (const uint32_t*)P->vert.p, (char*)P->tseq.p));
	} else CK(mga_h2d_s(sc, (char*)P->tseq.p + dp_tb, P->h_tseq.p, (size_t)hp_tb + 64));
	return 0;
}

/* ---- WFA over all gaps: sets c->gaps, the condition of this stage and of the three after it ---- */
static int chunk_wfa(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; const mg_mapopt_t *opt = c->in.opt; mga_batch_t *b = c->b; const unsigned long long *ptot = c->ptot;
	int64_t n_prob, pool_cap;
	mga_wfa_job_t job;
	int i;
	c->dp_chain = (int64_t)ptot[0], c->dp_item = (int64_t)ptot[1], c->dp_prob = (int64_t)ptot[2], c->dp_vert = (int64_t)ptot[3], c->dp_tb = (int64_t)ptot[4];
	c->hp_prob = mga_batch_n_wfa(b), c->hp_tb = mga_batch_wfa_target_bytes(b);
	n_prob = c->n_prob = c->dp_prob + c->hp_prob, c->n_tb = c->dp_tb + c->hp_tb;
	c->gaps = (opt->flag & MG_M_CIGAR) && (n_prob > 0 || (b->want_text && c->dp_chain + mga_batch_n_chains(b) > 0)); /* (text mode: chains made of ready operators only still need their text) */
	if (!c->gaps) return 0;
	c->n_item = c->dp_item + (b->want_text ? mga_batch_n_items(b) : 0), c->n_chain = c->dp_chain + (b->want_text ? mga_batch_n_chains(b) : 0), c->n_vert = c->dp_vert + (b->want_text ? mga_batch_n_verts(b) : 0);
	if (n_prob > 0x7fffffff) { mga_set_error("too many WFA problems in one chunk (%ld); lower MGA_CHUNK", (long)n_prob); return -1; }
	CK(wfa_inputs_upload(c));
	chunk_token_acquire(c, P->tok_wfa ? P->tok_wfa : &g_gpu_wfa);
	/* CIGAR pool: a global alignment has at most tl + ql operators, so target bases + query bases bound the chunk; + the abandoned block
	 * tails (<= 512 ops) of every resident wave.  Sized to the bound, the pool cannot overflow whatever the divergence. */
	pool_cap = c->n_tb + 4096 + 40000LL * 512 + MGA_WFA_FUSE_SLACK + (int64_t)ptot[5] + 4 * n_prob; /* (+ 4 per problem: k_wfa_tb reserves by an upper bound of the operator count) */
	for (i = 0; i < b->n_threads; ++i) pool_cap += b->tp[i].wfa_q_bases;
	CK(mga_dbuf_reserve(&P->pool, (size_t)pool_cap * 4)); CK(mga_dmemset_s(sc, P->used.p, 0, 8));
	/* the tier ladder runs on the device (k_wfa_sched.hip); the host never walks the problems */
	job = (mga_wfa_job_t){ (const mga_wfa_prob_t*)P->prob.p, (const char*)P->tseq.p, c->d_seq, (mga_wfa_res_t*)P->res.p, (uint32_t*)P->pool.p, pool_cap, (unsigned long long*)P->used.p };
	CK(mga_dev_wfa_solve(sc, &job, (int)n_prob, &c->cells));
	/* CIGARs back in problem order: one sequential stream for the host's stitching threads, or the input of the text kernel */
	CK(mga_dbuf_reserve(&P->ncig, (size_t)n_prob * 4 + 16)); CK(mga_dbuf_reserve(&P->cigoff, (size_t)(n_prob + 1) * 8)); CK(mga_dbuf_reserve(&P->ord, (size_t)pool_cap * 4));
	CK(mga_dev_wfa_gather(sc, &job, (int)n_prob, (int32_t*)P->ncig.p, (int64_t*)P->cigoff.p, (uint32_t*)P->ord.p, pool_cap, &c->n_ops));
	chunk_token_release(c); /* the gather kernel and what follows trail on this chunk's stream while the next chunk's kernels start */
	return 0;
}

/* ---- stitching, statistics, cg:Z and ds:Z on the device (k_text.hip): one lane per printed chain ---- */
static int chunk_text(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; const int n = c->in.n;
	const int tight = c->k.txt_tight;
	int64_t txt_cap = 4096, k;
	for (k = 0; k < n; ++k) txt_cap += (tight ? 1 : 3) * (int64_t)c->in.qlens[k] / (tight ? 4 : 1) + 1024;
	if (!c->dev_splice) CK(text_inputs_upload(c)); /* (with the targets spliced on the device these went up before the ladder) */
	for (k = 0;; ++k) { /* the pool is sized for ordinary reads (~1 byte of cg + ds per base); the kernel counts what it WOULD have written, so a chunk of
	                     * very divergent reads or many printed secondaries gets a pool of exactly that size and a second launch */
		CK(mga_dbuf_reserve(&P->txtpool, (size_t)txt_cap)); CK(mga_dmemset_s(sc, P->used.p, 0, 8));
		CK(mga_dev_text(sc, (int)c->n_chain, (const mga_txt_chain_t*)P->chain.p, (const mga_cigitem_t*)P->item.p, c->n_vert, (const uint32_t*)P->vert.p, &c->in.gi->B->dev, c->d_seq,
						c->n_item + c->n_ops, (const int32_t*)P->ncig.p, (const int64_t*)P->cigoff.p, (const uint32_t*)P->ord.p, (mga_txt_res_t*)P->txtres.p,
						(char*)P->txtpool.p, txt_cap, (unsigned long long*)P->used.p));
		CK(mga_d2h_s(sc, &c->txt_used, P->used.p, 8)); CK(mga_ssync(sc));
		if ((int64_t)c->txt_used <= txt_cap) break;
		if (k >= 2) { mga_set_error("text kernel: output of %lld bytes exceeds the pool of %lld", (long long)c->txt_used, (long long)txt_cap); return -1; }
		txt_cap = (int64_t)c->txt_used + ((int64_t)c->txt_used >> 4) + 4096;
	}
	CK(mga_hbuf_reserve(&P->h_txtres, (size_t)c->n_chain * sizeof(mga_txt_res_t) + 16));
	CK(mga_d2h_s(sc, P->h_txtres.p, P->txtres.p, (size_t)c->n_chain * sizeof(mga_txt_res_t)));
	return 0;
}

/* Round 6: the whole LINES are written on the device (k_gaf.hip) -- name, coordinates, path column, tags in front of the two strings, every line at its place in
 * the chunk's text -- unless the job asks for what only the host's writer prints (per-vertex lines of -S / --write-mz) or the chains are chromosome-scale
 * (their walks have 10^5 vertices: one wavefront per line would fold them alone); then the strings come down for the host's writer.  Either way the text results land here. */
static int chunk_gaf_dev(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; struct mg_idx_bucket_s *B = c->in.gi->B; const mg_mapopt_t *opt = c->in.opt; mga_batch_t *b = c->b; const int n = c->in.n; const char **qnames = c->in.qnames;
	const int64_t n_chain = c->n_chain;
	int64_t n_lines = -1, k;
	int i;
	if (c->in.gaf_part && B->dev.d_gaf_seg != 0 && !(opt->flag & (MG_M_WRITE_LCHAIN | MG_M_WRITE_MZ | MG_M_FRAG_MERGE)) && !(mg_dbg_flag & 0x8) && n_chain > 0 &&
		(c->n_item + c->n_ops) / n_chain < 32768 && n_chain < 0x7fffffffLL && c->k.dev_gaf) {
		CK(mga_hbuf_reserve(&P->h_gline, (size_t)(n_chain + n) * sizeof(mga_gaf_line_t) + 64));
		n_lines = gaf_lines_build(b, n, (mga_gaf_line_t*)P->h_gline.p);
	}
	if (n_lines > 0) { /* line records and names up, then count -> scan -> write */
		int64_t qn_bytes = 0, tot_b = 0, *qo;
		char *qn;
		for (i = 0; i < n; ++i) qn_bytes += qnames ? (int64_t)strlen(qnames[i]) : 1;
		CK(mga_hbuf_reserve(&P->h_gqn, (size_t)(n + 1) * 8 + (size_t)qn_bytes + 64));
		qo = (int64_t*)P->h_gqn.p, qn = (char*)(qo + n + 1);
		for (i = 0, qn_bytes = 0; i < n; ++i) { const char *nm = qnames ? qnames[i] : "*"; const size_t l = strlen(nm); qo[i] = qn_bytes; memcpy(qn + qn_bytes, nm, l); qn_bytes += (int64_t)l; }
		qo[n] = qn_bytes;
		CK(mga_dbuf_reserve(&P->g_line, (size_t)n_lines * sizeof(mga_gaf_line_t) + 64)); CK(mga_dbuf_reserve(&P->g_qoff, (size_t)(n + 1) * 8)); CK(mga_dbuf_reserve(&P->g_qn, (size_t)qn_bytes + 64));
		CK(mga_dbuf_reserve(&P->g_len, (size_t)(n_lines + 1) * 4)); CK(mga_dbuf_reserve(&P->g_off, (size_t)(n_lines + 2) * 8));
		CK(mga_h2d_s(sc, P->g_line.p, P->h_gline.p, (size_t)n_lines * sizeof(mga_gaf_line_t))); CK(mga_h2d_s(sc, P->g_qoff.p, qo, (size_t)(n + 1) * 8)); CK(mga_h2d_s(sc, P->g_qn.p, qn, (size_t)qn_bytes + 1));
		CK(mga_dev_gaf(sc, &B->dev, (int)n_lines, (const mga_gaf_line_t*)P->g_line.p, (const char*)P->g_qn.p, (const int64_t*)P->g_qoff.p, opt->flag, (const mga_txt_chain_t*)P->chain.p,
					   (const uint32_t*)P->vert.p, (const mga_txt_res_t*)P->txtres.p, (const char*)P->txtpool.p, (int32_t*)P->g_len.p, 0, 0));
		CK(mga_dev_scan_i32_to_i64(sc, (const int32_t*)P->g_len.p, n_lines, (int64_t*)P->g_off.p));
		CK(mga_d2h_s(sc, &tot_b, (int64_t*)P->g_off.p + n_lines, 8)); CK(mga_ssync(sc));
		CK(mga_dbuf_reserve(&P->g_out, (size_t)tot_b + 64)); CK(mga_hbuf_reserve(&P->h_gout, (size_t)tot_b + 64));
		CK(mga_dev_gaf(sc, &B->dev, (int)n_lines, (const mga_gaf_line_t*)P->g_line.p, (const char*)P->g_qn.p, (const int64_t*)P->g_qoff.p, opt->flag, (const mga_txt_chain_t*)P->chain.p,
					   (const uint32_t*)P->vert.p, (const mga_txt_res_t*)P->txtres.p, (const char*)P->txtpool.p, (int32_t*)P->g_len.p, (const int64_t*)P->g_off.p, (char*)P->g_out.p));
		if (tot_b > 0) CK(mga_d2h_s(sc, P->h_gout.p, P->g_out.p, (size_t)tot_b));
		b->gaf_dev = (const char*)P->h_gout.p, b->gaf_dev_len = tot_b;
	} else if (n_lines == 0) b->gaf_dev = "", b->gaf_dev_len = 0; /* (nothing of this chunk is printed) */
	else { CK(mga_hbuf_reserve(&P->h_txtpool, (size_t)c->txt_used + 16)); CK(mga_d2h_s(sc, P->h_txtpool.p, P->txtpool.p, (size_t)c->txt_used)); }
	CK(mga_ssync(sc));
	for (k = 0; k < n_chain; ++k)
		if (((const mga_txt_res_t*)P->h_txtres.p)[k].status != 0) { mga_set_error("text kernel: stitched CIGAR inconsistent with the chain coordinates (galign.c:140), chain %ld", (long)k); return -1; }
	b->txt_res = (const mga_txt_res_t*)P->h_txtres.p, b->txt_pool = b->gaf_dev ? 0 : (const char*)P->h_txtpool.p;
	return 0;
}

/* without the text kernel the CIGARs come down for the host's stitching threads */
static int chunk_cigars_to_host(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; const int64_t n_prob = c->n_prob, n_ops = c->n_ops;
	CK(mga_hbuf_reserve(&P->h_ncig, (size_t)n_prob * 4 + 16)); CK(mga_hbuf_reserve(&P->h_cigoff, (size_t)(n_prob + 1) * 8)); CK(mga_hbuf_reserve(&P->h_pool, (size_t)n_ops * 4 + 16));
	CK(mga_d2h_s(sc, P->h_ncig.p, P->ncig.p, (size_t)n_prob * 4)); CK(mga_d2h_s(sc, P->h_cigoff.p, P->cigoff.p, (size_t)(n_prob + 1) * 8));
	CK(mga_d2h_s(sc, P->h_pool.p, P->ord.p, (size_t)n_ops * 4)); CK(mga_ssync(sc));
	return 0;
}

/* ---- host: CIGAR stitching + ds ---- */
static int chunk_finish(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_batch_t *b = c->b;
	if (b->txt_res) return 0; /* nothing to stitch on the host: the GAF writer copies the device's text */
	if ((c->in.opt->flag & MG_M_CIGAR) && c->n_prob > 0) return mga_batch_finish_ordered(b, (const int32_t*)P->h_ncig.p, (const int64_t*)P->h_cigoff.p, (const uint32_t*)P->h_pool.p);
	return mga_batch_finish(b, 0, 0);
}

/* the chunk's device-made lines (b->gaf_dev): straight to their place in the job's output if this chunk is the one the output waits for, else into the chunk's pieces */
static int gaf_dev_emit(chunk_t *c)
{
	mga_batch_t *b = c->b; const gaf_sink_t *sink = c->in.sink; const int n_threads = c->in.n_threads;
	pcopy_t pc;
	int i, t_;
	pc.src = b->gaf_dev, pc.bytes = b->gaf_dev_len, pc.T = n_threads, pc.dst = 0;
	if (sink && c->k.gaf_direct && sink->try_reserve(sink->ctx, pc.bytes, &pc.dst)) {
		mga_parallel_for(n_threads, n_threads, pcopy_worker, &pc);
		sink->commit(sink->ctx, pc.bytes);
		c->in.st->gaf_bytes += pc.bytes;
	} else /* piece t takes the bytes [bytes t / T, bytes (t + 1) / T): the pieces are concatenated in order, wherever a line is cut */
		for (t_ = 0; t_ < n_threads; ++t_) {
			const int64_t pb = pc.bytes * t_ / n_threads, pe = pc.bytes * (t_ + 1) / n_threads;
			kstring_t *out = &c->in.gaf_part[t_];
			if (pe - pb > 0xfffffff0LL) { mga_set_error("more than 4 GB of GAF text in one output piece: use a smaller -K or more threads"); return -1; }
			if ((size_t)(pe - pb) + 1 > out->m) { size_t cap; char *p = strbuf_get((size_t)(pe - pb) + 1, &cap); if (cap > 0xfffffff0u) cap = 0xfffffff0u; free(out->s); out->s = p, out->m = (unsigned)cap; }
			memcpy(out->s, pc.src + pb, (size_t)(pe - pb));
			out->l = (unsigned)(pe - pb), out->s[out->l] = 0;
		}
	for (i = 0; i < c->in.n; ++i) { mg_gchain_free(b->gcs[i]); b->gcs[i] = 0; c->in.gcs_out[i] = 0; }
	return 0;
}

/* ---- the results leave: GAF text of this chunk, formatted while other chunks own the GPU (the chains are freed on the way), or in chain mode the chains themselves ---- */
static int chunk_emit(chunk_t *c)
{
	mga_batch_t *b = c->b; const gaf_sink_t *sink = c->in.sink; const int n = c->in.n, n_threads = c->in.n_threads;
	gafw_t w;
	int i, direct = 0;
	if (c->in.gaf_part == 0) {
		mg_gchains_t **r = mga_batch_take_results(b);
		for (i = 0; i < n; ++i) c->in.gcs_out[i] = r[i];
		free(r);
		return 0;
	}
	w.b = b, w.n = n, w.T = n_threads, w.part = c->in.gaf_part, w.mode = 0, w.bytes = w.off = 0, w.dst = 0;
	if (b->gaf_dev) { CK(gaf_dev_emit(c)); direct = 1; }
	else if (sink && b->txt_res && c->k.gaf_direct) { /* straight to the lines' place in the job's output, if this chunk is what the output waits for */
		int64_t *bo = MGA_CALLOC(int64_t, 2 * (size_t)n_threads + 2), tot_b = 0;
		int t_, fits = 1; /* kstring_t::l counts in 32 bits: a piece beyond that (chromosome-scale text on few threads) takes the piece path, which fails loudly at 4 GB (gaf.c: ks_room) */
		w.bytes = bo, w.off = bo + n_threads + 1, w.mode = 1;
		mga_parallel_for(n_threads, n_threads, gaf_worker, &w);
		for (t_ = 0; t_ < n_threads; ++t_) { w.off[t_] = tot_b, tot_b += w.bytes[t_]; if (w.bytes[t_] > 0xfffffff0LL) fits = 0; }
		if (fits && sink->try_reserve(sink->ctx, tot_b, &w.dst)) {
			w.mode = 2;
			mga_parallel_for(n_threads, n_threads, gaf_worker, &w);
			sink->commit(sink->ctx, tot_b);
			c->in.st->gaf_bytes += tot_b;
			direct = 1;
		}
		free(bo);
		w.mode = 0, w.bytes = w.off = 0;
	}
	if (!direct) mga_parallel_for(n_threads, n_threads, gaf_worker, &w);
	for (i = 0; i < n; ++i) c->in.gcs_out[i] = 0;
	return 0;
}

/* ---- --cov: the chunk's chains end in the job's integer accumulators instead of GAF lines (cal_cov.c:8-53; cov_core.h, k_cov.hip) ----
 * Every chain of every read is a 32-byte record (the fields of mg_gchain_t the count reads, MAPQ from the host's logf included) plus its walk, 4 bytes per vertex: both go
 * up, k_cov filters and counts.  Whichever side chained the read, its walk reaches the device the same way, so the reads the device handed to the host threads
 * (mga_gc_hdr_t::status != 0) need no path of their own.  The chains of -x asm and of chunks of ultra-long reads (walks of 10^5 vertices, a handful per chunk) are
 * counted by this thread through the host instantiation, into the job's host-side accumulators.  Nothing comes down here: the accumulators do, once, when the job ends. */
typedef struct { const mga_batch_t *b; const int64_t *c_off, *v_off; mga_cov_chain_t *chain; uint32_t *vert; } cov_export_t;
static void cov_export_worker(void *data, int64_t i, int tid)
{
	cov_export_t *e = (cov_export_t*)data;
	const mg_gchains_t *gcs = e->b->gcs[i];
	int64_t ci = e->c_off[i], vi = e->v_off[i];
	int32_t k, j;
	(void)tid;
	for (k = 0; gcs && k < gcs->n_gc; ++k) {
		const mg_gchain_t *gc = &gcs->gc[k];
		mga_cov_chain_t *r;
		if (gc->cnt <= 0) continue;
		r = &e->chain[ci++];
		r->vert_beg = vi, r->vert_cnt = gc->cnt, r->ps = gc->ps, r->pe = gc->pe, r->plen = gc->plen, r->mapq = (int32_t)gc->mapq, r->blen = gc->blen;
		for (j = 0; j < gc->cnt; ++j) e->vert[vi++] = gcs->lc[gc->off + j].v;
	}
}

static int chunk_cov(chunk_t *c)
{
	pipe_ctx_t *P = c->P; mga_sctx_t *sc = P->sc; mga_batch_t *b = c->b; mga_cov_job_t *J = c->in.cov; const int n = c->in.n;
	int64_t *off, n_chain = 0, n_vert = 0;
	cov_export_t e;
	int i, k, rc = -1;
	if (c->is_rmq || c->chunk_long) {
		for (i = 0; i < n; ++i) mga_cov_read_host(&J->G, b->gcs[i], J->min_mapq, J->min_blen, J->h_seg_bases, J->h_link_cnt, J->h_cnt);
		return 0;
	}
	off = MGA_MALLOC(int64_t, 2 * ((size_t)n + 1));
	for (i = 0; i < n; ++i) {
		const mg_gchains_t *gcs = b->gcs[i];
		off[i] = n_chain, off[n + 1 + i] = n_vert;
		for (k = 0; gcs && k < gcs->n_gc; ++k) if (gcs->gc[k].cnt > 0) ++n_chain, n_vert += gcs->gc[k].cnt;
	}
	off[n] = n_chain, off[2 * n + 1] = n_vert;
	if (n_chain > 0x7fffffffLL) { mga_set_error("too many graph chains in one chunk (%ld); lower MGA_CHUNK", (long)n_chain); goto done; }
	if (n_chain == 0) { rc = 0; goto done; }
	if (mga_hbuf_reserve(&P->h_cvchain, (size_t)n_chain * sizeof(mga_cov_chain_t) + 64) < 0 || mga_hbuf_reserve(&P->h_cvvert, (size_t)n_vert * 4 + 64) < 0 ||
		mga_dbuf_reserve(&P->cv_chain, (size_t)n_chain * sizeof(mga_cov_chain_t) + 64) < 0 || mga_dbuf_reserve(&P->cv_vert, (size_t)n_vert * 4 + 64) < 0) goto done;
	e.b = b, e.c_off = off, e.v_off = off + n + 1, e.chain = (mga_cov_chain_t*)P->h_cvchain.p, e.vert = (uint32_t*)P->h_cvvert.p;
	mga_parallel_for(c->in.n_threads, n, cov_export_worker, &e);
	if (mga_h2d_s(sc, P->cv_chain.p, P->h_cvchain.p, (size_t)n_chain * sizeof(mga_cov_chain_t)) < 0 || mga_h2d_s(sc, P->cv_vert.p, P->h_cvvert.p, (size_t)n_vert * 4) < 0 ||
		mga_dev_cov(sc, &c->in.gi->B->dev, (int)n_chain, (const mga_cov_chain_t*)P->cv_chain.p, (const uint32_t*)P->cv_vert.p, n_vert, J->min_mapq, J->min_blen,
					J->d_seg_bases, J->d_link_cnt, J->d_cnt) < 0 || mga_ssync(sc) < 0) goto done;
	rc = 0;
done:
	free(off);
	return rc;
}

static int chunk_stats(chunk_t *c)
{
	mga_stats_t *st = c->in.st; const int n = c->in.n;
	int64_t n_mz = 0; /* (c->n_mz is the capacity of the minimizer slots) */
	int i;
	for (i = 0; i < n; ++i) n_mz += c->h_nmz[i];
	st->n_reads += n, st->n_bases += c->tot, st->n_mz += n_mz, st->n_probe += n_mz, st->n_hit += c->n_a;
	for (i = 0; i < n && c->h_nb; ++i) st->n_anchor_chained += c->h_nb[i];
	for (i = 0; i < n && c->h_rflag; ++i) st->n_rescue_dev += c->h_rflag[i] == 1, st->n_rescue_host += c->h_rflag[i] == 2;
	mga_batch_stats(c->b, st);
	return 0;
}

static void chunk_release(chunk_t *c, int rc)
{
	if (rc < 0) mga_sctx_abort(c->P->sc); /* nothing of this chunk may still be in flight, and no staged read-back may outlive map_chunk()'s frame */
	chunk_token_release(c);
	if (c->b) mga_batch_destroy(c->b);
	free(c->q_off); free(c->h_mzoff); free(c->h_aoff); free(c->h_minioff); free(c->h_nmz); free(c->h_rep); free(c->h_nu); free(c->h_nb); free(c->h_rflag);
}

int map_chunk(pipe_ctx_t *P, const chunk_args_t *a)
{
	chunk_t c;
	mg_mapopt_t opt_cov;
	int rc = -1, i;
	memset(&c, 0, sizeof c);
	c.P = P, c.in = *a;
	if (a->cov) { /* a coverage reads the chain records alone (cal_cov.c:17: gc->blen, not the CIGAR's): no gap is listed or aligned, with or without -c */
		opt_cov = *a->opt, opt_cov.flag &= ~(uint64_t)MG_M_CIGAR, c.in.opt = &opt_cov;
		c.in.gaf_part = 0, c.in.sink = 0;
	}
	const mg_idx_t *gi = c.in.gi; const mg_mapopt_t *opt = c.in.opt; const int n = c.in.n, lr_long = c.in.lr_long; const int *qlens = c.in.qlens;
	mga_stats_t *st = c.in.st; const kstring_t *gaf_part = c.in.gaf_part; const mga_cov_job_t *cov = c.in.cov;
	chunk_knobs_read(&c.k);
	c.q_off = MGA_MALLOC(int64_t, n + 2), c.need_a = 1;
	c.want_text = gaf_part != 0 && (opt->flag & MG_M_CIGAR) && gi->B->dev.d_gseq != 0 && !c.k.host_text;
	c.is_rmq = !!(opt->flag & MG_M_RMQ);
	if (!c.is_rmq && n > 0 && (gi->k & 1) && !c.k.no_longq) { c.chunk_long = lr_long > 0; for (i = 0; i < n && c.chunk_long; ++i) if (qlens[i] < lr_long) c.chunk_long = 0; }
	c.long_q = (c.is_rmq || c.chunk_long) && (gi->k & 1) && !c.k.no_longq;
	if (opt->flag & (MG_M_SR | MG_M_HEAP_SORT | MG_M_SPLICE | MG_M_NO_DIAG)) { mga_set_error("mg_map_batch: short-read / splice / -D modes are outside the accelerated long-read path"); goto done; }
	c.t0 = mga_wtime();
	if (chunk_upload_reads(&c) < 0 || chunk_sketch(&c) < 0 || chunk_seed_count(&c) < 0) goto done;
	chunk_lap(&c, " sketch", &st->t_sketch);
	if (chunk_seed_fill(&c) < 0 || chunk_lchain(&c) < 0 || chunk_gchain_dev(&c) < 0 || chunk_front_readback(&c) < 0) goto done; /* (chunk_gchain_dev: the chunks that chunk_lchain placed on the device) */
	chunk_lap(&c, " lchain", &st->t_lchain);
	if (chunk_check(&c) < 0 || chunk_host_chain(&c) < 0) goto done;
	chunk_lap(&c, " hostchain", &st->t_host_chain);
	if (chunk_wfa(&c) < 0) goto done;
	if (c.gaps) { /* what chunk_wfa left in HBM becomes text on the device, or comes down for the host's stitching */
		if (c.want_text ? chunk_text(&c) < 0 || chunk_gaf_dev(&c) < 0 : chunk_cigars_to_host(&c) < 0) goto done;
		st->wfa_cells += c.cells;
		st->n_wfa += c.dp_prob, st->n_wfa_dev_plan += c.dp_prob, st->wfa_t_bases += c.dp_tb, st->wfa_q_bases += (int64_t)c.ptot[5];
	}
	chunk_lap(&c, " wfa", &st->t_wfa);
	if (chunk_finish(&c) < 0) goto done;
	chunk_lap(&c, " hostpost", &st->t_host_post);
	if (cov ? chunk_cov(&c) < 0 : chunk_emit(&c) < 0) goto done;
	if (gaf_part || cov) chunk_lap(&c, cov ? " cov" : " gaf", &st->t_gaf);
	rc = chunk_stats(&c);
done:
	chunk_release(&c, rc);
	return rc;
}

void pipe_ctx_free(pipe_ctx_t *P)
{
	size_t i;
	if (P->sc) mga_sctx_abort(P->sc);
	for (i = 0; i < sizeof P->dall / sizeof P->dall[0]; ++i) mga_dbuf_free(&P->dall[i]);
	for (i = 0; i < sizeof P->hall / sizeof P->hall[0]; ++i) mga_hbuf_free(&P->hall[i]);
	mga_sctx_destroy(P->sc);
	memset(P, 0, sizeof *P);
}
