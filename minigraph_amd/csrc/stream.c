/* stream.c -- mga_stream_t and the batch entry points on top of it (mg_map_batch and kin); mapper.c has the map of the pipeline. */
#include <stdio.h>
#include "mapper.h"
#include "chunk.h"

/* MGA_DEBUG_PIPE accounting (mga_dev.h: C_*, mga_host.h: cpu_now / CPU_ADD): switched on where a stream is opened, zeroed by a job's first batch, printed per collected batch */
static const char *g_cname[C_N] = { "lchain_copy", "lchain_rescue", "lchain_gen", "gchain_dp", "gchain_gen", "gchain_post", "plan_cigar", "apply_cigar", "gen_ds", "gaf", "export", "pipe_thread(all)", "of_which_ssync", "commit", "reader_thread", "fasta_scan_fill", "writer+collector" };
volatile int64_t g_cpu_ns[C_N];
int g_cpu_on = 0;
void mga_cpu_note(int which, int64_t ns) { if (g_cpu_on) __sync_fetch_and_add(&g_cpu_ns[which], ns); }
int64_t mga_cpu_now(void) { return cpu_now(); }

/* ------------------------------------------------------------------------------------------------
 * stream: the chunk pipeline as a persistent object
 *
 * A stream owns MGA_PIPE pipeline threads (each with its own HIP stream context and device / pinned buffers) that live as long
 * as the stream.  Batches are SUBMITTED (cut into chunks, queued) and COLLECTED in submission order; chunks of consecutive
 * batches follow each other through the workers without a drain in between -- the reference overlaps its mini-batches the same
 * way (kt_pipeline, gmap.c:163-184).  mg_map_files() keeps one stream for the whole job, the single-batch entry points
 * (mg_map_batch, mga_map_reads) use the index's own stream, one call at a time.
 * ---------------------------------------------------------------------------------------------- */
#define MGA_MAX_PIPE 8

typedef struct sbatch_s {
	struct sbatch_s *next;
	int n, flags;
	const int *qlens;
	const char **seqs, **qnames;
	mg_gchains_t **gcs;            /* chain mode: results; text mode: scratch array of NULLs */
	int own_gcs;
	const char *d_seq; const int64_t *q_off;
	int seqs_pinned;               /* seqs[] lie back to back in pinned host memory (+64 readable bytes): chunks upload straight from there */
	int want_gaf, n_threads;
	int n_chunks, *cstart, next_chunk, n_done;
	kstring_t *gaf_part; char *done; int next_commit;
	pthread_mutex_t cmtx;
	char *out; int64_t out_len, out_cap;
	int err, complete, inline_ok;
	char errmsg[512];
	void *user;
} sbatch_t;

struct mga_stream_s {
	const mg_idx_t *gi;
	mg_mapopt_t opt;
	int n_threads, n_pipe, chunk, max_inflight;
	int lr_long;                   /* ultra-long -x lr reads: at least this many bases (0: none); fixed when the options are set */
	int job_chunks;                /* chunks the current job has been cut into so far (the ramp-up of the chunk size belongs to the job) */
	gpu_token_t tok_front, tok_wfa; /* chunks of THIS stream in their front (sketch / seeds / chaining) and WFA phase: per stream since round 5 -- a stream opened for a rank's two
	                                 * threads after one for sixteen used to inherit the first one's counts */
	pthread_mutex_t m;
	pthread_cond_t c_work, c_done, c_space;
	sbatch_t *head, *tail, *cur;   /* submitted and not yet collected (FIFO); cur = first batch that still has chunks to hand out */
	int n_inflight, closing, started, n_submitted;
	pipe_ctx_t P[MGA_MAX_PIPE];
	pthread_t thr[MGA_MAX_PIPE];
	pthread_mutex_t api;           /* single-batch entry points on the index's stream: one call at a time */
	mga_cov_job_t *cov;            /* the job in flight is a coverage job (set and cleared by its owner while nothing is in flight) */
};

typedef struct { kstring_t *part; int64_t *off; char *dst; } gcopy_t;
static void gaf_copy_worker(void *data, int64_t i, int tid) { gcopy_t *g = (gcopy_t*)data; (void)tid; if (g->part[i].l) memcpy(g->dst + g->off[i], g->part[i].s, g->part[i].l); strbuf_put(g->part[i].s, g->part[i].m); g->part[i].s = 0, g->part[i].m = g->part[i].l = 0; }

/* room for `more` bytes (+ 1) at the end of the batch's output; the caller holds cmtx.  -1: out of memory, the buffer is what it was */
static int out_reserve(sbatch_t *b, int64_t more)
{
	if (b->out_len + more + 1 > b->out_cap) {
		const int64_t cap = (b->out_len + more + 1) * 3 / 2 + (1 << 20);
		char *p = (char*)realloc(b->out, (size_t)cap);
		if (p == 0) return -1;
		b->out = p, b->out_cap = cap;
	}
	return 0;
}

/* chunk c of batch b is formatted: append every chunk that is now complete AND next in read order to the batch's output buffer */
static void commit_chunks(sbatch_t *b, int c)
{
	pthread_mutex_lock(&b->cmtx);
	b->done[c] = 1;
	while (b->next_commit < b->n_chunks && b->done[b->next_commit]) {
		const int T = b->n_threads;
		gcopy_t g;
		int64_t off[T + 1], tot = 0;
		int k;
		g.part = b->gaf_part + (size_t)b->next_commit * T, g.off = off;
		for (k = 0; k < T; ++k) off[k] = tot, tot += g.part[k].l;
		if (out_reserve(b, tot) < 0) { /* the job fails loudly (the batch's error is what its caller gets back); the chunks behind this one are marked done and never copied */
			if (!b->err) { b->err = 1; snprintf(b->errmsg, sizeof b->errmsg, "out of memory: %lld bytes of GAF output", (long long)(b->out_len + tot)); }
			break;
		}
		g.dst = b->out + b->out_len;
		mga_parallel_for(T < 16 ? T : 16, T, gaf_copy_worker, &g);
		b->out_len += tot;
		++b->next_commit;
	}
	pthread_mutex_unlock(&b->cmtx);
}

pthread_mutex_t g_stats_mtx = PTHREAD_MUTEX_INITIALIZER; /* the index's counters are shared by every stream and mg_tbuf_t */
void stats_merge(mga_stats_t *d, const mga_stats_t *s)
{
	d->n_reads += s->n_reads, d->n_bases += s->n_bases, d->n_mz += s->n_mz, d->n_probe += s->n_probe, d->n_hit += s->n_hit;
	d->n_anchor_chained += s->n_anchor_chained, d->n_wfa += s->n_wfa, d->wfa_t_bases += s->wfa_t_bases, d->wfa_q_bases += s->wfa_q_bases;
	d->wfa_cells += s->wfa_cells;
	d->t_sketch += s->t_sketch, d->t_seed += s->t_seed, d->t_lchain += s->t_lchain, d->t_host_chain += s->t_host_chain, d->t_wfa += s->t_wfa, d->t_host_post += s->t_host_post;
	d->t_gaf += s->t_gaf;
	d->n_rescue_dev += s->n_rescue_dev, d->n_rescue_host += s->n_rescue_host;
	d->n_gwfa += s->n_gwfa, d->n_shortk += s->n_shortk, d->n_gc_retry += s->n_gc_retry, d->n_gc_host += s->n_gc_host;
	if (s->gc_arena_peak > d->gc_arena_peak) d->gc_arena_peak = s->gc_arena_peak;
	d->n_wfa_dev_plan += s->n_wfa_dev_plan;
	d->gaf_bytes += s->gaf_bytes;
}

/* the sink of a chunk's GAF lines (gaf_sink_t): room at the end of the batch's output, if every earlier chunk has been committed */
typedef struct { sbatch_t *b; int c; } gaf_sink_ctx_t;
static int sink_try_reserve(void *ctx_, int64_t bytes, char **dst)
{
	gaf_sink_ctx_t *x = (gaf_sink_ctx_t*)ctx_;
	sbatch_t *b = x->b;
	int ok = 0;
	pthread_mutex_lock(&b->cmtx);
	if (b->next_commit == x->c && !b->err) { /* nobody else can append until this chunk is marked done: the room stays where it is while the pieces are written */
		if (out_reserve(b, bytes) == 0) { *dst = b->out + b->out_len; ok = 1; } /* (no room: the chunk goes the piece-wise way, whose commit reports the failure) */
	}
	pthread_mutex_unlock(&b->cmtx);
	return ok;
}
static void sink_commit(void *ctx_, int64_t bytes)
{
	gaf_sink_ctx_t *x = (gaf_sink_ctx_t*)ctx_;
	pthread_mutex_lock(&x->b->cmtx);
	x->b->out_len += bytes; /* (commit_chunks() then marks the chunk done with empty pieces and lets the chunks behind it follow) */
	pthread_mutex_unlock(&x->b->cmtx);
}

/* one chunk of one batch on pipeline context P; the caller holds no lock */
static void stream_run_chunk(mga_stream_t *S, pipe_ctx_t *P, sbatch_t *b, int c)
{
	const int st = b->cstart[c], en = b->cstart[c + 1];
	mga_stats_t cst;
	double tc = mga_wtime();
	int64_t tcpu = cpu_now();
	int rc;
	gaf_sink_ctx_t sink_ctx = { b, c };
	gaf_sink_t sink = { sink_try_reserve, sink_commit, &sink_ctx };
	memset(&cst, 0, sizeof cst);
	rc = b->err ? 0 : map_chunk(P, &(chunk_args_t){ .gi = S->gi, .n = en - st, .qlens = b->qlens + st, .seqs = b->seqs + st, .qnames = b->qnames ? b->qnames + st : 0, .gcs_out = b->gcs + st,
								.opt = &S->opt, .n_threads = b->n_threads, .d_seq_res = b->d_seq, .q_off_res = b->q_off ? b->q_off + st : 0, .seqs_pinned = b->seqs_pinned, .st = &cst,
								.gaf_part = b->gaf_part ? b->gaf_part + (size_t)c * b->n_threads : 0, .lr_long = S->lr_long, .sink = b->gaf_part ? &sink : 0, .cov = S->cov });
	PIPE_LOG("map_chunk", c, tc);
	if (rc == 0 && b->gaf_part && !b->err) { /* the chunk's GAF text was formatted inside map_chunk(); append it to the output in read order */
		double t0 = mga_wtime();
		int k;
		for (k = 0; k < b->n_threads; ++k) cst.gaf_bytes += b->gaf_part[(size_t)c * b->n_threads + k].l;
		{ int64_t t_ = cpu_now(); commit_chunks(b, c); CPU_ADD(C_COMMIT, t_); }
		cst.t_gaf += mga_wtime() - t0;
	}
	CPU_ADD(C_PIPE, tcpu);
	pthread_mutex_lock(&g_stats_mtx); stats_merge(&S->gi->B->st, &cst); pthread_mutex_unlock(&g_stats_mtx);
	pthread_mutex_lock(&S->m);
	if (rc < 0 && !b->err) { b->err = 1; snprintf(b->errmsg, sizeof b->errmsg, "%s", mga_last_error()); }
	if (++b->n_done == b->n_chunks) { b->complete = 1; pthread_cond_broadcast(&S->c_done); }
	pthread_mutex_unlock(&S->m);
}

typedef struct { mga_stream_t *S; int k; } stream_thr_t;

static void *stream_worker(void *a)
{
	stream_thr_t *t = (stream_thr_t*)a;
	mga_stream_t *S = t->S;
	pipe_ctx_t *P = &S->P[t->k];
	free(t);
	if (mga_dev_bind_thread() < 0) return 0;
	pthread_mutex_lock(&S->m);
	for (;;) {
		sbatch_t *b;
		int c;
		while (!S->closing && (S->cur == 0 || S->cur->next_chunk >= S->cur->n_chunks)) {
			if (S->cur && S->cur->next) { S->cur = S->cur->next; continue; }
			pthread_cond_wait(&S->c_work, &S->m);
		}
		if (S->cur == 0 || S->cur->next_chunk >= S->cur->n_chunks) break; /* closing and nothing left */
		b = S->cur, c = b->next_chunk++;
		pthread_mutex_unlock(&S->m);
		stream_run_chunk(S, P, b, c);
		pthread_mutex_lock(&S->m);
	}
	pthread_mutex_unlock(&S->m);
	return 0;
}

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
static void segv_trace(int sig) { void *bt[64]; int n = backtrace(bt, 64); (void)sig; backtrace_symbols_fd(bt, n, 2); _exit(139); } /* MGA_SEGV_TRACE=1: frames of a crash to stderr (addr2line on the .so) */

mga_stream_t *mga_stream_open(const mg_idx_t *gi, const mg_mapopt_t *opt, int n_threads)
{
	mga_stream_t *S;
	int i;
	if (mga_dev_init() < 0) return 0;
	if (env_int("MGA_SEGV_TRACE", 0)) signal(SIGSEGV, segv_trace);
	chunk_init_once();
	g_cpu_on = g_dbg_pipe > 0;
	S = MGA_CALLOC(mga_stream_t, 1);
	S->gi = gi, S->opt = *opt, S->n_threads = n_threads > 0 ? n_threads : 1;
	S->lr_long = (opt->flag & MG_M_RMQ) ? 0 : lr_long_bases();
	/* round 5: a rank with 5 .. 12 host threads chains on the device (k_gchain: long-tailed launches, 117 ms of a 125 000-read step at a quarter of the wave slots): SIX chunks
	 * in flight, two of them in the front phase, fill those tails with other chunks' kernels -- [measured, bench workload, --placement device, 16 threads] 2.98 / 3.00 Gbp/s
	 * (4 chunks, one in the front phase) -> 3.24 (6 / 2) -> 3.27-3.30 with the persistent WFA grids at half size; with the chaining on the host threads the same knobs stay
	 * inside the run-to-run noise (3.51-3.60 vs 3.55-3.65) */
	S->n_pipe = env_int("MGA_PIPE", n_threads > 4 ? 6 : 4); /* round 6, chaining on the host threads, 16 of them (profiles/r06u_knobs.txt): 6 pipeline threads + 2 chunks in the front phase 4.68 Gbp/s, 5 + 2: 4.58, 4 + 1 (the default until then): 4.48-4.51 */ /* round 5, a rank pinned to 2 of 16 cores, two chunks in the front phase: 4 pipeline threads 2.51 Gbp/s, 3: 2.28 (round 4, one chunk in the front phase: 3 was the better one) */ /* [measured, round 4, a rank pinned to 2 of 16 cores] 3 pipeline threads: 2.31 Gbp/s at 0.70 CPU-s per step, 4: 2.23 at 0.82, 2: 2.07; with 16 threads and the chaining on the host 4 is the best (3.27 vs 2.96 vs 2.51) */
	if (S->n_pipe > MGA_MAX_PIPE) S->n_pipe = MGA_MAX_PIPE;
	if (S->n_pipe < 1) S->n_pipe = 1;
	S->chunk = env_int("MGA_CHUNK", 16384); /* [measured] larger launches amortise the tails of the WFA tiers: 4096 -> 8192 reads +5 %, -> 16384 another +5 % */
	if (S->chunk < 1) S->chunk = 1;
	S->max_inflight = env_int("MGA_INFLIGHT", 3);
	pthread_mutex_init(&S->m, 0); pthread_mutex_init(&S->api, 0);
	pthread_cond_init(&S->c_work, 0); pthread_cond_init(&S->c_done, 0); pthread_cond_init(&S->c_space, 0);
	pthread_mutex_init(&S->tok_front.m, 0); pthread_cond_init(&S->tok_front.c, 0); pthread_mutex_init(&S->tok_wfa.m, 0); pthread_cond_init(&S->tok_wfa.c, 0);
	/* this stream's own token pair: 2 and 2, where the process-wide pair of the mg_tbuf_t contexts has 2 and 1 (chunk.h: chunk_init_once) */
	S->tok_wfa.avail = env_int("MGA_WFA_SLOTS", 2);                 /* two chunks may be in their WFA phase: the second one fills the tails of the first */
	S->tok_front.avail = env_int("MGA_FRONT_SLOTS", 2); /* ... and with the chaining on the device two in the front phase ([measured] + 8 % at 16 threads, + 7 % at 2) */
	for (i = 0; i < S->n_pipe; ++i) {
		if ((S->P[i].sc = mga_sctx_create()) == 0) { while (--i >= 0) pipe_ctx_free(&S->P[i]); free(S); return 0; }
		S->P[i].tok_front = &S->tok_front, S->P[i].tok_wfa = &S->tok_wfa;
	}
	return S;
}

static void stream_start(mga_stream_t *S) /* worker threads are created with the first multi-chunk batch: one-read calls never need them */
{
	int i;
	if (S->started) return;
	for (i = 0; i < S->n_pipe; ++i) {
		stream_thr_t *t = MGA_CALLOC(stream_thr_t, 1);
		t->S = S, t->k = i;
		pthread_create(&S->thr[i], 0, stream_worker, t);
	}
	S->started = 1;
}

void mga_stream_set_opt(mga_stream_t *S, const mg_mapopt_t *opt, int n_threads) { S->opt = *opt; S->lr_long = (opt->flag & MG_M_RMQ) ? 0 : lr_long_bases(); if (n_threads > 0) S->n_threads = n_threads; } /* only while nothing is in flight */

/* chunk boundaries of a batch: MGA_CHUNK reads each at most; the FIRST batch of a job ramps up from chunk/4 and the LAST one ramps down
 * (fill and drain of the pipeline cost about one chunk time each).
 * MGA_CUT=1 (round 5, default): chunks of EQUAL size inside a batch instead of full chunks + a remainder -- a 50 000-read mini-batch is 4 x 12 500, not 3 x 16 384 + 848:
 * a chunk of a few hundred reads pays a pass's whole chain of launches and synchronisations for no work ([measured, bench workload] its three -K batches were cut into
 * 12 chunks, two of them of 848 and 424 reads).  MGA_TAIL=<levels>: the LAST batch ends in chunks of 1/2, 1/4, ... of a chunk (the drain of the pipeline: the last chunk
 * walks its stages with nothing behind it).  The output never depends on the cut (test_pipeline_knobs_do_not_change_the_output). */
typedef struct { int even, n_head, head_sz[8], n_tail, tail_tot, body_sz, tail_sz[8]; } cut_plan_t;

/* job_pos: chunks the JOB has been cut into before this batch; ramp_levels: the job's first chunks are chunk >> levels, ..., chunk >> 1 (round 5: the ramp belongs to the job,
 * not to its first batch -- the reader's first batch is a short one of 6 400 reads, so that the GPU starts early, and the ramp used to end with it) */
static void cut_plan_init(cut_plan_t *cp, int n, int chunk, int ramp, int flags, int even, int tail_levels, int job_pos, int ramp_levels)
{
	int k, used = 0, body;
	memset(cp, 0, sizeof *cp);
	cp->even = even, cp->body_sz = chunk;
	if (!even) return;
	if (ramp && (flags & MGA_SB_LAST)) for (k = 0; k < tail_levels && k < 8 && (chunk >> (k + 1)) >= 64; ++k) cp->tail_sz[cp->n_tail++] = chunk >> (k + 1), cp->tail_tot += chunk >> (k + 1);
	if (n < cp->tail_tot + chunk / 2) cp->n_tail = 0, cp->tail_tot = 0; /* too small for a tapered end */
	if (ramp_levels > 8) ramp_levels = 8;
	for (k = job_pos; ramp && k < ramp_levels; ++k) { /* the ramp pieces that are still due, as long as something of the batch is left behind them */
		const int sz = chunk >> (ramp_levels - k);
		if (sz < 1 || n - used - cp->tail_tot < sz + sz / 2) break;
		cp->head_sz[cp->n_head++] = sz, used += sz;
	}
	body = n - used - cp->tail_tot;
	if (body > 0) { const int nc = (body + chunk - 1) / chunk; cp->body_sz = (body + nc - 1) / nc; }
}

/* size of chunk number m of a batch of which `left` reads are left */
static int cut_plan_size(const cut_plan_t *cp, int chunk, int ramp, int flags, int m, int left)
{
	int sz = chunk, k, suf;
	if (!cp->even) { /* rounds 1-4: full chunks + what is left */
		if (ramp) {
			if (flags & MGA_SB_FIRST) { if (m == 0) sz = chunk / 4; else if (m == 1) sz = chunk / 2; }
			if ((flags & MGA_SB_LAST) && left <= chunk + chunk / 2) sz = left > chunk / 2 + chunk / 8 ? left - chunk / 2 : left; /* tail: the last chunk is chunk/2 (or what is left) */
		}
		return sz;
	}
	sz = m < cp->n_head ? cp->head_sz[m] : cp->body_sz;
	if (cp->n_tail > 0 && m >= cp->n_head) {
		if (left <= cp->tail_tot) { /* in the tail: the largest run of tail pieces that fits; what a base-capped chunk before left over is absorbed by this piece */
			for (k = 0, suf = cp->tail_tot; k < cp->n_tail && suf > left; ++k) suf -= cp->tail_sz[k];
			sz = k < cp->n_tail ? cp->tail_sz[k] + (left - suf) : left;
		} else if (left - sz < cp->tail_tot) sz = left - cp->tail_tot; /* the body's last chunk ends where the tail pieces begin */
	}
	return sz;
}

/* (tests) the read counts of the chunks a batch of n reads of equal length is cut into; returns their number */
int mga_debug_cut2(int n, int chunk, int flags, int even, int tail_levels, int job_pos, int ramp_levels, int *sizes, int max_sizes)
{
	cut_plan_t cp;
	int pos = 0, m = 0;
	const int ramp = n > 6 * chunk || (flags & (MGA_SB_FIRST | MGA_SB_LAST)) != (MGA_SB_FIRST | MGA_SB_LAST);
	cut_plan_init(&cp, n, chunk, ramp, flags, even, tail_levels, job_pos, ramp_levels);
	while (pos < n) {
		int sz = cut_plan_size(&cp, chunk, ramp, flags, m, n - pos);
		if (sz < 1) sz = 1;
		if (sz > n - pos) sz = n - pos;
		if (m < max_sizes) sizes[m] = sz;
		++m, pos += sz;
	}
	return m;
}
/* (the round-4 ramp: chunk / 4 and chunk / 2 at the head of the job's first batch) */
int mga_debug_cut(int n, int chunk, int flags, int even, int tail_levels, int *sizes, int max_sizes) { return mga_debug_cut2(n, chunk, flags, even, tail_levels, (flags & MGA_SB_FIRST) ? 0 : 2, 2, sizes, max_sizes); }

static void batch_cut(mga_stream_t *S, sbatch_t *b)
{
	const int n = b->n, chunk = S->chunk;
	const int ramp = env_int("MGA_RAMP", 1) && (n > 6 * chunk || (b->flags & (MGA_SB_FIRST | MGA_SB_LAST)) != (MGA_SB_FIRST | MGA_SB_LAST)); /* a batch of a longer job always ramps */
	/* a chunk is also bounded in BASES: its device buffers grow with bases and anchors, not with reads, and a chunk of 16384 reads of 100 kb
	 * each would be ten times the footprint every measurement was taken at.  MGA_CHUNK reads of 12 kb is the cap (10 kb reads: never reached). */
	const int64_t base_cap = (S->opt.flag & MG_M_RMQ) ? INT64_MAX : (int64_t)chunk * env_int("MGA_CHUNK_READ_BASES", 12288); /* (-x asm: a batch is a handful of contigs chained in phases over ALL of them) */
	int pos = 0, m = 0, cap = n / (chunk / 16 > 0 ? chunk / 16 : 1) + 16;
	cut_plan_t cp;
	{ /* MGA_JOBRAMP=<levels> (default 3): the job's first chunks are chunk/8, chunk/4, chunk/2, whatever batches they fall into; 0: the round-4 rule (chunk/4, chunk/2 in the first batch) */
		const int lv = env_int("MGA_JOBRAMP", 3);
		cut_plan_init(&cp, n, chunk, ramp, b->flags, env_int("MGA_CUT", 1), env_int("MGA_TAIL", 1), lv > 0 ? S->job_chunks : ((b->flags & MGA_SB_FIRST) ? 0 : 2), lv > 0 ? lv : 2);
	}
	b->cstart = MGA_MALLOC(int, cap + 1);
	while (pos < n) {
		int sz = cut_plan_size(&cp, chunk, ramp, b->flags, m, n - pos), left = n - pos, k;
		int64_t bases = 0;
		if (sz < 1) sz = 1;
		if (sz > left) sz = left;
		{ /* ultra-long -x lr reads (>= MGA_LONG_READ bases, default 256 k) travel in chunks of their own -- at most 64 Mbp of them -- through the long-query path (map_chunk) */
			const int lr_long = S->lr_long;
			const int first_long = lr_long > 0 && b->qlens[pos] >= lr_long;
			for (k = 0; k < sz; ++k) {
				if (lr_long > 0 && k > 0 && (b->qlens[pos + k] >= lr_long) != first_long) break;
				bases += b->qlens[pos + k];
				if ((bases > base_cap || (first_long && bases > (64LL << 20))) && k > 0) break; /* (a single read longer than the cap is a chunk of its own) */
			}
		}
		sz = k;
		if (m == cap) { cap += cap / 2 + 8; b->cstart = MGA_REALLOC(int, b->cstart, cap + 1); }
		b->cstart[m++] = pos; pos += sz;
	}
	b->cstart[m] = n;
	b->n_chunks = m;
	S->job_chunks += m;
}

/* Queue a batch.  Everything passed in is BORROWED until the batch has been collected.  gcs != NULL: chain mode (results in gcs[]);
 * want_gaf: text mode (GAF bytes of the batch, input order).  out/out_cap: an output buffer to reuse (may be NULL).  Blocks while
 * MGA_INFLIGHT batches are already in flight. */
int mga_stream_submit(mga_stream_t *S, int n, const int *qlens, const char **seqs, const char **qnames, mg_gchains_t **gcs, int want_gaf,
					  const char *d_seq, const int64_t *q_off, int seqs_pinned, int flags, char *out, int64_t out_cap, void *user)
{
	sbatch_t *b = MGA_CALLOC(sbatch_t, 1);
	int i;
	b->n = n, b->flags = flags, b->qlens = qlens, b->seqs = seqs, b->qnames = qnames, b->d_seq = d_seq, b->q_off = q_off, b->seqs_pinned = seqs_pinned;
	b->want_gaf = want_gaf, b->user = user, b->out = out, b->out_cap = out ? out_cap : 0;
	b->n_threads = S->n_threads;
	if (gcs) b->gcs = gcs; else b->gcs = MGA_CALLOC(mg_gchains_t*, n > 0 ? n : 1), b->own_gcs = 1;
	for (i = 0; i < n; ++i) b->gcs[i] = 0;
	if (flags & MGA_SB_FIRST) S->job_chunks = 0; /* a new job: its ramp starts over (batches are submitted by one thread) */
	batch_cut(S, b);
	if (want_gaf) { b->gaf_part = MGA_CALLOC(kstring_t, (size_t)(b->n_chunks > 0 ? b->n_chunks : 1) * b->n_threads); b->done = MGA_CALLOC(char, b->n_chunks > 0 ? b->n_chunks : 1); }
	pthread_mutex_init(&b->cmtx, 0);
	if (b->n_chunks == 0) b->complete = 1;
	pthread_mutex_lock(&S->m);
	while (S->n_inflight >= S->max_inflight) pthread_cond_wait(&S->c_space, &S->m);
	if (S->n_submitted++ == 0) { g_job_t0 = mga_wtime(); if (g_cpu_on) memset((void*)g_cpu_ns, 0, sizeof g_cpu_ns); }
	if (S->tail) S->tail->next = b; else S->head = b;
	S->tail = b;
	if (S->cur == 0) S->cur = b;
	++S->n_inflight;
	/* Only a job that is ONE single-chunk batch (FIRST|LAST: one-read calls, small mg_map_batch calls) may run inline on the collecting thread
	 * (mga_stream_collect, context 0).  Any other batch starts the workers NOW: a single-chunk first batch of a longer job (e.g. 64 Mbp of 50 kb reads)
	 * used to run inline on P[0] while the next batch started worker 0 on the SAME context -- two threads on one set of device / staging buffers
	 * (the "chunks of more than 16384 reads" fault of round 2: any chunk size that made the job's first batch a single chunk). */
	b->inline_ok = b->n_chunks <= 1 && !S->started && (flags & (MGA_SB_FIRST | MGA_SB_LAST)) == (MGA_SB_FIRST | MGA_SB_LAST);
	if (!b->inline_ok) { stream_start(S); pthread_cond_broadcast(&S->c_work); }
	pthread_mutex_unlock(&S->m);
	return 0;
}

/* Collect the oldest batch: blocks until all of its chunks are done.  Returns 1 (a batch: out, out_len and out_cap receive its GAF buffer,
 * now owned by the caller), 0 (nothing in flight) or -1 (the batch failed: message in mga_last_error()). */
int mga_stream_collect(mga_stream_t *S, char **out, int64_t *out_len, int64_t *out_cap, void **user)
{
	sbatch_t *b;
	int rc = 1, i;
	pthread_mutex_lock(&S->m);
	b = S->head;
	if (b == 0) { pthread_mutex_unlock(&S->m); return 0; }
	if (b->inline_ok && !S->started) { /* a single-chunk, single-batch job on a stream without workers runs right here, on context 0 (one-read calls: no thread hand-off) */
		while (b->next_chunk < b->n_chunks) {
			int c = b->next_chunk++;
			pthread_mutex_unlock(&S->m);
			stream_run_chunk(S, &S->P[0], b, c);
			pthread_mutex_lock(&S->m);
		}
	}
	while (!b->complete) pthread_cond_wait(&S->c_done, &S->m);
	S->head = b->next;
	if (S->head == 0) S->tail = 0;
	if (S->cur == b) S->cur = b->next;
	--S->n_inflight;
	pthread_cond_broadcast(&S->c_space);
	pthread_mutex_unlock(&S->m);
	if (b->err) {
		for (i = 0; i < b->n; ++i) { mg_gchain_free(b->gcs[i]); b->gcs[i] = 0; }
		if (b->gaf_part) for (i = 0; i < b->n_chunks * b->n_threads; ++i) strbuf_put(b->gaf_part[i].s, b->gaf_part[i].m);
		mga_set_error("%s", b->errmsg[0] ? b->errmsg : "mapping pipeline failed");
		rc = -1;
	}
	if (b->want_gaf) {
		if (b->out == 0) b->out = (char*)malloc(1), b->out_cap = 1;
		b->out[b->out_len] = 0;
	}
	if (out) *out = b->out; else free(b->out);
	if (out_len) *out_len = b->out_len;
	if (out_cap) *out_cap = b->out_cap;
	if (user) *user = b->user;
	if (g_cpu_on && rc > 0) {
		struct timespec ts;
		fprintf(stderr, "[pipe] host CPU seconds by stage (cumulative, batch of %d reads done at %.3f s):", b->n, mga_wtime() - g_job_t0);
		for (i = 0; i < C_N; ++i) fprintf(stderr, " %s %.3f", g_cname[i], g_cpu_ns[i] * 1e-9);
		clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &ts);
		fprintf(stderr, "; process total so far %.3f\n", ts.tv_sec + ts.tv_nsec * 1e-9);
	}
	pthread_mutex_destroy(&b->cmtx);
	if (b->own_gcs) free(b->gcs);
	free(b->cstart); free(b->gaf_part); free(b->done); free(b);
	return rc;
}

void mga_stream_close(mga_stream_t *S)
{
	int i;
	if (S == 0) return;
	while (mga_stream_collect(S, 0, 0, 0, 0) != 0) {} /* drop what was never collected */
	pthread_mutex_lock(&S->m);
	S->closing = 1;
	pthread_cond_broadcast(&S->c_work);
	pthread_mutex_unlock(&S->m);
	if (S->started) for (i = 0; i < S->n_pipe; ++i) pthread_join(S->thr[i], 0);
	for (i = 0; i < S->n_pipe; ++i) pipe_ctx_free(&S->P[i]);
	pthread_mutex_destroy(&S->m); pthread_mutex_destroy(&S->api);
	pthread_cond_destroy(&S->c_work); pthread_cond_destroy(&S->c_done); pthread_cond_destroy(&S->c_space);
	free(S);
}

/* the index's own stream: created on first use, closed by mg_idx_destroy() */
static pthread_mutex_t g_idx_stream_mtx = PTHREAD_MUTEX_INITIALIZER;
static mga_stream_t *idx_stream(const mg_idx_t *gi, const mg_mapopt_t *opt, int n_threads)
{
	struct mg_idx_bucket_s *B = gi->B;
	pthread_mutex_lock(&g_idx_stream_mtx);
	if (B->stream == 0) B->stream = mga_stream_open(gi, opt, n_threads);
	pthread_mutex_unlock(&g_idx_stream_mtx);
	return (mga_stream_t*)B->stream;
}
/* the index's stream for a whole job (mg_map_files): locked until released, so that its pipeline contexts -- device buffers, pinned staging,
 * HIP streams: hundreds of MB that are expensive to allocate -- are reused from job to job instead of being rebuilt */
mga_stream_t *mga_idx_stream_acquire(const mg_idx_t *gi, const mg_mapopt_t *opt, int n_threads)
{
	mga_stream_t *S = idx_stream(gi, opt, n_threads);
	if (S == 0) return 0;
	pthread_mutex_lock(&S->api);
	mga_stream_set_opt(S, opt, n_threads);
	S->n_submitted = 0; /* a new job: its first batch restarts the debug clocks */
	return S;
}
void mga_stream_set_cov(mga_stream_t *S, mga_cov_job_t *J) { S->cov = J; }
void mga_idx_stream_release(mga_stream_t *S) { pthread_mutex_unlock(&S->api); }

void mga_idx_stream_close(mg_idx_t *gi) { if (gi && gi->B && gi->B->stream) { mga_stream_close((mga_stream_t*)gi->B->stream); gi->B->stream = 0; } }

/* one batch through the index's stream, start to finish.  Calls are serialized per index (the pipeline contexts are
 * shared state); callers that want concurrency use one mg_tbuf_t per thread with mg_map()/mg_map_frag(), or their own stream. */
static int map_all(const mg_idx_t *gi, int n, const int *qlens, const char **seqs, const char **qnames, mg_gchains_t **gcs,
				   const mg_mapopt_t *opt, int n_threads, const char *d_seq, const int64_t *q_off, char **gaf, int64_t *gaf_len)
{
	mga_stream_t *S;
	struct mg_idx_bucket_s *B = gi->B;
	int rc, i;
	for (i = 0; i < n; ++i) gcs[i] = 0;
	if (n <= 0) return 0;
	if ((S = idx_stream(gi, opt, n_threads)) == 0) return -1;
	pthread_mutex_lock(&S->api);
	mga_stream_set_opt(S, opt, n_threads);
	if (gaf) {
		char *out = B->gaf_out; int64_t cap = B->gaf_cap, len = 0;
		B->gaf_out = 0, B->gaf_cap = 0;
		mga_stream_submit(S, n, qlens, seqs, qnames, gcs, 1, d_seq, q_off, 0, MGA_SB_FIRST | MGA_SB_LAST, out, cap, 0);
		rc = mga_stream_collect(S, &out, &len, &cap, 0);
		B->gaf_out = out, B->gaf_cap = cap; /* the GAF text stays owned by the index */
		*gaf = out, *gaf_len = rc > 0 ? len : 0;
	} else {
		mga_stream_submit(S, n, qlens, seqs, qnames, gcs, 0, d_seq, q_off, 0, MGA_SB_FIRST | MGA_SB_LAST, 0, 0, 0);
		rc = mga_stream_collect(S, 0, 0, 0, 0);
	}
	pthread_mutex_unlock(&S->api);
	return rc > 0 ? 0 : -1;
}

/* map + format: the GAF text (input order) of n reads; *gaf points into a grow-only buffer OWNED BY THE INDEX, valid until the
 * next call on this index or mg_idx_destroy(); chains are not returned */
int mga_map_gaf(const mg_idx_t *gi, int n, const int *qlens, const char **seqs, const char **qnames, const mg_mapopt_t *opt, int n_threads,
				const char *d_seq, const int64_t *q_off, char **gaf, int64_t *gaf_len)
{
	mg_gchains_t **gcs = MGA_CALLOC(mg_gchains_t*, n > 0 ? n : 1);
	int rc;
	*gaf = 0, *gaf_len = 0;
	rc = map_all(gi, n, qlens, seqs, qnames, gcs, opt, n_threads, d_seq, q_off, gaf, gaf_len);
	free(gcs);
	return rc;
}

int mg_map_batch(const mg_idx_t *gi, int n, const int *qlens, const char **seqs, const char **qnames, mg_gchains_t **gcs,
				 const mg_mapopt_t *opt, int n_threads)
{
	return map_all(gi, n, qlens, seqs, qnames, gcs, opt, n_threads, 0, 0, 0, 0);
}

/* same as mg_map_batch() for reads that already sit in HBM: d_seq holds the reads back to back (+64 readable bytes),
 * q_off[n+1] are their absolute offsets. */
int mga_map_batch_resident(const mg_idx_t *gi, int n, const int *qlens, const char **seqs, const char **qnames, mg_gchains_t **gcs,
						   const mg_mapopt_t *opt, int n_threads, const char *d_seq, const int64_t *q_off)
{
	return map_all(gi, n, qlens, seqs, qnames, gcs, opt, n_threads, d_seq, q_off, 0, 0);
}

void mga_get_stats(const mg_idx_t *gi, mga_stats_t *st, int reset)
{
	pthread_mutex_lock(&g_stats_mtx);
	*st = gi->B->st;
	if (reset) memset(&gi->B->st, 0, sizeof(mga_stats_t));
	pthread_mutex_unlock(&g_stats_mtx);
}
