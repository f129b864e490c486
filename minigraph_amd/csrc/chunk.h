/* chunk.h -- one chunk of reads through the stage sequence (chunk.c), for its two callers: the stream's pipeline threads (stream.c) and the per-read API (mapper.c) */
#ifndef MGA_CHUNK_H
#define MGA_CHUNK_H
#include <stdio.h>
#include <pthread.h>
#include "mga_host.h"

struct gpu_token_s;
typedef struct { /* one pipeline context: HIP stream + grow-only device and pinned buffers, reused from chunk to chunk */
	mga_sctx_t *sc;
	struct gpu_token_s *tok_front, *tok_wfa; /* the GPU phase tokens of the stream this context belongs to (NULL: the process-wide pair -- mg_tbuf_t contexts) */
	union {
		struct {
			mga_dbuf_t seq, qoff, cnt, mzoff, mz, occ, val, na, nmini, rep, aoff, minioff, a, tmp, mini, u, b, nu, nb, ws;
			mga_dbuf_t tseq, prob, res, pool, used, ncig, cigoff, ord, rflag, item, chain, vert, txtres, txtpool;
			mga_dbuf_t sk_item, sk_cnt, sk_off, sd_tk, sd_kf, sd_offa, sd_offm, sd_rkey, sd_rmax; /* long-query path (MG_M_RMQ): sketch pieces, per-minimizer scans */
			mga_dbuf_t hash, gchdr, gcpool, lcpool, apool, gcctl, gcretry; /* graph chaining on the device (k_gchain.hip) */
			mga_dbuf_t plcnt, ploff, pltot, plsrc, plrev; /* gap list on the device (k_plan.hip) */
			mga_dbuf_t lcord; /* k_lchain's launch order: reads by anchor count, most first */
			mga_dbuf_t rq_a, rq_f, rq_p, rq_v, rq_t, rq_pri, rq_ys, rq_cut, rq_ord, rq_stat, rq_cnt; /* forward pass of the RMQ chainer on the device (k_rmq.hip), one read at a time */
			mga_dbuf_t g_line, g_qn, g_qoff, g_len, g_off, g_out; /* whole GAF lines on the device (k_gaf.hip): line records, read names, line lengths / offsets, the text */
			mga_dbuf_t cv_chain, cv_vert; /* read coverage (k_cov.hip): chain records and walk vertices of the chunk */
		};
		mga_dbuf_t dall[75];
	};
	union {
		struct { mga_hbuf_t h_b, h_u, h_mini, h_tseq, h_prob, h_pool, h_seq, h_ncig, h_cigoff, h_item, h_chain, h_vert, h_txtres, h_txtpool, h_gchdr, h_gcpool, h_lcpool, h_apool, h_plrev, h_ploff, h_lcord, h_rq, h_rqs, h_plsrc, h_gline, h_gqn, h_gout, h_cvchain, h_cvvert; }; /* pinned staging */
		mga_hbuf_t hall[29];
	};
} pipe_ctx_t;
_Static_assert(sizeof(((pipe_ctx_t*)0)->dall) == 75 * sizeof(mga_dbuf_t) && sizeof(((pipe_ctx_t*)0)->hall) == 29 * sizeof(mga_hbuf_t), "pipe_ctx_t: buffer lists out of sync");

MGA_LOCAL void pipe_ctx_free(pipe_ctx_t *P);

MGA_LOCAL extern double g_job_t0; /* the clock of the MGA_DEBUG_PIPE log: restarted by a job's first batch */
MGA_LOCAL extern int g_dbg_pipe;  /* MGA_DEBUG_PIPE, read once per process (chunk_init_once) */
#define PIPE_LOG(what, c, tb) do { if (g_dbg_pipe > 0) fprintf(stderr, "[pipe] chunk %d %-10s %8.1f .. %8.1f ms\n", (c), (what), ((tb) - g_job_t0) * 1e3, (mga_wtime() - g_job_t0) * 1e3); } while (0)

/* Two pipeline threads that start together would run every stage in lockstep (both on the GPU, then both on the host).
 * One token per GPU phase staggers them: while one chunk fills gaps on the GPU, the other one's host stages run, and the
 * cheap front phase (sketch/seed/chain) of one chunk fills the tail of another chunk's WFA launches. */
typedef struct gpu_token_s { pthread_mutex_t m; pthread_cond_t c; int avail; } gpu_token_t;
/* Before the first chunk of a process, from whichever entry point gets there first (pthread_once: concurrent first calls of mg_map() are the documented use): reads
 * MGA_DEBUG_PIPE and the slots of the PROCESS-WIDE token pair, which the contexts of mg_tbuf_t share -- MGA_WFA_SLOTS (default 2) and MGA_FRONT_SLOTS (default 1).
 * A stream's OWN pair (mga_stream_open) reads the same two variables with the defaults 2 and 2: its chunks may chain on the device, where two in the front phase pay. */
MGA_LOCAL void chunk_init_once(void);

static inline int env_int(const char *name, int dflt) { const char *s = getenv(name); return s && *s ? atoi(s) : dflt; }
MGA_LOCAL int lr_long_bases(void);

/* where a chunk's GAF lines may go straight to their place in the job's output (stream.c: sink_try_reserve / sink_commit) */
typedef struct { int (*try_reserve)(void *ctx, int64_t bytes, char **dst); void (*commit)(void *ctx, int64_t bytes); void *ctx; } gaf_sink_t;

typedef struct { /* what map_chunk() is given; fields left out are 0 */
	const mg_idx_t *gi; const mg_mapopt_t *opt; int n, n_threads, seqs_pinned, lr_long;
	const int *qlens; const char **seqs, **qnames; mg_gchains_t **gcs_out; mga_stats_t *st; kstring_t *gaf_part; const gaf_sink_t *sink;
	const char *d_seq_res; const int64_t *q_off_res; /* the caller keeps the batch resident: the reads in HBM + absolute offsets */
	mga_cov_job_t *cov; /* a coverage job (--cov): the chunk ends in chunk_cov() -- no GAF, no chains handed out */
} chunk_args_t;
MGA_LOCAL int map_chunk(pipe_ctx_t *P, const chunk_args_t *a);
#endif
