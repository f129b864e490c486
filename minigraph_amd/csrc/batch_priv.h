/* batch_priv.h -- the inside of mga_batch_t (mapper.h), for the three sources that work on its fields: batch.c (the host halves), rqphase.c (the RMQ phases of
 * mga_batch_chain) and chunk.c (which feeds the halves from the device stages and reads their plans back) */
#ifndef MGA_BATCH_PRIV_H
#define MGA_BATCH_PRIV_H
#include <pthread.h>
#include "hchain.h"
#include "align.h"
#include "mapper.h"

/* mga_batch_t's device hook (chunk.c: rq_dev_fwd_hook): the forward pass of the runs order[0 .. n_order) of n_reads reads' x-sorted anchors; runs = beg, end, base triples,
 * chunk-level; < 0: the device call failed */
typedef int (*mga_rq_dev_fwd_f)(void *ctx, int n_reads, const int64_t *r_abs0, const int64_t *r_n, const mg128_t *const *r_a, int32_t *const *r_f, int64_t *const *r_p, int32_t *const *r_v,
								int n_runs, const int64_t *runs, int n_order, const int32_t *order, int bw, int32_t *status);

typedef struct {
	int32_t tid;          /* pool that holds this read's plan */
	int32_t n_gc;
	int64_t *item_off;    /* n_gc + 1 offsets into the pool's item[] */
	int64_t *chain_id;    /* text mode: per chain, its index in the pool's chain[] (-1: not printed) */
} read_plan_t;

struct mga_batch_s {
	const mg_idx_t *gi;
	mg_mapopt_t opt;
	int n, n_threads;
	const int *qlens;
	const char **seqs, **qnames;
	const int64_t *q_off;   /* offset of read i in the device read buffer */
	float pen_gap, pen_skip;
	mg_gchains_t **gcs;
	read_plan_t *plan;
	mga_tpool_t *tp;
	int64_t *tp_prob_base, *tp_t_base, *tp_item_base, *tp_chain_base, *tp_vert_base;
	int want_text;          /* the caller only wants GAF bytes: cg:Z / ds:Z come from the device (k_text.hip) */
	int want_src;           /* ... and the targets of the gaps are spliced on the device from descriptors (align.h: mga_tpool_t::want_src) */
	const mga_txt_res_t *txt_res; /* text-mode results, global chain order */
	const char *txt_pool;
	const char *gaf_dev; int64_t gaf_dev_len; /* the chunk's GAF lines as the device wrote them (k_gaf.hip), read order, back to back; NULL: the host formats */
	/* stage-1 inputs, valid during mga_batch_chain() only */
	const int32_t *n_mz, *rep_len, *mini_pos, *nu, *nb;
	const int64_t *mini_off, *a_off;
	const uint64_t *u;
	const mg128_t *a;
	int a_is_raw;
	struct rq_read_s *rq;   /* a_is_raw: per-read state of the phased RMQ chaining (rqphase.c) */
	/* round 5: the forward passes of the RMQ chainer on the device (k_rmq.hip), one read at a time on the chunk's stream; rq_harr = pinned arrays p | f | v | t of ALL the
	 * chunk's anchors (the device writes f, p, v straight into them), rq_tot = their length in anchors */
	mga_rq_dev_fwd_f rq_dev_fwd;
	void *rq_dev_ctx; char *rq_harr; int64_t rq_tot;
	pthread_mutex_t rq_dev_mtx;
	int rq_dev_err; char rq_dev_errmsg[256]; /* a device call of the hook failed (not: a run handed back): the chunk fails with this message -- no silent host path */
	int32_t *seg_len;       /* segment lengths as a flat array (the graph view of gc_core.h on the host) */
	/* graph chains made on the device (k_gchain.hip): per-read headers + record pools; status != 0 marks the reads the host still chains */
	const mga_gc_hdr_t *gc_hdr; const char *gc_pool; const mg_llchain_t *gc_lc; const mg128_t *gc_a; size_t gc_rec;
	const int32_t *rescue_flag; /* per read: what the chaining kernel did about the long-join rescue (NULL: decide here) */
	/* gap list made on the device (k_plan.hip) for the device-chained reads: first printed chain of read i in the device's chain table; the host
	 * fills one strand flag per printed chain (dp_rev); the pools above then only hold the plans of the reads chained HERE, appended after the device's */
	const int64_t *dp_chain_off; int32_t *dp_rev; int64_t dp_n_chain;
	/* stage-2 inputs */
	mga_cigsrc_t src;
	int err;
};

/* a read's state in the phased RMQ chaining: rq_chain_all() (rqphase.c) fills b->rq[], chain_worker takes out / u / n_lc from it, mga_batch_chain() frees the array */
typedef struct rq_read_s {
	mg128_t *a; int64_t n;           /* anchors being chained: the read's slice of the batch (pass 1) or `out` of pass 1 (pass 2) */
	int32_t *f, *v, *t; int64_t *p;
	int64_t *cut; int32_t n_cut;     /* run boundaries: cut[0] = 0 .. cut[n_cut] = n */
	mg128_t *out; uint64_t *u; int n_lc, pass2;
} rq_read_t;
MGA_LOCAL void rq_chain_all(mga_batch_t *b);

/* the GAF text of one chunk, piece t of T on thread t (batch.c has the whole story); chunk.c runs it */
typedef struct { mga_batch_t *b; int n, T, mode; kstring_t *part; int64_t *bytes, *off; char *dst; } gafw_t; /* mode 0: into the pieces; 1: measure; 2: into windows of dst */
MGA_LOCAL void gaf_worker(void *data, int64_t t, int tid);

/* what chunk.c tells a batch before mga_batch_chain(), and takes from it afterwards, beyond mapper.h */
uint32_t mga_read_hash(const char *qname, int qlen, int seed);
void mga_batch_set_want_src(mga_batch_t *b, int on);
void mga_batch_set_device_chains(mga_batch_t *b, const mga_gc_hdr_t *hdr, const void *gc_pool, const mg_llchain_t *lc_pool, const mg128_t *a_pool);
void mga_batch_set_device_plan(mga_batch_t *b, const int64_t *chain_off, int32_t *rev, int64_t n_chain);
void mga_batch_set_rq_device(mga_batch_t *b, mga_rq_dev_fwd_f fwd, void *ctx, char *harr, int64_t tot);
void mga_batch_wfa_export_src(const mga_batch_t *b, mga_wfa_prob_t *prob, char *tseq, mga_plan_src_t *src, int64_t vert_base);
int64_t mga_batch_n_items(const mga_batch_t *b);
int64_t mga_batch_n_chains(const mga_batch_t *b);
int64_t mga_batch_n_verts(const mga_batch_t *b);
void mga_batch_text_export(const mga_batch_t *b, mga_cigitem_t *item, mga_txt_chain_t *chain, uint32_t *vert);
#endif
