/*
 * mapper.c -- the map of the mapping pipeline, and the reference-compatible per-read wrappers mg_map() / mg_map_frag().
 *
 * The pipeline is the MI355X replacement for kt_for(n_threads, worker_for, ...) -> mg_map_frag() at the reference's gmap.c:99 / map-algo.c:340-495.  Four layers, one file each:
 *
 *   stream.c   mga_stream_t: batches are submitted, cut into chunks of MGA_CHUNK reads (cut_plan_*, batch_cut) and collected in order; MGA_PIPE pipeline threads, each with a
 *              pipe_ctx_t (HIP stream + grow-only device / pinned buffers), take the chunks; a chunk's GAF text is committed to the batch's output in read order.
 *              mg_map_batch(), mga_map_gaf() and kin run one batch through the index's own stream; mg_map_files() (mapfiles.c) keeps a stream for a whole job.
 *   chunk.c    map_chunk(): one chunk through the stage functions below, over one chunk_t.  Two GPU phase tokens (front, WFA) stagger the pipeline threads, so that the GPU
 *              work of one chunk overlaps the host work and the copies of the others.
 *   batch.c    mga_batch_t: the host halves between the GPU stages, per read on n_threads host threads (chain_worker, finish_worker, gaf_worker) + the flat exports for the uploads.
 *   rqphase.c  -x asm and ultra-long -x lr reads: the RMQ chainer of the whole batch as a task graph inside mga_batch_chain() (sort, forward runs, backtrack, twice).
 *
 * The stages of map_chunk(), in order (GPU: launched on the context's stream; host: on the chunk's pipeline thread, fanning out over the host threads):
 *
 *   GPU   chunk_upload_reads     reads -> HBM (front token taken)
 *   GPU   chunk_sketch           k_sketch: minimizers, a wavefront per read (per 64 kb piece for long queries)
 *   GPU   chunk_seed_count / chunk_seed_fill   k_seed_*: index lookup, anchors
 *   GPU   chunk_lchain           k_lchain: linear chaining + long-join rescue (not for long queries); decides where this chunk's graph chaining runs
 *   GPU   chunk_gchain_dev       k_gchain (+ k_plan's counting pass) for the chunks placed on the device
 *   GPU   chunk_front_readback   what the host chains from comes down (front token released)
 *   host  chunk_check            MGA_CHECK only
 *   host  chunk_host_chain       mga_batch_chain(): graph chaining (gc_core.h) of the reads not chained on the device, strand flags, the gap list; long queries: rqphase.c,
 *                                its forward passes back on the GPU through rq_dev_fwd_hook (k_rmq)
 *   GPU   chunk_wfa              export + uploads, k_plan's fill pass, then (WFA token) the WFA ladder in one sweep (k_wfa_sched) and the gather of the CIGARs
 *   GPU   chunk_text + chunk_gaf_dev    text mode: k_text (stitching, cg:Z, ds:Z) and k_gaf (whole lines); otherwise chunk_cigars_to_host
 *   host  chunk_finish           mga_batch_finish*(): CIGAR stitching + ds:Z, only where the device did not make the text
 *   host  chunk_emit             the lines to their place in the job's output or into the chunk's pieces (gaf_worker formats what the device did not); chain mode: the chains
 *         (--cov: chunk_cov instead -- chain records up, k_cov adds to the job's accumulators)
 *   host  chunk_stats, chunk_release
 */
#include <stdio.h>
#include "chunk.h"

/* ---- the reference's per-read API (map-algo.c:14-32,340-502).  Its threading contract is one mg_tbuf_t per worker thread
 * (gmap.c:84-86, ggen.c:36): here a mg_tbuf_t owns a pipeline context (HIP stream + device buffers), created on first use, so
 * that kt_for workers calling mg_map() concurrently never share device state.  b == NULL falls back to the index's stream. ---- */
struct mg_tbuf_s { pipe_ctx_t P; };
mg_tbuf_t *mg_tbuf_init(void) { return (mg_tbuf_t*)calloc(1, sizeof(mg_tbuf_t)); }
void mg_tbuf_destroy(mg_tbuf_t *b) { if (b == 0) return; if (b->P.sc) { mga_dev_bind_thread(); pipe_ctx_free(&b->P); } free(b); }

void mg_map_frag(const mg_idx_t *gi, int n_segs, const int *qlens, const char **seqs, mg_gchains_t **gcs, mg_tbuf_t *b, const mg_mapopt_t *opt, const char *qname)
{
	int i;
	for (i = 0; i < n_segs; ++i) gcs[i] = 0;
	if (n_segs != 1) { /* multi-segment (paired short reads) is outside the accelerated path: the reference itself returns NULLs for n_segs out of range */
		if (mg_verbose >= 1) fprintf(stderr, "[E::%s] only single-segment reads are supported by the MI355X path\n", __func__);
		return;
	}
	if (b) { /* the caller's own pipeline context: concurrent callers with distinct mg_tbuf_t never share device state */
		mga_stats_t cst;
		int rc;
		memset(&cst, 0, sizeof cst);
		chunk_init_once();
		rc = mga_dev_init() < 0 || mga_dev_bind_thread() < 0 || (b->P.sc == 0 && (b->P.sc = mga_sctx_create()) == 0) ? -1 : 0;
		if (rc == 0) rc = map_chunk(&b->P, &(chunk_args_t){ .gi = gi, .n = 1, .qlens = qlens, .seqs = seqs, .qnames = &qname, .gcs_out = gcs, .opt = opt, .n_threads = 1, .st = &cst,
															.lr_long = (opt->flag & MG_M_RMQ) ? 0 : lr_long_bases() });
		if (rc < 0) { fprintf(stderr, "[E::%s] %s\n", __func__, mga_last_error()); abort(); /* no CPU fallback */ }
		pthread_mutex_lock(&g_stats_mtx); stats_merge(&gi->B->st, &cst); pthread_mutex_unlock(&g_stats_mtx);
		return;
	}
	if (mg_map_batch(gi, 1, qlens, seqs, &qname, gcs, opt, 1) < 0) {
		fprintf(stderr, "[E::%s] %s\n", __func__, mga_last_error());
		abort(); /* no CPU fallback */
	}
}

mg_gchains_t *mg_map(const mg_idx_t *gi, int qlen, const char *seq, mg_tbuf_t *b, const mg_mapopt_t *opt, const char *qname)
{
	mg_gchains_t *gcs;
	mg_map_frag(gi, 1, &qlen, &seq, &gcs, b, opt, qname);
	return gcs;
}
