/*
 * batch.c -- mga_batch_t: what the host threads do to one chunk between its GPU stages (mapper.c has the map of the pipeline).
 *
 * mga_batch_chain() is host half 1 (chain_worker, per read: chains from the device or graph chaining here, then the gap list), mga_batch_finish*() host half 2
 * (finish_worker: CIGAR stitching + ds:Z where the device did not make the text); in between the *_export functions flatten the per-thread pools for the upload,
 * and gaf_worker formats the chunk's lines at the end.  The halves are exported separately so that the host logic is testable on its own; chunk.c is the only
 * caller that matters in production.
 */
#include <stdio.h>
#include <math.h>
#include <assert.h>
#include "batch_priv.h"

/* Grow-only scratch that is recycled across chunks instead of being freed: the per-thread planning pools and the GAF
 * pieces are tens of MB per chunk, and handing them back to malloc means mmap/munmap and a page fault per 4 KB on
 * every chunk ([measured] ~0.2 s of host CPU per 100k reads). */
#include <pthread.h>
static pthread_mutex_t g_cache_mtx = PTHREAD_MUTEX_INITIALIZER;
#define TP_CACHE_MAX 512
static mga_tpool_t g_tp_cache[TP_CACHE_MAX];
static int g_n_tp_cache = 0;
static void tpool_get(mga_tpool_t *tp)
{
	pthread_mutex_lock(&g_cache_mtx);
	if (g_n_tp_cache > 0) *tp = g_tp_cache[--g_n_tp_cache]; else memset(tp, 0, sizeof *tp);
	pthread_mutex_unlock(&g_cache_mtx);
	tp->n_t = tp->n_prob = tp->n_item = tp->n_chain = tp->n_vert = 0, tp->wfa_t_bases = tp->wfa_q_bases = 0, tp->want_src = 0;
}
static void tpool_put(mga_tpool_t *tp)
{
	pthread_mutex_lock(&g_cache_mtx);
	if (g_n_tp_cache < TP_CACHE_MAX) { g_tp_cache[g_n_tp_cache++] = *tp; pthread_mutex_unlock(&g_cache_mtx); return; }
	pthread_mutex_unlock(&g_cache_mtx);
	free(tp->tseq); free(tp->prob); free(tp->item); free(tp->chain); free(tp->vert); free(tp->src);
}
#define STR_CACHE_MAX 512
static struct { char *s; size_t m; } g_str_cache[STR_CACHE_MAX];
static int g_n_str_cache = 0;
char *strbuf_get(size_t want, size_t *cap) /* a cached buffer (possibly grown) of at least `want` bytes */
{
	char *p = 0;
	size_t m = 0;
	int i, best = -1;
	pthread_mutex_lock(&g_cache_mtx);
	for (i = g_n_str_cache - 1; i >= 0; --i) { if (g_str_cache[i].m >= want) { best = i; break; } if (best < 0 || g_str_cache[i].m > g_str_cache[best].m) best = i; }
	if (best >= 0) { p = g_str_cache[best].s, m = g_str_cache[best].m; g_str_cache[best] = g_str_cache[--g_n_str_cache]; }
	pthread_mutex_unlock(&g_cache_mtx);
	if (m < want) { p = (char*)realloc(p, want); m = want; }
	*cap = m;
	return p;
}
void strbuf_put(char *p, size_t m)
{
	if (p == 0) return;
	pthread_mutex_lock(&g_cache_mtx);
	if (g_n_str_cache < STR_CACHE_MAX) { g_str_cache[g_n_str_cache].s = p, g_str_cache[g_n_str_cache++].m = m; p = 0; }
	pthread_mutex_unlock(&g_cache_mtx);
	free(p);
}


/* ------------------------------------------------------------------------------------------------ */

mga_batch_t *mga_batch_init(const mg_idx_t *gi, const mg_mapopt_t *opt, int n, const int *qlens, const char **seqs, const char **qnames,
							const int64_t *q_off, int n_threads)
{
	mga_batch_t *b = MGA_CALLOC(mga_batch_t, 1);
	float tmp;
	b->gi = gi, b->opt = *opt, b->n = n, b->qlens = qlens, b->seqs = seqs, b->qnames = qnames, b->q_off = q_off;
	b->n_threads = n_threads > 0 ? n_threads : 1;
	tmp = expf(-opt->div * gi->k); /* map-algo.c:388-390 */
	b->pen_gap = opt->chn_pen_gap * tmp, b->pen_skip = opt->chn_pen_skip * tmp;
	b->gcs = MGA_CALLOC(mg_gchains_t*, n > 0 ? n : 1);
	b->plan = MGA_CALLOC(read_plan_t, n > 0 ? n : 1);
	b->tp = MGA_CALLOC(mga_tpool_t, b->n_threads);
	{ int t_; for (t_ = 0; t_ < b->n_threads; ++t_) tpool_get(&b->tp[t_]); }
	b->tp_prob_base = MGA_CALLOC(int64_t, b->n_threads + 1);
	b->tp_t_base = MGA_CALLOC(int64_t, b->n_threads + 1);
	b->tp_item_base = MGA_CALLOC(int64_t, b->n_threads + 1);
	b->tp_chain_base = MGA_CALLOC(int64_t, b->n_threads + 1);
	b->tp_vert_base = MGA_CALLOC(int64_t, b->n_threads + 1);
	return b;
}

void mga_batch_set_want_src(mga_batch_t *b, int on) { int t; b->want_src = on; for (t = 0; t < b->n_threads; ++t) b->tp[t].want_src = on; }

void mga_batch_set_device_chains(mga_batch_t *b, const mga_gc_hdr_t *hdr, const void *gc_pool, const mg_llchain_t *lc_pool, const mg128_t *a_pool)
{
	b->gc_hdr = hdr, b->gc_pool = (const char*)gc_pool, b->gc_lc = lc_pool, b->gc_a = a_pool, b->gc_rec = mga_gc_rec_bytes();
}

void mga_batch_set_device_plan(mga_batch_t *b, const int64_t *chain_off, int32_t *rev, int64_t n_chain) { b->dp_chain_off = chain_off, b->dp_rev = rev, b->dp_n_chain = n_chain; }

void mga_batch_set_rq_device(mga_batch_t *b, mga_rq_dev_fwd_f fwd, void *ctx, char *harr, int64_t tot)
{
	b->rq_dev_fwd = fwd, b->rq_dev_ctx = ctx, b->rq_harr = harr, b->rq_tot = tot, b->rq_dev_err = 0;
	pthread_mutex_init(&b->rq_dev_mtx, 0);
}

void mga_batch_lchain_par(const mg_idx_t *gi, const mg_mapopt_t *opt, int qlen_max, mga_lchain_par_t *par) /* map-algo.c:377-403 for long reads */
{
	float tmp = expf(-opt->div * gi->k);
	int gap_ref;
	(void)qlen_max;
	if (opt->max_gap_ref > 0) gap_ref = opt->max_gap_ref;
	else if (opt->max_frag_len > 0) gap_ref = opt->max_gap; /* the per-read value max(max_frag_len - qlen, max_gap) is applied inside k_lchain (mga_rescue_par_t::frag_len) */
	else gap_ref = opt->max_gap;
	par->max_dist_x = gap_ref, par->max_dist_y = opt->max_gap;
	par->bw = opt->bw, par->max_skip = opt->max_lc_skip, par->max_iter = opt->max_lc_iter;
	par->min_cnt = opt->min_lc_cnt, par->min_sc = opt->min_lc_score;
	par->chn_pen_gap = opt->chn_pen_gap * tmp, par->chn_pen_skip = opt->chn_pen_skip * tmp;
}

uint32_t mga_read_hash(const char *qname, int qlen, int seed) /* map-algo.c:362-364 */
{
	uint32_t hash = qname ? mga_hash_str(qname) : 0;
	hash ^= mga_hash_u32((uint32_t)qlen) + mga_hash_u32((uint32_t)seed);
	return mga_hash_u32(hash);
}

static void chain_worker(void *data, int64_t i, int tid)
{
	mga_batch_t *b = (mga_batch_t*)data;
	const mg_mapopt_t *opt = &b->opt;
	const mg_idx_t *gi = b->gi;
	const int qlen = b->qlens[i];
	const char *seq = b->seqs[i], *qname = b->qnames ? b->qnames[i] : 0;
	uint32_t hash;
	int32_t n_lc = 0, k;
	int64_t n_a = 0;
	uint64_t *u = 0;
	mg128_t *a = 0;
	mg_gchains_t *gcs;

	int64_t tc = cpu_now();
	b->gcs[i] = 0;
	if (qlen == 0) return; /* map-algo.c:359-360 */
	if (opt->max_qlen > 0 && qlen > opt->max_qlen) return;
	if (b->gc_hdr && b->gc_hdr[i].status == 0) { /* chained on the device: flat records -> the reference's object (div and MAPQ through the host's libm) */
		const mga_gc_hdr_t *h = &b->gc_hdr[i];
		gcs = mga_gchains_from_flat(h->n_gc, b->gc_pool + (size_t)h->gc_off * b->gc_rec, h->n_lc, b->gc_lc + h->lc_off, b->gc_a ? h->n_a : 0, b->gc_a ? b->gc_a + h->a_off : 0, /* (no anchors on the host when the gap list was made on the device) */
									b->rep_len[i], qlen, b->n_mz[i], opt->min_gc_score);
		b->gcs[i] = gcs;
		CPU_ADD(C_GCPOST, tc);
		goto plan;
	}
	hash = mga_read_hash(qname, qlen, opt->seed);

	if (b->a_is_raw) { /* MG_M_RMQ: the RMQ chainer is the primary chainer (map-algo.c:397-399); both of its passes ran in mga_batch_chain's phases */
		a = b->rq[i].out, u = b->rq[i].u, n_lc = b->rq[i].n_lc;
		b->rq[i].out = 0, b->rq[i].u = 0;
	} else { /* chains of the GPU DP */
		n_lc = b->nu[i], n_a = b->nb[i];
		if (n_lc > 0) {
			u = MGA_MALLOC(uint64_t, n_lc); memcpy(u, b->u + b->a_off[i], (size_t)n_lc * 8);
			a = MGA_MALLOC(mg128_t, n_a); memcpy(a, b->a + b->a_off[i], (size_t)n_a * 16);
		}
	}
	CPU_ADD(C_LCCOPY, tc);
	/* long-join rescue (map-algo.c:407-417) */
	if (b->a_is_raw) { /* done in the phases */
	} else if (b->rescue_flag) { /* the kernel evaluated the condition: 1 = done there, 2 = due but deferred to the host (priority tie) */
		if (b->rescue_flag[i] == 2) goto do_rescue;
	} else if (opt->bw_long > opt->bw && (opt->flag & (MG_M_SPLICE | MG_M_SR)) == 0 && n_lc > 1) {
		int32_t st = (int32_t)a[0].y, en = (int32_t)a[(int32_t)u[0] - 1].y;
		if (qlen - (en - st) > opt->rmq_rescue_size || qlen - (en - st) > qlen * opt->rmq_rescue_ratio) {
do_rescue:;
			mg128_t *a2;
			for (k = 0, n_a = 0; k < n_lc; ++k) n_a += (int32_t)u[k];
			free(u); u = 0;
			mga_ksort_128x(n_a, a);
			a2 = mga_lchain_rmq(opt->max_gap, opt->max_gap_pre, opt->bw_long, opt->max_lc_skip, opt->rmq_size_cap, opt->min_lc_cnt, opt->min_lc_score,
								b->pen_gap, b->pen_skip, n_a, a, &n_lc, &u);
			free(a); a = a2;
		}
	}
	CPU_ADD(C_LCRESCUE, tc);
	{ /* chain records, clean-up, graph chaining, bridging, ordering and filters: gc_core.h on this host thread (map-algo.c:422-474) */
		const int32_t *mini = b->mini_pos + b->mini_off[i];
		const int32_t n_mini = (int32_t)(b->mini_off[i + 1] - b->mini_off[i]);
		int64_t n_anchor = 0;
		for (k = 0; k < n_lc; ++k) n_anchor += (int32_t)u[k];
		gcs = mga_gchain_host_read(gi, b->seg_len, opt, b->pen_gap, qlen, hash, n_lc, u, a, (int32_t)n_anchor, n_mini, mini, seq, b->rep_len[i], b->n_mz[i], 0, 0);
	}
	free(u); u = 0;
	free(a);
	CPU_ADD(C_GCGEN, tc);
	b->gcs[i] = gcs;
plan:
	if ((opt->flag & MG_M_CIGAR) && b->dp_chain_off && b->gc_hdr && b->gc_hdr[i].status == 0) { /* the gaps were listed on the device (k_plan.hip): only the strand of each printed line is decided here */
		read_plan_t *pl = &b->plan[i];
		int64_t c = b->dp_chain_off[i];
		int rev_sign = 0;
		pl->tid = -1, pl->n_gc = gcs->n_gc;
		pl->chain_id = MGA_MALLOC(int64_t, gcs->n_gc > 0 ? gcs->n_gc : 1);
		for (k = 0; k < gcs->n_gc; ++k) {
			const mg_gchain_t *gc = &gcs->gc[k];
			pl->chain_id[k] = -1;
			if ((gc->id != gc->parent && !(opt->flag & MG_M_PRINT_2ND)) || gc->cnt == 0) continue;
			if (mga_gaf_chain_rev(gi->g, gcs, gc, opt->flag)) rev_sign = 1;
			b->dp_rev[c] = rev_sign;
			pl->chain_id[k] = c++;
		}
		assert(c == b->dp_chain_off[i + 1]);
		CPU_ADD(C_PLAN, tc);
	} else if (opt->flag & MG_M_CIGAR) { /* list the gaps of every chain for the WFA kernel */
		read_plan_t *pl = &b->plan[i];
		mga_tpool_t *tp = &b->tp[tid];
		pl->tid = tid, pl->n_gc = gcs->n_gc;
		int rev_sign = 0; /* carried from chain to chain like mg_write_gaf does (format.c:123) */
		pl->item_off = MGA_MALLOC(int64_t, gcs->n_gc + 1);
		if (b->want_text) pl->chain_id = MGA_MALLOC(int64_t, gcs->n_gc > 0 ? gcs->n_gc : 1);
		for (k = 0; k < gcs->n_gc; ++k) {
			const mg_gchain_t *gc = &gcs->gc[k];
			pl->item_off[k] = tp->n_item;
			if (b->want_text) {
				pl->chain_id[k] = -1;
				if ((gc->id != gc->parent && !(opt->flag & MG_M_PRINT_2ND)) || gc->cnt == 0) continue; /* not printed (format.c:135-136): no alignment needed */
			}
			const int64_t vert_beg = tp->n_vert;
			if (b->want_text) { int32_t j; for (j = 0; j < gc->cnt; ++j) { MGA_GROW(uint32_t, tp->vert, tp->n_vert, tp->m_vert); tp->vert[tp->n_vert++] = gcs->lc[gc->off + j].v; } } /* the chain's walk: what the text kernel prints, and what the device splices the gaps' targets from */
			mga_plan_cigar(gi->g, gi->es, gcs, k, b->q_off ? b->q_off[i] : 0, tp, vert_beg);
			if (b->want_text) { /* what the text kernel needs to know about this chain */
				mga_txt_chain_t *c;
				const int32_t off_a0 = gcs->lc[gc->off].off;
				if (mga_gaf_chain_rev(gi->g, gcs, gc, opt->flag)) rev_sign = 1;
				MGA_GROW(mga_txt_chain_t, tp->chain, tp->n_chain, tp->m_chain);
				c = &tp->chain[tp->n_chain];
				c->item_beg = pl->item_off[k], c->item_end = tp->n_item, c->prob_base = 0, c->q_base = b->q_off ? b->q_off[i] : 0;
				c->vert_beg = vert_beg, c->vert_cnt = gc->cnt;
				c->qs = gc->qs, c->qe = gc->qe, c->ps = gc->ps, c->pe = gc->pe;
				c->ss = (int32_t)gcs->a[off_a0].x + 1 - (int32_t)(gcs->a[off_a0].y >> 32 & 0xff); /* galign.c:128-129 */
				c->ee = (int32_t)gcs->a[off_a0 + gc->n_anchor - 1].x + 1;
				c->rev_sign = rev_sign;
				pl->chain_id[k] = tp->n_chain++;
			}
		}
		pl->item_off[gcs->n_gc] = tp->n_item;
		CPU_ADD(C_PLAN, tc);
	}
}

int mga_batch_chain(mga_batch_t *b, const int32_t *n_mz, const int32_t *rep_len, const int32_t *mini_pos, const int64_t *mini_off,
					const int32_t *nu, const int32_t *nb, const uint64_t *u, const mg128_t *a, const int64_t *a_off, int a_is_raw, const int32_t *rescue_flag)
{
	int t;
	if (b->seg_len == 0) { uint32_t s_; b->seg_len = MGA_MALLOC(int32_t, b->gi->g->n_seg + 1); for (s_ = 0; s_ < b->gi->g->n_seg; ++s_) b->seg_len[s_] = b->gi->g->seg[s_].len; }
	b->rescue_flag = rescue_flag;
	b->n_mz = n_mz, b->rep_len = rep_len, b->mini_pos = mini_pos, b->mini_off = mini_off;
	b->nu = nu, b->nb = nb, b->u = u, b->a = a, b->a_off = a_off, b->a_is_raw = a_is_raw;
	if (a_is_raw) rq_chain_all(b);
	mga_parallel_for(b->n_threads, b->n, chain_worker, b);
	if (b->rq) { free(b->rq); b->rq = 0; }
	for (t = 0; t < b->n_threads; ++t) {
		b->tp_prob_base[t + 1] = b->tp_prob_base[t] + b->tp[t].n_prob;
		b->tp_t_base[t + 1] = b->tp_t_base[t] + b->tp[t].n_t;
		b->tp_item_base[t + 1] = b->tp_item_base[t] + b->tp[t].n_item;
		b->tp_chain_base[t + 1] = b->tp_chain_base[t] + b->tp[t].n_chain;
		b->tp_vert_base[t + 1] = b->tp_vert_base[t] + b->tp[t].n_vert;
	}
	if (b->rq_dev_err) { mga_set_error("RMQ forward pass on the device failed: %s", b->rq_dev_errmsg); return -1; } /* fail loudly: a device error must not pass for a slow job */
	return 0;
}

int64_t mga_batch_n_wfa(const mga_batch_t *b) { return b->tp_prob_base[b->n_threads]; }
int64_t mga_batch_wfa_target_bytes(const mga_batch_t *b) { return b->tp_t_base[b->n_threads]; }

typedef struct { const mga_batch_t *b; mga_wfa_prob_t *prob; char *tseq; mga_plan_src_t *src; int64_t vert_base; } export_t;
static void export_worker(void *data, int64_t t, int tid)
{
	export_t *e = (export_t*)data;
	const mga_batch_t *b = e->b;
	const mga_tpool_t *tp = &b->tp[t];
	int64_t j;
	int64_t tc = cpu_now();
	(void)tid;
	if (!tp->want_src) memcpy(e->tseq + b->tp_t_base[t], tp->tseq, (size_t)tp->n_t);
	for (j = 0; j < tp->n_prob; ++j) {
		e->prob[b->tp_prob_base[t] + j] = tp->prob[j];
		e->prob[b->tp_prob_base[t] + j].t_off += b->tp_t_base[t];
		if (tp->want_src) { e->src[b->tp_prob_base[t] + j] = tp->src[j]; e->src[b->tp_prob_base[t] + j].lc0 += b->tp_vert_base[t] + e->vert_base; }
	}
	CPU_ADD(C_EXPORT, tc);
}

void mga_batch_wfa_export(const mga_batch_t *b, mga_wfa_prob_t *prob, char *tseq) { mga_batch_wfa_export_src(b, prob, tseq, 0, 0); }

/* (want_src: src[] receives one descriptor per problem, its first walk vertex as an index into the flattened vertex array + vert_base; tseq is not written) */
void mga_batch_wfa_export_src(const mga_batch_t *b, mga_wfa_prob_t *prob, char *tseq, mga_plan_src_t *src, int64_t vert_base)
{
	export_t e;
	e.b = b, e.prob = prob, e.tseq = tseq, e.src = src, e.vert_base = vert_base;
	mga_parallel_for(b->n_threads, b->n_threads, export_worker, &e);
}

/* text mode: plan items, printed chains and their vertices of all pools, flattened in pool order with global offsets */
int64_t mga_batch_n_items(const mga_batch_t *b) { return b->tp_item_base[b->n_threads]; }
int64_t mga_batch_n_chains(const mga_batch_t *b) { return b->tp_chain_base[b->n_threads]; }
int64_t mga_batch_n_verts(const mga_batch_t *b) { return b->tp_vert_base[b->n_threads]; }
typedef struct { const mga_batch_t *b; mga_cigitem_t *item; mga_txt_chain_t *chain; uint32_t *vert; } texport_t;
static void text_export_worker(void *data, int64_t t, int tid)
{
	texport_t *e = (texport_t*)data;
	const mga_batch_t *b = e->b;
	const mga_tpool_t *tp = &b->tp[t];
	int64_t j;
	(void)tid;
	memcpy(e->item + b->tp_item_base[t], tp->item, (size_t)tp->n_item * sizeof(mga_cigitem_t));
	memcpy(e->vert + b->tp_vert_base[t], tp->vert, (size_t)tp->n_vert * 4);
	for (j = 0; j < tp->n_chain; ++j) {
		mga_txt_chain_t *c = &e->chain[b->tp_chain_base[t] + j];
		*c = tp->chain[j];
		c->item_beg += b->tp_item_base[t], c->item_end += b->tp_item_base[t], c->vert_beg += b->tp_vert_base[t], c->prob_base = b->tp_prob_base[t];
	}
}
void mga_batch_text_export(const mga_batch_t *b, mga_cigitem_t *item, mga_txt_chain_t *chain, uint32_t *vert)
{
	texport_t e;
	e.b = b, e.item = item, e.chain = chain, e.vert = vert;
	mga_parallel_for(b->n_threads, b->n_threads, text_export_worker, &e);
}

static void finish_worker(void *data, int64_t i, int tid)
{
	mga_batch_t *b = (mga_batch_t*)data;
	mg_gchains_t *gcs = b->gcs[i];
	read_plan_t *pl = &b->plan[i];
	int32_t k;
	int64_t tc = cpu_now();
	(void)tid;
	if (gcs == 0 || pl->item_off == 0) return;
	for (k = 0; k < gcs->n_gc; ++k) {
		const mga_tpool_t *tp = &b->tp[pl->tid];
		int r = mga_apply_cigar(gcs, k, tp->item + pl->item_off[k], pl->item_off[k + 1] - pl->item_off[k], b->tp_prob_base[pl->tid], &b->src);
		if (r < 0) { b->err = r; return; }
	}
	CPU_ADD(C_APPLY, tc);
	mga_gen_ds(b->gi->es, b->seqs[i], gcs);
	CPU_ADD(C_DS, tc);
}

static int batch_finish(mga_batch_t *b);

int mga_batch_finish(mga_batch_t *b, const mga_wfa_res_t *res, const uint32_t *pool)
{
	memset(&b->src, 0, sizeof b->src);
	b->src.res = res, b->src.pool = pool;
	return batch_finish(b);
}

/* same with the CIGARs gathered in problem order by the device (k_wfa_sched.hip): ncig[j] operators at ord + off[j] */
int mga_batch_finish_ordered(mga_batch_t *b, const int32_t *ncig, const int64_t *off, const uint32_t *ord)
{
	memset(&b->src, 0, sizeof b->src);
	b->src.ncig = ncig, b->src.off = off, b->src.ord = ord;
	return batch_finish(b);
}

static int batch_finish(mga_batch_t *b)
{
	if (!(b->opt.flag & MG_M_CIGAR)) return 0;
	b->err = 0;
	mga_parallel_for(b->n_threads, b->n, finish_worker, b);
	if (b->err == -1) mga_set_error("a gap came back from the WFA ladder without an alignment (status != OK): the ladder's last tier or its chained fallback (k_wfa_sched.hip: wfs_fallback, miniwfa.c:776-834) gave up on it");
	else if (b->err < 0) mga_set_error("stitched CIGAR is inconsistent with the chain coordinates");
	return b->err;
}

mg_gchains_t **mga_batch_take_results(mga_batch_t *b) { mg_gchains_t **r = b->gcs; b->gcs = 0; return r; }

void mga_batch_stats(const mga_batch_t *b, mga_stats_t *st)
{
	int t;
	for (t = 0; t < b->n_threads; ++t) st->wfa_t_bases += b->tp[t].wfa_t_bases, st->wfa_q_bases += b->tp[t].wfa_q_bases;
	st->n_wfa += b->tp_prob_base[b->n_threads];
}

void mga_batch_destroy(mga_batch_t *b)
{
	int i;
	if (b == 0) return;
	for (i = 0; i < b->n; ++i) { free(b->plan[i].item_off); free(b->plan[i].chain_id); }
	for (i = 0; i < b->n_threads; ++i) tpool_put(&b->tp[i]);
	if (b->gcs) { for (i = 0; i < b->n; ++i) mg_gchain_free(b->gcs[i]); free(b->gcs); }
	free(b->seg_len);
	free(b->plan); free(b->tp); free(b->tp_prob_base); free(b->tp_t_base); free(b->tp_item_base); free(b->tp_chain_base); free(b->tp_vert_base);
	free(b);
}

/* GAF text of one chunk: T pieces in read order; in text mode cg:Z / ds:Z are copied from the device's output.
 * Round 5: when the chunk is the NEXT one the job's output is waiting for (the usual case: chunks finish nearly in order), its lines are written STRAIGHT to their place in
 * the output buffer -- a measuring pass (the same formatter with empty payloads + the payload lengths the device reported) gives every piece its offset, the writing pass
 * formats into windows of the output (gaf.c: MGA_KS_WINDOW).  [measured, round 4] the text went device -> pinned staging -> piece -> output: two host copies of 1.1 GB per
 * 125 000 reads; now one.  A chunk that finishes ahead of its predecessors takes the old way (pieces, copied when its turn comes). */

void gaf_worker(void *data, int64_t t, int tid)
{
	gafw_t *w = (gafw_t*)data;
	mga_batch_t *bt = w->b;
	const int n = w->n;
	int64_t b = (int64_t)n * t / w->T, e = (int64_t)n * (t + 1) / w->T, i, payload = 0;
	kstring_t win, *out = &w->part[t];
	mga_chain_text_t *txt = 0;
	int32_t m_txt = 0;
	int64_t tc = cpu_now();
	(void)tid;
	if (w->mode == 2) { win.s = w->dst + w->off[t], win.l = 0, win.m = MGA_KS_WINDOW; out = &win; mga_gaf_window_limit((size_t)w->bytes[t]); }
	else if (w->mode == 0) { /* one allocation per piece: a base-aligned read prints about one byte per base (cg + ds), an unaligned one ~120 bytes */
		size_t est = 4096;
		for (i = b; i < e; ++i) est += (bt->opt.flag & MG_M_CIGAR) ? (size_t)bt->qlens[i] + 512 : 512;
		if (est < 0xfffffff0u && est > out->m) { size_t cap; char *p = strbuf_get(est, &cap); if (cap > 0xfffffff0u) cap = 0xfffffff0u; free(out->s); out->s = p, out->m = (unsigned)cap, out->l = 0; }
	} else out->l = 0; /* (measure: the piece's own buffer serves as scratch for the lines without their payloads) */
	for (i = b; i < e; ++i) {
		int32_t ql = bt->qlens[i], k;
		const mg_gchains_t *gcs = bt->gcs[i];
		const read_plan_t *pl = &bt->plan[i];
		const mga_chain_text_t *tx = 0;
		if (bt->txt_res && gcs && pl->chain_id) {
			if (gcs->n_gc > m_txt) { m_txt = gcs->n_gc + 8; txt = MGA_REALLOC(mga_chain_text_t, txt, m_txt); }
			for (k = 0; k < gcs->n_gc; ++k) {
				txt[k].cg = txt[k].ds = 0;
				if (pl->chain_id[k] >= 0) {
					const mga_txt_res_t *r = &bt->txt_res[pl->tid < 0 ? pl->chain_id[k] : bt->dp_n_chain + bt->tp_chain_base[pl->tid] + pl->chain_id[k]]; /* device-planned chains first, then the pools' */
					txt[k].cg = bt->txt_pool + r->txt_off, txt[k].ds = txt[k].cg + r->cg_len;
					txt[k].cg_len = r->cg_len, txt[k].ds_len = r->ds_len, txt[k].mlen = r->mlen, txt[k].blen = r->blen;
					if (w->mode == 1) { /* printed or not is the formatter's decision: count what it would copy by letting it copy nothing */
						if (!((gcs->gc[k].id != gcs->gc[k].parent && !(bt->opt.flag & MG_M_PRINT_2ND)) || gcs->gc[k].cnt == 0)) payload += (int64_t)r->cg_len + r->ds_len;
						txt[k].cg_len = txt[k].ds_len = 0;
					}
				}
			}
			tx = txt;
		}
		if (w->mode == 1 && out->l > (1u << 20)) { payload += out->l; out->l = 0; } /* (the scratch does not have to hold the whole piece) */
		mga_write_gaf_append(out, bt->gi->g, gcs, 1, &ql, bt->qnames ? bt->qnames[i] : "*", bt->opt.flag, tx);
		if (w->mode != 1) { mg_gchain_free(bt->gcs[i]); bt->gcs[i] = 0; }
	}
	if (w->mode == 1) { w->bytes[t] = payload + out->l; out->l = 0; }
	else if (w->mode == 2) {
		if ((int64_t)win.l != w->bytes[t]) { fprintf(stderr, "[E::%s] GAF piece %ld: %u bytes written where %ld were measured\n", __func__, (long)t, win.l, (long)w->bytes[t]); abort(); } /* the two passes run the same formatter: cannot happen, and must not go unnoticed */
	}
	free(txt);
	CPU_ADD(C_GAF, tc);
}
