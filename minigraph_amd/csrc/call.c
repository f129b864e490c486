/*
 * call.c -- bubble alleles (--call) around k_call.hip: the interval index of mg_gc_index (ggsimple.c:11-101) reduced to what mg_call_asm reads, the chains flattened into the
 * records of call_core.h, the host instantiation, the pick of each bubble's winner, the BED text (asm-call.c:117-140) and the file-level job (ggen.c:128-139).
 */
#include <stdio.h>
#include "mga_host.h"
#include "call_core.h"

_Static_assert(sizeof(mga_call_seg_t) == 8 && sizeof(mga_call_pos_t) == 16 && sizeof(mga_call_chain_t) == 24 && sizeof(mga_call_intv_t) == 8 &&
			   sizeof(mga_call_cand_t) == 40 && sizeof(mga_call_warn_t) == 32, "the records of the call stage have one layout on both sides of PCIe");

static double g_call_t[6];
void mga_call_times(double t[6]) { memcpy(t, g_call_t, sizeof g_call_t); }

/* ---- picking the winners, ordering the warnings (shared by the device and the host entry) ---- */

/* per bubble the candidate of largest key; best != NULL: the keys the device's atomic maximum left -- a record is kept only when it carries that key */
int mga_call_pick(int32_t n_bb, int64_t n_cand, const mga_call_cand_t *cand, const uint64_t *best, mga_call_cand_t *win)
{
	int64_t k;
	int32_t b, rc = 0;
	memset(win, 0, (size_t)n_bb * sizeof *win);
	for (k = 0; k < n_cand; ++k) {
		const mga_call_cand_t *c = &cand[k];
		if (c->bid < 0 || c->bid >= n_bb) { rc = -1; continue; }
		if (best ? c->key == best[c->bid] : c->key > win[c->bid].key) win[c->bid] = *c;
	}
	for (b = 0; best && b < n_bb; ++b) if (best[b] != win[b].key) rc = -1; /* a maximum without its record */
	return rc;
}

static int warn_cmp(const void *a, const void *b)
{
	const uint64_t x = ((const mga_call_warn_t*)a)->key, y = ((const mga_call_warn_t*)b)->key;
	return x < y ? -1 : x > y;
}
void mga_call_sort_warn(int64_t n, mga_call_warn_t *w) { if (n > 1) qsort(w, (size_t)n, sizeof *w, warn_cmp); }

/* what both batch entries refuse before anything is followed */
int mga_call_batch_check(int n_chain, const mga_call_chain_t *chain, int64_t n_pos, const mga_call_pos_t *pos, uint32_t n_seg, const mga_call_seg_t *seg,
						 int n_seq, const int64_t *q_off, int32_t n_bb)
{
	int64_t k;
	int i;
	uint32_t s;
	for (i = 0; i < n_chain; ++i) {
		const mga_call_chain_t *c = &chain[i];
		if (c->cnt < 0 || c->pos_beg < 0 || c->pos_beg + c->cnt > n_pos) { mga_set_error("call: chain %d points outside the %ld walk positions", i, (long)n_pos); return -1; }
		if (c->t < 0 || c->t >= n_seq) { mga_set_error("call: chain %d names sequence %d of %d", i, c->t, n_seq); return -1; }
	}
	for (k = 0; k < n_pos; ++k) if ((pos[k].v >> 1) >= n_seg) { mga_set_error("call: walk position %ld names segment %u of %u", (long)k, pos[k].v >> 1, n_seg); return -1; }
	for (s = 0; s < n_seg; ++s) if (seg[s].bid < 0 || (seg[s].bid >= n_bb && (seg[s].bid != 0 || seg[s].is_stem))) { /* (a segment no bubble lists carries 0, also in a graph without bubbles) */ mga_set_error("call: segment %u carries bubble %d of %d", s, seg[s].bid, n_bb); return -1; }
	for (i = 0; i < n_seq; ++i) if (q_off[i] < 0 || q_off[i + 1] < q_off[i]) { mga_set_error("call: the query intervals of sequence %d are not a range", i); return -1; }
	return 0;
}

int mga_call_batch_host(int n_chain, const mga_call_chain_t *chain, int64_t n_pos, const mga_call_pos_t *pos, uint32_t n_seg, const mga_call_seg_t *seg, const int32_t *seg_len,
						int n_seq, const int64_t *q_off, const mga_call_intv_t *qintv, int32_t n_bb, mga_call_cand_t *win, mga_call_warn_t **warn, int64_t *n_warn)
{
	mga_call_cand_t *cand;
	mga_call_warn_t *w;
	int64_t n_cand = 0, nw = 0;
	int i, rc;
	*warn = 0, *n_warn = 0;
	if (mga_call_batch_check(n_chain, chain, n_pos, pos, n_seg, seg, n_seq, q_off, n_bb) < 0) return -1;
	cand = MGA_MALLOC(mga_call_cand_t, n_pos + 1), w = MGA_MALLOC(mga_call_warn_t, n_pos + 1);
	for (i = 0; i < n_chain; ++i) call_chain_host(&chain[i], pos, n_pos, seg, seg_len, n_seg, q_off, qintv, cand, &n_cand, w, &nw);
	rc = mga_call_pick(n_bb, n_cand, cand, 0, win);
	free(cand);
	mga_call_sort_warn(nw, w);
	*warn = w, *n_warn = nw;
	return rc;
}

/* ---- mg_call_asm ---- */

typedef struct {
	int32_t n_bb; mga_bubble_t *bb; uint32_t *bv;
	mga_call_seg_t *seg; int32_t *seg_len;
	int64_t *q_off; mga_call_intv_t *qintv;
	mga_call_chain_t *chain; int n_chain;
	mga_call_pos_t *pos; int64_t n_pos;
} call_job_t;

static void call_job_free(call_job_t *J)
{
	mga_bubbles_free(J->bb, J->bv);
	free(J->seg); free(J->seg_len); free(J->q_off); free(J->qintv); free(J->chain); free(J->pos);
}

static inline int chain_indexed(const mg_gchain_t *gc, int32_t min_mapq, int32_t min_blen) { return gc->id == gc->parent && gc->blen >= min_blen && (int32_t)gc->mapq >= min_mapq; }

/* mg_gc_index: the query intervals per sequence, and per segment only HOW MANY of its intervals overlap [0, len) -- capped at 2, which is all asm-call.c:78-80 reads.
 * Returns the largest anchor count of an indexed chain (0: nothing is indexed). */
static int32_t call_index(const gfa_t *g, int32_t n_seq, mg_gchains_t *const *gcs, int32_t min_mapq, int32_t min_blen, call_job_t *J, uint8_t *n_on_seg)
{
	int32_t t, i, j, max_acnt = 0;
	int64_t n = 0;
	J->q_off = MGA_CALLOC(int64_t, n_seq + 1);
	for (t = 0; t < n_seq; ++t) {
		const mg_gchains_t *gt = gcs[t];
		for (i = 0; gt && i < gt->n_gc; ++i) if (chain_indexed(&gt->gc[i], min_mapq, min_blen)) ++n;
		J->q_off[t + 1] = n;
	}
	J->qintv = MGA_MALLOC(mga_call_intv_t, n + 1);
	for (t = 0, n = 0; t < n_seq; ++t) {
		const mg_gchains_t *gt = gcs[t];
		for (i = 0; gt && i < gt->n_gc; ++i) {
			const mg_gchain_t *gc = &gt->gc[i];
			if (!chain_indexed(gc, min_mapq, min_blen)) continue;
			if (gc->n_anchor > max_acnt) max_acnt = gc->n_anchor;
			J->qintv[n].st = gc->qs, J->qintv[n].en = gc->qe, ++n;
			for (j = 0; j < gc->cnt; ++j) { /* the interval on the forward strand of the segment (ggsimple.c:62-80) */
				const mg_llchain_t *lc = &gt->lc[gc->off + j];
				const int32_t len = g->seg[lc->v >> 1].len;
				int32_t rs = 0, re = len;
				if (lc->cnt > 0) {
					const mg128_t *q0 = &gt->a[lc->off], *q1 = &gt->a[lc->off + lc->cnt - 1];
					if (j == 0) rs = gc->p ? gc->p->ss : (int32_t)q0->x + 1 - (int32_t)(q0->y >> 32 & 0xff);
					if (j == gc->cnt - 1) re = gc->p ? gc->p->ee : (int32_t)q1->x;
					if (lc->v & 1) { const int32_t tmp = rs; rs = len - re, re = len - tmp; }
				}
				if (rs < len && 0 < re && n_on_seg[lc->v >> 1] < 2) ++n_on_seg[lc->v >> 1];
			}
		}
	}
	return max_acnt;
}

static void call_segments(const gfa_t *g, call_job_t *J, const uint8_t *n_on_seg)
{
	uint32_t s;
	int32_t i, j;
	J->seg = MGA_CALLOC(mga_call_seg_t, g->n_seg + 1), J->seg_len = MGA_MALLOC(int32_t, g->n_seg + 1);
	for (s = 0; s < g->n_seg; ++s) J->seg_len[s] = g->seg[s].len, J->seg[s].over = n_on_seg[s] > 1;
	for (i = 0; i < J->n_bb; ++i) { /* asm-call.c:37-45 */
		const mga_bubble_t *b = &J->bb[i];
		const uint32_t *v = J->bv + b->v_off;
		for (j = 0; j < b->n_seg; ++j) J->seg[v[j] >> 1].bid = i;
		J->seg[v[0] >> 1].is_stem = J->seg[v[b->n_seg - 1] >> 1].is_stem = 1;
		J->seg[v[0] >> 1].is_src = 1;
	}
}

/* EVERY chain of every sequence (asm-call.c:47-52), in (t, i) order */
static void call_flatten(int32_t n_seq, mg_gchains_t *const *gcs, call_job_t *J)
{
	int32_t t, i, j;
	int64_t n_pos = 0;
	int n_chain = 0;
	for (t = 0; t < n_seq; ++t)
		for (i = 0; gcs[t] && i < gcs[t]->n_gc; ++i) ++n_chain, n_pos += gcs[t]->gc[i].cnt > 0 ? gcs[t]->gc[i].cnt : 0;
	J->chain = MGA_MALLOC(mga_call_chain_t, n_chain + 1), J->pos = MGA_MALLOC(mga_call_pos_t, n_pos + 1);
	J->n_chain = 0, J->n_pos = 0;
	for (t = 0; t < n_seq; ++t) {
		const mg_gchains_t *gt = gcs[t];
		for (i = 0; gt && i < gt->n_gc; ++i) {
			const mg_gchain_t *gc = &gt->gc[i];
			mga_call_chain_t *c = &J->chain[J->n_chain];
			c->pos_beg = J->n_pos, c->cnt = gc->cnt > 0 ? gc->cnt : 0, c->lc_off = gc->off, c->t = t, c->ord = J->n_chain++;
			for (j = 0; j < c->cnt; ++j) {
				const mg_llchain_t *lc = &gt->lc[gc->off + j];
				mga_call_pos_t *p = &J->pos[J->n_pos++];
				int64_t last = (int64_t)lc->off + lc->cnt - 1, first = lc->off; /* (cnt == 0: the anchor in front, as the reference reads it) */
				if (last < 0) last = 0;
				if (last >= gt->n_a) last = gt->n_a - 1;
				if (first >= gt->n_a) first = gt->n_a - 1;
				p->v = lc->v;
				if (gt->n_a > 0) p->yl1 = (int32_t)gt->a[last].y + 1, p->yf1 = (int32_t)gt->a[first].y + 1, p->span = (int32_t)(gt->a[first].y >> 32 & 0xff);
				else p->yl1 = p->yf1 = 1, p->span = 0;
			}
		}
	}
}

static void call_write_bed(const gfa_t *g, const call_job_t *J, const char *const *qnames, mg_gchains_t *const *gcs, const mga_call_cand_t *win, kstring_t *out)
{
	int32_t i, j;
	for (i = 0; i < J->n_bb; ++i) {
		const mga_bubble_t *b = &J->bb[i];
		const uint32_t v0 = J->bv[b->v_off], v1 = J->bv[b->v_off + b->n_seg - 1];
		const mga_call_cand_t *a = &win[i];
		mg_sprintf_lite(out, "%s\t%d\t%d\t%c%s\t%c%s\t", g->sseq[b->snid].name, b->ss, b->se, "><"[v0 & 1], g->seg[v0 >> 1].name, "><"[v1 & 1], g->seg[v1 >> 1].name);
		if (a->key != 0) {
			const mg_llchain_t *lc = gcs[a->t]->lc;
			if (a->st == a->en) mg_sprintf_lite(out, "*");
			else if (a->strand > 0) for (j = a->st; j < a->en; ++j) mg_sprintf_lite(out, "%c%s", "><"[lc[j].v & 1], g->seg[lc[j].v >> 1].name);
			else for (j = a->en - 1; j >= a->st; --j) mg_sprintf_lite(out, "%c%s", "<>"[lc[j].v & 1], g->seg[lc[j].v >> 1].name);
			mg_sprintf_lite(out, ":%d:%c:%s:%d:%d", a->glen, a->strand > 0 ? '+' : '-', qnames[a->t], a->qs, a->qe);
		} else mg_sprintf_lite(out, ".");
		mg_sprintf_lite(out, "\n");
	}
}

static int call_asm(const gfa_t *g, int on_device, int32_t n_seq, const char *const *qnames, mg_gchains_t *const *gcs, int32_t min_mapq, int32_t min_blen, kstring_t *out)
{
	call_job_t J;
	uint8_t *n_on_seg;
	mga_call_cand_t *win;
	mga_call_warn_t *warn = 0;
	int64_t n_warn = 0, k;
	double t0;
	int rc;
	memset(&J, 0, sizeof J);
	g_call_t[2] = g_call_t[3] = g_call_t[4] = g_call_t[5] = 0.0;
	if (on_device && mga_dev_init() < 0) return -1; /* no quiet host run in place of the kernel */
	t0 = mga_wtime();
	n_on_seg = MGA_CALLOC(uint8_t, g->n_seg + 1);
	if (call_index(g, n_seq, gcs, min_mapq, min_blen, &J, n_on_seg) == 0) { free(n_on_seg); call_job_free(&J); return 0; } /* nothing indexed: nothing printed (asm-call.c:32) */
	g_call_t[3] = mga_wtime() - t0, t0 = mga_wtime();
	J.bb = mga_bubbles(g, &J.n_bb, &J.bv);
	g_call_t[2] = mga_wtime() - t0, t0 = mga_wtime();
	call_segments(g, &J, n_on_seg);
	free(n_on_seg);
	call_flatten(n_seq, gcs, &J);
	g_call_t[3] += mga_wtime() - t0, t0 = mga_wtime();
	win = MGA_CALLOC(mga_call_cand_t, J.n_bb + 1);
	rc = (on_device ? mga_call_batch : mga_call_batch_host)(J.n_chain, J.chain, J.n_pos, J.pos, g->n_seg, J.seg, J.seg_len, n_seq, J.q_off, J.qintv, J.n_bb, win, &warn, &n_warn);
	g_call_t[4] = mga_wtime() - t0, t0 = mga_wtime();
	for (k = 0; rc == 0 && k < n_warn; ++k) /* the reference's two texts (asm-call.c:92-93,106-107), in its order */
		fprintf(stderr, "[W::mg_call_asm] type-%d folded inversion alignment around %c%s <=> %s:%d-%d\n", warn[k].type, "><"[warn[k].v & 1], g->seg[warn[k].v >> 1].name,
				qnames[warn[k].t], warn[k].qs, warn[k].qe);
	if (rc == 0) call_write_bed(g, &J, qnames, gcs, win, out);
	g_call_t[5] = mga_wtime() - t0;
	mga_free(warn); free(win);
	call_job_free(&J);
	return rc;
}

int mga_call_asm(const mg_idx_t *gi, int32_t n_seq, const char *const *qnames, mg_gchains_t *const *gcs, int32_t min_mapq, int32_t min_blen, kstring_t *out)
{
	return call_asm(gi->g, 1, n_seq, qnames, gcs, min_mapq, min_blen, out);
}

int mga_call_asm_host(const gfa_t *g, int32_t n_seq, const char *const *qnames, mg_gchains_t *const *gcs, int32_t min_mapq, int32_t min_blen, kstring_t *out)
{
	return call_asm(g, 0, n_seq, qnames, gcs, min_mapq, min_blen, out);
}

/* ---- mg_ggen_call ---- */

int mga_reads_read_host(const char *fn, int *n, int **qlens, char ***seqs, char ***names); /* mapfiles.c: every record of a FASTA/FASTQ(.gz) file, normalized as the mapper reads them */

int mga_call_files(gfa_t *g, const char *fn, const mg_idxopt_t *ipt, const mg_mapopt_t *opt0, const mg_ggopt_t *gpt, int n_threads, FILE *fp)
{
	mg_mapopt_t opt = *opt0;
	mg_idx_t *gi;
	mg_gchains_t **gcs = 0;
	kstring_t out = { 0, 0, 0 };
	int n = 0, *qlens = 0, i, rc = -1;
	char **seqs = 0, **names = 0;
	double t0 = mga_wtime(), t_idx, t_map;
	if (g == 0) return -1;
	if (opt.flag & MG_M_FRAG_MODE) { mga_set_error("--frag (multi-segment fragments) is outside the MI355X long-read path"); return -1; }
	if (n_threads < 1) n_threads = 1;
	mga_sort_ref_arc(g);
	if ((gi = mg_index(g, ipt, n_threads, &opt)) == 0) return -1;
	t_idx = mga_wtime() - t0, t0 = mga_wtime();
	if (mga_reads_read_host(fn, &n, &qlens, &seqs, &names) < 0) goto end;
	gcs = MGA_CALLOC(mg_gchains_t*, n + 1);
	if (n > 0 && mg_map_batch(gi, n, qlens, (const char**)seqs, (const char**)names, gcs, &opt, n_threads) < 0) goto end;
	t_map = mga_wtime() - t0;
	rc = mga_call_asm(gi, n, (const char *const*)names, gcs, gpt->min_mapq, gpt->min_map_len, &out);
	g_call_t[0] = t_idx, g_call_t[1] = t_map;
	if (rc == 0 && out.l > 0 && fwrite(out.s, 1, out.l, fp) != out.l) { mga_set_error("mga_call_files: short write"); rc = -1; }
end:
	for (i = 0; i < n; ++i) { if (gcs && gcs[i]) mg_gchain_free(gcs[i]); free(seqs[i]); free(names[i]); }
	free(gcs); free(seqs); free(names); free(qlens); free(out.s);
	mg_idx_destroy(gi);
	return rc;
}
