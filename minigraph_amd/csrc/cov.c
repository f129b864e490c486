/*
 * cov.c -- read coverage (--cov) around k_cov.hip: the job object that keeps the integer accumulators in HBM, the host instantiation of cov_core.h, the
 * final division, and gfa_aux_update_cv (gfa-base.c:475-503) for the caller's gfa_t.
 */
#include <stdio.h>
#include <stddef.h>
#include "mga_host.h"
#include "cov_core.h"

_Static_assert(sizeof(gfa_arc_t) == COV_ARC_BYTES && offsetof(gfa_arc_t, w) == COV_ARC_W, "cov_core.h reads gfa_arc_t::w by offset");
_Static_assert(sizeof(mga_cov_chain_t) == 32, "mga_cov_chain_t: one record is 32 bytes on both sides of PCIe");

/* ---- the job ---- */

mga_cov_job_t *mga_cov_job_open(const mg_idx_t *gi, const mg_mapopt_t *opt)
{
	const gfa_t *g = gi->g;
	mga_cov_job_t *J = MGA_CALLOC(mga_cov_job_t, 1);
	uint32_t s;
	J->n_seg = g->n_seg, J->n_arc = (int64_t)g->n_arc, J->min_mapq = opt->min_cov_mapq, J->min_blen = opt->min_cov_blen;
	J->G.seg_len = J->seg_len = MGA_MALLOC(int32_t, g->n_seg + 1); J->G.arc = g->arc; J->G.arc_idx = g->idx;
	for (s = 0; s < g->n_seg; ++s) J->seg_len[s] = g->seg[s].len;
	J->h_seg_bases = MGA_CALLOC(int64_t, J->n_seg + 1); J->h_link_cnt = MGA_CALLOC(int64_t, J->n_arc + 1);
	J->d_seg_bases = (int64_t*)mga_dmalloc((size_t)(J->n_seg + 1) * 8); J->d_link_cnt = (int64_t*)mga_dmalloc((size_t)(J->n_arc + 1) * 8); J->d_cnt = (int64_t*)mga_dmalloc(64);
	if (J->d_seg_bases == 0 || J->d_link_cnt == 0 || J->d_cnt == 0 || /* zeroed here, once per job; synchronous: every chunk's stream starts behind it */
		mga_dmemset(J->d_seg_bases, 0, (size_t)(J->n_seg + 1) * 8) < 0 || mga_dmemset(J->d_link_cnt, 0, (size_t)(J->n_arc + 1) * 8) < 0 || mga_dmemset(J->d_cnt, 0, 64) < 0 || mga_dsync() < 0) {
		mga_cov_job_close(J, 0, 0, 0);
		return 0;
	}
	return J;
}

/* the job ends: the device arrays come down (the one copy of the job) and are added, with what host threads counted, into the caller's arrays.
 * seg_bases == NULL: the job failed, release only */
int mga_cov_job_close(mga_cov_job_t *J, int64_t *seg_bases, int64_t *link_cnt, mga_cov_stats_t *st)
{
	int rc = 0;
	if (J == 0) return 0;
	if (seg_bases) {
		int64_t *t = MGA_MALLOC(int64_t, (J->n_seg > J->n_arc ? J->n_seg : J->n_arc) + 1), cnt[8], i;
		if (mga_dsync() < 0 || mga_d2h(t, J->d_seg_bases, (size_t)J->n_seg * 8) < 0) rc = -1;
		for (i = 0; rc == 0 && i < J->n_seg; ++i) seg_bases[i] += t[i] + J->h_seg_bases[i];
		if (rc == 0 && mga_d2h(t, J->d_link_cnt, (size_t)J->n_arc * 8) < 0) rc = -1;
		for (i = 0; rc == 0 && i < J->n_arc; ++i) link_cnt[i] += t[i] + J->h_link_cnt[i];
		if (rc == 0 && mga_d2h(cnt, J->d_cnt, 64) < 0) rc = -1;
		if (rc == 0 && st) {
			st->chains_counted += cnt[MGA_COV_CHAINS] + J->h_cnt[MGA_COV_CHAINS], st->links_counted += cnt[MGA_COV_LINKS] + J->h_cnt[MGA_COV_LINKS];
			st->links_skipped += cnt[MGA_COV_SKIPPED] + J->h_cnt[MGA_COV_SKIPPED];
		}
		free(t);
	}
	mga_dfree(J->d_seg_bases); mga_dfree(J->d_link_cnt); mga_dfree(J->d_cnt);
	free(J->h_seg_bases); free(J->h_link_cnt); free(J->seg_len); free(J);
	return rc;
}

/* ---- the host instantiation ---- */

static void cov_graph_of(const gfa_t *g, cov_graph_t *G, int32_t **seg_len)
{
	uint32_t s;
	*seg_len = MGA_MALLOC(int32_t, g->n_seg + 1);
	for (s = 0; s < g->n_seg; ++s) (*seg_len)[s] = g->seg[s].len;
	G->seg_len = *seg_len, G->arc = g->arc, G->arc_idx = g->idx;
}

/* one chain of a read as a record over the walk `v` (vert_beg = 0) */
static inline void cov_rec_of(const mg_gchain_t *gc, mga_cov_chain_t *c)
{
	c->vert_beg = 0, c->vert_cnt = gc->cnt, c->ps = gc->ps, c->pe = gc->pe, c->plen = gc->plen, c->mapq = (int32_t)gc->mapq, c->blen = gc->blen;
}

/* every chain of one read (cal_cov.c:13-17) into accumulators other threads may be adding to */
void mga_cov_read_host(const cov_graph_t *G, const mg_gchains_t *gt, int32_t min_mapq, int32_t min_blen, int64_t *seg_bases, int64_t *link_cnt, int64_t *cnt)
{
	uint32_t stack[256], *v = stack;
	int32_t i, j, m = 256;
	if (gt == 0) return;
	for (i = 0; i < gt->n_gc; ++i) {
		const mg_gchain_t *gc = &gt->gc[i];
		mga_cov_chain_t c;
		cov_rec_of(gc, &c);
		if (!cov_chain_counts(&c, min_mapq, min_blen)) continue;
		if (gc->cnt > m) { m = gc->cnt + (gc->cnt >> 1); v = v == stack ? MGA_MALLOC(uint32_t, m) : MGA_REALLOC(uint32_t, v, m); }
		for (j = 0; j < gc->cnt; ++j) v[j] = gt->lc[gc->off + j].v;
		cov_chain_host(G, &c, v, min_mapq, min_blen, seg_bases, link_cnt, cnt);
	}
	if (v != stack) free(v);
}

static void cov_stats_add(mga_cov_stats_t *st, const int64_t *cnt)
{
	if (st) st->chains_counted += cnt[MGA_COV_CHAINS], st->links_counted += cnt[MGA_COV_LINKS], st->links_skipped += cnt[MGA_COV_SKIPPED];
}

void mga_cov_gchains(const gfa_t *g, const mg_gchains_t *gt, int32_t min_mapq, int32_t min_blen, int64_t *seg_bases, int64_t *link_cnt, mga_cov_stats_t *st)
{
	cov_graph_t G;
	int32_t *seg_len;
	int64_t cnt[MGA_COV_N_CNT] = { 0, 0, 0 };
	cov_graph_of(g, &G, &seg_len);
	mga_cov_read_host(&G, gt, min_mapq, min_blen, seg_bases, link_cnt, cnt);
	cov_stats_add(st, cnt);
	free(seg_len);
}

void mga_cov_chains_host(const gfa_t *g, int n_chain, const mga_cov_chain_t *chain, const uint32_t *vert, int32_t min_mapq, int32_t min_blen,
						 int64_t *seg_bases, int64_t *link_cnt, mga_cov_stats_t *st)
{
	cov_graph_t G;
	int32_t *seg_len;
	int64_t cnt[MGA_COV_N_CNT] = { 0, 0, 0 };
	int i;
	cov_graph_of(g, &G, &seg_len);
	for (i = 0; i < n_chain; ++i) cov_chain_host(&G, &chain[i], vert, min_mapq, min_blen, seg_bases, link_cnt, cnt);
	cov_stats_add(st, cnt);
	free(seg_len);
}

/* ---- the job's end: the reference's doubles, once ---- */

void mga_cov_finish(const gfa_t *g, const int64_t *seg_bases, const int64_t *link_cnt, double *cov_seg, double *cov_link)
{
	uint64_t k;
	uint32_t i;
	for (i = 0; cov_seg && i < g->n_seg; ++i) cov_seg[i] = (double)seg_bases[i] / g->seg[i].len; /* (a segment of length 0 carries no chain: 0 / 0 = NaN here, 0.0 in the reference) */
	for (i = 0; cov_seg && i < g->n_seg; ++i) if (g->seg[i].len == 0) cov_seg[i] = 0.0;
	for (k = 0; cov_link && k < g->n_arc; ++k) cov_link[k] = (double)link_cnt[k];
}

/* ---- gfa_aux_update_cv ---- */

static const uint8_t *aux_skip(const uint8_t *s) /* behind the value whose type byte s points at */
{
	const int type = *s++;
	if (type == 'Z') { while (*s) ++s; return s + 1; }
	if (type == 'B') { const int sub = *s; int32_t n; memcpy(&n, s + 1, 4); return s + 5 + (size_t)(sub == 'C' || sub == 'c' || sub == 'A' ? 1 : sub == 'S' || sub == 's' ? 2 : sub == 'I' || sub == 'i' || sub == 'f' ? 4 : 0) * n; }
	return s + (type == 'C' || type == 'c' || type == 'A' ? 1 : type == 'S' || type == 's' ? 2 : type == 'I' || type == 'i' || type == 'f' ? 4 : 0);
}

/* gfa_aux_update_f: whatever `tag` is, the tag LOOKED FOR is cv; found: its value bytes are overwritten (the type byte stays); else tag:f:x is appended */
static void aux_update_f(gfa_aux_t *a, const char tag[2], float x)
{
	const uint8_t *s = a->aux, *e = a->aux + a->l_aux;
	while (a->l_aux > 0 && s < e) {
		if (s[0] == 'c' && s[1] == 'v') { memcpy((uint8_t*)s + 3, &x, 4); return; }
		s = aux_skip(s + 2);
	}
	if (a->l_aux + 7 + 1 > a->m_aux) { /* (kstring's ks_resize: room for l + 7, rounded up to a power of two) */
		uint32_t m = a->l_aux + 7;
		--m; m |= m >> 1; m |= m >> 2; m |= m >> 4; m |= m >> 8; m |= m >> 16; ++m;
		a->aux = MGA_REALLOC(uint8_t, a->aux, m), a->m_aux = m;
	}
	a->aux[a->l_aux] = (uint8_t)tag[0], a->aux[a->l_aux + 1] = (uint8_t)tag[1], a->aux[a->l_aux + 2] = 'f';
	memcpy(a->aux + a->l_aux + 3, &x, 4);
	a->l_aux += 7;
}

void mga_gfa_aux_update_cv(gfa_t *g, const char *tag, const double *cov_seg, const double *cov_link)
{
	uint64_t k;
	uint32_t i;
	for (i = 0; cov_seg && i < g->n_seg; ++i) aux_update_f(&g->seg[i].aux, tag, (float)cov_seg[i]);
	for (k = 0; cov_link && k < g->n_arc; ++k)
		if (g->arc[k].comp == 0) aux_update_f(&g->link_aux[g->arc[k].link_id], tag, (float)cov_link[k]);
}
