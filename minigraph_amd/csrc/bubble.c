/*
 * bubble.c -- the bubbles of a reference graph for --call (gfa-bbl.c:11-33 gfa_sort_ref_arc, :85-169 gfa_scc1, :244-372 gfa_bubble), on this library's gfa_t alone.
 *
 * --call reads four things of a bubble: its stable sequence, the two stable offsets, and the vertex list v[0 .. n_seg) (v[0] the source stem, v[n_seg - 1] the sink).  The
 * shortest / longest walk, the path count and the two sequences of the reference's record are not made here.  What IS reproduced is the traversal order, because the order of
 * the bubbles, the "last bubble that lists a segment wins" of mg_call_asm and the two stems all follow from it:
 *   - one depth-first pass per stable sequence, from its rank-0 segment of smallest offset, forward strand; arcs in g->arc order (after mga_sort_ref_arc: reference arc first);
 *   - one state array over ALL passes: a vertex numbered by an earlier pass is never entered again, and a vertex whose complement is on the component stack is not entered;
 *   - a pass lists its vertices in the reverse of the order in which Tarjan's components pop them;
 *   - a bubble closes at list position j when no arc from [jst, j) reaches beyond j and the stable offset has advanced.
 */
#include <stdio.h>
#include "mga_host.h"

void mga_sort_ref_arc(gfa_t *g)
{
	const uint32_t n_vtx = gfa_n_vtx(g);
	uint32_t v;
	for (v = 0; v < n_vtx; ++v) {
		const gfa_seg_t *s = &g->seg[v >> 1];
		gfa_arc_t *av = gfa_arc_a(g, v), tmp;
		const int32_t nv = (int32_t)gfa_arc_n(g, v);
		int32_t i, hit = -1;
		if (s->rank != 0) continue;
		for (i = 0; i < nv && hit < 0; ++i) { /* the arc to the next (forward) / previous (reverse) piece of the same stable sequence */
			const uint32_t w = av[i].w;
			const gfa_seg_t *t = &g->seg[w >> 1];
			if (t->rank != 0 || t->snid != s->snid || ((v ^ w) & 1)) continue;
			if ((v & 1) == 0 ? s->soff + s->len == t->soff : t->soff + t->len == s->soff) hit = i;
		}
		if (hit > 0) tmp = av[hit], av[hit] = av[0], av[0] = tmp; /* (none found: the reference asserts; here the order stays) */
	}
}

typedef struct { uint32_t index, low, pos, start; uint8_t on_stack; } scc_vtx_t; /* index == UINT32_MAX: not numbered yet; pos: place in the pass's list; start: the pass's first vertex */

typedef struct {
	scc_vtx_t *a;
	uint32_t next_index;
	uint32_t *cs; int64_t n_cs, m_cs;    /* component stack */
	uint64_t *ds; int64_t n_ds, m_ds;    /* DFS stack: vertex << 32 | arcs already taken */
	uint32_t *list; int64_t n_list, m_list;
} scc_t;

/* one pass from v0: S->list[0 .. n_list) in the reference's order, S->a[].pos / .start filled for its vertices */
static void scc_pass(const gfa_t *g, scc_t *S, uint32_t v0)
{
	int64_t k;
	S->n_list = 0, S->n_ds = 0;
	MGA_GROW(uint64_t, S->ds, S->n_ds, S->m_ds);
	S->ds[S->n_ds++] = (uint64_t)v0 << 32;
	while (S->n_ds > 0) {
		const uint64_t x = S->ds[--S->n_ds];
		const uint32_t v = (uint32_t)(x >> 32), taken = (uint32_t)x, nv = gfa_arc_n(g, v);
		scc_vtx_t *pv = &S->a[v];
		if (taken == 0) { /* first visit */
			pv->index = pv->low = S->next_index++, pv->on_stack = 1;
			MGA_GROW(uint32_t, S->cs, S->n_cs, S->m_cs);
			S->cs[S->n_cs++] = v;
		}
		if (taken < nv) { /* the next arc */
			const uint32_t w = gfa_arc_a(g, v)[taken].w;
			S->ds[S->n_ds++] = (uint64_t)v << 32 | (taken + 1);
			if (S->a[w].index == UINT32_MAX && !S->a[w ^ 1].on_stack) {
				MGA_GROW(uint64_t, S->ds, S->n_ds, S->m_ds);
				S->ds[S->n_ds++] = (uint64_t)w << 32;
			} else if (S->a[w].on_stack && S->a[w].index < pv->low) pv->low = S->a[w].index;
			continue;
		}
		if (pv->low == pv->index) { /* v roots a component: pop it, top first */
			uint32_t w;
			do {
				w = S->cs[--S->n_cs];
				S->a[w].on_stack = 0;
				MGA_GROW(uint32_t, S->list, S->n_list, S->m_list);
				S->list[S->n_list++] = w;
			} while (w != v);
		}
		if (S->n_ds > 0) { /* hand v's low to the vertex that entered it */
			scc_vtx_t *pu = &S->a[S->ds[S->n_ds - 1] >> 32];
			if (pv->low < pu->low) pu->low = pv->low;
		}
	}
	for (k = 0; k < S->n_list >> 1; ++k) { const uint32_t t = S->list[k]; S->list[k] = S->list[S->n_list - 1 - k], S->list[S->n_list - 1 - k] = t; }
	for (k = 0; k < S->n_list; ++k) S->a[S->list[k]].start = v0, S->a[S->list[k]].pos = (uint32_t)k;
}

mga_bubble_t *mga_bubbles(const gfa_t *g, int32_t *n_bb, uint32_t **vpool)
{
	const uint32_t n_vtx = gfa_n_vtx(g);
	uint32_t i, *first = MGA_MALLOC(uint32_t, g->n_sseq + 1), *pool = 0;
	int64_t n_pool = 0, m_pool = 0, m_bb = 0;
	mga_bubble_t *bb = 0;
	scc_t S;
	*n_bb = 0, *vpool = 0;
	memset(&S, 0, sizeof S);
	S.a = MGA_CALLOC(scc_vtx_t, n_vtx + 1);
	for (i = 0; i < n_vtx; ++i) S.a[i].index = S.a[i].start = UINT32_MAX;
	for (i = 0; i < g->n_sseq; ++i) first[i] = UINT32_MAX;
	{ /* per stable sequence: the rank-0 segment of smallest offset (the first of equals) */
		uint32_t *lo = MGA_MALLOC(uint32_t, g->n_sseq + 1);
		for (i = 0; i < g->n_sseq; ++i) lo[i] = UINT32_MAX;
		for (i = 0; i < g->n_seg; ++i) {
			const gfa_seg_t *s = &g->seg[i];
			if (s->rank != 0 || s->snid < 0 || (uint32_t)s->snid >= g->n_sseq) continue;
			if ((uint32_t)s->soff < lo[s->snid]) lo[s->snid] = (uint32_t)s->soff, first[s->snid] = i << 1;
		}
		free(lo);
	}
	for (i = 0; i < g->n_sseq; ++i) {
		int64_t j, jst = 0, reach = -1;
		int32_t far = -1; /* largest stable offset of this sequence seen since jst */
		if (first[i] == UINT32_MAX) continue;
		scc_pass(g, &S, first[i]);
		for (j = 0; j < S.n_list; ++j) {
			const uint32_t v = S.list[j], nv = gfa_arc_n(g, v);
			const gfa_arc_t *av = gfa_arc_a(g, v);
			const gfa_seg_t *s = &g->seg[v >> 1];
			uint32_t k;
			if (j == reach && s->soff > far) {
				const gfa_seg_t *s0 = &g->seg[S.list[jst] >> 1];
				if (s0->snid == (int32_t)i && s->snid == (int32_t)i) {
					mga_bubble_t *b;
					int64_t q;
					MGA_GROW(mga_bubble_t, bb, *n_bb, m_bb);
					b = &bb[(*n_bb)++];
					b->snid = (int32_t)i, b->ss = s0->soff + s0->len, b->se = s->soff, b->n_seg = (int32_t)(j - jst + 1), b->v_off = n_pool;
					for (q = jst; q <= j; ++q) { MGA_GROW(uint32_t, pool, n_pool, m_pool); pool[n_pool++] = S.list[q]; }
				}
				reach = -1, far = -1, jst = j;
			}
			for (k = 0; k < nv; ++k) /* arcs that stay inside this pass */
				if (S.a[av[k].w].start == first[i] && (int64_t)S.a[av[k].w].pos > reach) reach = S.a[av[k].w].pos;
			if (s->snid == (int32_t)i && s->soff > far) far = s->soff;
		}
	}
	free(S.a); free(S.cs); free(S.ds); free(S.list); free(first);
	if (pool == 0) pool = MGA_CALLOC(uint32_t, 1);
	if (bb == 0) bb = MGA_CALLOC(mga_bubble_t, 1);
	*vpool = pool;
	return bb;
}

void mga_bubbles_free(mga_bubble_t *bb, uint32_t *vpool) { free(bb); free(vpool); }
