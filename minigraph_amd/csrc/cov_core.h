/*
 * cov_core.h -- read coverage (--cov: cal_cov.c:8-53) of ONE graph chain, as integer arithmetic that runs on a GPU lane and on a host thread
 * from the same source.
 *
 * The reference adds (double)(e - s) / len per (chain, segment) and 1.0 per link in read order and stores each sum as a float.  Here the SUMS are
 * integers -- covered bases per segment, traversals per arc -- and the division happens once, when the job ends (mga_cov_finish): an integer sum
 * depends on neither the order of the atomics, nor the chunking, nor the number of ranks.
 *
 * Per counted chain with the walk v[0 .. cnt) (cal_cov.c:19-26 in the chain's own coordinates, gchain1.c:258-292: ps = first anchor's start on
 * the first segment, plen - pe = what the walk has left behind the last anchor on the last segment):
 *   first segment: s = ps; last segment: e = len(last) - (plen - pe); every other boundary is a segment's end.  cnt == 1: pe - ps.
 *   link j >= 1: a01 = arc v[j-1] -> v[j], a10 = arc v[j]^1 -> v[j-1]^1 (gfa-priv.h:141-148: exactly one matching arc, else "skip"); both are
 *   bumped, or neither.
 * The is_skip branch of cal_cov.c:34-39 compares the READ-segment ids of two anchors (mg_seg_id): with single-segment reads both are 0 and the
 * branch is never taken, so no anchor is needed here.  Multi-segment fragments (MG_M_FRAG_MODE) stay refused.
 * A chain counts when mapq >= min_cov_mapq && blen >= min_cov_blen; blen is the chain record's (cal_cov.c:17 reads gc->blen, which base
 * alignment never updates: galign.c:127-138 fills gc->p only), so -c does not change a coverage.
 *
 * No libm, no floating point.
 */
#ifndef MGA_COV_CORE_H
#define MGA_COV_CORE_H

#include <stdint.h>
#include "../../include/minigraph_amd.h"

#if defined(__HIPCC__)
#define COV_HD __host__ __device__ inline
#else
#define COV_HD static inline
#endif

/* (mga_cov_chain_t -- one graph chain of a read: its walk and what the filter and the two partial segments need -- is public: include/minigraph_amd.h) */
/* the graph: segment lengths, gfa_arc_t[] in the host's order, per-vertex arc index (offset << 32 | count) */
typedef struct { const int32_t *seg_len; const void *arc; const uint64_t *arc_idx; } cov_graph_t;
enum { MGA_COV_CHAINS = 0, MGA_COV_LINKS, MGA_COV_SKIPPED, MGA_COV_N_CNT }; /* chains counted, links counted (both arcs each), links skipped (none or several arcs: the reference's "[W] Multi/disconnected link") */

#define COV_ARC_BYTES 32 /* sizeof(gfa_arc_t); its w at byte 8 (cov.c asserts both) */
#define COV_ARC_W 8

COV_HD int cov_chain_counts(const mga_cov_chain_t *c, int32_t min_mapq, int32_t min_blen) { return c->vert_cnt > 0 && c->mapq >= min_mapq && c->blen >= min_blen; }

/* gfa_find_arc: index of the only arc v -> w; -1 none, -2 several */
COV_HD int64_t cov_find_arc(const cov_graph_t *G, uint32_t v, uint32_t w)
{
	const uint64_t x = G->arc_idx[v];
	const uint32_t n = (uint32_t)x;
	const int64_t off = (int64_t)(x >> 32);
	const char *a = (const char*)G->arc + off * COV_ARC_BYTES + COV_ARC_W;
	uint32_t i, nw = 0;
	int64_t k = -1;
	for (i = 0; i < n; ++i)
		if (*(const uint32_t*)(a + (int64_t)i * COV_ARC_BYTES) == w) ++nw, k = off + i;
	return nw == 1 ? k : nw == 0 ? -1 : -2;
}

/* bases of segment v[j] >> 1 that the chain covers */
COV_HD int32_t cov_vertex_bases(const cov_graph_t *G, const mga_cov_chain_t *c, uint32_t vj, int32_t j)
{
	const int32_t len = G->seg_len[vj >> 1];
	const int32_t s = j == 0 ? c->ps : 0, e = j == c->vert_cnt - 1 ? len - (c->plen - c->pe) : len;
	return e - s;
}

/* the link in front of v[j] (j >= 1): 1 and both arcs, or 0 */
COV_HD int cov_vertex_link(const cov_graph_t *G, uint32_t vprev, uint32_t vj, int64_t *a01, int64_t *a10)
{
	*a01 = cov_find_arc(G, vprev, vj);
	*a10 = cov_find_arc(G, vj ^ 1, vprev ^ 1);
	return *a01 >= 0 && *a10 >= 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* the host instantiation: one chain into accumulators that other threads may be adding to */
static inline void cov_chain_host(const cov_graph_t *G, const mga_cov_chain_t *c, const uint32_t *vert, int32_t min_mapq, int32_t min_blen,
								  int64_t *seg_bases, int64_t *link_cnt, int64_t *cnt)
{
	const uint32_t *v = vert + c->vert_beg;
	int32_t j;
	if (!cov_chain_counts(c, min_mapq, min_blen)) return;
	__sync_fetch_and_add(&cnt[MGA_COV_CHAINS], 1);
	for (j = 0; j < c->vert_cnt; ++j) {
		int64_t a01, a10;
		__sync_fetch_and_add(&seg_bases[v[j] >> 1], (int64_t)cov_vertex_bases(G, c, v[j], j));
		if (j == 0) continue;
		if (cov_vertex_link(G, v[j - 1], v[j], &a01, &a10)) {
			__sync_fetch_and_add(&link_cnt[a01], 1); __sync_fetch_and_add(&link_cnt[a10], 1);
			__sync_fetch_and_add(&cnt[MGA_COV_LINKS], 1);
		} else __sync_fetch_and_add(&cnt[MGA_COV_SKIPPED], 1);
	}
}
#endif

#endif
