/*
 * call_core.h -- bubble alleles (--call: mg_call_asm, asm-call.c:47-115) of ONE graph chain over flat records, from one source for a GPU wavefront and a host thread.
 *
 * The walk of a chain is v[0 .. cnt).  With stem(j) = "segment v[j] >> 1 is the first or last vertex of a bubble", the reference's scan over j = 1 .. cnt - 1 is
 *   stem(j-1) && !stem(j):  st = j                      (a non-stem run opens)
 *   stem(j-1) &&  stem(j):  st = en = j, a candidate    (two adjacent stems: a deletion)
 *  !stem(j-1) &&  stem(j):  en = j, a candidate if st was ever set in this chain
 * st is never cleared inside a chain, so at every j it is the LARGEST j' <= j with stem(j' - 1): a running maximum, which a wavefront takes as a scan (k_call.hip) and a host
 * thread as a variable.  st and en are reported as the reference holds them, as indices into the read's lc[] (chain's lc offset + j).
 *
 * A candidate [st, en) is judged from (the order of the tests is the reference's; the first that fails decides what is reported):
 *   qs = (int32)y_last(st - 1) + 1, qe = (int32)y_first(en) + 1 - span(st)    anchors around the flanks (asm-call.c:68-70); qe < qs when the flanks overlap on the query
 *   1. more than one indexed interval of the query overlaps [qs, qe)           dropped    (a.st < qe && qs < a.en, counted directly: only "> 1" is read)
 *   2. a segment of [st, en) carries more than one indexed interval            dropped    (a per-segment flag; glen = the int32 sum of the segment lengths of [st, en))
 *   3. bubble ids of the flanks A = v[st - 1], B = v[en]: A < B strand +, A > B strand -, equal: is_src(A) + is_src(B) must be 1 (else warning type 1), strand + iff is_src(A)
 *   4. every segment of [st, en) must carry the bubble id of the + flank       else warning type 2
 * 2. and 4. are range questions over [st, en): differences of running sums (lengths, flags, "bubble id differs from the previous position's").
 * What survives competes for its bubble by the ORDER KEY chain ordinal << 32 | j: the reference overwrites ba[bid] in (t, i, j) order, so the largest key wins.
 *
 * No floating point.
 */
#ifndef MGA_CALL_CORE_H
#define MGA_CALL_CORE_H

#include <stdint.h>
#include "../../include/minigraph_amd.h"

#if defined(__HIPCC__)
#define CALL_HD __host__ __device__ inline
#else
#define CALL_HD static inline
#endif

/* (mga_call_seg_t, mga_call_pos_t, mga_call_chain_t, mga_call_intv_t, mga_call_cand_t, mga_call_warn_t are public: include/minigraph_amd.h) */
enum { MGA_CALL_DROP = 0, MGA_CALL_KEEP = 1, MGA_CALL_WARN1 = 2, MGA_CALL_WARN2 = 3 };

CALL_HD int call_intv_hit(const mga_call_intv_t *a, int32_t qs, int32_t qe) { return a->st < qe && qs < a->en; }

/* does position j >= 1 set st (to j)? */
CALL_HD int call_sets_st(int stem_prev) { return stem_prev; }
/* does position j >= 1 close a candidate, given st after position j's own update (-1: never set; local to the chain) */
CALL_HD int call_closes(int stem, int stem_prev, int32_t st) { return stem && (stem_prev || st >= 1); }

/* tests 1-4 for one candidate.  n_q: query intervals overlapping [qs, qe), capped at 2; n_over: over-covered segments in [st, en); A, B: the flanks; bid_st: bubble id at st;
 * n_change: positions k in (st, en) whose bubble id differs from that of k - 1; len = en - st */
CALL_HD int call_judge(int n_q, int32_t n_over, const mga_call_seg_t A, const mga_call_seg_t B, int32_t bid_st, int32_t n_change, int32_t len, int32_t *strand, int32_t *bid)
{
	if (n_q > 1) return MGA_CALL_DROP;
	if (n_over > 0) return MGA_CALL_DROP;
	if (A.bid < B.bid) *strand = 1;
	else if (A.bid > B.bid) *strand = -1;
	else {
		if (A.is_src + B.is_src != 1) return MGA_CALL_WARN1;
		*strand = A.is_src ? 1 : -1;
	}
	*bid = *strand > 0 ? A.bid : B.bid;
	if (len > 0 && (bid_st != *bid || n_change != 0)) return MGA_CALL_WARN2;
	return MGA_CALL_KEEP;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* the host instantiation: one chain, records appended in j order.  cand / warn have room for cnt records each (a position closes at most one candidate).
 * Returns 0, or -1 when the chain points outside the arrays. */
static inline int call_chain_host(const mga_call_chain_t *C, const mga_call_pos_t *pos, int64_t n_pos, const mga_call_seg_t *seg, const int32_t *seg_len, uint32_t n_seg,
								  const int64_t *q_off, const mga_call_intv_t *qintv, mga_call_cand_t *cand, int64_t *n_cand, mga_call_warn_t *warn, int64_t *n_warn)
{
	const mga_call_pos_t *p = pos + C->pos_beg;
	const mga_call_intv_t *qa = qintv + q_off[C->t];
	const int64_t n_qa = q_off[C->t + 1] - q_off[C->t];
	int32_t j, st = -1;
	uint32_t len_at_st = 0; /* running sums at st, exclusive */
	int32_t over_at_st = 0, chg_at_st = 0;
	uint32_t len_sum = 0;   /* running sums at j, exclusive: over positions < j */
	int32_t over_sum = 0, chg_sum = 0;
	if (C->cnt < 0 || C->pos_beg < 0 || C->pos_beg + C->cnt > n_pos) return -1;
	for (j = 0; j < C->cnt; ++j) if ((p[j].v >> 1) >= n_seg) return -1;
	for (j = 0; j < C->cnt; ++j) {
		const mga_call_seg_t S = seg[p[j].v >> 1];
		const int32_t D = j > 0 && S.bid != seg[p[j - 1].v >> 1].bid; /* bubble id differs from the previous position's */
		if (j >= 1) {
			const mga_call_seg_t P = seg[p[j - 1].v >> 1];
			if (call_sets_st(P.is_stem)) st = j, len_at_st = len_sum, over_at_st = over_sum, chg_at_st = chg_sum + D; /* chg_at_st: changes at positions <= st */
			if (call_closes(S.is_stem, P.is_stem, st)) {
				const int32_t en = j, qs = p[st - 1].yl1, qe = p[en].yf1 - p[st].span;
				const mga_call_seg_t A = seg[p[st - 1].v >> 1], B = S;
				int32_t strand = 0, bid = -1, n_q = 0, what;
				int64_t k;
				for (k = 0; k < n_qa && n_q < 2; ++k) n_q += call_intv_hit(&qa[k], qs, qe);
				what = call_judge(n_q, over_sum - over_at_st, A, B, seg[p[st].v >> 1].bid, en - st >= 2 ? chg_sum - chg_at_st : 0, en - st, &strand, &bid);
				if (what == MGA_CALL_KEEP) {
					mga_call_cand_t *c = &cand[(*n_cand)++];
					c->key = (uint64_t)(uint32_t)C->ord << 32 | (uint32_t)j, c->bid = bid, c->st = C->lc_off + st, c->en = C->lc_off + en, c->strand = strand;
					c->qs = qs, c->qe = qe, c->glen = (int32_t)(len_sum - len_at_st), c->t = C->t;
				} else if (what != MGA_CALL_DROP) {
					mga_call_warn_t *w = &warn[(*n_warn)++];
					w->key = (uint64_t)(uint32_t)C->ord << 32 | (uint32_t)j, w->type = what == MGA_CALL_WARN1 ? 1 : 2, w->t = C->t, w->qs = qs, w->qe = qe, w->v = p[st].v, w->pad = 0;
				}
			}
		}
		len_sum += (uint32_t)seg_len[p[j].v >> 1], over_sum += S.over, chg_sum += D;
	}
	return 0;
}
#endif

#endif
