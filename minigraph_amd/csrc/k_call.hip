// k_call.hip -- the candidates of --call on the device (mg_call_asm's scan over every chain, reference asm-call.c:47-115; call_core.h has the formulation and the tests a
// candidate passes): per bubble the order key of the surviving candidate that the reference would have written LAST, plus the records of all survivors and of the
// folded-inversion warnings.
//
// Form: ONE WAVEFRONT PER CHAIN, four chains per 256-thread workgroup (k_cov's shape), lanes striding over the walk 64 positions at a time.  What the reference keeps in
// variables along a walk is carried from block to block in wave-uniform registers:
//   st          the largest j' <= j with a stem at j' - 1: an inclusive maximum scan (DPP, dev_lcscan.h) of "this position sets st", joined with the carry;
//   glen, "an over-covered segment in [st, en)", "a bubble id changes inside (st, en)": differences of inclusive sum scans at en and at st.  The sums AT st travel with st:
//               read from st's lane when st lies in this block (one ds_bpermute each), from the carry otherwise.  glen is a difference of 32-bit wrapping sums, which
//               equals the reference's int32 sum.
// A lane that closes a candidate gathers the two flank records from memory (positions st - 1 and st may lie any number of blocks back).  The query-overlap count runs
// per candidate with the whole wavefront striding over the sequence's intervals, counted by ballot, stopping at 2.
// Output: survivors take consecutive places in the pool behind ONE atomicAdd per wavefront and block; each raises best[bid] by a 64-bit atomicMax of its key.  The maximum
// does not depend on the order in which wavefronts arrive, so the winner is the reference's whatever the launch order; the pool's ORDER is arbitrary and never read.
// A walk is not cut into pieces: the chains of -x asm are few and long, so few wavefronts run -- whether that matters next to the mapping is unmeasured.
#include "mga_dev.h"
#include "dev_common.h"
#include "dev_lcscan.h"
#include "call_core.h"

__device__ __forceinline__ unsigned long long call_first_lane_u64(unsigned long long x)
{
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32));
	return (unsigned long long)hi << 32 | lo;
}

__global__ void __launch_bounds__(256) k_call(int n_chain, const mga_call_chain_t *__restrict__ chain, const mga_call_pos_t *__restrict__ pos, int64_t n_pos,
											  const mga_call_seg_t *__restrict__ seg, const int32_t *__restrict__ seg_len, uint32_t n_seg, int n_seq, const int64_t *__restrict__ q_off,
											  const mga_call_intv_t *__restrict__ qintv, int32_t n_bb, unsigned long long *__restrict__ best, mga_call_cand_t *__restrict__ cand,
											  int64_t cap_cand, mga_call_warn_t *__restrict__ warn, int64_t cap_warn, unsigned long long *__restrict__ cnt)
{
	const int ci = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (ci >= n_chain) return;
	const mga_call_chain_t C = chain[ci];
	if (C.cnt < 2 || C.pos_beg < 0 || C.pos_beg + C.cnt > n_pos || C.t < 0 || C.t >= n_seq) return; // (nothing to scan; a record that points outside its arrays is not followed)
	const mga_call_pos_t *p = pos + C.pos_beg;
	const mga_call_intv_t *qa = qintv + q_off[C.t];
	const int64_t n_qa = q_off[C.t + 1] - q_off[C.t];
	const mga_call_seg_t zero = { 0, 0, 0, 0, 0 };
	// carries, uniform over the wavefront: the position in front of the block, st with the sums at st, the sums over everything in front of the block
	int32_t c_stem = 0, c_bid = 0, c_st = -1, c_len_st = 0, c_over_st = 0, c_chg_st = 0, c_len = 0, c_over = 0, c_chg = 0;
	for (int32_t base = 0; base < C.cnt; base += 64) {
		const int32_t j = base + lane;
		const bool in = j < C.cnt;
		mga_call_pos_t P = { 0, 0, 0, 0 };
		mga_call_seg_t S = zero;
		int32_t len = 0;
		if (in) {
			P = p[j];
			if ((P.v >> 1) < n_seg) S = seg[P.v >> 1], len = seg_len[P.v >> 1];
		}
		const int32_t stem = S.is_stem, over = S.over ? 1 : 0;
		const int32_t stem_prev = lc_prev_lane(stem, c_stem), bid_prev = lc_prev_lane(S.bid, c_bid);
		const int32_t D = in && j > 0 && S.bid != bid_prev ? 1 : 0;
		const int32_t st_blk = lc_scan_max(in && j >= 1 && call_sets_st(stem_prev) ? j : -1, -1); // -1: st was not set in this block up to this lane
		const int32_t st = st_blk >= 0 ? st_blk : c_st;
		const int32_t len_in = (int32_t)((uint32_t)lc_scan_add(len, 0) + (uint32_t)c_len), over_in = lc_scan_add(over, 0) + c_over, chg_in = lc_scan_add(D, 0) + c_chg;
		// the sums at st: lengths and flags over the positions in front of st, changes up to and including st
		const int src = st_blk >= 0 ? st_blk - base : 0;
		int32_t len_st = __shfl((int32_t)((uint32_t)len_in - (uint32_t)len), src), over_st = __shfl(over_in - over, src), chg_st = __shfl(chg_in, src);
		if (st_blk < 0) len_st = c_len_st, over_st = c_over_st, chg_st = c_chg_st;

		const bool closes = in && j >= 1 && call_closes(stem, stem_prev, st); // st >= 1 here
		int32_t qs = 0, qe = 0, bid_st = 0;
		uint32_t v_st = 0;
		mga_call_seg_t A = zero;
		if (closes) {
			const mga_call_pos_t Pa = p[st - 1], Ps = p[st];
			qs = Pa.yl1, qe = P.yf1 - Ps.span, v_st = Ps.v;
			if ((Pa.v >> 1) < n_seg) A = seg[Pa.v >> 1];
			if ((Ps.v >> 1) < n_seg) bid_st = seg[Ps.v >> 1].bid;
		}
		// query intervals overlapping [qs, qe), candidate by candidate, the wavefront striding over the intervals
		int32_t n_q = 0;
		for (uint64_t cm = __ballot(closes); cm; cm &= cm - 1) {
			const int c = (int)__builtin_ctzll(cm);
			const int32_t cqs = __shfl(qs, c), cqe = __shfl(qe, c);
			int32_t n = 0;
			for (int64_t k0 = 0; k0 < n_qa && n < 2; k0 += 64) {
				bool hit = false;
				if (k0 + lane < n_qa) { const mga_call_intv_t a = qa[k0 + lane]; hit = call_intv_hit(&a, cqs, cqe); }
				n += (int32_t)__popcll(__ballot(hit));
			}
			if (lane == c) n_q = n;
		}
		int what = MGA_CALL_DROP;
		int32_t strand = 0, bid = -1;
		if (closes) what = call_judge(n_q, (over_in - over) - over_st, A, S, bid_st, j - st >= 2 ? (chg_in - D) - chg_st : 0, j - st, &strand, &bid);
		const bool keep = what == MGA_CALL_KEEP && bid >= 0 && bid < n_bb, wn = what == MGA_CALL_WARN1 || what == MGA_CALL_WARN2;
		const uint64_t km = __ballot(keep), wm = __ballot(wn), below = lane ? ~0ULL >> (64 - lane) : 0ULL;
		const uint64_t key = (uint64_t)(uint32_t)C.ord << 32 | (uint32_t)j;
		if (km) { // one atomic per wavefront for the places
			unsigned long long b0 = 0;
			if (lane == 0) b0 = atomicAdd(&cnt[0], (unsigned long long)__popcll(km));
			b0 = call_first_lane_u64(b0);
			const int64_t slot = (int64_t)b0 + __popcll(km & below);
			if (keep && slot < cap_cand) {
				mga_call_cand_t r;
				r.key = key, r.bid = bid, r.st = C.lc_off + st, r.en = C.lc_off + j, r.strand = strand, r.qs = qs, r.qe = qe;
				r.glen = (int32_t)(((uint32_t)len_in - (uint32_t)len) - (uint32_t)len_st), r.t = C.t;
				cand[slot] = r;
				atomicMax(&best[bid], (unsigned long long)key);
			}
		}
		if (wm) {
			unsigned long long b0 = 0;
			if (lane == 0) b0 = atomicAdd(&cnt[1], (unsigned long long)__popcll(wm));
			b0 = call_first_lane_u64(b0);
			const int64_t slot = (int64_t)b0 + __popcll(wm & below);
			if (wn && slot < cap_warn) {
				mga_call_warn_t r;
				r.key = key, r.type = what == MGA_CALL_WARN1 ? 1 : 2, r.t = C.t, r.qs = qs, r.qe = qe, r.v = v_st, r.pad = 0;
				warn[slot] = r;
			}
		}
		c_stem = __builtin_amdgcn_readlane(stem, 63), c_bid = __builtin_amdgcn_readlane(S.bid, 63), c_st = __builtin_amdgcn_readlane(st, 63);
		c_len_st = __builtin_amdgcn_readlane(len_st, 63), c_over_st = __builtin_amdgcn_readlane(over_st, 63), c_chg_st = __builtin_amdgcn_readlane(chg_st, 63);
		c_len = __builtin_amdgcn_readlane(len_in, 63), c_over = __builtin_amdgcn_readlane(over_in, 63), c_chg = __builtin_amdgcn_readlane(chg_in, 63);
	}
}

// d_best[n_bb] and d_cnt[2] (survivors, warnings) are zeroed by the caller; d_cand / d_warn hold cap_cand / cap_warn records (n_pos each never overflows: a position closes
// at most one candidate)
extern "C" int mga_dev_call(mga_sctx_t *sc, int n_chain, const mga_call_chain_t *d_chain, int64_t n_pos, const mga_call_pos_t *d_pos, uint32_t n_seg, const mga_call_seg_t *d_seg,
							const int32_t *d_seg_len, int n_seq, const int64_t *d_q_off, const mga_call_intv_t *d_qintv, int32_t n_bb, uint64_t *d_best, mga_call_cand_t *d_cand,
							int64_t cap_cand, mga_call_warn_t *d_warn, int64_t cap_warn, uint64_t *d_cnt)
{
	if (n_chain <= 0) return 0;
	hipLaunchKernelGGL(k_call, dim3((unsigned)((n_chain + 3) / 4)), dim3(256), 0, (hipStream_t)sc->stream, n_chain, d_chain, d_pos, n_pos, d_seg, d_seg_len, n_seg, n_seq, d_q_off, d_qintv,
					   n_bb, (unsigned long long*)d_best, d_cand, cap_cand, d_warn, cap_warn, (unsigned long long*)d_cnt);
	MGA_HIP_CHECK(hipGetLastError());
	return 0;
}
