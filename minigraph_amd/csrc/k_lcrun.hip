// k_lcrun.hip -- the linear chaining DP (mg_lchain_dp's forward loop, lchain.c:168-207) of ULTRA-LONG -x lr reads, run by run.
//
// k_lchain.hip gives a read one wavefront, which a 5 Mbp read turns into 3 x 10^5 dependent anchor steps.  The loop's sequential state -- the window's start st, the best
// anchor in reach max_ii, the marks t[] -- does not survive an anchor whose predecessor in x order lies on another (segment, strand) or more than dist_x behind it (the scan is
// empty, max_ii becomes the anchor itself, marks are only written below the cut and only compared against one i), so the host cuts a read's x-sorted anchors into independent
// work items there (rqphase.c: mga_lcdp_cut) and this kernel chains them, bit for bit what hchain.c: mga_lchain_dp_fwd computes over the whole read.  Two forms per launch:
//
//  * a WORKGROUP per work item (LCR_NW wavefronts), for the long ones.  The predecessors' window lives in LDS: a ring of the last LCR_RING + 1 anchors as struct-of-arrays --
//    tpos (low word of x: a window never leaves one (segment, strand)), qpos, span, f, v, p (relative to the work item) and the mark -- 28 bytes per anchor, 143 388 bytes of
//    gfx950's 160 KB.  A trip of the scan covers 64 * LCR_NW predecessors: wave w scores block w in visiting order (lane l <-> j0 - 64 w - l) from the ring and publishes the
//    marks t[p[j]] = i of its block (marks behind the eventual cut carry the value i, which no later anchor compares against); behind barrier (1) the waves read the marks and
//    the block maxima of the waves before them, which with the running maximum seed the exclusive prefix max inside the wave; each wave leaves its improve / skip-hit ballots
//    in LDS; behind barrier (2) EVERY wave replays the LCR_NW pairs of masks in order -- the skip counter carried from block to block by lc_skip_replay, uniform work -- and so
//    knows the cut and the winner without another exchange: the winner is the last improving lane before the cut (an improving lane beats everything visited before it, `>` is
//    strict: the nearest of equal predecessors wins, across waves too), and its score is recomputed from the ring.  The max_ii part follows from registers and the ring; thread
//    0 writes the anchor's f / v / p to the ring and to memory; barrier (3) ends the step.
//    Barriers per anchor: 2 per trip + 1, i.e. 3 for a window of up to 512 anchors, 1 for an anchor without predecessors; all of them sit on conditions computed from values
//    every thread holds identically.  The recomputation of max_ii (a first-maximum reduction of f over [st, i), descending j) is done by every wave on its own from the ring
//    instead of split over the waves: it is rare and a split would cost a barrier on every anchor that needs it.
//  * a WAVEFRONT per work item, LCR_NW items per workgroup at a time, for the thousands of short ones: k_lchain.hip's lc_dp over global memory (64 predecessors per trip,
//    exclusive prefix max + lc_skip_replay, marks published then read through a device scratch), with wave-level ordering only -- no workgroup barrier inside an item.
//
// Workgroups draw units from one counter, in the order the host lists the items (longest first): the first n_wg units are the workgroup-form items, every later unit is
// LCR_NW wave-form items.  Nothing waits for another workgroup.  Float arithmetic: lc_log2, mul / add without contraction (-ffp-contract=off), truncation by (int).
#include "mga_dev.h"
#include "dev_common.h"
#include "dev_lcscan.h"

#define LCR_NW 8
#define LCR_THREADS (64 * LCR_NW)
#define LCR_RING 5120 // the longest window (max_iter) the ring serves: the -x lr default max_lc_iter = 5000 fits
#define LCR_SLOTS (LCR_RING + 1) // ... and one slot more: anchor i is written while a slower wave may still read the window's first anchor, i - LCR_RING

struct lcr_item_t { int64_t beg, end, base, dist_x; }; // chunk-level [beg, end) of a read whose first anchor is `base`; dist_x = max(max_dist_x, bw) of that read (-F)
struct lcr_par_t { int32_t dist_y, bw, max_skip, max_iter, max_len; float pen_gap, pen_skip; };
struct lcr_lds_t {
	int32_t tpos[LCR_SLOTS], qpos[LCR_SLOTS], span[LCR_SLOTS], f[LCR_SLOTS], v[LCR_SLOTS], p[LCR_SLOTS], mark[LCR_SLOTS];
	int32_t blkmax[LCR_NW];
	uint64_t imp[LCR_NW], hit[LCR_NW];
	int32_t unit;
};

__device__ __forceinline__ int32_t lcr_score(int32_t xil, int32_t yil, int32_t xjl, int32_t yjl, int32_t span, int32_t dist_x, const lcr_par_t &P) // hchain.c: lcdp_pair, on the low words
{
	const int32_t dq = yil - yjl;
	if (dq <= 0 || dq > dist_x) return LC_NONE;
	const int32_t dr = xil - xjl;
	if (dr == 0 || dq > P.dist_y) return LC_NONE;
	const int32_t dd = dr > dq ? dr - dq : dq - dr;
	if (dd > P.bw) return LC_NONE;
	const int32_t dg = dr < dq ? dr : dq;
	int32_t sc = span < dg ? span : dg;
	if (dd || dg > span) {
		const float lin = P.pen_gap * (float)dd + P.pen_skip * (float)dg;
		const float lg = dd >= 1 ? lc_log2((float)(dd + 1)) : 0.0f;
		sc -= (int32_t)(lin + .5f * lg);
	}
	return sc;
}

__device__ __forceinline__ uint64_t lcr_uni64(uint64_t x) // a value every lane holds, into scalar registers
{
	return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(x >> 32)) << 32 | (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)x);
}

// visibility of a wave's own stores (global and LDS) to its other lanes; the waves of a workgroup share the CU's vector cache
__device__ __forceinline__ void lcr_wsync(void) { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); }

#define LCR_SLOT(j) ((uint32_t)(j) % (uint32_t)LCR_SLOTS)

// ---------------- a workgroup per work item: a, f, v, p point at the item's first anchor; rel = its index in the read ----------------
__device__ __forceinline__ void lcr_wg(const mg128_t *__restrict__ a, int32_t n, int64_t rel, int32_t dist_x, const lcr_par_t &P, int32_t *__restrict__ f, int32_t *__restrict__ v,
									   long long *__restrict__ p, lcr_lds_t *L, int tid)
{
	const int lane = tid & 63, w = tid >> 6;
	int32_t st = 0, seg0 = 0, max_ii = -1, hi_prev = 0;
	uint64_t am_x = 0; int32_t am_yl = 0, am_sp = 0, fm = 0, vm = 0; // the best-scoring anchor in reach (lchain.c: max_ii) with the values memory would give
	mg128_t cur = a[0];
	for (int32_t i = 0; i < n; ++i) {
		const uint64_t xi = cur.x;
		const int32_t xil = (int32_t)xi, xih = (int32_t)(xi >> 32), yil = (int32_t)cur.y, spi = (int32_t)(cur.y >> 32 & 0xff);
		if (i + 1 < n) cur = a[i + 1]; // (in flight while this anchor is chained)
		// lchain.c:171-172, the clamp first: the predicate is monotone in st (x ascending), so the result is the same and no slot older than the ring is read
		if (i == 0 || xih != hi_prev) seg0 = i;
		hi_prev = xih;
		if (st < seg0) st = seg0;
		if (i - st > P.max_iter) st = i - P.max_iter;
		while (st < i && (uint32_t)(xil - L->tpos[LCR_SLOT(st)]) > (uint32_t)dist_x) ++st;
		int32_t max_f = spi, max_j = -1, max_v = 0, n_skip = 0, end_j = st - 1;
		bool cut = false;
		for (int32_t j0 = i - 1; j0 >= st && !cut; j0 -= 64 * LCR_NW) {
			const int32_t j = j0 - 64 * w - lane;
			const uint32_t s = j >= st ? LCR_SLOT(j) : 0;
			int32_t sc = LC_NONE, pj = -1;
			if (j >= st) {
				sc = lcr_score(xil, yil, L->tpos[s], L->qpos[s], L->span[s], dist_x, P);
				if (sc != LC_NONE) sc += L->f[s], pj = L->p[s];
			}
			const bool valid = sc != LC_NONE;
			if (valid && pj >= st) L->mark[LCR_SLOT(pj)] = i; // lchain.c:188; a mark below st is never read for this i, and its slot may belong to a newer anchor
			const int32_t pm = lc_scan_max(valid ? sc : INT32_MIN, INT32_MIN);
			if (lane == 63) L->blkmax[w] = pm;
			__syncthreads(); // (1) the trip's marks and block maxima
			const bool hit_t = valid && L->mark[s] == i;
			int32_t carry = max_f;
			for (int k = 0; k < w; ++k) { const int32_t bm = L->blkmax[k]; if (carry < bm) carry = bm; }
			int32_t ex = lc_prev_lane(pm, INT32_MIN);
			if (ex < carry) ex = carry;
			const bool improve = valid && sc > ex;
			const uint64_t m_imp = __ballot(improve), m_hit = __ballot(hit_t && !improve);
			if (lane == 0) L->imp[w] = m_imp, L->hit[w] = m_hit;
			__syncthreads(); // (2) every wave's ballots
			int win = -1; // the winner's place in the trip's visiting order
			for (int k = 0; k < LCR_NW; ++k) {
				const uint64_t mi = lcr_uni64(L->imp[k]), mh = lcr_uni64(L->hit[k]);
				if ((mi | mh) == 0) continue; // (no event: the counter stays)
				const int cl = lc_skip_replay((mi >> lane & 1) != 0, (mh >> lane & 1) != 0, P.max_skip, &n_skip);
				const uint64_t ib = mi & (cl == 64 ? ~0ULL : (1ULL << cl) - 1ULL);
				if (ib) win = 64 * k + 63 - (int)__clzll(ib);
				if (cl < 64) { cut = true; end_j = j0 - 64 * k - cl; break; }
			}
			if (win >= 0) {
				max_j = j0 - win;
				const uint32_t sw = LCR_SLOT(max_j);
				max_f = L->f[sw] + lcr_score(xil, yil, L->tpos[sw], L->qpos[sw], L->span[sw], dist_x, P), max_v = L->v[sw];
			}
		}
		// lchain.c:191-196: the best-scoring anchor in reach, looked for again when it fell out of reach
		if (max_ii < 0 || xi - am_x > (uint64_t)(int64_t)dist_x) {
			int32_t bf = INT32_MIN, bj = -1;
			for (int32_t j = i - 1 - lane; j >= st; j -= 64) { const int32_t fj = L->f[LCR_SLOT(j)]; if (bf < fj) bf = fj, bj = j; } // descending j per lane: first max kept
			for (int d = 32; d > 0; d >>= 1) {
				const int32_t of = __shfl_xor(bf, d), oj = __shfl_xor(bj, d);
				if (of > bf || (of == bf && oj > bj)) bf = of, bj = oj; // ties: the larger j was met first
			}
			max_ii = __builtin_amdgcn_readfirstlane(bj);
			if (max_ii >= 0) { const uint32_t sm = LCR_SLOT(max_ii); am_x = (xi & ~0xffffffffULL) | (uint32_t)L->tpos[sm], am_yl = L->qpos[sm], am_sp = L->span[sm], fm = L->f[sm], vm = L->v[sm]; }
		}
		if (max_ii >= 0 && max_ii < end_j) { // lchain.c:197-202: the scan was cut before it got there
			const int32_t tmp = lcr_score(xil, yil, (int32_t)am_x, am_yl, am_sp, dist_x, P);
			if (tmp != LC_NONE && max_f < tmp + fm) max_f = tmp + fm, max_j = max_ii, max_v = vm;
		}
		const int32_t vi = max_j >= 0 && max_v > max_f ? max_v : max_f;
		if (tid == 0) {
			const uint32_t si = LCR_SLOT(i);
			L->tpos[si] = xil, L->qpos[si] = yil, L->span[si] = spi, L->f[si] = max_f, L->v[si] = vi, L->p[si] = max_j, L->mark[si] = -1;
			f[i] = max_f, v[i] = vi, p[i] = max_j >= 0 ? (long long)(rel + max_j) : -1LL;
		}
		if (max_ii < 0 || (xi - am_x <= (uint64_t)(int64_t)dist_x && fm < max_f)) max_ii = i, am_x = xi, am_yl = yil, am_sp = spi, fm = max_f, vm = vi; // lchain.c:205
		__syncthreads(); // (3) the anchor is in the ring
	}
}

// ---------------- a wavefront per work item: lc_dp (k_lchain.hip) over the item's slices; t = its slice of the marks' scratch ----------------
__device__ __forceinline__ void lcr_wave(const mg128_t *__restrict__ a, int32_t n, int64_t rel, int32_t dist_x, const lcr_par_t &P, int32_t *f, int32_t *v, long long *p, int32_t *t, int lane)
{
	for (int32_t i = lane; i < n; i += 64) t[i] = 0;
	lcr_wsync();
	int32_t st = 0, max_ii = -1;
	for (int32_t i = 0; i < n; ++i) {
		{ // a run of anchors without any predecessor in reach (k_lchain.hip:99-122): f = v = span, p = -1, written by the lanes at once
			const int32_t k = i + lane;
			bool iso = false;
			uint64_t yk = 0;
			if (k < n) {
				const uint64_t xk = a[k].x;
				yk = a[k].y;
				if (k == 0) iso = true;
				else { const uint64_t xp = a[k - 1].x; iso = xk >> 32 != xp >> 32 || xk > xp + (uint64_t)(int64_t)dist_x; }
			}
			const uint64_t m = __ballot(iso);
			const int r = (~m) ? (int)__builtin_ctzll(~m) : 64;
			if (r > 0) {
				if (lane < r) { const int32_t sp = (int32_t)(yk >> 32 & 0xff); f[k] = sp, p[k] = -1LL, v[k] = sp; }
				max_ii = i + r - 1;
				if (st < i + r - 1) st = i + r - 1;
				i += r - 1;
				lcr_wsync();
				continue;
			}
		}
		const uint64_t xi = a[i].x, yi = a[i].y;
		const int32_t xil = (int32_t)xi, yil = (int32_t)yi, spi = (int32_t)(yi >> 32 & 0xff);
		uint64_t xs0 = st < i ? a[st].x : 0;
		mg128_t am; am.x = am.y = 0;
		int32_t fm = 0, vm = 0;
		if (max_ii >= 0) am = a[max_ii], fm = f[max_ii], vm = v[max_ii];
		while (st < i) { // lchain.c:171
			if (xi >> 32 != xs0 >> 32 || xi > xs0 + (uint64_t)(int64_t)dist_x) { ++st; if (st < i) xs0 = a[st].x; } else break;
		}
		if (i - st > P.max_iter) st = i - P.max_iter;
		int32_t max_f = spi, max_j = -1, max_v = 0, n_skip = 0, end_j = st - 1;
		bool cut = false;
		for (int32_t j0 = i - 1; j0 >= st && !cut; j0 -= 64) {
			const int32_t j = j0 - lane;
			int32_t sc = LC_NONE, pj = -1, vj = 0;
			if (j >= st) {
				const mg128_t aj = a[j];
				const int32_t fj = f[j];
				const long long pr = p[j];
				vj = v[j];
				sc = lcr_score(xil, yil, (int32_t)aj.x, (int32_t)aj.y, (int32_t)(aj.y >> 32 & 0xff), dist_x, P); // (every j >= st shares the anchor's segment and strand)
				if (sc != LC_NONE) { sc += fj; if (pr >= 0) pj = (int32_t)(pr - rel); }
			}
			const bool valid = sc != LC_NONE;
			if (valid && pj >= 0) t[pj] = i; // lchain.c:188
			lcr_wsync();
			const bool hit_t = valid && t[j] == i;
			const int32_t pm = lc_scan_max(valid ? sc : INT32_MIN, INT32_MIN);
			int32_t ex = lc_prev_lane(pm, INT32_MIN);
			if (ex < max_f) ex = max_f;
			const bool improve = valid && sc > ex;
			const uint64_t m_imp = __ballot(improve);
			const int cut_lane = lc_skip_replay(improve, hit_t && !improve, P.max_skip, &n_skip);
			const uint64_t imp_b = m_imp & (cut_lane == 64 ? ~0ULL : (1ULL << cut_lane) - 1ULL);
			if (imp_b) {
				const int bl = 63 - (int)__clzll(imp_b);
				max_f = __shfl(sc, bl), max_v = __shfl(vj, bl), max_j = j0 - bl;
			}
			if (cut_lane < 64) { cut = true; end_j = j0 - cut_lane; }
		}
		if (max_ii < 0 || xi - am.x > (uint64_t)(int64_t)dist_x) { // lchain.c:191-196
			int32_t bf = INT32_MIN, bj = -1;
			for (int32_t j = i - 1 - lane; j >= st; j -= 64) { const int32_t fj = f[j]; if (bf < fj) bf = fj, bj = j; }
			for (int d = 32; d > 0; d >>= 1) {
				const int32_t of = __shfl_xor(bf, d), oj = __shfl_xor(bj, d);
				if (of > bf || (of == bf && oj > bj)) bf = of, bj = oj;
			}
			max_ii = __builtin_amdgcn_readfirstlane(bj);
			if (max_ii >= 0) am = a[max_ii], fm = f[max_ii], vm = v[max_ii];
		}
		if (max_ii >= 0 && max_ii < end_j) { // lchain.c:197-202
			const int32_t tmp = lcr_score(xil, yil, (int32_t)am.x, (int32_t)am.y, (int32_t)(am.y >> 32 & 0xff), dist_x, P);
			if (tmp != LC_NONE && max_f < tmp + fm) max_f = tmp + fm, max_j = max_ii, max_v = vm;
		}
		const int32_t vi = max_j >= 0 && max_v > max_f ? max_v : max_f;
		if (lane == 0) { f[i] = max_f; p[i] = max_j >= 0 ? (long long)(rel + max_j) : -1LL; v[i] = vi; }
		if (max_ii < 0 || (xi - am.x <= (uint64_t)(int64_t)dist_x && fm < max_f)) max_ii = i;
		lcr_wsync();
	}
}

// status: 0 done; 3 left to the host (longer than max_len, or a workgroup-form item whose max_iter the ring does not hold); an item never drawn keeps what the host put there
__global__ void __launch_bounds__(LCR_THREADS) k_lcrun_fwd(int n_order, int n_wg, const lcr_item_t *__restrict__ items, const int32_t *__restrict__ order, const mg128_t *__restrict__ a,
															lcr_par_t P, int32_t *__restrict__ f, long long *__restrict__ p, int32_t *__restrict__ v, int32_t *__restrict__ t,
															int32_t *__restrict__ status, int *__restrict__ counter)
{
	__shared__ lcr_lds_t L;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const int n_units = n_wg + (n_order - n_wg + LCR_NW - 1) / LCR_NW;
	for (;;) {
		if (tid == 0) L.unit = atomicAdd(counter, 1);
		__syncthreads();
		const int u = L.unit;
		__syncthreads(); // (read by all before the next draw overwrites it)
		if (u >= n_units) break;
		if (u < n_wg) {
			const int r = order[u];
			const lcr_item_t it = items[r];
			const int64_t n = it.end - it.beg;
			if (n > P.max_len || P.max_iter > LCR_RING) { if (tid == 0) status[r] = 3; }
			else {
				if (n > 0) lcr_wg(a + it.beg, (int32_t)n, it.beg - it.base, (int32_t)it.dist_x, P, f + it.beg, v + it.beg, p + it.beg, &L, tid);
				if (tid == 0) status[r] = 0;
			}
		} else {
			const int k = n_wg + (u - n_wg) * LCR_NW + w;
			if (k < n_order) {
				const int r = order[k];
				const lcr_item_t it = items[r];
				const int64_t n = it.end - it.beg;
				if (n > P.max_len) { if (lane == 0) status[r] = 3; }
				else {
					if (n > 0) lcr_wave(a + it.beg, (int32_t)n, it.beg - it.base, (int32_t)it.dist_x, P, f + it.beg, v + it.beg, p + it.beg, t + it.beg, lane);
					if (lane == 0) status[r] = 0;
				}
			}
		}
		__syncthreads();
	}
}

// the DP over the work items d_items[d_order[0 .. n_order)] ({ beg, end, base, dist_x } as four int64) of a CHUNK's x-sorted anchor array d_a (n_total < 2^31); the first n_wg
// of the order take the workgroup form.  d_t: n_total int32 of scratch (the wave form's marks); d_counter: one int.  f / v / p (relative to base, -1: none) per anchor.
extern "C" int mga_dev_lcdp_fwd(mga_sctx_t *sc, int64_t n_total, const mg128_t *d_a, int n_order, int n_wg, const void *d_items, const int32_t *d_order, int max_dist_y, int bw,
								int max_skip, int max_iter, int64_t max_len, float pen_gap, float pen_skip, int32_t *d_f, int64_t *d_p, int32_t *d_v, int32_t *d_t, int32_t *d_status, int *d_counter)
{
	if (n_total <= 0 || n_order <= 0) return 0;
	if (n_total >= 0x7fffffffLL) { mga_set_error("lcdp_fwd: more than 2^31 anchors in one chunk"); return -1; }
	if (n_wg < 0 || n_wg > n_order || d_order == 0) { mga_set_error("lcdp_fwd: bad work list"); return -1; }
	hipStream_t st = (hipStream_t)sc->stream;
	lcr_par_t P;
	P.dist_y = max_dist_y < bw ? bw : max_dist_y, P.bw = bw, P.max_skip = max_skip, P.max_iter = max_iter, P.max_len = (int32_t)(max_len < 0x7fffffffLL ? max_len : 0x7fffffffLL);
	P.pen_gap = pen_gap, P.pen_skip = pen_skip;
	const int n_units = n_wg + (n_order - n_wg + LCR_NW - 1) / LCR_NW;
	MGA_HIP_CHECK(hipMemsetAsync(d_counter, 0, 4, st));
	mga_prof_begin(sc->stream, MGA_K_LCHAIN);
	hipLaunchKernelGGL(k_lcrun_fwd, dim3(n_units < 1024 ? n_units : 1024), dim3(LCR_THREADS), 0, st, n_order, n_wg, (const lcr_item_t*)d_items, d_order, d_a, P, d_f, (long long*)d_p, d_v, d_t,
					   d_status, d_counter);
	mga_prof_end(sc->stream, MGA_K_LCHAIN);
	MGA_HIP_CHECK(hipGetLastError());
	return 0;
}

extern "C" void mga_dev_lcdp_shape(int *nw, int *ring) { *nw = LCR_NW, *ring = LCR_RING; }
