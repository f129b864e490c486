// k_wfa_seg.hip -- exact 2-piece affine-gap WFA in bounded memory: the rung behind the last HBM tier of k_wfa.hip.
//
// The reference closes the stretches of its chained fallback with mwf_wfa_exact(step = 5000) (miniwfa.c:829-832), i.e. in the low-memory
// mode mwf_wfa_seg (miniwfa.c:440-601): a first pass that keeps no traceback, only the 17-slice ring of wavefront values plus a second
// ring of ORIGINS, and takes a snapshot of the origins every `step` scores; the chain of snapshots names one cell (s, d) of the optimal
// path per snapshot.  A second pass (mwf_wfa_core with seg[], miniwfa.c:413-416) is the ordinary traceback pass, except that its band
// collapses to the single diagonal d when it reaches score s -- its traceback rows are as wide as the narrowed band, not as the full one.
// The CIGAR equals the full mode's for every step (tests/test_wfa_seg.py pins that to the unmodified reference), so the step is the
// device's to choose: the host takes the one that needs the least memory (wseg_plan below; formula in DESIGN.md 4).
//
// One WORKGROUP (up to 1024 threads) per problem, threads strided over the diagonals of a slice.  What k_wfa.hip states about the
// recurrence, NEG_INF outside a slice, band growth, the 256-score trim and the extension on raw bytes holds here verbatim.
//
// Barriers.  Slice s+1 reads H of the slices s-3, s-5 and s-15 and E/F of the slices s and s-1: never H of slice s, which is all the
// extension of slice s writes, and every thread extends the cells it computed itself.  So a score costs ONE barrier:
//     extend slice s (own cells)  |  compute slice s+1  ||barrier||  termination?  band edges of s+1
// The termination flag and the two band-edge flags live in LDS, double-buffered by the parity of the score, so that a wave that is one
// barrier ahead never overwrites what a slower wave still has to read.  Slice s+1 is therefore computed before the workgroup knows that
// slice s terminated; it is then simply dropped.  Snapshots (every `step` scores) and trims (every 256) take extra barriers, on
// conditions that are uniform over the workgroup.  Every exit from the score loop is decided by values all threads read from LDS after
// a barrier, or by values every thread computes identically.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mga_dev.h"
#include "dev_common.h"

#define WS_NEG_INF (-0x40000000)
#define WS_NSLOT 17

enum { WSEG_OK = 0, WSEG_E_BOUND = 1 /* score bound reached */, WSEG_E_ROOM = 2 /* ring / traceback / snapshot room */, WSEG_E_WALK = 3 /* snapshot chain broken */,
	   WSEG_E_POOL = 4, WSEG_E_CIGAR = 5 };

struct wseg_snap_t { int64_t off; int32_t max_s, n; int32_t lo[WS_NSLOT], w[WS_NSLOT]; }; // slices oldest first: scores max_s-16 .. max_s
struct wseg_chk_t { int32_t s, d; };

// sizes of one problem's workspace (host: wseg_plan); the parts lie in this order, the whole is rounded up to 256 bytes
struct wseg_job_t {
	int32_t pi, tl, ql, step;
	int32_t smax, wmax, cigcap, max_snap;
	int64_t tbcap, snapcap;   // traceback bytes of pass 2, int32 cells of all snapshots
	int64_t ws_off;           // of this problem's workspace in the launch's buffer
};
struct wseg_out_t { int32_t score, n_snap, status, pad; int64_t n_iter; };
struct wseg_pen_t { int32_t x, o1, e1, o2, e2; };

struct wseg_ws_t { int64_t *row; wseg_snap_t *meta; int32_t *ring, *oring, *rlo; uint32_t *cig; int32_t *snapx; wseg_chk_t *seg; uint8_t *tb; };

struct wseg_parts_t { int64_t row, meta, ring, oring, rlo, cig, snapx, seg, tb, total; };

__host__ __device__ __forceinline__ wseg_parts_t wseg_parts(const wseg_job_t &j)
{
	wseg_parts_t p;
	p.row = (int64_t)(j.smax + 1) * 8;
	p.meta = (int64_t)j.max_snap * (int64_t)sizeof(wseg_snap_t);
	p.ring = (int64_t)WS_NSLOT * 5 * 4 * j.wmax;
	p.oring = p.ring;
	p.rlo = (int64_t)(j.smax + 1) * 4;
	p.cig = (int64_t)j.cigcap * 4;
	p.snapx = j.snapcap * 4;
	p.seg = (int64_t)j.max_snap * 8;
	p.tb = j.tbcap;
	p.total = (p.row + p.meta + p.ring + p.oring + p.rlo + p.cig + p.snapx + p.seg + p.tb + 255) & ~(int64_t)255;
	return p;
}

__device__ __forceinline__ wseg_ws_t wseg_carve(char *base, const wseg_job_t &j)
{
	const wseg_parts_t p = wseg_parts(j);
	wseg_ws_t w;
	w.row = (int64_t*)base; base += p.row;
	w.meta = (wseg_snap_t*)base; base += p.meta;
	w.ring = (int32_t*)base; base += p.ring;
	w.oring = (int32_t*)base; base += p.oring;
	w.rlo = (int32_t*)base; base += p.rlo;
	w.cig = (uint32_t*)base; base += p.cig;
	w.snapx = (int32_t*)base; base += p.snapx;
	w.seg = (wseg_chk_t*)base; base += p.seg;
	w.tb = (uint8_t*)base;
	return w;
}

// number of leading equal bytes of a[0..maxlen) and b[0..maxlen); buffers are padded by >= 8 bytes
__device__ __forceinline__ int32_t wseg_lcp(const char *a, const char *b, int32_t maxlen)
{
	int32_t n = 0;
	while (n < maxlen) {
		uint64_t x, y;
		__builtin_memcpy(&x, a + n, 8);
		__builtin_memcpy(&y, b + n, 8);
		const uint64_t c = x ^ y;
		if (c) { n += __builtin_ctzll(c) >> 3; break; }
		n += 8;
	}
	return n < maxlen ? n : maxlen;
}

struct wseg_lds_t {
	int32_t lo[WS_NSLOT], hi[WS_NSLOT];
	int32_t term[2], last[2], elo[2], ehi[2];
	int32_t tmin, tmax;
	unsigned long long pool_off;
};

struct wseg_fwd_t { int32_t s, status, last, n_snap; int64_t n_iter; };

// One forward pass.  PASS 1: values + origins, snapshots, no traceback.  PASS 2: values + traceback rows, the band restarts at the checkpoints.
template<int PASS>
__device__ wseg_fwd_t wseg_forward(wseg_lds_t &S, const wseg_ws_t &W, const wseg_job_t &J, const wseg_pen_t &P, const char *ts, const char *qs, int32_t n_seg)
{
	const int tid = threadIdx.x, NT = blockDim.x;
	const int32_t tl = J.tl, ql = J.ql, wmax = J.wmax;
	const int32_t oe1 = P.o1 + P.e1, oe2 = P.o2 + P.e2;
#define VR(slot, arr) (W.ring + ((size_t)(slot) * 5 + (arr)) * wmax)
#define OR(slot, arr) (W.oring + ((size_t)(slot) * 5 + (arr)) * wmax)
	// offset of diagonal d in the slice of score sc, or -1 (outside the slice / before score 0: the value AND the origin there are NEG_INF)
	auto at = [&](int32_t sc, int32_t d, int &slot) -> int32_t {
		if (sc < 0) return -1;
		slot = sc % WS_NSLOT;
		const int32_t lo = S.lo[slot], hi = S.hi[slot];
		return d < lo || d > hi ? -1 : d - lo;
	};
	if (tid < WS_NSLOT) { S.lo[tid] = 1; S.hi[tid] = 0; }
	if (tid < 2) S.term[tid] = 0;
	__syncthreads();
	if (tid == 0) {
		S.lo[0] = 0; S.hi[0] = 0;
		VR(0, 0)[0] = -1;
		VR(0, 1)[0] = VR(0, 2)[0] = VR(0, 3)[0] = VR(0, 4)[0] = WS_NEG_INF;
		if (PASS == 1) { OR(0, 0)[0] = -1; OR(0, 1)[0] = OR(0, 2)[0] = OR(0, 3)[0] = OR(0, 4)[0] = WS_NEG_INF; }
		else { W.row[0] = 0; W.rlo[0] = 0; W.tb[0] = 0; }
	}
	__syncthreads();

	wseg_fwd_t R;
	R.s = 0, R.status = WSEG_OK, R.last = 0, R.n_snap = 0, R.n_iter = 0;
	int32_t s = 0, wlo = 0, whi = 0, lo = 0, hi = 0, sid = 0;
	int64_t tb_used = 1, row_cur = 0, snap_used = 0;

	for (;;) {
		const int slot = s % WS_NSLOT, par = s & 1;
		// ---- extend the own cells of slice s along exact matches (miniwfa.c:399-411 / :572-581); only the diagonal ql - tl can terminate
		{
			int32_t *Hc = VR(slot, 0);
			for (int32_t d = lo + tid; d <= hi; d += NT) {
				const int32_t k0 = Hc[d - lo];
				if (k0 < -1 || d + k0 < -1 || k0 >= tl || d + k0 >= ql) continue;
				int32_t room = tl - (k0 + 1);
				if (ql - (d + k0 + 1) < room) room = ql - (d + k0 + 1);
				const int32_t k = k0 + wseg_lcp(ts + k0 + 1, qs + d + k0 + 1, room);
				if (k == tl - 1 && d + k == ql - 1) {
					if (PASS == 1) S.last[par] = OR(slot, 0)[d - lo];
					else S.last[par] = k == k0 ? (int32_t)(W.tb[row_cur + (d - lo)] & 7) : 0;
					S.term[par] = 1;
				} else Hc[d - lo] = k;
			}
		}
		if (PASS == 2 && sid < n_seg && W.seg[sid].s == s) { wlo = whi = W.seg[sid].d; ++sid; } // miniwfa.c:413-416 (an `if`: a checkpoint whose score has passed is never taken, nor any after it)
		const int32_t nlo = wlo > -tl ? wlo - 1 : -tl;
		const int32_t nhi = whi < ql ? whi + 1 : ql;
		const int32_t width = nhi - nlo + 1;
		const bool bound = s + 1 > J.smax;
		const bool ok = !(bound || width > wmax || (PASS == 2 && tb_used + width > J.tbcap));
		if (PASS == 1 && ok && (s + 1) % J.step == 0) { // ---- wf_snapshot1 (miniwfa.c:451-474): the reference takes it only when slice s did not terminate
			__syncthreads();
			if (S.term[par]) break;
			int64_t n = 0;
			for (int k = 0; k < WS_NSLOT; ++k) { const int32_t sc = s - (WS_NSLOT - 1) + k; if (sc >= 0) { const int sl = sc % WS_NSLOT; n += 5 * (int64_t)(S.hi[sl] - S.lo[sl] + 1); } }
			if (R.n_snap >= J.max_snap || snap_used + n > J.snapcap) { R.status = WSEG_E_ROOM; break; }
			int32_t *X = W.snapx + snap_used;
			int32_t base = 0;
			for (int k = 0; k < WS_NSLOT; ++k) {
				const int32_t sc = s - (WS_NSLOT - 1) + k;
				int32_t l = 0, w = 0;
				if (sc >= 0) {
					const int sl = sc % WS_NSLOT;
					l = S.lo[sl], w = S.hi[sl] - l + 1;
					for (int a = 0; a < 5; ++a) {
						int32_t *O = OR(sl, a);
						for (int32_t o = tid; o < w; o += NT) { const int32_t t = base + a * w + o; X[t] = O[o]; O[o] = t; }
					}
				}
				if (tid == 0) { W.meta[R.n_snap].lo[k] = l; W.meta[R.n_snap].w[k] = w; }
				base += 5 * w;
			}
			if (tid == 0) { W.meta[R.n_snap].off = snap_used; W.meta[R.n_snap].max_s = s; W.meta[R.n_snap].n = base; }
			++R.n_snap, snap_used += n;
			__syncthreads();
		}
		const int npar = (s + 1) & 1;
		if (ok) { // ---- slice s + 1 (wf_next_tb, miniwfa.c:281-308; origins as wf_next_seg, :495-526)
			const int nslot = (s + 1) % WS_NSLOT;
			if (tid == 0) {
				S.lo[nslot] = nlo; S.hi[nslot] = nhi; // (no thread reads this slot's bounds while it computes slice s + 1: the penalties are 1 .. 16)
				if (PASS == 2) { W.row[s + 1] = tb_used; W.rlo[s + 1] = nlo; }
			}
			int32_t *Hn = VR(nslot, 0), *E1n = VR(nslot, 1), *F1n = VR(nslot, 2), *E2n = VR(nslot, 3), *F2n = VR(nslot, 4);
			const int32_t s1 = s + 1;
			for (int32_t d = nlo + tid; d <= nhi; d += NT) {
				int sl_o1, sl_e1, sl_o2, sl_e2, sl_x;
				const int32_t a_o1l = at(s1 - oe1, d - 1, sl_o1), a_e1l = at(s1 - P.e1, d - 1, sl_e1), a_o2l = at(s1 - oe2, d - 1, sl_o2), a_e2l = at(s1 - P.e2, d - 1, sl_e2);
				const int32_t a_o1r = at(s1 - oe1, d + 1, sl_o1), a_e1r = at(s1 - P.e1, d + 1, sl_e1), a_o2r = at(s1 - oe2, d + 1, sl_o2), a_e2r = at(s1 - P.e2, d + 1, sl_e2);
				const int32_t a_x = at(s1 - P.x, d, sl_x);
#define RDV(a_, sl_, arr_) ((a_) < 0 ? WS_NEG_INF : VR(sl_, arr_)[a_])
#define RDO(a_, sl_, arr_) ((a_) < 0 ? WS_NEG_INF : OR(sl_, arr_)[a_])
				const int32_t ho1l = RDV(a_o1l, sl_o1, 0), e1l = RDV(a_e1l, sl_e1, 1);
				const int32_t ho2l = RDV(a_o2l, sl_o2, 0), e2l = RDV(a_e2l, sl_e2, 3);
				const int32_t ho1r = RDV(a_o1r, sl_o1, 0), f1r = RDV(a_e1r, sl_e1, 2);
				const int32_t ho2r = RDV(a_o2r, sl_o2, 0), f2r = RDV(a_e2r, sl_e2, 4);
				const int32_t hx = RDV(a_x, sl_x, 0);
				uint32_t bits = 0;
				if (!(ho1l >= e1l)) bits |= 0x08;
				const int32_t E1 = ho1l >= e1l ? ho1l : e1l;
				if (!(ho2l >= e2l)) bits |= 0x20;
				const int32_t E2 = ho2l >= e2l ? ho2l : e2l;
				const uint32_t ze = E1 >= E2 ? 1 : 3;
				const int32_t e = E1 >= E2 ? E1 : E2;
				if (!(ho1r >= f1r)) bits |= 0x10;
				const int32_t F1 = (ho1r >= f1r ? ho1r : f1r) + 1;
				if (!(ho2r >= f2r)) bits |= 0x40;
				const int32_t F2 = (ho2r >= f2r ? ho2r : f2r) + 1;
				const uint32_t zf = F1 >= F2 ? 2 : 4;
				const int32_t f = F1 >= F2 ? F1 : F2;
				uint32_t z = e >= f ? ze : zf;
				const int32_t h = e >= f ? e : f;
				if (hx + 1 >= h) z = 0;
				const int32_t H = hx + 1 >= h ? hx + 1 : h;
				const int32_t o = d - nlo;
				Hn[o] = H; E1n[o] = E1; F1n[o] = F1; E2n[o] = E2; F2n[o] = F2;
				if (PASS == 1) { // every array of the cell inherits the origin of the predecessor that won it
					const int32_t oE1 = bits & 0x08 ? RDO(a_e1l, sl_e1, 1) : RDO(a_o1l, sl_o1, 0);
					const int32_t oF1 = bits & 0x10 ? RDO(a_e1r, sl_e1, 2) : RDO(a_o1r, sl_o1, 0);
					const int32_t oE2 = bits & 0x20 ? RDO(a_e2l, sl_e2, 3) : RDO(a_o2l, sl_o2, 0);
					const int32_t oF2 = bits & 0x40 ? RDO(a_e2r, sl_e2, 4) : RDO(a_o2r, sl_o2, 0);
					const int32_t oH = z == 0 ? RDO(a_x, sl_x, 0) : z == 1 ? oE1 : z == 2 ? oF1 : z == 3 ? oE2 : oF2;
					OR(nslot, 0)[o] = oH; OR(nslot, 1)[o] = oE1; OR(nslot, 2)[o] = oF1; OR(nslot, 3)[o] = oE2; OR(nslot, 4)[o] = oF2;
				} else W.tb[tb_used + o] = (uint8_t)(bits | z);
#undef RDV
#undef RDO
				const int32_t reach = H >= -1 || E1 >= -1 || F1 >= -1 || E2 >= -1 || F2 >= -1; // band bookkeeping (miniwfa.c:323-324)
				if (d == nlo) S.elo[npar] = reach;
				if (d == nhi) S.ehi[npar] = reach;
			}
		}
		__syncthreads();
		if (S.term[par]) break;
		if (!ok) { R.status = bound ? WSEG_E_BOUND : WSEG_E_ROOM; break; }
		++s;
		lo = nlo, hi = nhi, row_cur = tb_used;
		tb_used += width, R.n_iter += width;
		if (S.elo[npar]) wlo = nlo;
		if (S.ehi[npar]) whi = nhi;
		if ((s & 0xff) == 0) { // ---- wf_stripe_shrink (miniwfa.c:139-169): first and last diagonal of [wlo, whi] with a live cell anywhere in the ring
			auto alive = [&](int32_t d) -> bool {
				for (int j = 0; j < WS_NSLOT; ++j) {
					const int32_t sc = s - j;
					if (sc < 0) break;
					const int sl = sc % WS_NSLOT;
					const int32_t l2 = S.lo[sl], h2 = S.hi[sl];
					if (d < l2 || d > h2) continue;
					for (int a = 0; a < 5; ++a) {
						const int32_t k = VR(sl, a)[d - l2];
						if (k >= -1 && k < tl && d + k >= -1 && d + k < ql) return true;
					}
				}
				return false;
			};
			if (tid == 0) { S.tmin = 0x7fffffff; S.tmax = -0x7fffffff; }
			__syncthreads();
			int32_t v = 0x7fffffff;
			for (int32_t d0 = wlo; d0 <= whi; d0 += NT) {
				const int32_t d = d0 + tid;
				if (d <= whi && alive(d)) atomicMin(&S.tmin, d);
				__syncthreads();
				v = S.tmin;
				__syncthreads();
				if (v != 0x7fffffff) break;
			}
			wlo = v != 0x7fffffff ? v : whi + 1; // (the reference asserts that a live diagonal exists)
			v = -0x7fffffff;
			for (int32_t d0 = whi; d0 >= wlo; d0 -= NT) {
				const int32_t d = d0 - tid;
				if (d >= wlo && alive(d)) atomicMax(&S.tmax, d);
				__syncthreads();
				v = S.tmax;
				__syncthreads();
				if (v != -0x7fffffff) break;
			}
			whi = v != -0x7fffffff ? v : wlo - 1;
		}
	}
#undef VR
#undef OR
	R.s = s;
	if (R.status == WSEG_OK) R.last = S.last[s & 1];
	return R;
}

__global__ void __launch_bounds__(1024) k_wfa_seg(const wseg_job_t *__restrict__ jobs, const mga_wfa_prob_t *__restrict__ prob, const char *__restrict__ tseq, const char *__restrict__ qseq,
												  mga_wfa_res_t *__restrict__ res, wseg_out_t *__restrict__ out, uint32_t *__restrict__ pool, long long pool_cap, unsigned long long *pool_used,
												  char *__restrict__ ws_base, wseg_pen_t P)
{
	__shared__ wseg_lds_t S;
	__shared__ int32_t walk_s;
	const int tid = threadIdx.x;
	const wseg_job_t J = jobs[blockIdx.x];
	const wseg_ws_t W = wseg_carve(ws_base + J.ws_off, J);
	const mga_wfa_prob_t pb = prob[J.pi];
	const char *ts = tseq + pb.t_off, *qs = qseq + pb.q_off;
	const int32_t oe1 = P.o1 + P.e1, oe2 = P.o2 + P.e2;
	int32_t status = WSEG_OK, n_seg = 0;

	if (J.max_snap > 0) { // ---- pass 1 (a problem whose score bound lies below the step takes no snapshot: nothing to learn from it)
		const wseg_fwd_t F = wseg_forward<1>(S, W, J, P, ts, qs, 0);
		status = F.status, n_seg = F.n_snap;
		__syncthreads(); // the snapshots of every wave are visible to the walk
		if (tid == 0) { // wf_traceback_seg (miniwfa.c:528-549): one dependent read per snapshot
			int32_t last = F.last, bad = 0;
			for (int32_t j = n_seg - 1; status == WSEG_OK && j >= 0; --j) {
				const wseg_snap_t *M = &W.meta[j];
				if (last < 0 || last >= M->n) { bad = 1; break; }
				int32_t k = 0, m = 0;
				while (last >= m + 5 * M->w[k]) m += 5 * M->w[k], ++k;
				W.seg[j].s = M->max_s - (WS_NSLOT - 1) + k;
				W.seg[j].d = M->lo[k] + (last - m) % M->w[k];
				last = W.snapx[M->off + last];
			}
			walk_s = bad || (status == WSEG_OK && last != -1);
		}
		__syncthreads();
		if (status == WSEG_OK && walk_s) status = WSEG_E_WALK;
	}

	int32_t score = -1, n_cig = 0;
	int64_t n_iter = 0, cig_off = 0;
	if (status == WSEG_OK) { // ---- pass 2
		const wseg_fwd_t F = wseg_forward<2>(S, W, J, P, ts, qs, n_seg);
		status = F.status, n_iter = F.n_iter, score = F.s;
		__syncthreads(); // the traceback rows of every wave are visible to the walk
		if (status == WSEG_OK && tid < 64) { // ---- traceback (miniwfa.c:329-377) by the first wave: match runs by ballot, state walk uniform
			const int lane = tid;
			int32_t i = J.ql - 1, k = J.tl - 1, sc = F.s, last = F.last;
			int32_t cur_op = -1, cur_len = 0;
			bool overflow = false;
#define PUSH(op, len) do { \
				if (cur_op == (op)) cur_len += (len); \
				else { \
					if (cur_op >= 0) { if (n_cig < J.cigcap) { if (lane == 0) W.cig[n_cig] = (uint32_t)cur_len << 4 | (uint32_t)cur_op; } else overflow = true; ++n_cig; } \
					cur_op = (op), cur_len = (len); \
				} \
			} while (0)
			while (i >= 0 && k >= 0) {
				if (last == 0) {
					int32_t tot = 0;
					for (;;) {
						const bool eq = (i - lane >= 0 && k - lane >= 0) && qs[i - lane] == ts[k - lane];
						const uint64_t m = __ballot(eq);
						const int run = m == ~0ULL ? 64 : __builtin_ctzll(~m);
						tot += run, i -= run, k -= run;
						if (run < 64) break;
					}
					if (tot > 0) PUSH(7, tot);
					if (i < 0 || k < 0) break;
				}
				if (sc < 0 || sc > F.s) { overflow = true; n_cig = -1; break; } // (cannot happen: the walk stays inside the rows pass 2 wrote; never read outside the workspace)
				const int64_t at_tb = W.row[sc] + ((i - k) - W.rlo[sc]);
				if (at_tb < W.row[sc] || at_tb >= J.tbcap) { overflow = true; n_cig = -1; break; }
				const uint32_t x = W.tb[at_tb];
				const int32_t state = last == 0 ? (int32_t)(x & 7) : last;
				const int32_t ext = state > 0 ? (int32_t)(x >> (state + 2) & 1) : 0;
				if (state == 0) { PUSH(8, 1); --i, --k, sc -= P.x; }
				else if (state == 1) { PUSH(1, 1); --i, sc -= ext ? P.e1 : oe1; }
				else if (state == 3) { PUSH(1, 1); --i, sc -= ext ? P.e2 : oe2; }
				else if (state == 2) { PUSH(2, 1); --k, sc -= ext ? P.e1 : oe1; }
				else { PUSH(2, 1); --k, sc -= ext ? P.e2 : oe2; }
				last = state > 0 && ext ? state : 0;
			}
			if (n_cig >= 0) {
				if (i >= 0) PUSH(1, i + 1);
				else if (k >= 0) PUSH(2, k + 1);
				PUSH(15, 0); // flush the pending operator
			}
#undef PUSH
			if (lane == 0) {
				S.tmin = n_cig, S.tmax = n_cig < 0 ? WSEG_E_WALK : overflow ? WSEG_E_CIGAR : WSEG_OK;
				if (!overflow) {
					S.pool_off = atomicAdd(pool_used, (unsigned long long)n_cig);
					if ((long long)(S.pool_off + n_cig) > pool_cap) S.tmax = WSEG_E_POOL;
				}
			}
		}
		__syncthreads();
		if (status == WSEG_OK) {
			n_cig = S.tmin, status = S.tmax;
			if (status == WSEG_OK) {
				const unsigned long long o = S.pool_off;
				for (int32_t j = tid; j < n_cig; j += blockDim.x) pool[o + j] = W.cig[n_cig - 1 - j]; // built back-to-front
				cig_off = (int64_t)o;
			}
		}
	}
	if (tid == 0) {
		mga_wfa_res_t r;
		r.score = status == WSEG_OK ? score : -1;
		r.n_cigar = status == WSEG_OK ? n_cig : 0;
		r.cig_off = cig_off, r.status = status == WSEG_OK ? MGA_WFA_OK : status == WSEG_E_POOL ? MGA_WFA_POOL_FULL : MGA_WFA_RETRY_TIER, r.pad = 0, r.n_iter = n_iter;
		res[J.pi] = r;
		wseg_out_t o;
		o.score = r.score, o.n_snap = n_seg, o.status = status, o.pad = 0, o.n_iter = n_iter;
		out[blockIdx.x] = o;
	}
}

// ---- host: sizes -------------------------------------------------------------------------------
// W = tl + ql + 1 diagonals exist; at score s the band holds at most B(s) = min(W, 2 s + 1) of them.
// S = the score bound: an alignment of two gaps (all of the target deleted, all of the query inserted) always exists, as does one of min(tl, ql)
// mismatches and one gap of |tl - ql|; the optimum is no worse than the cheaper of them, and the kernel stops with an error there.
static const wseg_pen_t g_pen = { 4, 4, 2, 15, 1 };

static int64_t wseg_score_bound(int32_t tl, int32_t ql)
{
	const int64_t two = 2LL * g_pen.o2 + (int64_t)g_pen.e2 * ((int64_t)tl + ql);
	const int64_t mn = tl < ql ? tl : ql, g = tl < ql ? ql - tl : tl - ql;
	const int64_t g1 = g_pen.o1 + g_pen.e1 * g, g2 = g_pen.o2 + g_pen.e2 * g;
	const int64_t one = g_pen.x * mn + (g == 0 ? 0 : g1 < g2 ? g1 : g2);
	return two < one ? two : one;
}

// fills the capacities of J for (J.tl, J.ql, J.step); -1: the problem is beyond 32-bit indices
static int wseg_plan(wseg_job_t &J)
{
	const int64_t Wd = (int64_t)J.tl + J.ql + 1, S = wseg_score_bound(J.tl, J.ql), step = J.step;
	if (S > 0x3fffffff || Wd * 5 * WS_NSLOT > 0x7fffffff) return -1;
	auto B = [&](int64_t s) { return 2 * s + 1 < Wd ? 2 * s + 1 : Wd; };
	J.smax = (int32_t)S, J.wmax = (int32_t)B(S), J.cigcap = (int32_t)(Wd + 1);
	J.max_snap = (int32_t)(S / step); // a snapshot is taken before slice s + 1 when (s + 1) % step == 0
	int64_t cells = 0;
	for (int64_t j = 0; j < J.max_snap; ++j) {
		const int64_t ms = (j + 1) * step - 1;
		for (int64_t sc = ms - (WS_NSLOT - 1) < 0 ? 0 : ms - (WS_NSLOT - 1); sc <= ms; ++sc) cells += 5 * B(sc);
	}
	J.snapcap = cells;
	// pass 2: checkpoint j lies at a score in [(j+1) step - 17, (j+1) step - 1]; for step >= 17 these scores ascend strictly and every checkpoint is taken, so the
	// slice of score s >= step is at most 2 (s - (floor(s / step) step - 17)) + 1 wide.  Below 17 a checkpoint may be passed over (miniwfa.c:413): full band.
	int64_t tb = 1;
	for (int64_t s = 1; s <= S; ++s) {
		int64_t w = B(s);
		if (step >= WS_NSLOT && s >= step) { const int64_t n = 2 * (s - s / step * step + WS_NSLOT) + 1; if (n < w) w = n; }
		tb += w;
	}
	J.tbcap = tb;
	return 0;
}

static int64_t wseg_bytes_at(int32_t tl, int32_t ql, int32_t step)
{
	wseg_job_t J;
	memset(&J, 0, sizeof(J));
	J.tl = tl, J.ql = ql, J.step = step;
	if (wseg_plan(J) < 0) return -1;
	return wseg_parts(J).total;
}

// the step that needs the least memory, among 5000 x 2^(k/4): the reference's 5000 unless another is strictly smaller (never below the ring depth)
static int32_t wseg_choose_step(int32_t tl, int32_t ql)
{
	int32_t best = 5000;
	int64_t best_b = wseg_bytes_at(tl, ql, best);
	if (best_b < 0) return best;
	static const double q[4] = { 1.0, 1.189207115002721, 1.414213562373095, 1.681792830507429 };
	for (int k = 1; k <= 32; ++k)
		for (int sign = 1; sign >= -1; sign -= 2) {
			const int kk = sign * k, oct = kk >= 0 ? kk / 4 : -((-kk + 3) / 4), fr = kk - oct * 4;
			double v = 5000.0 * q[fr];
			v = oct >= 0 ? v * (double)(1LL << oct) : v / (double)(1LL << -oct);
			const int32_t st = (int32_t)(v + .5);
			if (st < WS_NSLOT || v > 1e9) continue;
			const int64_t b = wseg_bytes_at(tl, ql, st);
			if (b >= 0 && b < best_b) best_b = b, best = st;
		}
	return best;
}

static int32_t wseg_step_for(int32_t tl, int32_t ql, int32_t step)
{
	if (step > 0) return step;
	const char *e = getenv("MGA_WFA_SEG_STEP");
	if (e && atoi(e) > 0) return atoi(e);
	return wseg_choose_step(tl, ql);
}

extern "C" int64_t mga_wfa_seg_bytes(int32_t tl, int32_t ql, int32_t step)
{
	if (tl <= 0 || ql <= 0) return -1;
	return wseg_bytes_at(tl, ql, wseg_step_for(tl, ql, step));
}

extern "C" int32_t mga_wfa_seg_step(int32_t tl, int32_t ql) { return tl > 0 && ql > 0 ? wseg_step_for(tl, ql, 0) : -1; }

static long long g_seg_problems, g_seg_snapshots, g_seg_last_step, g_seg_ns, g_seg_cells;
extern "C" void mga_wfa_seg_stats(int64_t *problems, int64_t *snapshots, int reset)
{
	if (problems) *problems = __atomic_load_n(&g_seg_problems, __ATOMIC_RELAXED);
	if (snapshots) *snapshots = __atomic_load_n(&g_seg_snapshots, __ATOMIC_RELAXED);
	if (reset) { __atomic_store_n(&g_seg_problems, 0, __ATOMIC_RELAXED); __atomic_store_n(&g_seg_snapshots, 0, __ATOMIC_RELAXED); __atomic_store_n(&g_seg_ns, 0, __ATOMIC_RELAXED); __atomic_store_n(&g_seg_cells, 0, __ATOMIC_RELAXED); }
}
// what tools/wfa_seg_check.py reports next to the stats: wall seconds spent in this rung and wavefront cells of its second pass (= bytes of traceback it wrote, the band narrowed)
// since the last reset, and the step of the last problem it ran
extern "C" double mga_wfa_seg_seconds(void) { return 1e-9 * (double)__atomic_load_n(&g_seg_ns, __ATOMIC_RELAXED); }
extern "C" int64_t mga_wfa_seg_cells(void) { return __atomic_load_n(&g_seg_cells, __ATOMIC_RELAXED); }
extern "C" int32_t mga_wfa_seg_last_step(void) { return (int32_t)__atomic_load_n(&g_seg_last_step, __ATOMIC_RELAXED); }

// ---- host: driver ------------------------------------------------------------------------------
// Runs the n problems ids[] (NULL: 0 .. n-1) of d_prob, whose lengths the caller read back into h_tl / h_ql (indexed like ids), as many side by side as fit
// MGA_WFA_SEG_BUDGET bytes of workspace (default 32 GiB; a single problem may take more, up to what the device has free).  Results in d_res / the pool.
extern "C" int mga_dev_wfa_seg(mga_sctx_t *sc, const mga_wfa_job_t *jb, int n, const int32_t *ids, const int32_t *h_tl, const int32_t *h_ql, int32_t step)
{
	if (n <= 0) return 0;
	const double t0 = mga_wtime();
	hipStream_t st = (hipStream_t)sc->stream;
	int64_t budget = 32LL << 30; // (what the tier before this rung holds for one problem)
	struct ws_guard { mga_dbuf_t *b; ~ws_guard() { mga_dbuf_free(b); } } guard{&sc->wfa_seg_ws}; // a rare rung does not keep gigabytes for the rest of the run
	{ const char *e = getenv("MGA_WFA_SEG_BUDGET"); if (e && atoll(e) > 0) budget = atoll(e); }
	std::vector<wseg_job_t> job((size_t)n);
	std::vector<int64_t> bytes((size_t)n);
	for (int i = 0; i < n; ++i) {
		wseg_job_t &J = job[i];
		memset(&J, 0, sizeof(J));
		J.pi = ids ? ids[i] : i, J.tl = h_tl[i], J.ql = h_ql[i], J.step = wseg_step_for(J.tl, J.ql, step);
		if (wseg_plan(J) < 0) { mga_set_error("WFA low-memory rung: a problem of %d x %d bases is beyond its 32-bit indices", J.tl, J.ql); return -1; }
		bytes[i] = wseg_parts(J).total;
	}
	std::vector<wseg_out_t> out;
	for (int i0 = 0; i0 < n;) {
		int i1 = i0;
		int64_t tot = 0;
		int32_t wtop = 0;
		while (i1 < n && i1 - i0 < 1024 && (i1 == i0 || tot + bytes[i1] <= budget)) { job[i1].ws_off = tot; tot += bytes[i1]; if (job[i1].wmax > wtop) wtop = job[i1].wmax; ++i1; }
		const int nb = i1 - i0;
		if (mga_dbuf_reserve(&sc->wfa_seg_ws, (size_t)tot) < 0) { // whatever made the allocation fail, the message carries the computed figure
			size_t fr = 0, all = 0;
			if (hipMemGetInfo(&fr, &all) != hipSuccess) fr = 0;
			(void)hipGetLastError();
			mga_set_error("WFA low-memory rung: %d problem(s), the first of %d x %d bases at step %d, need %lld bytes of workspace; the device could not provide them (%lld bytes free)",
						  nb, job[i0].tl, job[i0].ql, job[i0].step, (long long)tot, (long long)fr);
			return -1;
		}
		if (mga_dbuf_reserve(&sc->wfa_seg_job, (size_t)nb * (sizeof(wseg_job_t) + sizeof(wseg_out_t))) < 0) return -1;
		wseg_job_t *d_job = (wseg_job_t*)sc->wfa_seg_job.p;
		wseg_out_t *d_out = (wseg_out_t*)(d_job + nb);
		if (mga_h2d(d_job, job.data() + i0, (size_t)nb * sizeof(wseg_job_t)) < 0) return -1;
		int nt = (wtop + 63) / 64 * 64;
		nt = nt < 64 ? 64 : nt > 1024 ? 1024 : nt;
		const int kid = MGA_K_WFA0 + 8; // accounted with the widest HBM tier, like the unbounded one (k_wfa.hip)
		mga_prof_begin(st, kid);
		hipLaunchKernelGGL(k_wfa_seg, dim3(nb), dim3(nt), 0, st, (const wseg_job_t*)d_job, jb->d_prob, jb->d_tseq, jb->d_qseq, jb->d_res, d_out, jb->d_pool, (long long)jb->pool_cap, jb->d_pool_used,
						   (char*)sc->wfa_seg_ws.p, g_pen);
		mga_prof_end(st, kid);
		MGA_HIP_CHECK(hipGetLastError());
		out.resize((size_t)nb);
		if (mga_ssync(sc) < 0 || mga_d2h(out.data(), d_out, (size_t)nb * sizeof(wseg_out_t)) < 0) return -1;
		for (int i = 0; i < nb; ++i) {
			const wseg_job_t &J = job[i0 + i];
			if (out[i].status != WSEG_OK) {
				static const char *why[] = { "", "reached its score bound", "outgrew its workspace", "lost its chain of snapshots", "found the CIGAR pool full", "outgrew its CIGAR buffer" };
				mga_set_error("WFA low-memory rung: a problem of %d x %d bases (step %d, score bound %d, %lld bytes) %s", J.tl, J.ql, J.step, J.smax, (long long)bytes[i0 + i],
							  why[out[i].status >= 1 && out[i].status <= 5 ? out[i].status : 0]);
				return -1;
			}
			__atomic_fetch_add(&g_seg_problems, 1LL, __ATOMIC_RELAXED);
			__atomic_fetch_add(&g_seg_snapshots, (long long)out[i].n_snap, __ATOMIC_RELAXED);
			__atomic_fetch_add(&g_seg_cells, (long long)out[i].n_iter, __ATOMIC_RELAXED);
			__atomic_store_n(&g_seg_last_step, (long long)J.step, __ATOMIC_RELAXED);
		}
		i0 = i1;
	}
	__atomic_fetch_add(&g_seg_ns, (long long)((mga_wtime() - t0) * 1e9), __ATOMIC_RELAXED);
	return 0;
}
