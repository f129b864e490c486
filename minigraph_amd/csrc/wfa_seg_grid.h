// wfa_seg_grid.h -- the grid-wide form of the low-memory rung (MGA_WFA_SEG_GRID=1): tiles of diagonals, a workgroup per tile.  PASS 1 always, PASS 2 unless MGA_WFA_SEG_GRID_P2=0.
// Part of k_wfa_seg.hip (included there: it uses that file's structs, wseg_lcp, wseg_walk, wseg_tail and wseg_finish); DESIGN.md 4 has the argument in full.
//
// Reach.  A cell of slice s at diagonal d reads diagonals d-1, d, d+1 of the slices s-1 .. s-16 (the penalties are 1 .. 16), and its extension reads the two
// sequences only.  So a tile that knows the diagonals [a-h, b+h] of the 17 ring slices can compute [a-(h-j), b+(h-j)] of the j-th slice after them, j = 1 .. h,
// without hearing from anyone: a trapezoid.  One launch of k_wseg_grid_block advances every tile of every problem by a block of n <= h scores.
//
// Tiles.  With [wlo0, whi0] the band at the start of the block, tile t owns [wlo0 + t TILE, wlo0 + (t+1) TILE - 1]; the first tile also owns everything to the left of
// the band and the last one the remainder (< 2 TILE) and everything to the right, i.e. the diagonals the band grows into.  The first tile therefore follows the lower
// band edge exactly and the last tile the upper one, as the workgroup form does; a tile in between needs neither: with n <= TILE its trapezoid lies inside
// [wlo0, whi0], which every slice of the block covers (between two trims a band edge only moves outwards), so for it every neighbour in a slice of the block is inside
// that slice; the slices from before the block have their bounds in the problem's state.
//
// Memory.  The rings stay where they were, in global memory, but indexed by the diagonal itself (d + tl) so that a tile needs no slice bound to find a cell; a tile
// writes its OWNED diagonals there and nothing else, so no two tiles write one cell.  Its halo -- the neighbours' diagonals [a-n, a-1] and [b+1, b+n] -- lives in a
// staging area of its own (2 sides x 17 slices x 10 arrays x BLOCK int32; 5 arrays in pass 2): k_wseg_grid_stage fills it from the neighbours' owned cells before the
// block, and the block kernel keeps the halo cells it recomputes there.  Without it a tile would read a ring cell that its owner, some scores ahead, has already reused
// for a newer slice.  LDS holds what the workgroup form keeps there: the slice bounds, and the termination and band-edge flags by the parity of the score.
//
// Synchronisation between workgroups is the kernel boundary and nothing else: stage | block | stage | block ..., enqueued back to back; no kernel here waits on
// another workgroup.  A problem's state is double-buffered by the parity of the block (read state[k & 1], write state[(k + 1) & 1]); every field of the state written
// has one writer: the first tile (s, the lower edge, the lower slice bounds), the last tile (the upper ones), tile 0 of the stage kernel (the snapshot counters).
//
// Events lie on launch boundaries: a block is cut short so that it ends at a multiple of 256 (trim) and at a score s with (s + 1) % step == 0 (snapshot).  The trim
// is found by every tile over its owned diagonals at the end of that block (atomicMin / atomicMax into the next state) and applied by every reader of the state;
// the snapshot is taken by the stage kernel, every tile for its owned diagonals.  Termination: only the owner of diagonal ql - tl reports it, at the lowest score
// of the block that terminates; it sets the problem's `done`, on which every later launch returns at once.  What other tiles computed past that score is dropped.
//
// PASS 2 (wseg_forward<2> on the same tiles; the stage and block kernels are templates over the pass).  No origins and no snapshots: the staging area holds the five
// value arrays only.  Its event is the checkpoint (miniwfa.c:413-416): a block is cut short so that it ends at the next checkpoint's score, and the view of the next
// launch collapses the band to the checkpoint's diagonal, which re-derives the tiling (one tile, growing back).  In the state, n_snap is the index of the next checkpoint
// and snap_used the traceback bytes handed out so far; tile 0 of the stage kernel writes both.
// Traceback rows.  A band edge moves outwards by one diagonal per score only if its edge cell is reachable (miniwfa.c:325-326), which the first and the last tile learn
// as they go; the other tiles cannot know the exact bounds of a slice of their block.  So the rows of a block are laid out for the widest the slices can be: slice
// s0 + j gets room for [max(wlo0 - j, -tl), min(whi0 + j, ql)], which every tile derives from the state.  The first tile, which knows the slice's true lower bound lo,
// writes rlo[s0 + j] = lo and row[s0 + j] = (the room's offset) + (lo - the room's lower bound): row + (d - rlo) is then the byte of diagonal d for the walk of
// wseg_tail as it stands, and each tile stores the bytes of its owned diagonals at the same address without reading row[].  The rows are a superset of the workgroup
// form's (equal where both edges move every score) and stay inside the tbcap of wseg_plan, whose bound is the same widest growth from the same checkpoints.  The last
// tile keeps the true upper bounds (in the origin ring's memory, dead after the snapshot walk), from which the tail counts the cells as the workgroup form does.
#define WSG_BIG 0x3fffffff

struct wseg_gjob_t { wseg_job_t J; int32_t tile, block; int64_t stage_off; }; // stage_off: of the tiles' staging areas in the launch's buffer
struct wseg_gstate_t { int32_t s, wlo, whi, trim, tmin, tmax, n_snap, pad; int64_t snap_used; int32_t lo[WS_NSLOT], hi[WS_NSLOT]; }; // (pass 2: n_snap / snap_used as above)
struct wseg_gres_t { int32_t done, status, score, last, n_snap, max_tiles; };

// what every tile derives, identically, from a problem's state at the start of a launch; pass 2 only: sid (the next checkpoint, after the one taken at s0 if any),
// room (0: the block was cut short by the traceback room), tb0 (traceback bytes handed out before the block)
struct wseg_gview_t { int32_t s0, n, wlo0, whi0, nt, snap, sid, room; int64_t tb0; };

// pass 2: bytes of the traceback rows of the first m slices of a block, each as wide as the band can have grown: sum over i = 1 .. m of min(whi0 + i, ql) - max(wlo0 - i, -tl) + 1
__device__ __forceinline__ int64_t wseg_grows(const wseg_gview_t &v, const wseg_job_t &J, int32_t m)
{
	const int64_t ch = J.ql - v.whi0 < m ? J.ql - v.whi0 : m, cl = v.wlo0 + J.tl < m ? v.wlo0 + J.tl : m; // scores until the edge is clipped
	const int64_t hi = ch * v.whi0 + ch * (ch + 1) / 2 + (m - ch) * J.ql;
	const int64_t lo = cl * v.wlo0 - cl * (cl + 1) / 2 - (m - cl) * J.tl;
	return hi - lo + m;
}

// seg / n_seg (pass 2): the checkpoints the snapshot walk left
template<int PASS>
__device__ __forceinline__ wseg_gview_t wseg_gview(const wseg_gstate_t &G, const wseg_gjob_t &g, const wseg_chk_t *seg, int32_t n_seg)
{
	wseg_gview_t v;
	v.s0 = G.s, v.wlo0 = G.wlo, v.whi0 = G.whi;
	if (G.trim) { // wf_stripe_shrink, as the workgroup form leaves the band: empty behind whi when no diagonal is alive
		v.wlo0 = G.tmin != 0x7fffffff ? G.tmin : G.whi + 1;
		v.whi0 = G.tmax != -0x7fffffff ? G.tmax : v.wlo0 - 1;
	}
	v.snap = 0, v.sid = 0, v.room = 1, v.tb0 = 0;
	int32_t n = g.block;
	if (256 - (v.s0 & 0xff) < n) n = 256 - (v.s0 & 0xff);
	if (PASS == 1) {
		const int32_t r = (v.s0 + 1) % g.J.step;
		if (g.J.step - r < n) n = g.J.step - r;
		v.snap = r == 0;
	} else {
		v.sid = G.n_snap, v.tb0 = G.snap_used;
		if (v.sid < n_seg && seg[v.sid].s == v.s0) { v.wlo0 = v.whi0 = seg[v.sid].d; ++v.sid; } // an `if`, after the trim: a checkpoint whose score has passed is never taken, nor any after it
		if (v.sid < n_seg && seg[v.sid].s > v.s0 && seg[v.sid].s - v.s0 < n) n = seg[v.sid].s - v.s0;
	}
	if (g.J.smax - v.s0 < n) n = g.J.smax - v.s0;
	if (PASS == 2) while (n > 0 && v.tb0 + wseg_grows(v, g.J, n) > g.J.tbcap) --n, v.room = 0;
	v.n = n;
	v.snap = v.snap && n > 0;
	const int32_t w0 = v.whi0 - v.wlo0 + 1;
	v.nt = w0 / g.tile > 1 ? w0 / g.tile : 1;
	return v;
}

struct wseg_gtile_t { int32_t a, b, first, last, ownlo, ownhi; };

__device__ __forceinline__ wseg_gtile_t wseg_gtile(const wseg_gview_t &v, const wseg_gjob_t &g, int t)
{
	wseg_gtile_t T;
	T.first = t == 0, T.last = t == v.nt - 1;
	T.a = v.wlo0 + t * g.tile;
	T.b = T.last ? v.whi0 : T.a + g.tile - 1;
	T.ownlo = T.first ? -g.J.tl : T.a;
	T.ownhi = T.last ? g.J.ql : T.b;
	return T;
}

// int32 of one tile's staging area: [side][slot][values 0-4, origins 5-9][BLOCK]; pass 2 (na = 5): [side][slot][values 0-4][BLOCK], in the same memory
__host__ __device__ __forceinline__ int64_t wseg_gstage_len(int32_t block, int na = 10) { return 2LL * WS_NSLOT * na * block; }

__global__ void k_wseg_grid_init(const wseg_gjob_t *__restrict__ gjobs, const mga_wfa_prob_t *__restrict__ prob, const char *__restrict__ tseq, const char *__restrict__ qseq,
								 wseg_gstate_t *__restrict__ state, wseg_gres_t *__restrict__ gres, char *__restrict__ ws_base)
{
	if (threadIdx.x != 0) return;
	const wseg_gjob_t g = gjobs[blockIdx.x];
	const wseg_job_t &J = g.J;
	const wseg_ws_t W = wseg_carve(ws_base + J.ws_off, J);
	const mga_wfa_prob_t pb = prob[J.pi];
	const char *ts = tseq + pb.t_off, *qs = qseq + pb.q_off;
	wseg_gres_t R;
	R.done = 0, R.status = WSEG_OK, R.score = 0, R.last = 0, R.n_snap = 0, R.max_tiles = 0;
	wseg_gstate_t G;
	G.s = 0, G.wlo = G.whi = 0, G.trim = 0, G.tmin = 0x7fffffff, G.tmax = -0x7fffffff, G.n_snap = 0, G.pad = 0, G.snap_used = 0;
	for (int k = 0; k < WS_NSLOT; ++k) G.lo[k] = 1, G.hi[k] = 0;
	G.lo[0] = G.hi[0] = 0;
	if (J.max_snap <= 0) R.done = 1; // the score bound lies below the step: no snapshot to take, pass 2 alone (as the workgroup form)
	else { // slice 0: the cell (0, -1) and its extension
		const int32_t room = J.tl < J.ql ? J.tl : J.ql;
		const int32_t k = -1 + wseg_lcp(ts, qs, room);
		const size_t o = (size_t)J.tl; // diagonal 0
		for (int a = 0; a < 5; ++a) {
			W.ring[(size_t)a * J.wmax + o] = a == 0 ? k : WS_NEG_INF;
			W.oring[(size_t)a * J.wmax + o] = a == 0 ? -1 : WS_NEG_INF;
		}
		if (k == J.tl - 1 && k == J.ql - 1) R.done = 1, R.last = -1; // score 0
	}
	state[2 * blockIdx.x] = G;
	state[2 * blockIdx.x + 1] = G;
	gres[blockIdx.x] = R;
}

// Before pass 2 (launched with one wave per problem): the walk over the chain of snapshots, which leaves the checkpoints in W.seg, then the state and slice 0 of pass 2.
// gres: how pass 1 ended; gres2: the outcome of pass 2, n_snap = the number of checkpoints.
__global__ void k_wseg_grid_init2(const wseg_gjob_t *__restrict__ gjobs, const mga_wfa_prob_t *__restrict__ prob, const char *__restrict__ tseq, const char *__restrict__ qseq,
								  wseg_gstate_t *__restrict__ state, const wseg_gres_t *__restrict__ gres, wseg_gres_t *__restrict__ gres2, char *__restrict__ ws_base)
{
	__shared__ int32_t walk_s;
	const wseg_gjob_t g = gjobs[blockIdx.x];
	const wseg_job_t &J = g.J;
	const wseg_ws_t W = wseg_carve(ws_base + J.ws_off, J);
	const wseg_gres_t R1 = gres[blockIdx.x];
	const int32_t status = wseg_walk(walk_s, J, W, R1.done ? R1.status : WSEG_E_BOUND, R1.n_snap, R1.last);
	if (threadIdx.x != 0) return;
	const mga_wfa_prob_t pb = prob[J.pi];
	const char *ts = tseq + pb.t_off, *qs = qseq + pb.q_off;
	wseg_gres_t R;
	R.done = status != WSEG_OK, R.status = status, R.score = 0, R.last = 0, R.n_snap = R1.n_snap, R.max_tiles = 0;
	wseg_gstate_t G;
	G.s = 0, G.wlo = G.whi = 0, G.trim = 0, G.tmin = 0x7fffffff, G.tmax = -0x7fffffff, G.n_snap = 0, G.pad = 0, G.snap_used = 1;
	for (int k = 0; k < WS_NSLOT; ++k) G.lo[k] = 1, G.hi[k] = 0;
	G.lo[0] = G.hi[0] = 0;
	if (status == WSEG_OK) { // slice 0: the cell (0, -1), its extension and its row of one byte
		const int32_t room = J.tl < J.ql ? J.tl : J.ql;
		const int32_t k = -1 + wseg_lcp(ts, qs, room);
		for (int a = 0; a < 5; ++a) W.ring[(size_t)a * J.wmax + (size_t)J.tl] = a == 0 ? k : WS_NEG_INF;
		W.row[0] = 0, W.rlo[0] = 0, W.oring[0] = 0, W.tb[0] = 0;
		if (k == J.tl - 1 && k == J.ql - 1) R.done = 1; // score 0
	}
	state[2 * blockIdx.x] = G;
	state[2 * blockIdx.x + 1] = G;
	gres2[blockIdx.x] = R;
}

// Before block k: the snapshot when one is due (pass 1), and the halos of every tile copied out of the neighbours' owned cells.  gres: the outcome of this pass.
template<int PASS>
__global__ void __launch_bounds__(1024) k_wseg_grid_stage(const wseg_gjob_t *__restrict__ gjobs, wseg_gstate_t *__restrict__ state, wseg_gres_t *__restrict__ gres,
														   char *__restrict__ ws_base, int par)
{
	constexpr int NA = PASS == 1 ? 10 : 5;
	const int tid = threadIdx.x, NT = blockDim.x, t = blockIdx.x;
	wseg_gres_t *R = gres + blockIdx.y;
	if (R->done) return;
	const wseg_gjob_t g = gjobs[blockIdx.y];
	const wseg_job_t &J = g.J;
	const wseg_gstate_t &G = state[2 * blockIdx.y + par];
	wseg_gstate_t &Gn = state[2 * blockIdx.y + (par ^ 1)];
	const wseg_ws_t W = wseg_carve(ws_base + J.ws_off, J);
	const wseg_gview_t v = wseg_gview<PASS>(G, g, W.seg, R->n_snap);
	if (t >= v.nt) return;
	if (v.n <= 0) { // the score bound is reached and the problem has not terminated (pass 2: or its traceback rows are full)
		if (t == 0 && tid == 0) { R->status = v.room ? WSEG_E_BOUND : WSEG_E_ROOM; R->done = 1; }
		return;
	}
	if (PASS == 2 && v.nt > (int32_t)gridDim.x) { // (cannot happen: the host sizes the grid by the widest the band can be; never run with a tile missing)
		if (t == 0 && tid == 0) { R->status = WSEG_E_ROOM; R->done = 1; }
		return;
	}
	const wseg_gtile_t T = wseg_gtile(v, g, t);
	const int32_t wmax = J.wmax, tl = J.tl;
	// the 17 slices of the ring, oldest first (scores s0-16 .. s0): bounds, and where each begins in the snapshot
	int32_t sl_lo[WS_NSLOT], sl_w[WS_NSLOT], sl_base[WS_NSLOT];
	int64_t ncell = 0;
	for (int k = 0; k < WS_NSLOT; ++k) {
		const int32_t sc = v.s0 - (WS_NSLOT - 1) + k;
		sl_lo[k] = 0, sl_w[k] = 0, sl_base[k] = (int32_t)ncell;
		if (sc >= 0) { const int sl = sc % WS_NSLOT; sl_lo[k] = G.lo[sl], sl_w[k] = G.hi[sl] - G.lo[sl] + 1; ncell += 5 * (int64_t)sl_w[k]; }
	}
	if (v.snap && (G.n_snap >= J.max_snap || G.snap_used + ncell > J.snapcap)) {
		if (t == 0 && tid == 0) { R->status = WSEG_E_ROOM; R->done = 1; }
		return;
	}
	if (t == 0 && tid == 0) { // the parts of the next state that the block kernel does not write
		Gn.tmin = 0x7fffffff, Gn.tmax = -0x7fffffff;
		if (PASS == 1) Gn.n_snap = G.n_snap + v.snap, Gn.snap_used = G.snap_used + (v.snap ? ncell : 0);
		else Gn.n_snap = v.sid, Gn.snap_used = v.tb0 + wseg_grows(v, J, v.n);
	}
	if (v.snap) { // ---- wf_snapshot1 (miniwfa.c:451-474) over the owned diagonals: X[t] = origin, origin = t, with t the cell's index in the snapshot
		int32_t *X = W.snapx + G.snap_used;
		for (int k = 0; k < WS_NSLOT; ++k) {
			const int32_t sc = v.s0 - (WS_NSLOT - 1) + k;
			if (sc < 0) continue;
			const int sl = sc % WS_NSLOT;
			const int32_t l = sl_lo[k], w = sl_w[k];
			const int32_t d0 = l > T.ownlo ? l : T.ownlo, d1 = l + w - 1 < T.ownhi ? l + w - 1 : T.ownhi;
			for (int a = 0; a < 5; ++a) {
				int32_t *O = W.oring + ((size_t)sl * 5 + a) * wmax + tl;
				for (int32_t d = d0 + tid; d <= d1; d += NT) { const int32_t x = sl_base[k] + a * w + (d - l); X[x] = O[d]; O[d] = x; }
			}
		}
		if (t == 0 && tid == 0) {
			wseg_snap_t *M = &W.meta[G.n_snap];
			for (int k = 0; k < WS_NSLOT; ++k) M->lo[k] = sl_lo[k], M->w[k] = sl_w[k];
			M->off = G.snap_used, M->max_s = v.s0, M->n = (int32_t)ncell;
		}
	}
	// ---- halos: values as they are; origins as they are, or, at a snapshot, as their owner is rewriting them right now (a function of the cell alone)
	int32_t *stage = (int32_t*)(ws_base + g.stage_off) + (int64_t)t * wseg_gstage_len(g.block, NA);
	for (int side = 0; side < 2; ++side) {
		if (side == 0 ? T.first : T.last) continue;
		for (int k = 0; k < WS_NSLOT; ++k) {
			const int32_t sc = v.s0 - (WS_NSLOT - 1) + k;
			if (sc < 0) continue;
			const int sl = sc % WS_NSLOT;
			const int32_t l = sl_lo[k], w = sl_w[k];
			for (int a = 0; a < 5; ++a) {
				const int32_t *Vg = W.ring + ((size_t)sl * 5 + a) * wmax + tl, *Og = W.oring + ((size_t)sl * 5 + a) * wmax + tl;
				int32_t *Vs = stage + (((int64_t)side * WS_NSLOT + sl) * NA + a) * g.block, *Os = Vs + 5 * (int64_t)g.block;
				for (int32_t i = tid; i < v.n; i += NT) {
					const int32_t d = side == 0 ? T.a - 1 - i : T.b + 1 + i;
					const bool in = d >= l && d < l + w; // outside its slice a cell is never read
					Vs[i] = in ? Vg[d] : WS_NEG_INF;
					if (PASS == 1) Os[i] = !in ? WS_NEG_INF : v.snap ? sl_base[k] + a * w + (d - l) : Og[d];
				}
			}
		}
	}
}

// Block k: every tile advances its trapezoid by v.n scores.  gres: the outcome of this pass.
template<int PASS>
__global__ void __launch_bounds__(1024) k_wseg_grid_block(const wseg_gjob_t *__restrict__ gjobs, const mga_wfa_prob_t *__restrict__ prob, const char *__restrict__ tseq,
														   const char *__restrict__ qseq, wseg_gstate_t *__restrict__ state, wseg_gres_t *__restrict__ gres, char *__restrict__ ws_base,
														   wseg_pen_t P, int par)
{
	constexpr int NA = PASS == 1 ? 10 : 5;
	__shared__ wseg_lds_t S;
	const int tid = threadIdx.x, NT = blockDim.x, t = blockIdx.x;
	wseg_gres_t *R = gres + blockIdx.y;
	if (R->done) return;
	const wseg_gjob_t g = gjobs[blockIdx.y];
	const wseg_job_t &J = g.J;
	const wseg_gstate_t &G = state[2 * blockIdx.y + par];
	wseg_gstate_t &Gn = state[2 * blockIdx.y + (par ^ 1)];
	const wseg_ws_t W = wseg_carve(ws_base + J.ws_off, J);
	const wseg_gview_t v = wseg_gview<PASS>(G, g, W.seg, R->n_snap);
	if (t >= v.nt || v.n <= 0 || (PASS == 2 && v.nt > (int32_t)gridDim.x)) return;
	const wseg_gtile_t T = wseg_gtile(v, g, t);
	const mga_wfa_prob_t pb = prob[J.pi];
	const char *ts = tseq + pb.t_off, *qs = qseq + pb.q_off;
	const int32_t tl = J.tl, ql = J.ql, wmax = J.wmax, n = v.n, hb = g.block;
	const int32_t oe1 = P.o1 + P.e1, oe2 = P.o2 + P.e2;
	int32_t *stage = (int32_t*)(ws_base + g.stage_off) + (int64_t)t * wseg_gstage_len(hb, NA);
	// the cell (slot, array 0-4 values / 5-9 origins, d): the ring when the tile owns d, else its own halo
	auto cell = [&](int slot, int arr, int32_t d) -> int32_t* {
		if (d >= T.ownlo && d <= T.ownhi) return (arr < 5 ? W.ring : W.oring) + ((size_t)slot * 5 + (arr < 5 ? arr : arr - 5)) * wmax + (d + tl);
		if (d < T.ownlo) return stage + ((int64_t)slot * NA + arr) * hb + (T.a - 1 - d);
		return stage + (((int64_t)WS_NSLOT + slot) * NA + arr) * hb + (d - T.b - 1);
	};
	// is diagonal d inside the slice of score sc?  (a slice of this block is unbounded on a side whose band edge this tile does not follow: see the head of the file)
	auto at = [&](int32_t sc, int32_t d, int &slot) -> bool {
		if (sc < 0) return false;
		slot = sc % WS_NSLOT;
		return d >= S.lo[slot] && d <= S.hi[slot];
	};
	if (tid < WS_NSLOT) { S.lo[tid] = G.lo[tid]; S.hi[tid] = G.hi[tid]; }
	if (tid < 2) S.term[tid] = 0;
	__syncthreads();

	int32_t wlo = v.wlo0, whi = v.whi0, term_j = 0;
	for (int32_t j = 1; j <= n; ++j) {
		const int32_t s1 = v.s0 + j;
		const int nslot = s1 % WS_NSLOT, np = s1 & 1;
		const int32_t nlo = T.first ? (wlo > -tl ? wlo - 1 : -tl) : T.a - (n - j);
		const int32_t nhi = T.last ? (whi < ql ? whi + 1 : ql) : T.b + (n - j);
		// pass 2: this slice's traceback row as every tile derives it -- room for [rlo_w, min(whi0 + j, ql)] at offset row_w (the head of the file)
		const int32_t rlo_w = v.wlo0 - j > -tl ? v.wlo0 - j : -tl;
		const int64_t row_w = PASS == 2 ? v.tb0 + wseg_grows(v, J, j - 1) : 0;
		if (tid == 0) {
			S.lo[nslot] = T.first ? nlo : -WSG_BIG; S.hi[nslot] = T.last ? nhi : WSG_BIG; // (no thread reads this slot's bounds while it computes slice s1)
			if (PASS == 2 && T.first) { W.row[s1] = row_w + (nlo - rlo_w); W.rlo[s1] = nlo; }
			if (PASS == 2 && T.last) W.oring[s1] = nhi; // the slice's upper bound, for the tail's count of cells
		}
		for (int32_t d = nlo + tid; d <= nhi; d += NT) { // ---- the cell (wf_next_tb, miniwfa.c:281-308; origins as wf_next_seg, :495-526), as in wseg_forward
			int sl_o1 = 0, sl_e1 = 0, sl_o2 = 0, sl_e2 = 0, sl_x = 0;
			const bool a_o1l = at(s1 - oe1, d - 1, sl_o1), a_e1l = at(s1 - P.e1, d - 1, sl_e1), a_o2l = at(s1 - oe2, d - 1, sl_o2), a_e2l = at(s1 - P.e2, d - 1, sl_e2);
			const bool a_o1r = at(s1 - oe1, d + 1, sl_o1), a_e1r = at(s1 - P.e1, d + 1, sl_e1), a_o2r = at(s1 - oe2, d + 1, sl_o2), a_e2r = at(s1 - P.e2, d + 1, sl_e2);
			const bool a_x = at(s1 - P.x, d, sl_x);
#define RDC(a_, sl_, arr_, d_) ((a_) ? *cell(sl_, arr_, d_) : WS_NEG_INF)
			const int32_t ho1l = RDC(a_o1l, sl_o1, 0, d - 1), e1l = RDC(a_e1l, sl_e1, 1, d - 1);
			const int32_t ho2l = RDC(a_o2l, sl_o2, 0, d - 1), e2l = RDC(a_e2l, sl_e2, 3, d - 1);
			const int32_t ho1r = RDC(a_o1r, sl_o1, 0, d + 1), f1r = RDC(a_e1r, sl_e1, 2, d + 1);
			const int32_t ho2r = RDC(a_o2r, sl_o2, 0, d + 1), f2r = RDC(a_e2r, sl_e2, 4, d + 1);
			const int32_t hx = RDC(a_x, sl_x, 0, d);
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
			int32_t H = hx + 1 >= h ? hx + 1 : h;
			const bool own = d >= T.ownlo && d <= T.ownhi;
			int32_t oH = 0, oE1 = 0, oF1 = 0, oE2 = 0, oF2 = 0;
			if (PASS == 1) {
				oE1 = bits & 0x08 ? RDC(a_e1l, sl_e1, 6, d - 1) : RDC(a_o1l, sl_o1, 5, d - 1);
				oF1 = bits & 0x10 ? RDC(a_e1r, sl_e1, 7, d + 1) : RDC(a_o1r, sl_o1, 5, d + 1);
				oE2 = bits & 0x20 ? RDC(a_e2l, sl_e2, 8, d - 1) : RDC(a_o2l, sl_o2, 5, d - 1);
				oF2 = bits & 0x40 ? RDC(a_e2r, sl_e2, 9, d + 1) : RDC(a_o2r, sl_o2, 5, d + 1);
				oH = z == 0 ? RDC(a_x, sl_x, 5, d) : z == 1 ? oE1 : z == 2 ? oF1 : z == 3 ? oE2 : oF2;
			} else if (own) W.tb[row_w + (d - rlo_w)] = (uint8_t)(bits | z); // (a recomputed halo cell stores none: its owner does)
#undef RDC
			const int32_t reach = H >= -1 || E1 >= -1 || F1 >= -1 || E2 >= -1 || F2 >= -1; // band bookkeeping (miniwfa.c:323-324)
			if (T.first && d == nlo) S.elo[np] = reach;
			if (T.last && d == nhi) S.ehi[np] = reach;
			// the extension of the cell (miniwfa.c:399-411 / :572-581) at once: no later slice of this score reads H; only the diagonal ql - tl can terminate
			if (!(H < -1 || d + H < -1 || H >= tl || d + H >= ql)) {
				int32_t room = tl - (H + 1);
				if (ql - (d + H + 1) < room) room = ql - (d + H + 1);
				const int32_t k = H + wseg_lcp(ts + H + 1, qs + d + H + 1, room);
				if (k == tl - 1 && d + k == ql - 1) {
					if (own) { S.last[np] = PASS == 1 ? oH : k == H ? (int32_t)z : 0; S.term[np] = 1; } // (a neighbour that sees it in its halo leaves it to the owner; pass 2: miniwfa.c:406-407)
				} else H = k;
			}
			*cell(nslot, 0, d) = H; *cell(nslot, 1, d) = E1; *cell(nslot, 2, d) = F1; *cell(nslot, 3, d) = E2; *cell(nslot, 4, d) = F2;
			if (PASS == 1) { *cell(nslot, 5, d) = oH; *cell(nslot, 6, d) = oE1; *cell(nslot, 7, d) = oF1; *cell(nslot, 8, d) = oE2; *cell(nslot, 9, d) = oF2; }
		}
		__syncthreads();
		if (S.term[np]) { term_j = j; break; }
		if (T.first && S.elo[np]) wlo = nlo;
		if (T.last && S.ehi[np]) whi = nhi;
	}
	if (term_j) { // uniform over the tile; only the owner of diagonal ql - tl comes here
		if (tid == 0) {
			R->score = v.s0 + term_j, R->last = S.last[(v.s0 + term_j) & 1], R->status = WSEG_OK;
			if (PASS == 1) R->n_snap = Gn.n_snap;
			__threadfence();
			R->done = 1;
		}
		return;
	}
	const int32_t s = v.s0 + n;
	const bool trim = (s & 0xff) == 0;
	if (tid == 0) { // this tile's part of the next state
		if (T.first) {
			Gn.s = s, Gn.wlo = wlo, Gn.trim = trim;
			for (int k = 0; k < WS_NSLOT; ++k) Gn.lo[k] = S.lo[k];
			if (v.nt > R->max_tiles) R->max_tiles = v.nt;
		}
		if (T.last) {
			Gn.whi = whi;
			for (int k = 0; k < WS_NSLOT; ++k) Gn.hi[k] = S.hi[k];
		}
	}
	if (trim) { // ---- wf_stripe_shrink (miniwfa.c:139-169), this tile's share: first and last of its owned diagonals of the band with a live cell anywhere in the ring
		const int32_t d0 = T.first ? wlo : T.a, d1 = T.last ? whi : T.b;
		auto alive = [&](int32_t d) -> bool {
			for (int q = 0; q < WS_NSLOT; ++q) {
				const int32_t sc = s - q;
				if (sc < 0) break;
				const int sl = sc % WS_NSLOT;
				if (d < S.lo[sl] || d > S.hi[sl]) continue;
				for (int a = 0; a < 5; ++a) {
					const int32_t k = W.ring[((size_t)sl * 5 + a) * wmax + (d + tl)];
					if (k >= -1 && k < tl && d + k >= -1 && d + k < ql) return true;
				}
			}
			return false;
		};
		if (tid == 0) { S.tmin = 0x7fffffff; S.tmax = -0x7fffffff; }
		__syncthreads();
		int32_t f = 0x7fffffff;
		for (int32_t c = d0; c <= d1; c += NT) {
			const int32_t d = c + tid;
			if (d <= d1 && alive(d)) atomicMin(&S.tmin, d);
			__syncthreads();
			f = S.tmin;
			__syncthreads();
			if (f != 0x7fffffff) break;
		}
		if (f != 0x7fffffff) { // (then a last one exists too, at f or above)
			int32_t l = -0x7fffffff;
			for (int32_t c = d1; c >= f; c -= NT) {
				const int32_t d = c - tid;
				if (d >= f && alive(d)) atomicMax(&S.tmax, d);
				__syncthreads();
				l = S.tmax;
				__syncthreads();
				if (l != -0x7fffffff) break;
			}
			if (tid == 0) { atomicMin(&Gn.tmin, f); atomicMax(&Gn.tmax, l); }
		}
	}
}

// Pass 2 and what goes with it, on one workgroup per problem: wseg_finish as the workgroup form runs it, from the outcome the tiles left in gres.
__global__ void __launch_bounds__(1024) k_wseg_grid_p2(const wseg_gjob_t *__restrict__ gjobs, const wseg_gres_t *__restrict__ gres, const mga_wfa_prob_t *__restrict__ prob,
														const char *__restrict__ tseq, const char *__restrict__ qseq, mga_wfa_res_t *__restrict__ res, wseg_out_t *__restrict__ out,
														uint32_t *__restrict__ pool, long long pool_cap, unsigned long long *pool_used, char *__restrict__ ws_base, wseg_pen_t P)
{
	__shared__ wseg_lds_t S;
	__shared__ int32_t walk_s;
	const wseg_job_t J = gjobs[blockIdx.x].J;
	const wseg_gres_t R = gres[blockIdx.x];
	const wseg_ws_t W = wseg_carve(ws_base + J.ws_off, J);
	const mga_wfa_prob_t pb = prob[J.pi];
	wseg_finish(S, walk_s, J, W, P, tseq + pb.t_off, qseq + pb.q_off, R.done ? R.status : WSEG_E_BOUND, R.n_snap, R.last, res, out + blockIdx.x, pool, pool_cap, pool_used);
}

// After the tiles of pass 2, on one workgroup per problem: the cells pass 2 computed (the true slice widths, summed), then wseg_tail -- the traceback walk by the first wave,
// the CIGAR into the pool and the result record -- from the outcome the tiles left in gres2.
__global__ void __launch_bounds__(1024) k_wseg_grid_tail(const wseg_gjob_t *__restrict__ gjobs, const wseg_gres_t *__restrict__ gres2, const mga_wfa_prob_t *__restrict__ prob,
														  const char *__restrict__ tseq, const char *__restrict__ qseq, mga_wfa_res_t *__restrict__ res, wseg_out_t *__restrict__ out,
														  uint32_t *__restrict__ pool, long long pool_cap, unsigned long long *pool_used, char *__restrict__ ws_base, wseg_pen_t P)
{
	__shared__ wseg_lds_t S;
	const wseg_job_t J = gjobs[blockIdx.x].J;
	const wseg_gres_t R = gres2[blockIdx.x];
	const wseg_ws_t W = wseg_carve(ws_base + J.ws_off, J);
	const mga_wfa_prob_t pb = prob[J.pi];
	const int32_t status = R.done ? R.status : WSEG_E_BOUND;
	if (threadIdx.x == 0) S.pool_off = 0;
	__syncthreads();
	if (status == WSEG_OK) {
		unsigned long long c = 0;
		for (int32_t s = 1 + threadIdx.x; s <= R.score; s += blockDim.x) c += (unsigned long long)(W.oring[s] - W.rlo[s] + 1);
		if (c) atomicAdd(&S.pool_off, c);
	}
	__syncthreads();
	const int64_t n_iter = (int64_t)S.pool_off; // (read before the barrier at which wseg_tail starts; it reuses the field after that barrier)
	wseg_tail(S, J, W, P, tseq + pb.t_off, qseq + pb.q_off, status, status == WSEG_OK ? R.score : -1, R.last, n_iter, R.n_snap, res, out + blockIdx.x, pool, pool_cap, pool_used);
}
