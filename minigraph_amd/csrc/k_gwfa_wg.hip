// k_gwfa_wg.hip -- ONE bridge (a GWFA call: gc_gwfa, gc_core.h; gfa-ed.c:190-302, 405-507) on a WORKGROUP of GWG_NW wavefronts.
//
// k_gchain_p2 gives every bridge a wavefront, and the launch lasts as long as its longest bridge: a call over a query gap of a couple of thousand bases runs for
// milliseconds on 64 lanes, most of it waiting on LDS / L2 round trips of ONE wavefront.  Here the few long bridges get 512 lanes and their wavefronts of cells live in LDS.
// The routine computes what gc_gwfa computes -- status, edit distance, the walk's vertices in order, the fall-through to the shortest-walk search -- cell for cell: the wave
// form (and through it the reference) is its specification, and every place where the ORDER of cells decides something keeps that order (below).
//
// NW = 8.  The state in LDS (below) leaves room for one workgroup per CU whatever NW is, so further waves cost no occupancy; the extension phase is a dependent chain of 8-byte
// loads per cell (HBM / L2), and with 512 lanes a wavefront of up to GWG_CAP = 1 024 cells is two trips of independent chains instead of sixteen.  A barrier of 8 waves costs
// about what one of 4 does (one s_barrier per wave); 16 waves would halve the trips once more but the phases between barriers are already short.
//
// Where things live (LDS: 160 KB per workgroup on gfx950; this kernel takes ~146 KB, one workgroup per CU):
//   buf[3][GWG_CAP]  96 KB  three buffers of 1 024 32-byte cells (gc_diag_t) that take turns as the current wavefront, the next one, and the scratch of the sort / the
//                            compaction.  GWG_CAP bounds a wavefront as it is consumed AND as it is produced, before the dedup (runs emit up to n + 2 per run, head cells push more).
//   head[1024]       32 KB  cells sitting on a vertex or query end (what the runs hand to the head loop, plus what the head loop queues itself): a wide wavefront reaches
//                            the end of a vertex, or of the query, nearly as one
//   done[512]         8 KB  the finished (vertex, diagonal) ranges: canonical union, ascending
//   fresh[512]        8 KB  this step's additions to it
//   z, A, G, P, scan partials, flags: < 2 KB.  The (vertex, query position) map `seen`, the traceback node map and the traceback forest stay in the job's HBM ARENA, through
//   gc_core.h's own routines: only the head loop touches them, a handful of times per step.
//   NOT staged: the query gap and the vertices' sequences.  gc_extend1 reads 8 bytes at byte offsets that differ from cell to cell; the gap is a few KB that L2 keeps, and
//   unaligned 8-byte reads through LDS would have to be split.
// A job that does not fit -- a wavefront beyond GWG_CAP, more head cells / ranges than their blocks hold, a sort the form does not replay (in-order cells out of order: never
// seen), an arena that runs out -- is HANDED BACK: the routine returns a status, nothing of the job has been written, and the wave form redoes it from the start.
//
// A step (gc_gw_step), phase by phase; `all` = the 512 lanes, `wave 0` = the first wavefront running gc_core.h's code REPLICATED the way k_gchain runs it:
//   R1 all     extension along the diagonals (gc_extend1, 8 bases per compare): independent per cell, a lane per cell.                                  barrier 1
//   R2 all     expansion.  The reference takes the RUNS of adjacent diagonals in order and emits, per run: the cell left of it, the run's cells, the cell right of it; cells that
//              ran off the vertex to `fresh`, cells on a vertex / query end to `head`.  A cell sees from its two neighbours whether it starts / ends a run, so every cell emits its
//              own 0-3 cells (left edge, itself, right edge -- the order inside a run and across runs), 0-3 ranges, 0-1 head cells; places come from ONE exclusive scan of the three
//              counts packed into an unsigned word: DPP scan inside the wave (dev_lcscan.h's steps), the waves' totals through LDS.                                       1 barrier per 512 cells + 1
//   H  wave 0  the head loop: inherently sequential (a head cell updates the last cells of the next wavefront, queues further head cells, enters the `seen` and traceback maps in
//              order -- the order in which traceback nodes get their ids).  It is the reference's loop on one wave, so ids come out in the sequential order.  Then this
//              step's ranges join `done` (gc_intv_add_wave: ~30 ranges, one wave's worth).                                                                barrier 3
//   D  all     gwf_dedup, only behind a step with head cells, as in the reference:
//              D1 is the wavefront out of order at all?                                                                                                  1 barrier
//              D2 if so: stable partition into in-order and flagged cells (scan), the flagged ones sorted -- up to 64 by rank (klib sorts them by insertion: stable), more by
//                 replaying klib's radix sort (gc_ksort) on wave 0 --, merged by rank: an in-order cell goes behind the flagged ones that are strictly smaller, a flagged one behind
//                 the in-order ones that are smaller or equal.                                                                                           3-4 barriers
//              D3 the first of the furthest cells of every (vertex, diagonal) that is not on a finished diagonal survives: verdict per cell, scan, compaction into the scratch
//                 buffer, which BECOMES the wavefront (the buffers rotate; nothing is compacted in place).                                              1 barrier per 512 cells + 1
//   P  wave 0  the pruning of every 16th step when more than max_chk = 1 000 cells are left (gc_gw_prune): with GWG_CAP = 1 024 nearly never.             1 barrier, when taken
// So a step without head cells costs 4 barriers for up to 512 cells, one with head cells 8 (in order) to 12 (sort).  Every barrier sits in code all 512 lanes run: whatever
// decides a branch around one (counts, flags, the status of wave 0's code) is read from LDS behind a barrier or computed alike by every lane.  gc_core.h's GC_TRY returns happen
// inside wave 0's replicated code only -- all of its lanes leave together -- and come out as a status in LDS that every lane reads behind the next barrier.
//
// Behind the GWFA call of a mapping job that found no walk, wave 0 runs the existing shortest-walk search (gc_shortest_k), as gc_bridge_walk does: handing the job back would
// run its GWFA call -- s_term steps, the longest kind there is -- a second time.
#include <stdio.h>
#include <stdlib.h>
#include "mga_dev.h"
#include "dev_common.h"
#include "dev_lcscan.h"
#define GC_PARSORT 5
#include "gc_core.h"

#define GWG_NW 8
#define GWG_T (64 * GWG_NW)
#define GWG_CAP 1024   // cells of a wavefront
#define GWG_HCAP 1024  // head cells of a step
#define GWG_DCAP 512   // finished ranges
#define GWG_FCAP 512   // ... added by one step

#define GWG_OK 0
#define GWG_BACK_CELLS 1   // a wavefront, the head cells or the ranges outgrew their block
#define GWG_BACK_SORT 2    // in-order cells out of order
#define GWG_BACK_ARENA 3   // the job's arena ran out

struct __attribute__((aligned(16))) gwg_lds_t {
	gc_diag_t buf[3][GWG_CAP];
	gc_diag_t head[GWG_HCAP];
	gc_intv_t done[GWG_DCAP];
	gc_intv_t fresh[GWG_FCAP];
	gc_gw_t z;                 // gc_core.h's state of the call: its vectors point into the blocks above (capacity = the block: they never grow), its maps into the arena
	gc_arena_t A;
	gc_graph_t G;
	gc_par_t P;
	uint32_t wsum[2][GWG_NW];   // the waves' totals of a scan, double-buffered: one barrier per scan
	int32_t nB, rc, reached, unsorted, b_unsorted, n_path, job_ok;
	long long draw;
	int32_t *path;
};
static_assert(sizeof(gwg_lds_t) <= 152 * 1024, "gwg_lds_t must leave room for the static LDS of gc_core.h's routines");

struct gwg_prob_t { const char *q; int32_t ql; uint32_t v0; int32_t off0; uint32_t v1; int32_t off1, max_lag, s_term; };

// inclusive sum over the wave's lanes by DPP, the steps of dev_lcscan.h's LC_SCAN on UNSIGNED words: the packed counts below use all 32 bits
__device__ __forceinline__ uint32_t gwg_wave_scan(uint32_t v)
{
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); /* row_bcast:15 into rows 1 and 3 */
	v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); /* row_bcast:31 into rows 2 and 3 */
	return v;
}

// exclusive prefix of `pack` over the workgroup's lanes in thread order, and the total; *par flips per call (which half of wsum this scan uses)
__device__ __forceinline__ uint32_t gwg_scan(gwg_lds_t &L, int *par, uint32_t pack, uint32_t *tot)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = (*par ^= 1);
	const uint32_t incl = gwg_wave_scan(pack);
	if (lane == 63) L.wsum[p][w] = incl;
	__syncthreads();
	uint32_t pre = 0, all = 0;
	for (int k = 0; k < GWG_NW; ++k) { const uint32_t s = L.wsum[p][k]; all += s; if (k < w) pre += s; }
	*tot = all;
	return pre + incl - pack;
}

// wave 0: the state of a call (gfa_ed_init, gc_gwfa's prologue)
__device__ int gwg_init(gwg_lds_t &L, const gwg_prob_t &pr, char *arena_mem, int64_t arena_bytes)
{
	gc_gw_t *z = &L.z;
	gc_arena_init(&L.A, arena_mem, arena_bytes, 0);
	memset(z, 0, sizeof *z);
	z->G = &L.G, z->ql = pr.ql, z->q = pr.q;
	z->max_chk = 1000, z->bw_dyn = 1000, z->max_lag = pr.max_lag, z->i_term = 500000000LL; /* gchain1.c:361-363 */
	z->head.a = L.head, z->head.m = GWG_HCAP;
	z->done.a = L.done, z->done.m = GWG_DCAP;
	z->fresh.a = L.fresh, z->fresh.m = GWG_FCAP;
	gc_diag_t c;
	memset(&c, 0, sizeof c);
	c.vd = gc_mk_vd(pr.v0, -pr.off0), c.k = pr.off0 - 1;
	L.buf[0][0] = c;
	{ gc_trace_t *t; GC_PUSH(&L.A, z->tr, t); t->v = -1, t->pre = -1; } /* root of the traceback forest (gfa-ed.c:568) */
	z->end_v = (uint32_t)-1, z->end_off = z->end_tb = -1;
	return GC_OK;
}

// wave 0: the head loop of gc_gw_step (gfa-ed.c:405-507) over z->head, pushing into B = z->wf[0] (a view of the next wavefront's buffer); then this step's ranges join `done`.
// The blocks do not grow: a head cell that could outgrow one ends the call with GWG_BACK_CELLS before it has pushed anything.
__device__ int gwg_heads(gwg_lds_t &L, uint32_t v1, int32_t off1, int do_dedup, int *reached)
{
	gc_arena_t *A = &L.A;
	gc_gw_t *z = &L.z;
	const gc_graph_t *G = z->G;
	gc_diag_v *B = &z->wf[0], *H = &z->head;
	int32_t head = 0;
	*reached = 0;
	while (head < H->n) {
		const gc_diag_t t = H->a[head++];
		const uint32_t v = (uint32_t)(t.vd >> 32), ooo = t.xo & 1;
		const int32_t d = (int32_t)t.vd - GC_DSHIFT, vl = gc_vlen(G, v);
		const int32_t k = gc_extend1(d, t.k, vl, gc_vseq(G, v), z->ql, z->q), qi = k + d;
		const uint32_t x0 = (t.xo >> 1) + ((uint32_t)(k - t.k) << 1);
		if (k + 1 < vl && qi + 1 < z->ql) { /* inside a vertex */
			int push1 = 1, push2 = 1;
			if (B->n + 3 > GWG_CAP) return GWG_BACK_CELLS;
			if (B->n >= 2) push1 = gc_diag_update(&B->a[B->n - 2], v, d - 1, k + 1, x0 + 1, ooo, t.t);
			if (B->n >= 1) push2 = gc_diag_update(&B->a[B->n - 1], v, d, k + 1, x0 + 2, ooo, t.t);
			if (push1) GC_TRY(gc_diag_push(A, B, v, d - 1, k + 1, x0 + 1, 1, t.t));
			if (push2 || push1) GC_TRY(gc_diag_push(A, B, v, d, k + 1, x0 + 2, 1, t.t));
			GC_TRY(gc_diag_push(A, B, v, d + 1, k, x0 + 1, ooo, t.t));
		} else if (qi + 1 < z->ql) { /* end of the vertex, query not finished: fan out over the arcs */
			const int32_t nv = gc_n_arc(G, v);
			const gc_arc_t *av = gc_arcs(G, v);
			int32_t n_ext = 0, tw;
			if (B->n + 2 * nv + 1 > GWG_CAP || H->n + nv > GWG_HCAP || z->fresh.n + 1 > GWG_FCAP) return GWG_BACK_CELLS;
			gc_intv_t *iv = &z->fresh.a[z->fresh.n++];
			iv->vd0 = gc_mk_vd(v, d), iv->vd1 = iv->vd0 + 1;
			GC_TRY(gc_trace_push(A, z, (int32_t)v, t.t, &tw));
			for (int32_t j = 0; j < nv; ++j) {
				const uint32_t w = av[j].w;
				const int32_t ol = av[j].ow;
				int absent;
				int32_t *dummy;
				GC_TRY(gc_u64map_put(A, &z->seen, (uint64_t)w << 32 | (uint32_t)(qi + 1), &dummy, &absent));
				if (z->q[qi + 1] == gc_vseq(G, w)[ol]) {
					++n_ext;
					if (absent) {
						gc_diag_t *p = &H->a[H->n++];
						p->vd = gc_mk_vd(w, qi + 1 - ol), p->k = ol, p->xo = (x0 + 2) << 1 | 1, p->t = tw, p->len = 0, p->pad_[0] = p->pad_[1] = 0;
					}
				} else if (absent) {
					GC_TRY(gc_diag_push(A, B, w, qi - ol, ol, x0 + 1, 1, tw));
					GC_TRY(gc_diag_push(A, B, w, qi + 1 - ol, ol, x0 + 2, 1, tw));
				}
			}
			if (nv == 0 || n_ext != nv) GC_TRY(gc_diag_push(A, B, v, d + 1, k, x0 + 1, 1, t.t));
		} else if (v1 == (uint32_t)-1 || (v == v1 && k == off1)) { /* query finished at the requested end */
			z->end_v = v, z->end_off = k, z->end_tb = t.t;
			B->n = 0;
			*reached = 1;
			return GC_OK;
		} else if (k + 1 < vl) { /* query finished inside a vertex: delete the next target base */
			if (B->n + 1 > GWG_CAP) return GWG_BACK_CELLS;
			GC_TRY(gc_diag_push(A, B, v, d - 1, k + 1, x0 + 1, ooo, t.t));
		} else if (v != v1) { /* query and vertex both finished, not the last vertex */
			const int32_t nv = gc_n_arc(G, v);
			const gc_arc_t *av = gc_arcs(G, v);
			int32_t tw;
			if (B->n + nv > GWG_CAP) return GWG_BACK_CELLS;
			GC_TRY(gc_trace_push(A, z, (int32_t)v, t.t, &tw));
			for (int32_t j = 0; j < nv; ++j) GC_TRY(gc_diag_push(A, B, av[j].w, qi - av[j].ow, av[j].ow, x0 + 1, 1, tw));
		}
	}
	if (do_dedup) { /* this step's finished diagonals (without a dedup they are dropped, as gc_gw_step drops them) */
		if (z->done.n + z->fresh.n > GWG_DCAP) return GWG_BACK_CELLS;
#if defined(__HIP_DEVICE_COMPILE__) /* (a device-only routine of gc_core.h) */
		GC_TRY(gc_intv_add_wave(A, &z->done, z->fresh.n, z->fresh.a));
#endif
	}
	z->fresh.n = 0;
	return GC_OK;
}

// wave 0: more than 64 flagged cells (c(j) = tmp[n - 1 - j], j < n_c) sorted the way klib's radix sort leaves them (not stable: replayed move by move, gc_ksort), into cs[]
__device__ int gwg_sort_flagged(gwg_lds_t &L, int32_t n, int32_t n_c, const gc_diag_t *tmp, gc_diag_t *cs)
{
	gc_arena_t *A = &L.A;
	const int64_t mark = A->top;
	gc_kv_t *kv;
	GC_ALLOC(A, gc_kv_t, kv, n_c);
	GC_PAR_FOR(i, n_c) kv[i].key = tmp[n - 1 - i].vd, kv[i].val = (uint64_t)i;
	gc_sync();
	GC_TRY(gc_ksort(A, kv, n_c, 8));
	gc_sync();
	GC_PAR_FOR(i, n_c) { gc_diag_t c = tmp[n - 1 - (int32_t)kv[i].val]; c.xo &= 0xfffffffeU; cs[i] = c; }
	gc_sync();
	A->top = mark;
	return GC_OK;
}

// wave 0: gwf_traceback (gfa-ed.c:509-522): the walk's vertices into the arena
__device__ int gwg_traceback(gwg_lds_t &L, int32_t **path, int32_t *n_path)
{
	gc_gw_t *z = &L.z;
	int32_t i = z->end_tb, n = 1, *p;
	while (i >= 0 && z->tr.a[i].v >= 0) ++n, i = z->tr.a[i].pre;
	GC_ALLOC(&L.A, int32_t, p, n);
	i = z->end_tb, n = 0;
	p[n++] = (int32_t)z->end_v;
	while (i >= 0 && z->tr.a[i].v >= 0) p[n++] = z->tr.a[i].v, i = z->tr.a[i].pre;
	for (i = 0; i < n >> 1; ++i) { const int32_t k = p[i]; p[i] = p[n - 1 - i], p[n - 1 - i] = k; }
	*path = p, *n_path = n;
	return GC_OK;
}

// The call, by all lanes of the workgroup; every lane returns the same status.  GWG_OK: *ed (-1: not reached), the walk in the arena (*path, *n_path), *peak = the
// largest wavefront.  Otherwise the job is handed back.  L.G must be set; the arena is the workgroup's.
__device__ int gwg_gwfa(gwg_lds_t &L, const gwg_prob_t &pr, char *arena_mem, int64_t arena_bytes, int32_t *ed, int32_t **path, int32_t *n_path, int32_t *peak)
{
	const int tid = threadIdx.x, wave = tid >> 6;
	int par = 0, cur = 0, bi = 1, ti = 2;
	int32_t n = 1, s = 0;
	int64_t n_iter = 0;
	*ed = -1, *path = 0, *n_path = 0, *peak = 1;
	__syncthreads(); // (the previous job's readers of L are through)
	if (wave == 0) { const int rc = gwg_init(L, pr, arena_mem, arena_bytes); if (tid == 0) L.rc = rc; }
	__syncthreads();
	if (L.rc != GC_OK) return GWG_BACK_ARENA;
	const gc_graph_t *G = &L.G;
	const int32_t ql = pr.ql;
	const char *q = pr.q;
	int reached = 0;
	while (n > 0) {
		gc_diag_t *a = L.buf[cur], *B = L.buf[bi], *tmp = L.buf[ti];
		int32_t nB = 0, nF = 0, nH = 0;
		int ovf = 0, f_ovf = 0;
		// ---- R1: extension ----
		for (int32_t i = tid; i < n; i += GWG_T) {
			const uint64_t vd = a[i].vd;
			const uint32_t v = (uint32_t)(vd >> 32);
			const int32_t k0 = a[i].k, k = gc_extend1((int32_t)vd - GC_DSHIFT, k0, gc_vlen(G, v), gc_vseq(G, v), ql, q);
			a[i].len = k - k0, a[i].xo += (uint32_t)(k - k0) << 2, a[i].k = k;
		}
		if (wave == 0) gc_u64map_clear(&L.z.seen);
		__syncthreads();
		// ---- R2: expansion, in the order of the runs ----
		for (int32_t base = 0; base < n; base += GWG_T) {
			const int32_t i = base + tid;
			const int in = i < n;
			gc_diag_t me;
			me.vd = 0, me.k = 0, me.len = 0, me.xo = 0, me.t = 0, me.pad_[0] = me.pad_[1] = 0;
			int keep0 = 0, keepM = 0, keepN = 0, fin0 = 0, finM = 0, finN = 0, at_end = 0;
			uint32_t mx = 0;
			int32_t mk = 0, mt = 0;
			if (in) {
				me = a[i];
				const int32_t vl = gc_vlen(G, (uint32_t)(me.vd >> 32)), d = (int32_t)me.vd - GC_DSHIFT;
				const int first = i == 0 || a[i - 1].vd + 1 != me.vd, last = i == n - 1 || a[i + 1].vd != me.vd + 1; // my cell starts / ends a run of adjacent diagonals
				mx = me.xo + 4, mk = me.k + 1, mt = me.t;                                                                // mismatch ...
				if (!first && a[i - 1].k > me.k + 1) mx = a[i - 1].xo + 2, mk = a[i - 1].k, mt = a[i - 1].t;             // ... unless the insertion from the left gets further
				if (!last && !(mk > a[i + 1].k + 1)) mx = a[i + 1].xo + 2, mt = a[i + 1].t, mk = a[i + 1].k + 1;         // deletion from the right, when it gets at least as far
				at_end = me.k == vl - 1 || d + me.k == ql - 1;
				const int32_t k0 = me.k + 1, kN = me.k;
				keep0 = first && (d - 1) + k0 < ql && k0 < vl, fin0 = first && !keep0 && k0 == vl;
				keepM = d + mk < ql && mk < vl, finM = !keepM && mk == vl;
				keepN = last && (d + 1) + kN < ql && kN < vl, finN = last && !keepN && kN == vl;
			}
			const uint32_t pack = (uint32_t)(keep0 + keepM + keepN) | (uint32_t)(fin0 + finM + finN) << 11 | (uint32_t)at_end << 22;
			uint32_t tot;
			const uint32_t ex = gwg_scan(L, &par, pack, &tot);
			const int32_t tB = (int32_t)(tot & 0x7ff), tF = (int32_t)(tot >> 11 & 0x7ff), tH = (int32_t)(tot >> 22 & 0x3ff);
			if (nB + tB > GWG_CAP || nH + tH > GWG_HCAP) { ovf = 1; break; } // (the same totals in every lane)
			if (nF + tF > GWG_FCAP) f_ovf = 1; // more ranges than the block holds: they matter only when this step dedups, i.e. has head cells (below)
			if (in) {
				gc_diag_t *b = &B[nB + (ex & 0x7ff)];
				gc_intv_t *fr = &L.fresh[f_ovf ? 0 : nF + (int32_t)(ex >> 11 & 0x7ff)];
				gc_diag_t c = me;
				c.len = 0;
				if (keep0) { c.vd = me.vd - 1, c.k = me.k + 1, c.xo = me.xo + 2, c.t = me.t; *b++ = c; }
				if (keepM) { c.vd = me.vd, c.k = mk, c.xo = mx, c.t = mt; *b++ = c; }
				if (keepN) { c.vd = me.vd + 1, c.k = me.k, c.xo = me.xo + 2, c.t = me.t; *b++ = c; }
				if (fin0 && !f_ovf) { fr->vd0 = me.vd - 1, fr->vd1 = me.vd; ++fr; }
				if (finM && !f_ovf) { fr->vd0 = me.vd, fr->vd1 = me.vd + 1; ++fr; }
				if (finN && !f_ovf) { fr->vd0 = me.vd + 1, fr->vd1 = me.vd + 2; ++fr; }
				if (at_end) { gc_diag_t h = me; h.xo |= 1; L.head[nH + (ex >> 22 & 0x3ff)] = h; }
			}
			nB += tB, nF += tF, nH += tH;
		}
		if (ovf || (f_ovf && nH != 0)) return GWG_BACK_CELLS;
		if (f_ovf) nF = 0; // (no head cells: no dedup, and the step's ranges are dropped, as gc_gw_step drops them)
		__syncthreads();
		// ---- H: the head loop and the finished ranges, on wave 0 ----
		const int do_dedup = nH != 0;
		if (wave == 0) {
			gc_gw_t *z = &L.z;
			z->wf[0].a = B, z->wf[0].n = nB, z->wf[0].m = GWG_CAP;
			z->head.n = nH, z->fresh.n = nF;
			int r = 0;
			const int rc = gwg_heads(L, pr.v1, pr.off1, do_dedup, &r);
			if (tid == 0) L.rc = rc, L.reached = r, L.nB = z->wf[0].n, L.unsorted = 0, L.b_unsorted = 0;
		}
		__syncthreads();
		if (L.rc != GC_OK) return L.rc == GC_E_ARENA ? GWG_BACK_ARENA : GWG_BACK_CELLS;
		reached = L.reached;
		nB = L.nB;
		if (reached) break;
		if (do_dedup) { // ---- D: gwf_dedup ----
			int uns = 0;
			for (int32_t i = tid; i < nB; i += GWG_T) if (i > 0 && B[i - 1].vd > B[i].vd) uns = 1;
			if (uns) L.unsorted = 1;
			__syncthreads();
			if (L.unsorted) { // in-order cells keep their place, the flagged ones are sorted, stable merge (gfa-ed.c:143-171)
				gc_diag_t *cs = a; // (the consumed wavefront's buffer: the sorted flagged cells)
				int32_t n_b = 0, n_c = 0;
				for (int32_t base = 0; base < nB; base += GWG_T) { // stable partition: in-order cells from the bottom of tmp, flagged ones from its top down
					const int32_t i = base + tid;
					const int in = i < nB;
					gc_diag_t me;
					int flag = 0;
					if (in) me = B[i], flag = me.xo & 1;
					uint32_t tot;
					const uint32_t ex = gwg_scan(L, &par, (uint32_t)(in && !flag) | (uint32_t)flag << 16, &tot);
					if (in) { if (flag) tmp[nB - 1 - (n_c + (int32_t)(ex >> 16))] = me; else tmp[n_b + (int32_t)(ex & 0xffff)] = me; }
					n_b += (int32_t)(tot & 0xffff), n_c += (int32_t)(tot >> 16);
				}
				__syncthreads();
				int bu = 0;
				for (int32_t i = tid; i < n_b; i += GWG_T) if (i > 0 && tmp[i - 1].vd > tmp[i].vd) bu = 1;
				if (bu) L.b_unsorted = 1;
				if (n_c <= 64) { // klib sorts up to 64 records by insertion, a stable sort: a cell's place is the number of cells with a smaller key, plus equal ones in front of it
					if (tid < n_c) {
						gc_diag_t me = tmp[nB - 1 - tid];
						int32_t r = 0;
						for (int32_t j = 0; j < n_c; ++j) { const uint64_t kj = tmp[nB - 1 - j].vd; r += (kj < me.vd) | ((kj == me.vd) & (j < tid)); }
						me.xo &= 0xfffffffeU;
						cs[r] = me;
					}
				} else if (wave == 0) { const int rc = gwg_sort_flagged(L, nB, n_c, tmp, cs); if (tid == 0) L.rc = rc; }
				__syncthreads();
				if (L.rc != GC_OK) return GWG_BACK_ARENA;
				if (L.b_unsorted) return GWG_BACK_SORT;
				for (int32_t i = tid; i < n_b; i += GWG_T) { // an in-order cell goes behind the flagged ones that are strictly smaller
					const gc_diag_t me = tmp[i];
					int32_t lo = 0, hi = n_c;
					while (lo < hi) { const int32_t m = (lo + hi) >> 1; if (cs[m].vd < me.vd) lo = m + 1; else hi = m; }
					B[i + lo] = me;
				}
				for (int32_t j = tid; j < n_c; j += GWG_T) { // a flagged cell goes behind the in-order ones that are smaller or equal
					const gc_diag_t me = cs[j];
					int32_t lo = 0, hi = n_b;
					while (lo < hi) { const int32_t m = (lo + hi) >> 1; if (tmp[m].vd <= me.vd) lo = m + 1; else hi = m; }
					B[j + lo] = me;
				}
				__syncthreads();
			}
			const int32_t n_done = L.z.done.n;
			int32_t m = 0;
			for (int32_t base = 0; base < nB; base += GWG_T) { // the first of the furthest cells of a (vertex, diagonal) stays, unless the diagonal is finished
				const int32_t i = base + tid;
				gc_diag_t me;
				int keep = 0;
				if (i < nB) {
					me = B[i];
					keep = 1;
					for (int32_t j = i - 1; j >= 0 && B[j].vd == me.vd; --j) if (!(B[j].k < me.k)) { keep = 0; break; } /* an earlier cell at least as far */
					if (keep) for (int32_t j = i + 1; j < nB && B[j].vd == me.vd; ++j) if (me.k < B[j].k) { keep = 0; break; } /* a later cell strictly further */
					if (keep && n_done > 0) {
						int32_t lo = 0, hi = n_done;
						while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (L.done[mid].vd1 <= me.vd) lo = mid + 1; else hi = mid; }
						keep = !(lo < n_done && me.vd >= L.done[lo].vd0);
					}
				}
				uint32_t tot;
				const uint32_t ex = gwg_scan(L, &par, (uint32_t)keep, &tot);
				if (keep) { me.len = 0; tmp[m + (int32_t)ex] = me; }
				m += (int32_t)tot;
			}
			__syncthreads();
			{ const int x = bi; bi = ti, ti = x; } // the scratch buffer is the wavefront now
			nB = m;
		}
		if (pr.max_lag > 0 && nB > 1000 && ((s + 1) & 0xf) == 0) { // ---- P: gfa-ed.c:286-307 ----
			__syncthreads(); // (every lane has read the count the head loop left in L.nB)
			if (wave == 0) { const int32_t m = gc_gw_prune(nB, L.buf[bi], (uint32_t)pr.max_lag, 1000); if (tid == 0) L.nB = m; }
			__syncthreads();
			nB = L.nB;
		}
		{ const int x = cur; cur = bi, bi = x; }
		n = nB;
		if (n > *peak) *peak = n;
		n_iter += n;
		if (n == 0) break;
		if (pr.s_term >= 0 && s >= pr.s_term) break;
		if (n_iter > 500000000LL) break;
		++s;
	}
	if (reached) {
		if (wave == 0) { int32_t *p = 0, np = 0; const int rc = gwg_traceback(L, &p, &np); if (tid == 0) L.rc = rc, L.path = p, L.n_path = np; }
		__syncthreads();
		if (L.rc != GC_OK) return GWG_BACK_ARENA;
		*path = L.path, *n_path = L.n_path, *ed = s;
	}
	return GWG_OK;
}

// ---- the mapping path: the bridges of the top gap classes of a chunk, a workgroup each, in front of k_gchain_p2 (k_gchain.hip) ------------------------------------
// Persistent workgroups draw blocks of 16 jobs and take those of a class below n_cls.  A job served is written exactly as k_gchain_p2 writes it and marked (read = GC_JOB_TAKEN):
// k_gchain_p2 passes it by.  A job handed back is left as it was: k_gchain_p2 takes it with its class.  ctl[9] / ctl[10] of the chunk count the two.
__global__ void __launch_bounds__(GWG_T) k_gwfa_wg_jobs(gc_job_t *jobs, int64_t jobs_cap, int32_t *mid, int64_t mid_cap, unsigned long long *sctl, int n_cls, gc_graph_t G_arg, gc_par_t P_arg,
														char *arena_mem, int64_t arena_bytes, unsigned long long *ctl)
{
	extern __shared__ __attribute__((aligned(16))) char gwg_smem[];
	gwg_lds_t &L = *(gwg_lds_t*)gwg_smem;
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	char *my_arena = arena_mem + (int64_t)blockIdx.x * arena_bytes;
	if (tid == 0) L.G = G_arg, L.P = P_arg;
	__syncthreads();
	long long n_jobs = (long long)sctl[1];
	if (n_jobs > jobs_cap) n_jobs = jobs_cap;
	for (;;) {
		__syncthreads(); // (everyone has read the previous draw)
		if (tid == 0) L.draw = (long long)atomicAdd(&sctl[5], 16ULL);
		__syncthreads();
		const long long base = L.draw;
		if (base >= n_jobs) break;
		for (long long j = base; j < base + 16 && j < n_jobs; ++j) {
			gc_job_t *jq = &jobs[j];
			if (gc_job_class(jq) >= n_cls) continue; // (the same job in every lane)
			const long long t0 = (long long)clock64();
			const gc_chain_t c0 = *jq->c0, c1 = *jq->c1;
			const int32_t span = jq->span, qs = c0.qe - span, qe = c1.qs + span;
			gwg_prob_t pr;
			pr.q = jq->qseq + qs, pr.ql = qe - qs, pr.v0 = c0.v, pr.off0 = c0.re - span, pr.v1 = c1.v, pr.off1 = c1.rs + span - 1, pr.max_lag = L.P.gdp_max_ed / 2, pr.s_term = L.P.gdp_max_ed;
			int32_t ed, *path, n_path, peak;
			const int st = gwg_gwfa(L, pr, my_arena, arena_bytes, &ed, &path, &n_path, &peak);
			if (wave == 0) { // what gc_bridge_walk does behind the call, and what k_gchain_p2 does with the result
				gc_arena_t *A = &L.A;
				int ok = st == GWG_OK, failed = 0;
				int32_t n_mid = 0, n_shortk = 0, status = GC_JOB_OK;
				const int32_t *midp = 0;
				long long mo = 0;
				if (ok && ed >= 0) n_mid = n_path - 2 > 0 ? n_path - 2 : 0, midp = path + 1; /* the inner vertices */
				else if (ok) { /* no walk within the edit bound: the shortest walk of the length the DP chose (gchain1.c:319-338) */
					gc_dst_t dst;
					gc_walkv_t *w = 0;
					int32_t n_w = 0;
					A->top = 0;
					memset(&dst, 0, sizeof dst);
					dst.v = c0.v ^ 1, dst.target_dist = c1.dist_pre, dst.target_hash = c1.hash_pre, dst.check_hash = 1;
					const int rc = gc_shortest_k(A, &L.G, c1.v ^ 1, 1, &dst, dst.target_dist, MG_MAX_SHORT_K, &w, &n_w);
					if (rc == GC_E_ARENA) ok = 0;
					else {
						n_shortk = 1;
						if (rc != GC_OK || n_w == 0 || dst.target_hash != dst.hash) failed = 1; /* "chain skiped" */
						else {
							n_mid = n_w - 2 > 0 ? n_w - 2 : 0;
							int32_t *p = (int32_t*)gc_alloc(A, (int64_t)(n_mid > 0 ? n_mid : 1) * 4);
							if (p == 0) ok = 0;
							else { for (int32_t x = n_w - 2, k = 0; x >= 1; --x) p[k++] = (int32_t)(w[x].v ^ 1); gc_sync(); midp = p; } /* found backwards: reverse and flip */
						}
					}
				}
				if (ok) {
					status = failed ? GC_JOB_FAILED : GC_JOB_OK;
					if (failed) n_mid = 0;
					if (status == GC_JOB_OK && n_mid > 0) {
						if (lane == 0) mo = (long long)atomicAdd(&sctl[2], (unsigned long long)n_mid);
						mo = __shfl(mo, 0);
						if (mo + n_mid > mid_cap) status = GC_JOB_ARENA, mo = 0;
						else for (int32_t x = lane; x < n_mid; x += 64) mid[mo + x] = midp[x];
					}
					if (lane == 0) {
						jq->status = status, jq->ed = ed, jq->n_mid = n_mid, jq->n_gwfa = 1, jq->n_shortk = n_shortk, jq->mid_off = mo;
						jq->n_fast = (int32_t)(((long long)clock64() - t0) >> 10); // (the job's duration in 1024-cycle units, as k_gchain_p2 leaves it)
						jq->read = GC_JOB_TAKEN;
						atomicAdd(&ctl[9], 1ULL);
						atomicMax(&ctl[7], (unsigned long long)A->peak);
					}
				} else if (lane == 0) atomicAdd(&ctl[10], 1ULL);
			}
		}
	}
}

extern "C" void mga_dev_gwfa_wg_shape(int *nw, int *cells) { *nw = GWG_NW, *cells = GWG_CAP; }

static int gwg_lds_attr(const void *kern)
{
	MGA_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(gwg_lds_t)));
	return 0;
}

// G, P: the launcher's gc_graph_t / gc_par_t (k_gchain.hip); arena: n_groups blocks of arena_bytes
extern "C" int mga_dev_gwfa_wg_jobs(mga_sctx_t *sc, void *jobs, int64_t jobs_cap, int32_t *mid, int64_t mid_cap, unsigned long long *sctl, int n_cls, const void *G, const void *P,
									char *arena, int64_t arena_bytes, int n_groups, unsigned long long *d_ctl)
{
	static int attr = 0;
	if (!attr) { if (gwg_lds_attr((const void*)k_gwfa_wg_jobs) < 0) return -1; attr = 1; }
	hipLaunchKernelGGL(k_gwfa_wg_jobs, dim3(n_groups), dim3(GWG_T), sizeof(gwg_lds_t), (hipStream_t)sc->stream, (gc_job_t*)jobs, jobs_cap, mid, mid_cap, sctl, n_cls,
					   *(const gc_graph_t*)G, *(const gc_par_t*)P, arena, arena_bytes, d_ctl);
	MGA_HIP_CHECK(hipGetLastError());
	return 0;
}

// ---- the stage entry: n bridge problems, either form (stage_api.hip: mga_gwfa_bridge_batch) -----------------------------------------------------------------------
// out per problem: ed, n_path, status, peak; the walk at path + i * path_cap (a walk longer than path_cap: status MGA_GWFA_E_ROOM, nothing written)
__device__ __forceinline__ void gwg_stage_prob(const mga_gwfa_prob_t *p, const char *qseq, gwg_prob_t *pr)
{
	pr->q = qseq + p->q_off, pr->ql = p->ql, pr->v0 = p->v0, pr->off0 = p->off0, pr->v1 = p->v1, pr->off1 = p->off1, pr->max_lag = p->max_lag, pr->s_term = p->s_term;
}

__global__ void __launch_bounds__(GWG_T) k_gwfa_wg_stage(int n_list, const int32_t *list, const mga_gwfa_prob_t *prob, const char *qseq, gc_graph_t G_arg, char *arena_mem, int64_t arena_bytes,
														 int32_t path_cap, int32_t *out, int32_t *path_out, unsigned long long *counter)
{
	extern __shared__ __attribute__((aligned(16))) char gwg_smem[];
	gwg_lds_t &L = *(gwg_lds_t*)gwg_smem;
	const int tid = threadIdx.x;
	char *my_arena = arena_mem + (int64_t)blockIdx.x * arena_bytes;
	if (tid == 0) L.G = G_arg;
	for (;;) {
		__syncthreads();
		if (tid == 0) L.draw = (long long)atomicAdd(counter, 1ULL);
		__syncthreads();
		const long long k = L.draw;
		if (k >= n_list) break;
		const int i = list[k];
		gwg_prob_t pr;
		gwg_stage_prob(&prob[i], qseq, &pr);
		int32_t ed, *path, n_path, peak;
		const int st = gwg_gwfa(L, pr, my_arena, arena_bytes, &ed, &path, &n_path, &peak);
		int32_t status = st == GWG_OK ? MGA_GWFA_WG : MGA_GWFA_BACK;
		if (st == GWG_OK && n_path > path_cap) status = MGA_GWFA_E_ROOM, ed = -1, n_path = 0;
		if (st == GWG_OK) for (int32_t x = tid; x < n_path; x += GWG_T) path_out[(int64_t)i * path_cap + x] = path[x];
		if (tid == 0) out[4 * i] = st == GWG_OK ? ed : -1, out[4 * i + 1] = st == GWG_OK ? n_path : 0, out[4 * i + 2] = status, out[4 * i + 3] = peak;
	}
}

// the wave form: gc_gwfa as k_gchain_p2 runs it, a wavefront per problem
__global__ void __launch_bounds__(64) k_gwfa_wave_stage(int n_list, const int32_t *list, const mga_gwfa_prob_t *prob, const char *qseq, gc_graph_t G_arg, char *arena_mem, int64_t arena_bytes,
														 int32_t path_cap, int32_t status_ok, int32_t *out, int32_t *path_out, unsigned long long *counter)
{
	__shared__ gc_graph_t G_lds;
	__shared__ gc_arena_t A_lds;
	const int lane = threadIdx.x;
	char *my_arena = arena_mem + (int64_t)blockIdx.x * arena_bytes;
	G_lds = G_arg;
	mga_wave_sync();
	for (;;) {
		long long k = 0;
		if (lane == 0) k = (long long)atomicAdd(counter, 1ULL);
		k = (long long)__builtin_amdgcn_readfirstlane((int32_t)k);
		if (k >= n_list) break;
		const int i = __builtin_amdgcn_readfirstlane(list[k]);
		gwg_prob_t pr;
		gwg_stage_prob(&prob[i], qseq, &pr);
		int32_t ed = -1, *path = 0, n_path = 0, status = status_ok;
		gc_arena_init(&A_lds, my_arena, arena_bytes, 0);
		const int rc = gc_gwfa(&A_lds, &G_lds, pr.ql, pr.q, pr.v0, pr.off0, pr.v1, pr.off1, pr.max_lag, pr.s_term, &ed, &path, &n_path);
		if (rc != GC_OK) status = MGA_GWFA_E_ROOM, ed = -1, n_path = 0;
		else if (n_path > path_cap) status = MGA_GWFA_E_ROOM, ed = -1, n_path = 0;
		mga_wave_sync();
		for (int32_t x = lane; x < n_path; x += 64) path_out[(int64_t)i * path_cap + x] = path[x];
		if (lane == 0) out[4 * i] = ed, out[4 * i + 1] = n_path, out[4 * i + 2] = status; // (out[4 i + 3], the peak, stays what the workgroup form left there, or 0)
		mga_wave_sync();
	}
}

// One launch over the listed problems, device pointers throughout; form 0: wave (status_ok says what a served problem reports), 1: workgroup.
extern "C" int mga_dev_gwfa_stage(mga_sctx_t *sc, const mga_didx_t *ix, int form, int n_list, const int32_t *d_list, const mga_gwfa_prob_t *d_prob, const char *d_qseq, char *d_arena,
								  int64_t arena_bytes, int n_groups, int32_t path_cap, int32_t status_ok, int32_t *d_out, int32_t *d_path, unsigned long long *d_counter)
{
	gc_graph_t G;
	if (n_list <= 0) return 0;
	if (ix->d_arc == 0 || ix->d_gseq_rc == 0) { mga_set_error("gwfa_bridge_batch needs the graph replica (mga_dev_graph_upload)"); return -1; }
	memset(&G, 0, sizeof G);
	G.arc = (const gc_arc_t*)ix->d_arc, G.idx = ix->d_arc_idx, G.seg_len = ix->d_seg_len, G.es = 0, G.seq_fw = ix->d_gseq, G.seq_rc = ix->d_gseq_rc, G.seq_off = ix->d_gseq_off;
	if (form == 1) {
		static int attr = 0;
		if (!attr) { if (gwg_lds_attr((const void*)k_gwfa_wg_stage) < 0) return -1; attr = 1; }
		hipLaunchKernelGGL(k_gwfa_wg_stage, dim3(n_groups), dim3(GWG_T), sizeof(gwg_lds_t), (hipStream_t)sc->stream, n_list, d_list, d_prob, d_qseq, G, d_arena, arena_bytes, path_cap, d_out, d_path, d_counter);
	} else hipLaunchKernelGGL(k_gwfa_wave_stage, dim3(n_groups), dim3(64), 0, (hipStream_t)sc->stream, n_list, d_list, d_prob, d_qseq, G, d_arena, arena_bytes, path_cap, status_ok, d_out, d_path, d_counter);
	MGA_HIP_CHECK(hipGetLastError());
	return 0;
}
