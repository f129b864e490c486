// k_gwfa_wgx.hip -- the WIDE workgroup form of one bridge (a GWFA call: gc_gwfa, gc_core.h; gfa-ed.c:190-302, 405-507): wavefronts of up to GWX_WIDE = 3 072 cells.
//
// k_gwfa_wg.hip holds three buffers of 1 024 32-byte cells in LDS and hands a bridge back as soon as a wavefront of cells, before or after the dedup, passes 1 024: the
// bridges of long, diverged gaps -- every bridge between contigs' chains -- end on the lone wavefront of the wave form.  The reference prunes only every 16th step, and only by
// band and lag (gfa-ed.c:286-307), so a wavefront of 1 000 cells grows by two cells per run and step in between and by three per head cell: a form that serves these bridges
// needs about three times the room, which 32-byte cells in three LDS buffers cannot give (160 KB).  This form computes what gc_gwfa computes, cell for cell, with another layout:
//
//   LDS (~140 KB, one workgroup of GWX_NW = 8 wavefronts per CU):
//     buf[2]      120 KB  TWO buffers of 3 072 cells as a STRUCTURE OF ARRAYS, 20 bytes per cell (vd 8, k 4, xo 4, t 4; gc_diag_t's `len` and padding are not kept: `len` is
//                         dead between steps).  Lane i reads vd[i], k[i], ...: consecutive lanes hit consecutive banks, where the 32-byte cell of the 1 024-cell form strides
//                         over 8 banks.  The two take turns as the wavefront that is consumed and the one that is produced.
//     done[1024]   16 KB  the finished (vertex, diagonal) ranges: every lane searches them in the dedup
//     z, A, G, scan partials, flags: < 2 KB
//   HBM (the front of the workgroup's arena block, 236 KB, L2-resident):
//     S            60 KB  the third buffer, same layout: only the dedup of a wavefront that is OUT OF ORDER uses it (the in-order cells of the stable partition), written and
//                         read with lane i at element i of each array
//     hb[3072]     96 KB  gc_diag_t cells: what the head loop pushes.  The head loop is gc_core.h's sequential code on wave 0 and works on 32-byte cells (gc_diag_push,
//                         gc_diag_update); it only ever touches the LAST TWO cells of the next wavefront and appends, so it gets those two and an empty vector behind them, and
//                         all lanes copy its cells behind the buffer's own afterwards
//     head[2048]   64 KB  cells on a vertex / query end: written by every lane in the expansion, read by wave 0 once each
//     fresh[1024]  16 KB  this step's finished ranges, consumed by gc_intv_add_wave
//   then the job's arena proper: the `seen` map, the traceback node map and forest, the sort's replay scratch.
//
// A step, phase by phase (`all` = 512 lanes; a scan is one barrier per 512 cells):
//   R1 all     extension (gc_extend1)                                                                                        barrier 1
//   R2 all     expansion in the order of the runs, as in k_gwfa_wg.hip: places from one packed exclusive scan                 1 per 512 cells + 1
//   H  wave 0  only when the step has head cells: head loop on hb, ranges into `done`; then all lanes append hb                 2 barriers
//   D  all     gwf_dedup, only behind head cells:
//              D1 out of order at all?                                                                                       1 barrier
//              D2 if so: stable partition (in-order cells -> S, flagged cells -> the consumed buffer), the flagged cells sorted BY RANK ON ALL 8 WAVES whatever their
//                 number (below), merged by rank into the consumed buffer                                                     1 per 512 cells + 3
//              D3 survivors compacted into the other buffer                                                                  1 per 512 cells + 1
//   P  all     the pruning of every 16th step above 1 000 cells (gc_gw_prune), on all waves: the cell with the largest edit count, first of equals, from a max-reduction
//              over (edits << 32 | ~index); verdict per cell, scan, compaction into the other buffer                           1 per 512 cells + 2, when taken
// A step without head cells costs 3 barriers + 1 per 512 cells and no wave-0 phase at all.
//
// THE SORT.  The sequential routine sorts the flagged cells with klib's radix sort (gc_diag_sort -> gc_ksort), which is NOT stable above 64 records.  Here every flagged cell
// takes the place (cells with a smaller key) + (cells with an equal key in front of it): the stable order.  The two orders differ only inside groups of equal key vd, and the
// sort is always followed by D3, which keeps ONE cell per vd: the first of those with the largest k, in-order cells (which the merge puts in front, in their own order, in both
// routines) before flagged ones.  So the outcome depends on the order of the flagged cells of a group only if two of them share vd AND k and differ in what they carry
// (edits, traceback id).  Every cell looks for such a twin while it counts its rank; if none exists, keys (vd, k) are distinct among cells that differ and the wavefront after
// D3 is the sequential routine's, cell for cell.  If one exists (and there are more than 64 flagged cells: up to 64 klib sorts by insertion, the stable order), wave 0 replays
// klib's moves (gc_ksort) for this step -- a slower step, not a hand-back.
//
// HANDED BACK (status, nothing written, the wave form redoes the bridge): more than 3 072 cells in a wavefront before the dedup, more than 2 048 head cells or 1 024 ranges in a
// step, in-order cells out of order (never seen), an exhausted arena.
#include <stdio.h>
#include <stdlib.h>
#include "mga_dev.h"
#include "dev_common.h"
#define GC_PARSORT 5
#include "gc_core.h"

#define GWX_NW 8
#define GWX_T (64 * GWX_NW)
#define GWX_WIDE 3072  // cells of a wavefront, consumed or produced
#define GWX_HCAP 2048  // head cells of a step
#define GWX_DCAP 1024  // finished ranges
#define GWX_FCAP 1024  // ... added by one step

#define GWX_OK 0
#define GWX_BACK_CELLS 1
#define GWX_BACK_SORT 2
#define GWX_BACK_ARENA 3

struct gwx_cells_t { uint64_t vd[GWX_WIDE]; int32_t k[GWX_WIDE]; uint32_t xo[GWX_WIDE]; int32_t t[GWX_WIDE]; };

struct __attribute__((aligned(16))) gwx_lds_t {
	gwx_cells_t buf[2];
	gc_intv_t done[GWX_DCAP];
	gc_gw_t z;                  // gc_core.h's state of the call: its vectors point into the blocks (they never grow), its maps into the arena
	gc_arena_t A;
	gc_graph_t G;
	uint32_t wsum[2][GWX_NW];   // the waves' totals of a scan, double-buffered: one barrier per scan
	unsigned long long red[GWX_NW];
	int32_t nB, rc, reached, unsorted, b_unsorted, twin, n_path;
	int32_t max_flag, n_replay; // of this workgroup's problems: the most flagged cells one dedup sorted, the steps replayed with gc_ksort (mga_gwfa_wgx_stats)
	long long draw;
	int32_t *path;
};
static_assert(sizeof(gwx_lds_t) <= 152 * 1024, "gwx_lds_t must leave room for the static LDS of gc_core.h's routines");

struct __attribute__((aligned(16))) gwx_hbm_t { gwx_cells_t S; gc_diag_t hb[GWX_WIDE]; gc_diag_t head[GWX_HCAP]; gc_intv_t fresh[GWX_FCAP]; };
static_assert(sizeof(gwx_hbm_t) % 16 == 0, "the arena behind gwx_hbm_t stays 16-byte aligned");

struct gwx_prob_t { const char *q; int32_t ql; uint32_t v0; int32_t off0; uint32_t v1; int32_t off1, max_lag, s_term; };

__device__ __forceinline__ gc_diag_t gwx_ld(const gwx_cells_t *b, int32_t i)
{
	gc_diag_t c;
	c.vd = b->vd[i], c.k = b->k[i], c.len = 0, c.xo = b->xo[i], c.t = b->t[i], c.pad_[0] = c.pad_[1] = 0;
	return c;
}
__device__ __forceinline__ void gwx_st(gwx_cells_t *b, int32_t i, uint64_t vd, int32_t k, uint32_t xo, int32_t t) { b->vd[i] = vd, b->k[i] = k, b->xo[i] = xo, b->t[i] = t; }

// inclusive sum over the wave's lanes by DPP on unsigned words (the packed counts use all 32 bits)
__device__ __forceinline__ uint32_t gwx_wave_scan(uint32_t v)
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
__device__ __forceinline__ uint32_t gwx_scan(gwx_lds_t &L, int *par, uint32_t pack, uint32_t *tot)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = (*par ^= 1);
	const uint32_t incl = gwx_wave_scan(pack);
	if (lane == 63) L.wsum[p][w] = incl;
	__syncthreads();
	uint32_t pre = 0, all = 0;
	for (int k = 0; k < GWX_NW; ++k) { const uint32_t s = L.wsum[p][k]; all += s; if (k < w) pre += s; }
	*tot = all;
	return pre + incl - pack;
}

// wave 0: the state of a call (gfa_ed_init, gc_gwfa's prologue)
__device__ int gwx_init(gwx_lds_t &L, gwx_hbm_t *Hm, const gwx_prob_t &pr, char *arena_mem, int64_t arena_bytes)
{
	gc_gw_t *z = &L.z;
	gc_arena_init(&L.A, arena_mem, arena_bytes, 0);
	memset(z, 0, sizeof *z);
	z->G = &L.G, z->ql = pr.ql, z->q = pr.q;
	z->max_chk = 1000, z->bw_dyn = 1000, z->max_lag = pr.max_lag, z->i_term = 500000000LL; /* gchain1.c:361-363 */
	z->head.a = Hm->head, z->head.m = GWX_HCAP;
	z->done.a = L.done, z->done.m = GWX_DCAP;
	z->fresh.a = Hm->fresh, z->fresh.m = GWX_FCAP;
	gwx_st(&L.buf[0], 0, gc_mk_vd(pr.v0, -pr.off0), pr.off0 - 1, 0, 0);
	{ gc_trace_t *t; GC_PUSH(&L.A, z->tr, t); t->v = -1, t->pre = -1; } /* root of the traceback forest (gfa-ed.c:568) */
	z->end_v = (uint32_t)-1, z->end_off = z->end_tb = -1;
	return GC_OK;
}

// wave 0: the head loop of gc_gw_step (gfa-ed.c:405-507) over z->head, pushing into B = z->wf[0]: the LAST cells of the next wavefront (at most two on entry) and what the
// loop appends; `base` cells lie in front of them in the LDS buffer.  Then this step's ranges join `done`.  The blocks do not grow: a head cell that could outgrow one ends
// the call with GWX_BACK_CELLS before it has pushed anything.
__device__ int gwx_heads(gwx_lds_t &L, int32_t base, uint32_t v1, int32_t off1, int *reached)
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
			if (base + B->n + 3 > GWX_WIDE) return GWX_BACK_CELLS;
			if (B->n >= 2) push1 = gc_diag_update(&B->a[B->n - 2], v, d - 1, k + 1, x0 + 1, ooo, t.t);
			if (B->n >= 1) push2 = gc_diag_update(&B->a[B->n - 1], v, d, k + 1, x0 + 2, ooo, t.t);
			if (push1) GC_TRY(gc_diag_push(A, B, v, d - 1, k + 1, x0 + 1, 1, t.t));
			if (push2 || push1) GC_TRY(gc_diag_push(A, B, v, d, k + 1, x0 + 2, 1, t.t));
			GC_TRY(gc_diag_push(A, B, v, d + 1, k, x0 + 1, ooo, t.t));
		} else if (qi + 1 < z->ql) { /* end of the vertex, query not finished: fan out over the arcs */
			const int32_t nv = gc_n_arc(G, v);
			const gc_arc_t *av = gc_arcs(G, v);
			int32_t n_ext = 0, tw;
			if (base + B->n + 2 * nv + 1 > GWX_WIDE || H->n + nv > GWX_HCAP || z->fresh.n + 1 > GWX_FCAP) return GWX_BACK_CELLS;
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
			if (base + B->n + 1 > GWX_WIDE) return GWX_BACK_CELLS;
			GC_TRY(gc_diag_push(A, B, v, d - 1, k + 1, x0 + 1, ooo, t.t));
		} else if (v != v1) { /* query and vertex both finished, not the last vertex */
			const int32_t nv = gc_n_arc(G, v);
			const gc_arc_t *av = gc_arcs(G, v);
			int32_t tw;
			if (base + B->n + nv > GWX_WIDE) return GWX_BACK_CELLS;
			GC_TRY(gc_trace_push(A, z, (int32_t)v, t.t, &tw));
			for (int32_t j = 0; j < nv; ++j) GC_TRY(gc_diag_push(A, B, av[j].w, qi - av[j].ow, av[j].ow, x0 + 1, 1, tw));
		}
	}
	if (z->done.n + z->fresh.n > GWX_DCAP) return GWX_BACK_CELLS; /* this step's finished diagonals */
#if defined(__HIP_DEVICE_COMPILE__) /* (a device-only routine of gc_core.h) */
	GC_TRY(gc_intv_add_wave(A, &z->done, z->fresh.n, z->fresh.a));
#endif
	z->fresh.n = 0;
	return GC_OK;
}

// wave 0: the flagged cells F[0 .. n_c) in the order klib's radix sort leaves them (not stable: replayed move by move, gc_ksort), into out[0 .. n_c)
__device__ int gwx_sort_replay(gwx_lds_t &L, int32_t n_c, const gwx_cells_t *F, gwx_cells_t *out)
{
	gc_arena_t *A = &L.A;
	const int64_t mark = A->top;
	gc_kv_t *kv;
	GC_ALLOC(A, gc_kv_t, kv, n_c);
	GC_PAR_FOR(i, n_c) kv[i].key = F->vd[i], kv[i].val = (uint64_t)i;
	gc_sync();
	GC_TRY(gc_ksort(A, kv, n_c, 8));
	gc_sync();
	GC_PAR_FOR(i, n_c) { const int32_t j = (int32_t)kv[i].val; gwx_st(out, i, F->vd[j], F->k[j], F->xo[j] & 0xfffffffeU, F->t[j]); }
	gc_sync();
	A->top = mark;
	return GC_OK;
}

// wave 0: gwf_traceback (gfa-ed.c:509-522): the walk's vertices into the arena
__device__ int gwx_traceback(gwx_lds_t &L, int32_t **path, int32_t *n_path)
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

// The call, by all lanes of the workgroup; every lane returns the same status.  GWX_OK: *ed (-1: not reached), the walk in the arena (*path, *n_path), *peak = the
// largest wavefront.  Otherwise the job is handed back.  L.G must be set; block = the workgroup's arena block of block_bytes (> sizeof(gwx_hbm_t): the launcher sees to it).
__device__ int gwx_gwfa(gwx_lds_t &L, const gwx_prob_t &pr, char *block, int64_t block_bytes, int32_t *ed, int32_t **path, int32_t *n_path, int32_t *peak)
{
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	gwx_hbm_t *Hm = (gwx_hbm_t*)block;
	gwx_cells_t *cur = &L.buf[0], *nxt = &L.buf[1], *S = &Hm->S;
	int par = 0;
	int32_t n = 1, s = 0;
	int64_t n_iter = 0;
	*ed = -1, *path = 0, *n_path = 0, *peak = 1;
	__syncthreads(); // (the previous job's readers of L are through)
	if (wave == 0) { const int rc = gwx_init(L, Hm, pr, block + sizeof(gwx_hbm_t), block_bytes - (int64_t)sizeof(gwx_hbm_t)); if (tid == 0) L.rc = rc; }
	__syncthreads();
	if (L.rc != GC_OK) return GWX_BACK_ARENA;
	const gc_graph_t *G = &L.G;
	const int32_t ql = pr.ql;
	const char *q = pr.q;
	int reached = 0;
	while (n > 0) {
		gwx_cells_t *a = cur, *B = nxt;
		int32_t nB = 0, nF = 0, nH = 0;
		int ovf = 0, f_ovf = 0;
		// ---- R1: extension ----
		for (int32_t i = tid; i < n; i += GWX_T) {
			const uint64_t vd = a->vd[i];
			const uint32_t v = (uint32_t)(vd >> 32);
			const int32_t k0 = a->k[i], k = gc_extend1((int32_t)vd - GC_DSHIFT, k0, gc_vlen(G, v), gc_vseq(G, v), ql, q);
			a->xo[i] += (uint32_t)(k - k0) << 2, a->k[i] = k;
		}
		if (wave == 0) gc_u64map_clear(&L.z.seen);
		__syncthreads();
		// ---- R2: expansion, in the order of the runs ----
		for (int32_t base = 0; base < n; base += GWX_T) {
			const int32_t i = base + tid;
			const int in = i < n;
			gc_diag_t me;
			me.vd = 0, me.k = 0, me.len = 0, me.xo = 0, me.t = 0, me.pad_[0] = me.pad_[1] = 0;
			int keep0 = 0, keepM = 0, keepN = 0, fin0 = 0, finM = 0, finN = 0, at_end = 0;
			uint32_t mx = 0;
			int32_t mk = 0, mt = 0;
			if (in) {
				me = gwx_ld(a, i);
				const int32_t vl = gc_vlen(G, (uint32_t)(me.vd >> 32)), d = (int32_t)me.vd - GC_DSHIFT;
				const int first = i == 0 || a->vd[i - 1] + 1 != me.vd, last = i == n - 1 || a->vd[i + 1] != me.vd + 1; // my cell starts / ends a run of adjacent diagonals
				mx = me.xo + 4, mk = me.k + 1, mt = me.t;                                                              // mismatch ...
				if (!first && a->k[i - 1] > me.k + 1) mx = a->xo[i - 1] + 2, mk = a->k[i - 1], mt = a->t[i - 1];       // ... unless the insertion from the left gets further
				if (!last && !(mk > a->k[i + 1] + 1)) mx = a->xo[i + 1] + 2, mt = a->t[i + 1], mk = a->k[i + 1] + 1;   // deletion from the right, when it gets at least as far
				at_end = me.k == vl - 1 || d + me.k == ql - 1;
				const int32_t k0 = me.k + 1, kN = me.k;
				keep0 = first && (d - 1) + k0 < ql && k0 < vl, fin0 = first && !keep0 && k0 == vl;
				keepM = d + mk < ql && mk < vl, finM = !keepM && mk == vl;
				keepN = last && (d + 1) + kN < ql && kN < vl, finN = last && !keepN && kN == vl;
			}
			const uint32_t pack = (uint32_t)(keep0 + keepM + keepN) | (uint32_t)(fin0 + finM + finN) << 11 | (uint32_t)at_end << 22; // (per trip: at most 1 536, 1 536 and 512)
			uint32_t tot;
			const uint32_t ex = gwx_scan(L, &par, pack, &tot);
			const int32_t tB = (int32_t)(tot & 0x7ff), tF = (int32_t)(tot >> 11 & 0x7ff), tH = (int32_t)(tot >> 22 & 0x3ff);
			if (nB + tB > GWX_WIDE || nH + tH > GWX_HCAP) { ovf = 1; break; } // (the same totals in every lane)
			if (nF + tF > GWX_FCAP) f_ovf = 1; // more ranges than the block holds: they matter only when this step dedups, i.e. has head cells (below)
			if (in) {
				int32_t b = nB + (int32_t)(ex & 0x7ff);
				gc_intv_t *fr = &Hm->fresh[f_ovf ? 0 : nF + (int32_t)(ex >> 11 & 0x7ff)];
				if (keep0) gwx_st(B, b++, me.vd - 1, me.k + 1, me.xo + 2, me.t);
				if (keepM) gwx_st(B, b++, me.vd, mk, mx, mt);
				if (keepN) gwx_st(B, b++, me.vd + 1, me.k, me.xo + 2, me.t);
				if (fin0 && !f_ovf) { fr->vd0 = me.vd - 1, fr->vd1 = me.vd; ++fr; }
				if (finM && !f_ovf) { fr->vd0 = me.vd, fr->vd1 = me.vd + 1; ++fr; }
				if (finN && !f_ovf) { fr->vd0 = me.vd + 1, fr->vd1 = me.vd + 2; ++fr; }
				if (at_end) { gc_diag_t h = me; h.xo |= 1; Hm->head[nH + (int32_t)(ex >> 22 & 0x3ff)] = h; }
			}
			nB += tB, nF += tF, nH += tH;
		}
		if (ovf || (f_ovf && nH != 0)) return GWX_BACK_CELLS;
		__syncthreads();
		gwx_cells_t *wf = B, *other = a; // where the next wavefront lies, and the buffer that is free
		if (nH != 0) {
			// ---- H: the head loop and the finished ranges, on wave 0, over the last two cells of B and what it appends ----
			const int32_t n_tail = nB < 2 ? nB : 2, base = nB - n_tail;
			if (wave == 0) {
				gc_gw_t *z = &L.z;
				if (lane < n_tail) Hm->hb[lane] = gwx_ld(B, base + lane);
				gc_sync();
				z->wf[0].a = Hm->hb, z->wf[0].n = n_tail, z->wf[0].m = GWX_WIDE;
				z->head.n = nH, z->fresh.n = nF;
				int r = 0;
				const int rc = gwx_heads(L, base, pr.v1, pr.off1, &r);
				if (tid == 0) L.rc = rc, L.reached = r, L.nB = z->wf[0].n, L.unsorted = 0, L.b_unsorted = 0, L.twin = 0;
			}
			__syncthreads();
			if (L.rc != GC_OK) return L.rc == GC_E_ARENA ? GWX_BACK_ARENA : GWX_BACK_CELLS;
			reached = L.reached;
			if (reached) break;
			const int32_t n_hb = L.nB; // (base + n_hb <= GWX_WIDE: gwx_heads checks before every push)
			for (int32_t j = tid; j < n_hb; j += GWX_T) { const gc_diag_t c = Hm->hb[j]; gwx_st(B, base + j, c.vd, c.k, c.xo, c.t); }
			nB = base + n_hb;
			__syncthreads();
			// ---- D: gwf_dedup ----
			int uns = 0;
			for (int32_t i = tid; i < nB; i += GWX_T) if (i > 0 && B->vd[i - 1] > B->vd[i]) uns = 1;
			if (uns) L.unsorted = 1;
			__syncthreads();
			gwx_cells_t *src = B, *dst = a;
			if (L.unsorted) { // in-order cells keep their place, the flagged ones are sorted, stable merge (gfa-ed.c:143-171)
				gwx_cells_t *F = a; // (the consumed wavefront's buffer: the flagged cells, in their order)
				int32_t n_b = 0, n_c = 0;
				for (int32_t base2 = 0; base2 < nB; base2 += GWX_T) { // stable partition
					const int32_t i = base2 + tid;
					const int in = i < nB;
					gc_diag_t me;
					int flag = 0;
					if (in) me = gwx_ld(B, i), flag = me.xo & 1;
					uint32_t tot;
					const uint32_t ex = gwx_scan(L, &par, (uint32_t)(in && !flag) | (uint32_t)flag << 16, &tot);
					if (in) { if (flag) gwx_st(F, n_c + (int32_t)(ex >> 16), me.vd, me.k, me.xo, me.t); else gwx_st(S, n_b + (int32_t)(ex & 0xffff), me.vd, me.k, me.xo, me.t); }
					n_b += (int32_t)(tot & 0xffff), n_c += (int32_t)(tot >> 16);
				}
				__syncthreads();
				int bu = 0, tw = 0;
				for (int32_t i = tid; i < n_b; i += GWX_T) if (i > 0 && S->vd[i - 1] > S->vd[i]) bu = 1;
				if (bu) L.b_unsorted = 1;
				for (int32_t i = tid; i < n_c; i += GWX_T) { // a flagged cell's place in the stable order, into B (whose cells the partition has moved out); and has it a twin (above)?
					const gc_diag_t me = gwx_ld(F, i);
					int32_t r = 0;
					for (int32_t j = 0; j < n_c; ++j) {
						const uint64_t kj = F->vd[j];
						r += (kj < me.vd) | ((kj == me.vd) & (j < i));
						if (kj == me.vd && j != i && F->k[j] == me.k && (((F->xo[j] ^ me.xo) >> 1) != 0 || F->t[j] != me.t)) tw = 1;
					}
					gwx_st(B, r, me.vd, me.k, me.xo & 0xfffffffeU, me.t);
				}
				if (tw && n_c > 64) L.twin = 1;
				if (tid == 0 && n_c > L.max_flag) L.max_flag = n_c;
				__syncthreads();
				if (L.b_unsorted) return GWX_BACK_SORT;
				if (L.twin) { // (the same in every lane) klib's own order decides which twin survives: replay its moves
					if (wave == 0) { const int rc = gwx_sort_replay(L, n_c, F, B); if (tid == 0) L.rc = rc, ++L.n_replay; }
					__syncthreads();
					if (L.rc != GC_OK) return GWX_BACK_ARENA;
				}
				for (int32_t i = tid; i < n_b; i += GWX_T) { // an in-order cell goes behind the flagged ones that are strictly smaller
					const gc_diag_t me = gwx_ld(S, i);
					int32_t lo = 0, hi = n_c;
					while (lo < hi) { const int32_t m = (lo + hi) >> 1; if (B->vd[m] < me.vd) lo = m + 1; else hi = m; }
					gwx_st(a, i + lo, me.vd, me.k, me.xo, me.t);
				}
				for (int32_t j = tid; j < n_c; j += GWX_T) { // a flagged cell goes behind the in-order ones that are smaller or equal
					const gc_diag_t me = gwx_ld(B, j);
					int32_t lo = 0, hi = n_b;
					while (lo < hi) { const int32_t m = (lo + hi) >> 1; if (S->vd[m] <= me.vd) lo = m + 1; else hi = m; }
					gwx_st(a, j + lo, me.vd, me.k, me.xo, me.t);
				}
				__syncthreads();
				src = a, dst = B;
			}
			const int32_t n_done = L.z.done.n;
			int32_t m = 0;
			for (int32_t base2 = 0; base2 < nB; base2 += GWX_T) { // the first of the furthest cells of a (vertex, diagonal) stays, unless the diagonal is finished
				const int32_t i = base2 + tid;
				gc_diag_t me;
				int keep = 0;
				if (i < nB) {
					me = gwx_ld(src, i);
					keep = 1;
					for (int32_t j = i - 1; j >= 0 && src->vd[j] == me.vd; --j) if (!(src->k[j] < me.k)) { keep = 0; break; } /* an earlier cell at least as far */
					if (keep) for (int32_t j = i + 1; j < nB && src->vd[j] == me.vd; ++j) if (me.k < src->k[j]) { keep = 0; break; } /* a later cell strictly further */
					if (keep && n_done > 0) {
						int32_t lo = 0, hi = n_done;
						while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (L.done[mid].vd1 <= me.vd) lo = mid + 1; else hi = mid; }
						keep = !(lo < n_done && me.vd >= L.done[lo].vd0);
					}
				}
				uint32_t tot;
				const uint32_t ex = gwx_scan(L, &par, (uint32_t)keep, &tot);
				if (keep) gwx_st(dst, m + (int32_t)ex, me.vd, me.k, me.xo, me.t);
				m += (int32_t)tot;
			}
			__syncthreads();
			wf = dst, other = src, nB = m;
		}
		if (pr.max_lag > 0 && nB > 1000 && ((s + 1) & 0xf) == 0) { // ---- P: gfa-ed.c:286-307, on all waves ----
			unsigned long long best = 0; // edits << 32 | ~index: the largest edit count, the first cell of those that have it (the sequential scan takes a cell on `>` only)
			for (int32_t i = tid; i < nB; i += GWX_T) {
				const uint32_t x = wf->xo[i] >> 1;
				const unsigned long long key = (unsigned long long)x << 32 | (0xffffffffU - (uint32_t)i);
				if (x > 0 && key > best) best = key;
			}
			for (int d = 32; d > 0; d >>= 1) {
				const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), d);
				const unsigned long long o = (unsigned long long)hi << 32 | lo;
				if (o > best) best = o;
			}
			if (lane == 0) L.red[wave] = best;
			__syncthreads();
			best = 0;
			for (int k = 0; k < GWX_NW; ++k) if (L.red[k] > best) best = L.red[k];
			if (best != 0) { // (the same in every lane)
				const uint32_t max_x = (uint32_t)(best >> 32), max_lag = (uint32_t)pr.max_lag;
				const int32_t max_i = (int32_t)(0xffffffffU - (uint32_t)best);
				const int32_t iq = (int32_t)wf->vd[max_i] - GC_DSHIFT + wf->k[max_i], dq = (int32_t)max_x - iq - iq;
				int32_t m = 0;
				for (int32_t base2 = 0; base2 < nB; base2 += GWX_T) {
					const int32_t i = base2 + tid;
					gc_diag_t p;
					int keep = 0;
					if (i < nB) {
						p = gwx_ld(wf, i);
						const int32_t ip = (int32_t)p.vd - GC_DSHIFT + p.k, dp = (int32_t)(p.xo >> 1) - ip - ip, w = dp > dq ? dp - dq : dq - dp;
						keep = !(w > 1000) && !((p.xo >> 1) + max_lag < max_x); /* bw_dyn = 1000 */
					}
					uint32_t tot;
					const uint32_t ex = gwx_scan(L, &par, (uint32_t)keep, &tot);
					if (keep) gwx_st(other, m + (int32_t)ex, p.vd, p.k, p.xo, p.t);
					m += (int32_t)tot;
				}
				__syncthreads();
				{ gwx_cells_t *x = wf; wf = other, other = x; }
				nB = m;
			}
		}
		cur = wf, nxt = other;
		n = nB;
		if (n > *peak) *peak = n;
		n_iter += n;
		if (n == 0) break;
		if (pr.s_term >= 0 && s >= pr.s_term) break;
		if (n_iter > 500000000LL) break;
		++s;
	}
	if (reached) {
		if (wave == 0) { int32_t *p = 0, np = 0; const int rc = gwx_traceback(L, &p, &np); if (tid == 0) L.rc = rc, L.path = p, L.n_path = np; }
		__syncthreads();
		if (L.rc != GC_OK) return GWX_BACK_ARENA;
		*path = L.path, *n_path = L.n_path, *ed = s;
	}
	return GWX_OK;
}

// ---- the stage entry (stage_api.hip: mga_gwfa_bridge_batch, form MGA_GWFA_FORM_WGX): persistent workgroups draw the listed problems in list order (the caller lists
// the longest query gaps first) ----
// out per problem: ed, n_path, status, peak; the walk at path + i * path_cap (a walk longer than path_cap: status MGA_GWFA_E_ROOM, nothing written)
__global__ void __launch_bounds__(GWX_T) k_gwfa_wgx_stage(int n_list, const int32_t *list, const mga_gwfa_prob_t *prob, const char *qseq, gc_graph_t G_arg, char *arena_mem, int64_t arena_bytes,
														  int32_t path_cap, int32_t *out, int32_t *path_out, unsigned long long *counter)
{
	extern __shared__ __attribute__((aligned(16))) char gwx_smem[];
	gwx_lds_t &L = *(gwx_lds_t*)gwx_smem;
	const int tid = threadIdx.x;
	char *my_block = arena_mem + (int64_t)blockIdx.x * arena_bytes;
	if (tid == 0) L.G = G_arg, L.max_flag = 0, L.n_replay = 0;
	for (;;) {
		__syncthreads();
		if (tid == 0) L.draw = (long long)atomicAdd(counter, 1ULL);
		__syncthreads();
		const long long k = L.draw;
		if (k >= n_list) break;
		const int i = list[k];
		const mga_gwfa_prob_t *p = &prob[i];
		gwx_prob_t pr;
		pr.q = qseq + p->q_off, pr.ql = p->ql, pr.v0 = p->v0, pr.off0 = p->off0, pr.v1 = p->v1, pr.off1 = p->off1, pr.max_lag = p->max_lag, pr.s_term = p->s_term;
		int32_t ed, *path, n_path, peak;
		const int st = gwx_gwfa(L, pr, my_block, arena_bytes, &ed, &path, &n_path, &peak);
		int32_t status = st == GWX_OK ? MGA_GWFA_WGX : MGA_GWFA_BACK;
		if (st == GWX_OK && n_path > path_cap) status = MGA_GWFA_E_ROOM, ed = -1, n_path = 0;
		if (st == GWX_OK) for (int32_t x = tid; x < n_path; x += GWX_T) path_out[(int64_t)i * path_cap + x] = path[x];
		if (tid == 0) out[4 * i] = st == GWX_OK ? ed : -1, out[4 * i + 1] = st == GWX_OK ? n_path : 0, out[4 * i + 2] = status, out[4 * i + 3] = peak;
	}
	if (tid == 0) atomicMax(counter + 1, (unsigned long long)L.max_flag), atomicAdd(counter + 2, (unsigned long long)L.n_replay); // counter[0]: the draw
}

extern "C" void mga_dev_gwfa_wgx_shape(int *nw, int *cells_cur, int *cells_wide) { *nw = GWX_NW, *cells_cur = GWX_WIDE, *cells_wide = GWX_WIDE; }

// One launch over the listed problems, device pointers throughout; d_arena: n_groups blocks of arena_bytes
extern "C" int mga_dev_gwfa_wgx_stage(mga_sctx_t *sc, const mga_didx_t *ix, int n_list, const int32_t *d_list, const mga_gwfa_prob_t *d_prob, const char *d_qseq, char *d_arena,
									  int64_t arena_bytes, int n_groups, int32_t path_cap, int32_t *d_out, int32_t *d_path, unsigned long long *d_counter)
{
	static int attr = 0;
	gc_graph_t G;
	if (n_list <= 0) return 0;
	if (ix->d_arc == 0 || ix->d_gseq_rc == 0) { mga_set_error("gwfa_bridge_batch needs the graph replica (mga_dev_graph_upload)"); return -1; }
	if (arena_bytes < (int64_t)sizeof(gwx_hbm_t) + (1 << 20) || (arena_bytes & 15)) { mga_set_error("gwfa_bridge_batch: the wide form needs arena blocks of more than %ld bytes", (long)sizeof(gwx_hbm_t) + (1 << 20)); return -1; }
	memset(&G, 0, sizeof G);
	G.arc = (const gc_arc_t*)ix->d_arc, G.idx = ix->d_arc_idx, G.seg_len = ix->d_seg_len, G.es = 0, G.seq_fw = ix->d_gseq, G.seq_rc = ix->d_gseq_rc, G.seq_off = ix->d_gseq_off;
	if (!attr) { MGA_HIP_CHECK(hipFuncSetAttribute((const void*)k_gwfa_wgx_stage, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(gwx_lds_t))); attr = 1; }
	hipLaunchKernelGGL(k_gwfa_wgx_stage, dim3(n_groups), dim3(GWX_T), sizeof(gwx_lds_t), (hipStream_t)sc->stream, n_list, d_list, d_prob, d_qseq, G, d_arena, arena_bytes, path_cap, d_out, d_path, d_counter);
	MGA_HIP_CHECK(hipGetLastError());
	return 0;
}
