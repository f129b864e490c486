// k_gaf_vert.hip -- the per-vertex lines of -S / --write-mz on the device: one '*' line per vertex of a printed chain's walk, behind the chain's own line
// (mg_write_gaf, reference format.c:252-289; gaf.c restates it on the host).
//
//   *  >|< segment name  segment length  cnt  [ div  x0+1-span  xn+1  y0+1-span  yn+1  [ span  target distances  query distances ] ]
//
// k_gaf.hip writes the chain's line and stays as it is.  This kernel follows its two passes over the SAME line records: the counting pass keeps a copy of the header's
// length (what k_gaf counted) and adds the bytes of the chain's vertex lines to the line's length, the one scan places the lines, and the writing pass starts at
// line_off[line] + hdr_len[line].  A wavefront per printed chain, two forms:
//
//   -S alone       the lanes take VERTICES, 64 per trip: a lane formats its own line (one template counts and writes), the lines' offsets inside the trip come from a DPP
//                  prefix sum of their lengths, a wave-uniform carry runs from trip to trip.
//   --write-mz     the wavefront takes ONE vertex at a time.  Its scalar columns go through the staged formatter of dev_gaf.h; then the lanes stride over the anchors,
//                  64 per trip: a lane loads a[k] (128 bits), takes a[k-1] from its neighbour by DPP (lane 0: the last anchor of the trip before), forms the distance, its
//                  decimal width with sign and comma, and a DPP scan gives every lane the byte its number starts at.  The target sweep leaves the anchors' query
//                  positions in LDS, so the query sweep reads no global memory (beyond VERT_YCAP anchors of one vertex it loads them again).
//
// div = log(n_mz / cnt) / span is computed here in double.  The device's log is not glibc's bit for bit, and "%.4f" rounds at the fourth decimal: when div * 10^4 lies
// within 1e-9 of k + 1/2 (a last-bit difference could change the text) the kernel raises hb[0] and the caller gives the chunk to the host writer; so it does for a span
// of 0 or a non-positive n_mz (the host prints inf / nan there).  hb[1]: a line's bytes pass an int32.
#include "mga_dev.h"
#include "dev_common.h"
#include "dev_gaf.h"
#include "dev_lcscan.h"

#define VERT_YCAP 2048 // anchors of one vertex whose query positions stay in LDS between the two sweeps (8 kB)

__device__ __forceinline__ int32_t vert_uni(int32_t x) { return __builtin_amdgcn_readfirstlane(x); }

// "%.4f" of div as (integer part, four decimals), or the zero form; *hand_back: the host has to print it
struct vert_div_t { uint32_t ip, fp; bool zero; };
__device__ __forceinline__ vert_div_t vert_div(int32_t n_mz, int32_t cnt, int32_t span, bool *hand_back)
{
	vert_div_t r; r.ip = r.fp = 0, r.zero = n_mz == cnt;
	if (r.zero) return r; // (the host does not call log either)
	if (span <= 0 || n_mz <= 0) { *hand_back = true; return r; }
	const double q = n_mz > cnt ? (double)n_mz / cnt : (double)cnt / n_mz;
	const double s = log(q) / span * 10000.0, t = rint(s);
	if (0.5 - fabs(s - t) < 1e-9) *hand_back = true;
	const uint32_t u = (uint32_t)t;
	r.ip = u / 10000u, r.fp = u % 10000u;
	return r;
}

// a lane's own writer: bytes straight to global memory (WRITE) or counted
template<bool WRITE> struct vert_w_t {
	char *p; int32_t n;
	__device__ __forceinline__ void c(char ch) { if (WRITE) p[n] = ch; ++n; }
	__device__ __forceinline__ void u(uint32_t x) { const int32_t nd = gaf_ndig(x); if (WRITE) gaf_put_u(p + n, x, nd); n += nd; }
	__device__ __forceinline__ void d(int32_t x) { if (x < 0) { c('-'); u((uint32_t)-(int64_t)x); } else u((uint32_t)x); }
	__device__ __forceinline__ void tab_d(int32_t x) { c('\t'); d(x); }
	__device__ __forceinline__ void copy(const char *__restrict__ src, int32_t len) { if (WRITE) for (int32_t i = 0; i < len; ++i) p[n + i] = src[i]; n += len; }
};
template<class W> __device__ __forceinline__ void vert_put_div(W &O, const vert_div_t &dv)
{
	if (dv.zero) { O.c('0'); return; }
	O.u(dv.ip); O.c('.');
	O.c((char)('0' + dv.fp / 1000u)); O.c((char)('0' + dv.fp / 100u % 10u)); O.c((char)('0' + dv.fp / 10u % 10u)); O.c((char)('0' + dv.fp % 10u));
}

// the columns every vertex line has, up to the last query coordinate (format.c:252-270); returns the k-mer span of the vertex's anchors (0 without anchors)
template<class W> __device__ __forceinline__ int32_t vert_head(W &O, const gaf_tabs_t &G, const gaf_seg_t &t, uint32_t v, int32_t cnt, const mg128_t *__restrict__ a, bool *hand_back)
{
	O.c('*'); O.c('\t'); O.c(v & 1 ? '<' : '>');
	O.copy(G.names + t.name_off, t.name_len);
	O.tab_d(t.len); O.tab_d(cnt);
	if (cnt <= 0) return 0;
	const uint4 f = *(const uint4*)&a[0], z = *(const uint4*)&a[cnt - 1]; // (x low, x high, y low, y high)
	const int32_t span = (int32_t)(f.w & 0xff);
	const int32_t n_mz = (int32_t)z.y - (int32_t)f.y + 1; // minimizers of the read between the first and the last anchor
	O.c('\t'); vert_put_div(O, vert_div(n_mz, cnt, span, hand_back));
	O.tab_d((int32_t)f.x + 1 - span); O.tab_d((int32_t)z.x + 1);
	O.tab_d((int32_t)f.z + 1 - span); O.tab_d((int32_t)z.z + 1);
	return span;
}

template<bool WRITE, bool MZ>
__global__ void __launch_bounds__(64) k_gaf_vert(int n_lines, const mga_gaf_vline_t *__restrict__ vline, const mg_llchain_t *__restrict__ lc0, const mg128_t *__restrict__ a0,
												 const mg_llchain_t *__restrict__ lc1, const mg128_t *__restrict__ a1, gaf_tabs_t G,
												 int32_t *__restrict__ line_len, int32_t *__restrict__ hdr_len, int32_t *__restrict__ hb, const int64_t *__restrict__ line_off, char *__restrict__ out)
{
	__shared__ char stage[MZ ? GAF_STAGE : 4];
	__shared__ int32_t ybuf[MZ ? VERT_YCAP : 1];
	const int li = blockIdx.x, lane = threadIdx.x;
	if (li >= n_lines) return;
	const mga_gaf_vline_t L = vline[li];
	if (L.n_lc <= 0) return; // an unmapped read's line has no vertex lines
	const mg_llchain_t *lc = (L.src ? lc1 : lc0) + L.lc_beg;
	const mg128_t *A = (L.src ? a1 : a0) + L.a_base;
	char *dst = WRITE ? out + line_off[li] + hdr_len[li] : 0;
	int64_t total = 0;
	bool hand_back = false;
	if (!MZ) { // lanes over vertices
		for (int32_t j0 = 0; j0 < L.n_lc; j0 += 64) {
			const int32_t j = j0 + lane;
			const bool have = j < L.n_lc;
			int32_t off = 0, cnt = 0, len = 0;
			uint32_t v = 0;
			gaf_seg_t t; t.name_off = 0, t.name_len = 0, t.snid = -1, t.soff = 0, t.len = 0;
			if (have) {
				off = lc[j].off, cnt = lc[j].cnt, v = lc[j].v, t = G.seg[v >> 1];
				vert_w_t<false> C; C.p = 0, C.n = 0;
				(void)vert_head(C, G, t, v, cnt, A + off, &hand_back);
				len = C.n + 1;
			}
			const int32_t incl = lc_scan_add(len, 0);
			if (WRITE && have) {
				bool dummy = false;
				vert_w_t<true> O; O.p = dst + total + (incl - len), O.n = 0;
				(void)vert_head(O, G, t, v, cnt, A + off, &dummy);
				O.c('\n');
			}
			total += __builtin_amdgcn_readlane(incl, 63);
		}
	} else { // the wavefront over one vertex after the other, lanes over its anchors
		gaf_out_t<WRITE> O;
		O.stage = stage, O.dst = dst, O.n = 0, O.total = 0, O.lane = lane;
		for (int32_t j = 0; j < L.n_lc; ++j) {
			const int32_t off = vert_uni(lc[j].off), cnt = vert_uni(lc[j].cnt);
			const uint32_t v = (uint32_t)vert_uni((int32_t)lc[j].v);
			gaf_seg_t t = G.seg[v >> 1];
			t.name_len = vert_uni(t.name_len);
			const mg128_t *a = A + off;
			const int32_t span = vert_head(O, G, t, v, cnt, a, &hand_back);
			if (cnt > 0) {
				O.tab_d(span);
				for (int axis = 0; axis < 2; ++axis) { // minimizer-to-minimizer distances on the target, then on the query
					O.c('\t'); O.flush(); // the numbers go straight to their bytes behind O.dst
					int64_t run = 0;
					int32_t carry = 0;
					for (int32_t k0 = 0; k0 < cnt; k0 += 64) {
						const int32_t k = k0 + lane;
						int32_t cur = 0;
						if (k < cnt) {
							if (axis == 0) { const uint4 q = *(const uint4*)&a[k]; cur = (int32_t)q.x; if (k < VERT_YCAP) ybuf[k] = (int32_t)q.z; }
							else cur = k < VERT_YCAP ? ybuf[k] : (int32_t)a[k].y; // (written by this very lane in the target sweep)
						}
						const int32_t prev = lc_prev_lane(cur, carry);
						carry = __builtin_amdgcn_readlane(cur, 63);
						const bool valid = k >= 1 && k < cnt;
						const int32_t d = (int32_t)((uint32_t)cur - (uint32_t)prev);
						const uint32_t ad = d < 0 ? (uint32_t)-(int64_t)d : (uint32_t)d;
						const int32_t nd = gaf_ndig(ad), w = valid ? nd + (d < 0) + (k > 1) : 0;
						const int32_t incl = lc_scan_add(w, 0);
						if (WRITE && valid) {
							char *p = O.dst + run + (incl - w);
							if (k > 1) *p++ = ',';
							if (d < 0) *p++ = '-';
							gaf_put_u(p, ad, nd);
						}
						run += __builtin_amdgcn_readlane(incl, 63);
					}
					if (WRITE) O.dst += run;
					O.total += run;
				}
			}
			O.c('\n');
		}
		O.flush();
		total = O.total;
	}
	if (!WRITE) {
		if (hand_back) hb[0] = 1;
		if (lane == 0) { // the line's length: k_gaf's header + the vertex lines; the header's length stays behind for the writing pass
			const int32_t hdr = line_len[li];
			const int64_t sum = (int64_t)hdr + total;
			hdr_len[li] = hdr;
			if (sum > 0x7fffffffLL) hb[1] = 1; else line_len[li] = (int32_t)sum;
		}
	}
}

// pass 1 (d_out == NULL): d_hdr[i] = d_len[i], d_len[i] += bytes of line i's vertex lines, d_hb[0..1] raised (zeroed by the caller).  pass 2: the vertex lines at
// d_out + d_off[i] + d_hdr[i].  Pool 0 / pool 1 are the two places a line's records may lie (mga_gaf_vline_t::src).
extern "C" int mga_dev_gaf_vert(mga_sctx_t *sc, const mga_didx_t *ix, int n_lines, const mga_gaf_vline_t *d_vline, const mg_llchain_t *d_lc0, const mg128_t *d_a0,
								const mg_llchain_t *d_lc1, const mg128_t *d_a1, uint64_t flag, int32_t *d_len, int32_t *d_hdr, int32_t *d_hb, const int64_t *d_off, char *d_out)
{
	if (n_lines <= 0) return 0;
	if (ix->d_gaf_seg == 0) { mga_set_error("gaf vertex kernel: the index holds no device copy of the graph's names"); return -1; }
	gaf_tabs_t G;
	G.seg = (const gaf_seg_t*)ix->d_gaf_seg, G.sseq = (const gaf_sseq_t*)ix->d_gaf_sseq, G.names = ix->d_gaf_names;
	hipStream_t st = (hipStream_t)sc->stream;
	const bool mz = (flag & MG_M_WRITE_MZ) != 0;
#define VERT_LAUNCH(W, M) hipLaunchKernelGGL((k_gaf_vert<W, M>), dim3(n_lines), dim3(64), 0, st, n_lines, d_vline, d_lc0, d_a0, d_lc1, d_a1, G, d_len, d_hdr, d_hb, d_off, d_out)
	if (d_out == 0) { if (mz) VERT_LAUNCH(false, true); else VERT_LAUNCH(false, false); }
	else { if (mz) VERT_LAUNCH(true, true); else VERT_LAUNCH(true, false); }
#undef VERT_LAUNCH
	MGA_HIP_CHECK(hipGetLastError());
	return 0;
}
