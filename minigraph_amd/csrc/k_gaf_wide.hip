// k_gaf_wide.hip -- the GAF line of a chromosome-scale chain: a WORKGROUP per line, the path column built by scans (mg_write_gaf, reference format.c:121-250).
//
// k_gaf.hip gives a line to one wavefront and folds the walk serially (four readlanes and a branch per vertex, twice per pass): right for reads, whose walks have a few
// vertices, and ~4 x 10^5 serial steps for a -x asm contig's walk of 10^5.  Here 8 wavefronts take the walk in tiles of GAFW_T = 512 vertices, one vertex per thread, and
// nothing in it is serial:
//
//   pieces   Vertex j continues the open interval of format.c:152-180 exactly when it and vertex j-1 are both printed as intervals, lie on the same stable sequence and strand,
//            and j starts where j-1 ends (reverse strand: ends where j-1 starts) -- the open interval's moving end is always the previous vertex's.  So "j starts a piece" is
//            a flag of j's record and its left neighbour's: one shuffle inside the wave, the wave's last record through LDS across waves, the tile's last record carried
//            across tiles.  The number of pieces is a ballot + popcount sum.
//   closers  A piece is printed by the thread of the vertex BEHIND it: the next piece's head, or the position one past the walk (so the tiles cover cnt + 1 positions and
//            no thread looks ahead).  That thread already holds the piece's tail (its left neighbour); the piece's head reaches it through a max-scan of
//            (position << 32 | the head's fixed end), run as a wave scan + per-wave maxima in LDS + the open piece's head carried across tiles.  Forward pieces are
//            soff[head] .. soff[tail] + len[tail], reverse ones soff[tail] .. soff[head] + len[head].
//   places   The closer knows the bytes of ">name:st-en" (">name" for a vertex printed by name); an exclusive prefix sum of those -- wave scan, per-wave totals in LDS,
//            a 64-bit running carry across tiles -- places every piece.  The counting pass ends there; the writing pass has each closer format its piece straight to its
//            place.  DIRECT STORES, no LDS stage for the path bytes: a piece has no upper bound (names are copied in a per-piece loop), so a stage would need an overflow
//            path beside it; neighbouring threads' pieces are neighbours in memory, so their stores meet in the same L2 lines; and the path column is a few per cent of a
//            line next to cg:Z / ds:Z.
//   scalars  The read name, the numeric columns, the compact form and the tags (~150 bytes) go through k_gaf's own gaf_out_t / gaf_put_div templates (dev_gaf.h): every
//            thread runs them in counting mode (uniform scalar work: that is the offset bookkeeping, the path column lands between the columns), wavefront 0 runs them
//            once more with stores, through an LDS stage.
//   strings  cg:Z / ds:Z are copied from the text pool by all 8 wavefronts: bytewise up to the 16-byte alignment of the DESTINATION, then 16 bytes per thread (an aligned
//            vector load where the source happens to be aligned as well, else whatever the compiler makes of an unaligned 16-byte read), the tail bytewise.
//
// A line's length is kept in 64 bits.  One that does not fit line_len's int32 is reported -- len -1, a count behind the lengths -- and the launcher returns
// MGA_GAF_WIDE_TOO_LONG: the caller sends the chunk to the host writer; nothing is clamped, nothing partial is written.  Every loop with a barrier in it has a trip count
// that is uniform over the workgroup (the walk's length, read by all threads); no thread leaves before the last barrier.  The line of an unmapped read is wavefront 0's alone.
#include "mga_dev.h"
#include "dev_common.h"
#include "dev_gaf.h"

#define GAFW_T  512          // threads of a workgroup = vertices of a tile
#define GAFW_NW (GAFW_T / 64)

__device__ __forceinline__ int32_t gafw_ndig(int32_t x) // bytes of "%d"
{
	uint32_t y = x < 0 ? (uint32_t)-(int64_t)x : (uint32_t)x;
	int32_t nd = x < 0 ? 2 : 1;
	for (; y >= 10; y /= 10) ++nd;
	return nd;
}
__device__ __forceinline__ char *gafw_put_d(char *p, int32_t x) // "%d" at p; returns the end
{
	uint32_t y = x < 0 ? (uint32_t)-(int64_t)x : (uint32_t)x;
	const int32_t nd = gafw_ndig(x);
	if (x < 0) *p = '-';
	for (int32_t i = nd - 1; i >= (x < 0 ? 1 : 0); --i) { p[i] = (char)('0' + y % 10); y /= 10; }
	return p + nd;
}

// len bytes from src to dst by the n_thr threads of the workgroup (tid = 0 .. n_thr-1).  No barrier inside.
__device__ __forceinline__ void gafw_copy(char *__restrict__ dst, const char *__restrict__ src, int64_t len, int tid, int n_thr)
{
	if (len <= 0) return;
	int64_t head = (int64_t)(-(intptr_t)dst & 15);
	if (head > len) head = len;
	if (tid < head) dst[tid] = src[tid];
	const int64_t n16 = (len - head) >> 4;
	char *d = dst + head;
	const char *s = src + head;
	if (((intptr_t)s & 15) == 0)
		for (int64_t b = tid; b < n16; b += n_thr) ((uint4*)d)[b] = ((const uint4*)s)[b];
	else
		for (int64_t b = tid; b < n16; b += n_thr) { uint4 v; __builtin_memcpy(&v, s + (b << 4), 16); ((uint4*)d)[b] = v; }
	const int64_t done = head + (n16 << 4);
	if (tid < len - done) dst[done + tid] = src[done + tid];
}

// the columns in front of the path column: name, length, query interval, strand
template<bool WRITE> __device__ __forceinline__ void gafw_front(gaf_out_t<WRITE> &O, const mga_gaf_line_t &L, const char *qname, int32_t qname_len, bool minus)
{
	O.copy(qname, qname_len);
	O.tab_d(L.qlen);
	if (L.chain < 0) { O.lit("\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n", 21); return; } // an unmapped read's line (MG_M_SHOW_UNMAP, format.c:126-131)
	O.tab_d(L.qs); O.tab_d(L.qe);
	O.c('\t'); O.c(minus ? '-' : '+'); O.c('\t');
}
// the compact form of the path column (format.c:187-198): the stable sequence, its length, the interval of the alignment on it
template<bool WRITE> __device__ __forceinline__ void gafw_compact(gaf_out_t<WRITE> &O, const gaf_tabs_t &G, const mga_gaf_line_t &L, const gaf_sseq_t &sq, int32_t t_soff, bool rev)
{
	const int32_t beg = rev ? L.plen - L.pe : L.ps, end = rev ? L.plen - L.ps : L.pe;
	O.copy(G.names + sq.name_off, sq.name_len);
	O.tab_d(sq.max); O.tab_d(t_soff + beg); O.tab_d(t_soff + end);
}
// what follows the path column, up to and including "\tcg:Z:"
template<bool WRITE> __device__ __forceinline__ void gafw_tags(gaf_out_t<WRITE> &O, const mga_gaf_line_t &L, const mga_txt_res_t &T, bool compact)
{
	if (!compact) { O.tab_d(L.plen); O.tab_d(L.ps); O.tab_d(L.pe); }
	O.tab_d(T.mlen); O.tab_d(T.blen); O.tab_d(L.mapq);
	O.lit("\ttp:A:", 6); O.c(L.primary ? 'P' : 'S');
	O.lit("\tNM:i:", 6); O.d(T.blen - T.mlen);
	O.lit("\tcm:i:", 6); O.d(L.n_anchor);
	O.lit("\ts1:i:", 6); O.d(L.score);
	O.lit("\ts2:i:", 6); O.d(L.subsc);
	if (L.div >= 0.0f && L.div <= 1.0f) { O.lit("\tdv:f:", 6); gaf_put_div(O, L.div); }
	O.lit("\tcg:Z:", 6);
}

template<bool WRITE>
__global__ void __launch_bounds__(GAFW_T) k_gaf_wide(int n_lines, const mga_gaf_line_t *__restrict__ line, const char *__restrict__ qnames, const int64_t *__restrict__ qname_off,
													 gaf_tabs_t G, uint64_t flag, const mga_txt_chain_t *__restrict__ chain, const uint32_t *__restrict__ vert,
													 const mga_txt_res_t *__restrict__ tres, const char *__restrict__ tpool,
													 int32_t *__restrict__ line_len, const int64_t *__restrict__ line_off, char *__restrict__ out)
{
	__shared__ char stage[GAF_STAGE];              // wavefront 0's scalar columns
	__shared__ int32_t s_last[GAFW_NW][4];         // a wave's last record: vertex, snid, soff, len
	__shared__ unsigned long long s_key[GAFW_NW];  // a wave's latest piece head: (position in the tile + 1) << 32 | fixed end
	__shared__ int32_t s_cnt[GAFW_NW];             // a wave's piece heads
	__shared__ uint32_t s_len[GAFW_NW];            // a wave's piece bytes
	const int li = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6; // (the grid is n_lines workgroups: li < n_lines)
	const mga_gaf_line_t L = line[li];
	const bool mapped = L.chain >= 0;
	const int64_t q0 = qname_off[L.read];
	const int32_t qname_len = (int32_t)(qname_off[L.read + 1] - q0);
	mga_txt_chain_t C; C.vert_beg = 0, C.vert_cnt = 0;
	mga_txt_res_t T; T.txt_off = 0, T.cg_len = T.ds_len = 0, T.mlen = T.blen = 0;
	if (mapped) C = chain[L.chain], T = tres[L.chain];
	const uint32_t *V = vert + C.vert_beg;
	const int32_t cnt = mapped ? C.vert_cnt : 0;
	const bool by_name = (flag & MG_M_VERTEX_COOR) != 0;
	const bool may_compact = !(flag & (MG_M_VERTEX_COOR | MG_M_NO_COMP_PATH));

	// where the path column starts: the front columns' bytes do not depend on the strand sign
	gaf_out_t<false> N;
	N.stage = 0, N.dst = 0, N.n = 0, N.total = 0, N.lane = lane;
	gafw_front<false>(N, L, qnames + q0, qname_len, false);
	char *const path_at = WRITE ? out + line_off[li] + N.total : 0;

	// ---- the path column: tiles of GAFW_T positions over 0 .. cnt (position cnt closes the last piece) ----
	int64_t c_off = 0;            // bytes of the pieces closed so far
	int32_t c_heads = 0;          // pieces begun so far
	int32_t c_hval = 0;           // the open piece's fixed end (forward: its start; reverse: its end)
	int32_t p_v = 0, p_snid = -1, p_soff = 0, p_len = 0; // the previous tile's last record
	const int32_t n_tile = cnt > 0 ? cnt / GAFW_T + 1 : 0; // = ceil((cnt + 1) / GAFW_T): uniform
	for (int32_t it = 0; it < n_tile; ++it) {
		const int32_t j = it * GAFW_T + tid;
		int32_t v = 0, snid = -1, soff = 0, len = 0;
		if (j < cnt) { v = (int32_t)V[j]; const gaf_seg_t sg = G.seg[(uint32_t)v >> 1]; snid = sg.snid, soff = sg.soff, len = sg.len; }
		if (lane == 63) s_last[wv][0] = v, s_last[wv][1] = snid, s_last[wv][2] = soff, s_last[wv][3] = len;
		int32_t l_v = __shfl_up(v, 1), l_snid = __shfl_up(snid, 1), l_soff = __shfl_up(soff, 1), l_len = __shfl_up(len, 1); // the left neighbour's record
		__syncthreads();
		if (lane == 0) {
			if (wv > 0) l_v = s_last[wv - 1][0], l_snid = s_last[wv - 1][1], l_soff = s_last[wv - 1][2], l_len = s_last[wv - 1][3];
			else l_v = p_v, l_snid = p_snid, l_soff = p_soff, l_len = p_len;
		}
		p_v = s_last[GAFW_NW - 1][0], p_snid = s_last[GAFW_NW - 1][1], p_soff = s_last[GAFW_NW - 1][2], p_len = s_last[GAFW_NW - 1][3];
		const int32_t rev = v & 1, l_rev = l_v & 1;
		const bool iv = j < cnt && !by_name && snid >= 0, l_iv = j > 0 && !by_name && l_snid >= 0;
		const bool cont = iv && l_iv && snid == l_snid && rev == l_rev && (rev ? soff + len == l_soff : soff == l_soff + l_len);
		const bool head = j < cnt && !cont;
		const bool closer = j > 0 && j <= cnt && !cont; // closes the piece that ends at j - 1
		// the head of the piece that ends at j - 1: the latest head in front of this position
		unsigned long long key = head ? (unsigned long long)(tid + 1) << 32 | (uint32_t)(rev ? soff + len : soff) : 0ULL;
		for (int d = 1; d < 64; d <<= 1) { const unsigned long long y = __shfl_up(key, d); if (lane >= d && y > key) key = y; }
		const uint64_t hb = __ballot(head);
		if (lane == 63) s_key[wv] = key;
		if (lane == 0) s_cnt[wv] = __popcll(hb);
		key = __shfl_up(key, 1);
		if (lane == 0) key = 0;
		__syncthreads();
		int32_t heads_before = c_heads + __popcll(hb & mga_lanemask_lt()), heads_tile = 0;
		unsigned long long key_tile = 0;
		for (int w = 0; w < GAFW_NW; ++w) {
			const unsigned long long kw = s_key[w];
			if (w < wv) { heads_before += s_cnt[w]; if (kw > key) key = kw; }
			heads_tile += s_cnt[w];
			if (kw > key_tile) key_tile = kw;
		}
		const int32_t hval = key ? (int32_t)(uint32_t)key : c_hval;
		// the closer's piece
		uint32_t pl = 0;
		bool named = false, skip = false;
		int32_t st = 0, en = 0;
		gaf_sseq_t sq; sq.name_off = 0, sq.name_len = 0, sq.min = sq.max = sq.rank = -1;
		if (closer) {
			named = by_name || l_snid < 0;
			if (named) { const gaf_seg_t sg = G.seg[(uint32_t)l_v >> 1]; sq.name_off = sg.name_off, sq.name_len = sg.name_len; pl = 1u + (uint32_t)sg.name_len; }
			else {
				sq = G.sseq[l_snid];
				if (l_rev) st = l_soff, en = hval; else st = hval, en = l_soff + l_len;
				pl = 1u + (uint32_t)sq.name_len + 1u + (uint32_t)gafw_ndig(st) + 1u + (uint32_t)gafw_ndig(en);
				skip = may_compact && j == cnt && heads_before == 1 && sq.rank == 0 && sq.min == 0; // the line's only piece and of the compact form: the columns say it
			}
		}
		uint32_t ps = pl;
		for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(ps, d); if (lane >= d) ps += y; }
		if (lane == 63) s_len[wv] = ps;
		__syncthreads();
		int64_t at = c_off + (ps - pl), tile_bytes = 0;
		for (int w = 0; w < GAFW_NW; ++w) { if (w < wv) at += s_len[w]; tile_bytes += s_len[w]; }
		if (WRITE && closer && !skip) {
			char *p = path_at + at;
			const char *nm = G.names + sq.name_off;
			*p++ = l_rev ? '<' : '>';
			for (int32_t i = 0; i < sq.name_len; ++i) p[i] = nm[i];
			p += sq.name_len;
			if (!named) { *p++ = ':'; p = gafw_put_d(p, st); *p++ = '-'; (void)gafw_put_d(p, en); }
		}
		c_off += tile_bytes, c_heads += heads_tile;
		if (key_tile) c_hval = (int32_t)(uint32_t)key_tile;
	}

	// ---- the columns around it ----
	bool compact = false;
	gaf_sseq_t sq0; sq0.name_off = 0, sq0.name_len = 0, sq0.min = sq0.max = sq0.rank = -1;
	int32_t t_soff = 0;
	const bool first_rev = cnt > 0 && (V[0] & 1);
	if (cnt > 0 && may_compact && c_heads == 1) {
		const gaf_seg_t s0 = G.seg[V[0] >> 1];
		if (s0.snid >= 0) {
			sq0 = G.sseq[s0.snid];
			compact = sq0.rank == 0 && sq0.min == 0;
			t_soff = first_rev ? G.seg[V[cnt - 1] >> 1].soff : s0.soff; // the segment the path's coordinates count from
		}
	}
	if (mapped) {
		if (compact) gafw_compact<false>(N, G, L, sq0, t_soff, first_rev); else N.total += c_off;
		gafw_tags<false>(N, L, T, compact);
	}
	const int64_t cg_at = N.total;                                                       // (unmapped: the whole line)
	const int64_t total = mapped ? cg_at + T.cg_len + 6 + T.ds_len + 1 : cg_at;
	if (!WRITE) {
		if (tid == 0) {
			const int32_t l32 = mga_gaf_len32(total);
			line_len[li] = l32;
			if (l32 < 0) atomicAdd(&line_len[n_lines], 1);
		}
		return; // (no barrier follows in the counting pass)
	}
	if (wv == 0) { // the scalar columns, staged in LDS; the stage is this wavefront's alone
		gaf_out_t<WRITE> O;
		O.stage = stage, O.dst = WRITE ? out + line_off[li] : 0, O.n = 0, O.total = 0, O.lane = lane;
		gafw_front<WRITE>(O, L, qnames + q0, qname_len, compact && first_rev);
		if (mapped) {
			if (compact) gafw_compact<WRITE>(O, G, L, sq0, t_soff, first_rev);
			else { O.flush(); if (WRITE) O.dst += c_off; O.total += c_off; }
			gafw_tags<WRITE>(O, L, T, compact);
			O.flush(); if (WRITE) O.dst += T.cg_len; O.total += T.cg_len;
			O.lit("\tds:Z:", 6);
			O.flush(); if (WRITE) O.dst += T.ds_len; O.total += T.ds_len;
			O.c('\n');
		}
		O.flush();
	}
	if (WRITE && mapped) { // the two strings: a stripe per thread
		char *const o = out + line_off[li] + cg_at;
		gafw_copy(o, tpool + T.txt_off, T.cg_len, tid, GAFW_T);
		gafw_copy(o + T.cg_len + 6, tpool + T.txt_off + T.cg_len, T.ds_len, tid, GAFW_T);
	}
}

extern "C" int mga_dev_gaf_wide_tile(void) { return GAFW_T; }
extern "C" int32_t mga_gaf_len32_host(int64_t total) { return mga_gaf_len32(total); }

// pass 1 (d_out == NULL): d_len[i] = bytes of line i, -1 where they do not fit; d_len[n_lines] = how many such lines.  Waits for the kernel and returns
// MGA_GAF_WIDE_TOO_LONG if there is one.  pass 2: the lines at d_out + d_off[i].
extern "C" int mga_dev_gaf_wide(mga_sctx_t *sc, const mga_didx_t *ix, int n_lines, const mga_gaf_line_t *d_line, const char *d_qnames, const int64_t *d_qname_off, uint64_t flag,
								const mga_txt_chain_t *d_chain, const uint32_t *d_vert, const mga_txt_res_t *d_tres, const char *d_tpool,
								int32_t *d_len, const int64_t *d_off, char *d_out)
{
	if (n_lines <= 0) return 0;
	if (ix->d_gaf_seg == 0) { mga_set_error("gaf kernel: the index holds no device copy of the graph's names"); return -1; }
	gaf_tabs_t G;
	G.seg = (const gaf_seg_t*)ix->d_gaf_seg, G.sseq = (const gaf_sseq_t*)ix->d_gaf_sseq, G.names = ix->d_gaf_names;
	hipStream_t st = (hipStream_t)sc->stream;
	if (d_out == 0) {
		int32_t n_long = 0;
		if (mga_dmemset_s(sc, d_len + n_lines, 0, 4) < 0) return -1;
		mga_prof_begin(sc->stream, MGA_K_GAFW);
		hipLaunchKernelGGL(k_gaf_wide<false>, dim3(n_lines), dim3(GAFW_T), 0, st, n_lines, d_line, d_qnames, d_qname_off, G, flag, d_chain, d_vert, d_tres, d_tpool, d_len, d_off, d_out);
		mga_prof_end(sc->stream, MGA_K_GAFW);
		MGA_HIP_CHECK(hipGetLastError());
		if (mga_d2h_s(sc, &n_long, d_len + n_lines, 4) < 0 || mga_ssync(sc) < 0) return -1;
		return n_long != 0 ? MGA_GAF_WIDE_TOO_LONG : 0;
	}
	mga_prof_begin(sc->stream, MGA_K_GAFW);
	hipLaunchKernelGGL(k_gaf_wide<true>, dim3(n_lines), dim3(GAFW_T), 0, st, n_lines, d_line, d_qnames, d_qname_off, G, flag, d_chain, d_vert, d_tres, d_tpool, d_len, d_off, d_out);
	mga_prof_end(sc->stream, MGA_K_GAFW);
	MGA_HIP_CHECK(hipGetLastError());
	return 0;
}
