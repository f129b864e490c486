// dev_gaf.h -- what the two forms of the GAF line kernel share (k_gaf.hip: a wavefront per line; k_gaf_wide.hip: a workgroup per line): the name tables of the graph in HBM,
// the staged formatter of the scalar columns and printf's "%.4f".  Included by those two files and by k_gaf_vert.hip (the per-vertex lines of -S / --write-mz) only.
#ifndef MGA_DEV_GAF_H
#define MGA_DEV_GAF_H

#include "dev_common.h"

struct gaf_seg_t { int64_t name_off; int32_t name_len, snid, soff, len; };   // per segment (gfa_seg_t: name, snid, soff, len)
struct gaf_sseq_t { int64_t name_off; int32_t name_len, min, max, rank; };   // per stable sequence (gfa_sseq_t)

#define GAF_STAGE 1024 // bytes of the LDS stage; a token (a number, a tag) is at most 16 bytes, longer strings are copied in pieces

// the decimal text of an unsigned number, for every writer of GAF bytes on the device: its width, then its digits at w[0 .. nd)
__device__ __forceinline__ int32_t gaf_ndig(uint32_t x) { int32_t nd = 1; for (uint32_t y = x; y >= 10; y /= 10) ++nd; return nd; }
__device__ __forceinline__ void gaf_put_u(char *w, uint32_t x, int32_t nd) { for (int32_t i = nd - 1; i >= 0; --i) { w[i] = (char)('0' + x % 10); x /= 10; } }

template<bool WRITE> struct gaf_out_t {
	char *stage;      // LDS
	char *dst;        // where the next flush goes
	int32_t n;        // bytes in the stage
	int64_t total;    // bytes of the line so far (flushed + staged)
	int lane;
	__device__ __forceinline__ void flush()
	{
		if (WRITE) {
			mga_wave_sync();
			for (int32_t b = lane; b < n; b += 64) dst[b] = stage[b];
			mga_wave_sync();
			dst += n;
		}
		n = 0;
	}
	__device__ __forceinline__ void room(int32_t need) { if (n + need > GAF_STAGE) flush(); }
	__device__ __forceinline__ void c(char ch) { room(1); if (WRITE && lane == 0) stage[n] = ch; ++n, ++total; }
	__device__ __forceinline__ void lit(const char *s, int32_t len) { room(len); if (WRITE && lane == 0) for (int32_t i = 0; i < len; ++i) stage[n + i] = s[i]; n += len, total += len; }
	__device__ __forceinline__ void u(uint32_t x)
	{
		const int32_t nd = gaf_ndig(x);
		room(nd);
		if (WRITE && lane == 0) gaf_put_u(stage + n, x, nd);
		n += nd, total += nd;
	}
	__device__ __forceinline__ void d(int32_t x) { if (x < 0) { c('-'); u((uint32_t)-(int64_t)x); } else u((uint32_t)x); }
	__device__ __forceinline__ void tab_d(int32_t x) { c('\t'); d(x); }
	// len bytes of global memory behind the staged ones (names, alignment strings): all lanes copy
	__device__ __forceinline__ void copy(const char *__restrict__ src, int32_t len)
	{
		if (len <= 0) return;
		if (!WRITE) { total += len; return; }
		if (len <= 64) { // short: through the stage, one byte per lane
			room(len);
			if (lane < len) stage[n + lane] = src[lane];
			n += len, total += len;
			return;
		}
		flush();
		// dwords where source and destination are both reachable as (possibly unaligned) dwords; the tail bytewise
		const int32_t n4 = len & ~3;
		for (int32_t b = lane * 4; b < n4; b += 256) { uint32_t v; __builtin_memcpy(&v, src + b, 4); __builtin_memcpy(dst + b, &v, 4); }
		if (lane < len - n4) dst[n4 + lane] = src[n4 + lane];
		dst += len, total += len;
	}
};

// "%.4f" of a float in [0, 1], "0" for exactly zero (format.c:200-203).  A float times 10^4 is exact in a double (24 + 14 bits), so rounding THAT to an integer half-to-even
// is printf's rounding of the exact decimal expansion (tests/test_gpu_stages.py: test_gaf_div_text, against snprintf)
template<bool WRITE> __device__ __forceinline__ void gaf_put_div(gaf_out_t<WRITE> &O, float div)
{
	if (div == 0.0f) { O.c('0'); return; }
	const uint32_t r = (uint32_t)rint((double)div * 10000.0);
	O.u(r / 10000u); O.c('.');
	const uint32_t f = r % 10000u;
	O.c((char)('0' + f / 1000u)); O.c((char)('0' + f / 100u % 10u)); O.c((char)('0' + f / 10u % 10u)); O.c((char)('0' + f % 10u));
}

struct gaf_tabs_t { const gaf_seg_t *seg; const gaf_sseq_t *sseq; const char *names; };

// a line's byte count, kept in 64 bits on the device, as line_len's int32 holds it: the count, or -1 (never a clamped length)
static __host__ __device__ inline int32_t mga_gaf_len32(int64_t total) { return total > 0x7fffffffLL ? -1 : (int32_t)total; }

#endif
