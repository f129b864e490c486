// k_cov.hip -- read coverage on the device (--cov: mg_cov_map, reference cal_cov.c:8-53) for the job that wants no GAF: the chunk's chains end in integer
// accumulators that stay in HBM for the whole job -- covered bases per segment, traversals per arc (cov_core.h has the formulation and why it is exact).
//
// Form: ONE WAVEFRONT PER CHAIN, lanes striding over the walk's vertices.  A walk has 1 to thousands of vertices; the filter (mapq, blen) is uniform over a chain, so
// a chain that fails it costs one 32-byte load and its wavefront retires; the flat lane-per-vertex form would need a scan over the walk lengths and a search per
// lane for the chain it belongs to, to save lanes in a kernel that is a few atomics per vertex.  Four chains per 256-thread workgroup.
//
// Atomics: 64-bit atomicAdd on global memory (vector atomics executed at L2).  Equal segment ids are NOT combined inside a wavefront: the lanes of a wavefront hold
// distinct vertices of ONE walk, which repeats a segment only on a cycle -- the contention of a hot linear stretch is between wavefronts, where a ballot does not reach.
// That contention is unmeasured.
#include "mga_dev.h"
#include "dev_common.h"
#include "cov_core.h"

__global__ void __launch_bounds__(256) k_cov(int n_chain, const mga_cov_chain_t *__restrict__ chain, const uint32_t *__restrict__ vert, int64_t n_vert, cov_graph_t G, uint32_t n_seg,
											 int32_t min_mapq, int32_t min_blen, unsigned long long *__restrict__ seg_bases, unsigned long long *__restrict__ link_cnt,
											 unsigned long long *__restrict__ cnt)
{
	const int ci = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (ci >= n_chain) return;
	const mga_cov_chain_t C = chain[ci];
	if (!cov_chain_counts(&C, min_mapq, min_blen)) return; // the filter, uniform over the wavefront
	if (C.vert_beg < 0 || C.vert_beg + C.vert_cnt > n_vert) return; // (a record that points outside the walk array is not followed)
	const uint32_t *v = vert + C.vert_beg;
	int32_t n_link = 0, n_skip = 0;
	for (int32_t j = lane; j < C.vert_cnt; j += 64) {
		const uint32_t vj = v[j];
		if ((vj >> 1) >= n_seg) continue;
		atomicAdd(&seg_bases[vj >> 1], (unsigned long long)(int64_t)cov_vertex_bases(&G, &C, vj, j));
		if (j == 0) continue;
		const uint32_t vp = v[j - 1];
		int64_t a01, a10;
		if ((vp >> 1) >= n_seg) continue;
		if (cov_vertex_link(&G, vp, vj, &a01, &a10)) { atomicAdd(&link_cnt[a01], 1ULL); atomicAdd(&link_cnt[a10], 1ULL); ++n_link; }
		else ++n_skip;
	}
	for (int d = 32; d > 0; d >>= 1) { n_link += __shfl_xor(n_link, d); n_skip += __shfl_xor(n_skip, d); }
	if (lane == 0) {
		atomicAdd(&cnt[MGA_COV_CHAINS], 1ULL);
		if (n_link) atomicAdd(&cnt[MGA_COV_LINKS], (unsigned long long)n_link);
		if (n_skip) atomicAdd(&cnt[MGA_COV_SKIPPED], (unsigned long long)n_skip);
	}
}

// d_seg_bases[ix->n_seg], d_link_cnt[n_arc of the graph replica], d_cnt[MGA_COV_N_CNT]: added to, never cleared here
extern "C" int mga_dev_cov(mga_sctx_t *sc, const mga_didx_t *ix, int n_chain, const mga_cov_chain_t *d_chain, const uint32_t *d_vert, int64_t n_vert,
						   int32_t min_mapq, int32_t min_blen, int64_t *d_seg_bases, int64_t *d_link_cnt, int64_t *d_cnt)
{
	if (n_chain <= 0) return 0;
	if (ix->d_arc == 0 || ix->d_arc_idx == 0 || ix->d_seg_len == 0) { mga_set_error("coverage kernel: the index holds no device copy of the graph's arcs"); return -1; }
	cov_graph_t G;
	G.seg_len = ix->d_seg_len, G.arc = ix->d_arc, G.arc_idx = ix->d_arc_idx;
	mga_prof_begin(sc->stream, MGA_K_COV);
	hipLaunchKernelGGL(k_cov, dim3((unsigned)((n_chain + 3) / 4)), dim3(256), 0, (hipStream_t)sc->stream, n_chain, d_chain, d_vert, n_vert, G, (uint32_t)ix->n_seg, min_mapq, min_blen,
					   (unsigned long long*)d_seg_bases, (unsigned long long*)d_link_cnt, (unsigned long long*)d_cnt);
	mga_prof_end(sc->stream, MGA_K_COV);
	MGA_HIP_CHECK(hipGetLastError());
	return 0;
}
