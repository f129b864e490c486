// stage_api.hip -- public stage-level entry points of include/minigraph_amd.h (host pointers in/out).
// These are what the parity tests and foreign-language bindings call; the mapping pipeline itself
// keeps intermediate results in HBM and calls the mga_dev_* launchers directly.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "mga_dev.h"
#include "dev_common.h"

extern "C" void mga_ksort_128x(int64_t n, mg128_t *a); // ksortx.c: radix_sort_128x with the reference's exact permutation
extern "C" void mga_host_unpin(void *p);
extern "C" void mga_free(void *p) { mga_host_unpin(p); free(p); } // (a buffer the library handed out may have been page-locked with mga_host_pin)

namespace {
struct dptr { // RAII for a device allocation
	void *p = 0;
	~dptr() { mga_dfree(p); }
	bool alloc(size_t n) { p = mga_dmalloc(n); return p != 0; }
	template<class T> T *as() const { return (T*)p; }
};
}

extern "C" int mga_sketch_batch(int n, const char *seq, const int64_t *off, const uint32_t *rid, int w, int k,
								mg128_t **mz, int64_t **mz_off)
{
	*mz = 0, *mz_off = 0;
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	if (n <= 0) { *mz_off = (int64_t*)calloc(1, 8); return 0; }
	const int64_t tot = off[n];
	dptr d_seq, d_off, d_rid, d_cnt, d_mzoff, d_mz;
	if (!d_seq.alloc(tot + 64) || !d_off.alloc((n + 1) * 8) || !d_cnt.alloc(n * 4) || !d_mzoff.alloc((n + 1) * 8)) return -1;
	if (rid && !d_rid.alloc(n * 4)) return -1;
	if (mga_h2d(d_seq.p, seq, tot) < 0 || mga_h2d(d_off.p, off, (n + 1) * 8) < 0) return -1;
	if (rid && mga_h2d(d_rid.p, rid, n * 4) < 0) return -1;
	struct planes_guard { mga_sctx_t *sc; ~planes_guard() { sc->sk_planes_src = 0; } } pg{SC}; // (the packed form belongs to d_seq, which dies with this call)
	{ const char *e = getenv("MGA_SKETCH_2BIT"); if (e && atoi(e) > 0 && mga_dev_pack2(SC, d_seq.as<char>(), tot) < 0) return -1; } // the sketch reads bit planes instead of bytes (k_sketch.hip)
	// long sequences are sketched in pieces (k odd: see k_sketch.hip); piece offsets are folded back into per-sequence offsets
	const int32_t PIECE = 1 << 16;
	std::vector<int32_t> items, first_item(n + 1);
	bool pieces = false;
	if (k & 1) for (int i = 0; i < n; ++i) if (off[i + 1] - off[i] > PIECE) pieces = true;
	if (pieces) {
		for (int i = 0; i < n; ++i) {
			const int64_t l = off[i + 1] - off[i];
			int64_t b = 0;
			first_item[i] = (int32_t)(items.size() / 4);
			do { items.push_back(i); items.push_back((int32_t)b); items.push_back((int32_t)(b + PIECE < l ? b + PIECE : l)); items.push_back(0); b += PIECE; } while (b < l);
		}
		first_item[n] = (int32_t)(items.size() / 4);
	}
	const int n_items = pieces ? (int)(items.size() / 4) : n;
	dptr d_items;
	if (pieces) {
		mga_dfree(d_cnt.p); mga_dfree(d_mzoff.p); d_cnt.p = d_mzoff.p = 0;
		if (!d_items.alloc(items.size() * 4) || !d_cnt.alloc((size_t)n_items * 4) || !d_mzoff.alloc((size_t)(n_items + 1) * 8)) return -1;
		if (mga_h2d(d_items.p, items.data(), items.size() * 4) < 0) return -1;
		if (mga_dev_sketch_items(SC, n_items, d_items.as<int32_t>(), d_seq.as<char>(), d_off.as<int64_t>(), d_rid.as<uint32_t>(), w, k, d_cnt.as<int32_t>(), 0, 0) < 0) return -1;
	} else if (mga_dev_sketch(SC, n, d_seq.as<char>(), d_off.as<int64_t>(), d_rid.as<uint32_t>(), w, k, d_cnt.as<int32_t>(), 0, 0) < 0) return -1;
	if (mga_dev_scan_i32_to_i64(SC, d_cnt.as<int32_t>(), n_items, d_mzoff.as<int64_t>()) < 0) return -1;
	std::vector<int64_t> it_off((size_t)n_items + 1);
	if (mga_ssync(SC) < 0 || mga_d2h(it_off.data(), d_mzoff.p, ((size_t)n_items + 1) * 8) < 0) return -1;
	const int64_t n_mz = it_off[n_items];
	int64_t *h_off = (int64_t*)malloc((n + 1) * 8);
	for (int i = 0; i <= n; ++i) h_off[i] = pieces ? it_off[first_item[i]] : it_off[i];
	if (!d_mz.alloc((size_t)n_mz * 16 + 16)) { free(h_off); return -1; }
	if (pieces) { if (mga_dev_sketch_items(SC, n_items, d_items.as<int32_t>(), d_seq.as<char>(), d_off.as<int64_t>(), d_rid.as<uint32_t>(), w, k, 0, d_mzoff.as<int64_t>(), d_mz.as<mg128_t>()) < 0) { free(h_off); return -1; } }
	else if (mga_dev_sketch(SC, n, d_seq.as<char>(), d_off.as<int64_t>(), d_rid.as<uint32_t>(), w, k, 0, d_mzoff.as<int64_t>(), d_mz.as<mg128_t>()) < 0) { free(h_off); return -1; }
	mg128_t *h_mz = (mg128_t*)malloc((size_t)n_mz * 16 + 16);
	if (mga_ssync(SC) < 0 || mga_d2h(h_mz, d_mz.p, (size_t)n_mz * 16) < 0) { free(h_off); free(h_mz); return -1; }
	*mz = h_mz, *mz_off = h_off;
	return 0;
}

// seg_step < 0: the ladder (mga_dev_wfa_solve); >= 0: every problem through the low-memory rung alone (k_wfa_seg.hip) at that step (0: the host's choice)
static int wfa_batch_impl(int n, const char *tseq, const int64_t *t_off, const char *qseq, const int64_t *q_off, int seg_step,
						  int32_t **score, uint32_t **cigar, int64_t **cig_off)
{
	*score = 0, *cigar = 0, *cig_off = 0;
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	if (n <= 0) { *cig_off = (int64_t*)calloc(1, 8); return 0; }
	const int64_t tt = t_off[n], tq = q_off[n];
	std::vector<mga_wfa_prob_t> prob(n);
	for (int i = 0; i < n; ++i) {
		prob[i].t_off = t_off[i], prob[i].q_off = q_off[i];
		prob[i].tl = (int32_t)(t_off[i + 1] - t_off[i]), prob[i].ql = (int32_t)(q_off[i + 1] - q_off[i]);
		if (prob[i].tl <= 0 || prob[i].ql <= 0) { mga_set_error("wfa: problem %d has an empty sequence (the caller handles those, galign.c:98-100)", i); return -1; }
	}
	dptr d_t, d_q, d_prob, d_res, d_pool, d_used;
	int64_t pool_cap = (tt + tq) / 4 + n * 4 + 1024 + 40000LL * 512 + MGA_WFA_FUSE_SLACK;
	if (!d_t.alloc(tt + 64) || !d_q.alloc(tq + 64) || !d_prob.alloc((size_t)n * sizeof(mga_wfa_prob_t)) ||
		!d_res.alloc((size_t)n * sizeof(mga_wfa_res_t)) || !d_used.alloc(8)) return -1;
	if (mga_h2d(d_t.p, tseq, tt) < 0 || mga_h2d(d_q.p, qseq, tq) < 0 || mga_h2d(d_prob.p, prob.data(), (size_t)n * sizeof(mga_wfa_prob_t)) < 0) return -1;
	if (mga_dmemset_s(SC, (char*)d_t.p + tt, 0, 64) < 0 || mga_dmemset_s(SC, (char*)d_q.p + tq, 0, 64) < 0) return -1;

	std::vector<mga_wfa_res_t> res(n);
	if (!d_pool.alloc((size_t)pool_cap * 4) || mga_dmemset_s(SC, d_used.p, 0, 8) < 0) return -1;
	const mga_wfa_job_t job = { d_prob.as<mga_wfa_prob_t>(), d_t.as<char>(), d_q.as<char>(), d_res.as<mga_wfa_res_t>(), d_pool.as<uint32_t>(), pool_cap, (unsigned long long*)d_used.p };
	if (seg_step >= 0) {
		std::vector<int32_t> tl(n), ql(n);
		for (int i = 0; i < n; ++i) tl[i] = prob[i].tl, ql[i] = prob[i].ql;
		if (mga_dev_wfa_seg(SC, &job, n, 0, tl.data(), ql.data(), seg_step) < 0) return -1;
	} else if (mga_dev_wfa_solve(SC, &job, n, 0) < 0) return -1;
	if (mga_dsync() < 0 || mga_d2h(res.data(), d_res.p, (size_t)n * sizeof(mga_wfa_res_t)) < 0) return -1;
	unsigned long long used = 0;
	if (mga_dsync() < 0 || mga_d2h(&used, d_used.p, 8) < 0) return -1;
	std::vector<uint32_t> hpool((size_t)used + 1);
	if (used && mga_d2h(hpool.data(), d_pool.p, (size_t)used * 4) < 0) return -1;
	int32_t *h_score = (int32_t*)malloc((size_t)n * 4);
	int64_t *h_off = (int64_t*)malloc((size_t)(n + 1) * 8);
	int64_t tot = 0;
	for (int i = 0; i < n; ++i) { h_off[i] = tot; h_score[i] = res[i].score; if (res[i].status == MGA_WFA_OK) tot += res[i].n_cigar; }
	h_off[n] = tot;
	uint32_t *h_cig = (uint32_t*)malloc((size_t)tot * 4 + 4);
	for (int i = 0; i < n; ++i)
		if (res[i].status == MGA_WFA_OK && res[i].n_cigar)
			memcpy(h_cig + h_off[i], hpool.data() + res[i].cig_off, (size_t)res[i].n_cigar * 4);
	*score = h_score, *cigar = h_cig, *cig_off = h_off;
	return 0;
}

extern "C" int mga_wfa_batch(int n, const char *tseq, const int64_t *t_off, const char *qseq, const int64_t *q_off,
							 int32_t **score, uint32_t **cigar, int64_t **cig_off)
{
	return wfa_batch_impl(n, tseq, t_off, qseq, q_off, -1, score, cigar, cig_off);
}

extern "C" int mga_wfa_seg_batch(int n, const char *tseq, const int64_t *t_off, const char *qseq, const int64_t *q_off, int32_t step,
								 int32_t **score, uint32_t **cigar, int64_t **cig_off)
{
	if (step < 0) { mga_set_error("wfa_seg: negative step %d", step); return -1; }
	return wfa_batch_impl(n, tseq, t_off, qseq, q_off, step, score, cigar, cig_off);
}

struct mg_idx_bucket_s_view { mga_didx_t dev; }; // first member of the hidden index struct (mga_host.h)

extern "C" int mga_seed_batch(const mg_idx_t *gi, int n, const mg128_t *mz, const int64_t *mz_off, int max_occ,
							  mg128_t **a, int64_t **a_off, int32_t **rep_len, int32_t **mini_pos, int64_t **mini_off)
{
	*a = 0, *a_off = 0, *rep_len = 0, *mini_pos = 0, *mini_off = 0;
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	if (n <= 0) { *a_off = (int64_t*)calloc(1, 8); *mini_off = (int64_t*)calloc(1, 8); return 0; }
	const mga_didx_t *ix = &((const mg_idx_bucket_s_view*)gi->B)->dev;
	const int64_t n_mz = mz_off[n];
	dptr d_mz, d_mzoff, d_occ, d_val, d_na, d_nmini, d_rep, d_aoff, d_minioff, d_a, d_tmp, d_mini;
	if (!d_mz.alloc((size_t)n_mz * 16 + 16) || !d_mzoff.alloc((n + 1) * 8) || !d_occ.alloc((size_t)n_mz * 4 + 4) || !d_val.alloc((size_t)n_mz * 8 + 8) ||
		!d_na.alloc(n * 4) || !d_nmini.alloc(n * 4) || !d_rep.alloc(n * 4) || !d_aoff.alloc((n + 1) * 8) || !d_minioff.alloc((n + 1) * 8)) return -1;
	if (mga_h2d(d_mz.p, mz, (size_t)n_mz * 16) < 0 || mga_h2d(d_mzoff.p, mz_off, (n + 1) * 8) < 0) return -1;
	// MGA_SEED_LONG=1: the intra-read parallel kernels of the long-query path (k_seed.hip), anchors sorted here like the host chainer does
	const char *e_long = getenv("MGA_SEED_LONG");
	const bool use_long = e_long && atoi(e_long) > 0;
	dptr d_tk, d_kf, d_offa, d_offm, d_rkey, d_rmax;
	if (use_long) {
		if (!d_tk.alloc((size_t)n_mz * 4 + 4) || !d_kf.alloc((size_t)n_mz * 4 + 4) || !d_offa.alloc((size_t)(n_mz + 1) * 8) || !d_offm.alloc((size_t)(n_mz + 1) * 8) ||
			!d_rkey.alloc((size_t)n_mz * 8 + 8) || !d_rmax.alloc((size_t)n_mz * 8 + 8)) return -1;
		if (mga_dev_seed_long_count(SC, ix, n, d_mz.as<mg128_t>(), d_mzoff.as<int64_t>(), n_mz, max_occ, d_occ.as<int32_t>(), d_val.as<uint64_t>(), d_tk.as<int32_t>(), d_kf.as<int32_t>(),
									d_offa.as<int64_t>(), d_offm.as<int64_t>(), d_rkey.as<uint64_t>(), d_rmax.as<uint64_t>(), d_aoff.as<int64_t>(), d_minioff.as<int64_t>(), d_rep.as<int32_t>()) < 0) return -1;
	} else {
		if (mga_dev_seed_count(SC, ix, n, d_mz.as<mg128_t>(), d_mzoff.as<int64_t>(), 0, max_occ, d_occ.as<int32_t>(), d_val.as<uint64_t>(),
							   d_na.as<int32_t>(), d_nmini.as<int32_t>(), d_rep.as<int32_t>()) < 0) return -1;
		if (mga_dev_scan_i32_to_i64(SC, d_na.as<int32_t>(), n, d_aoff.as<int64_t>()) < 0) return -1;
		if (mga_dev_scan_i32_to_i64(SC, d_nmini.as<int32_t>(), n, d_minioff.as<int64_t>()) < 0) return -1;
	}
	int64_t *h_aoff = (int64_t*)malloc((n + 1) * 8), *h_moff = (int64_t*)malloc((n + 1) * 8);
	int32_t *h_rep = (int32_t*)malloc(n * 4);
	if (mga_ssync(SC) < 0 || mga_d2h(h_aoff, d_aoff.p, (n + 1) * 8) < 0 || mga_d2h(h_moff, d_minioff.p, (n + 1) * 8) < 0 || mga_d2h(h_rep, d_rep.p, n * 4) < 0) return -1;
	const int64_t n_a = h_aoff[n], n_m = h_moff[n];
	if (!d_a.alloc((size_t)n_a * 16 + 64) || !d_mini.alloc((size_t)n_m * 4 + 16)) return -1;
	if (use_long) {
		if (mga_dev_seed_long_fill(SC, ix, n, d_mz.as<mg128_t>(), d_mzoff.as<int64_t>(), n_mz, max_occ, d_occ.as<int32_t>(), d_val.as<uint64_t>(), d_offa.as<int64_t>(), d_offm.as<int64_t>(),
								   d_a.as<mg128_t>(), d_mini.as<int32_t>()) < 0) return -1;
	} else {
		if (!d_tmp.alloc((size_t)n_a * 16 + 64)) return -1;
		if (mga_dev_seed_fill(SC, ix, n, d_mz.as<mg128_t>(), d_mzoff.as<int64_t>(), 0, max_occ, d_occ.as<int32_t>(), d_val.as<uint64_t>(),
							  d_aoff.as<int64_t>(), d_a.as<mg128_t>(), d_minioff.as<int64_t>(), d_mini.as<int32_t>(), d_tmp.as<mg128_t>()) < 0) return -1;
	}
	mg128_t *h_a = (mg128_t*)malloc((size_t)n_a * 16 + 16);
	int32_t *h_mini = (int32_t*)malloc((size_t)n_m * 4 + 4);
	if (mga_ssync(SC) < 0 || mga_d2h(h_a, d_a.p, (size_t)n_a * 16) < 0 || mga_d2h(h_mini, d_mini.p, (size_t)n_m * 4) < 0) return -1;
	if (use_long) for (int i = 0; i < n; ++i) mga_ksort_128x(h_aoff[i + 1] - h_aoff[i], h_a + h_aoff[i]); // radix_sort_128x, map-algo.c:189
	*a = h_a, *a_off = h_aoff, *rep_len = h_rep, *mini_pos = h_mini, *mini_off = h_moff;
	return 0;
}

extern "C" int mga_gaf_div_batch(int n, const float *div, char *out)
{
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	if (n <= 0) return 0;
	dptr d_div, d_out;
	if (!d_div.alloc((size_t)n * 4 + 16) || !d_out.alloc((size_t)n * 8 + 16)) return -1;
	if (mga_h2d(d_div.p, div, (size_t)n * 4) < 0 || mga_dev_gaf_div(SC, n, d_div.as<float>(), d_out.as<char>()) < 0) return -1;
	if (mga_ssync(SC) < 0 || mga_d2h(out, d_out.p, (size_t)n * 8) < 0) return -1;
	return 0;
}

extern "C" int mga_sort128x_batch(int n, mg128_t *a, const int64_t *a_off)
{
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	if (n <= 0) return 0;
	const int64_t tot = a_off[n];
	dptr d_a, d_aoff, d_tmp, d_stk;
	if (!d_a.alloc((size_t)tot * 16 + 16) || !d_aoff.alloc((n + 1) * 8) || !d_tmp.alloc((size_t)tot * 16 + 16) || !d_stk.alloc((size_t)tot * 12 + (size_t)n * 32 + 64)) return -1;
	if (mga_h2d(d_a.p, a, (size_t)tot * 16) < 0 || mga_h2d(d_aoff.p, a_off, (n + 1) * 8) < 0) return -1;
	if (mga_dev_sort128x(SC, n, d_a.as<mg128_t>(), d_aoff.as<int64_t>(), d_tmp.as<mg128_t>(), d_stk.as<int32_t>()) < 0) return -1;
	if (mga_ssync(SC) < 0 || mga_d2h(a, d_a.p, (size_t)tot * 16) < 0) return -1;
	return 0;
}

// resc / qlen / flag all given: the long-join rescue of k_lchain is on (mga_lchain_rescue_batch); all 0: the first pass alone (mga_lchain_batch)
static int lchain_batch_impl(int n, const mg128_t *a, const int64_t *a_off, const mga_lchain_par_t *par, const mga_rescue_par_t *resc, const int32_t *qlen,
							 uint64_t **u, int64_t **u_off, mg128_t **b, int64_t **b_off, int32_t *flag)
{
	*u = 0, *u_off = 0, *b = 0, *b_off = 0;
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	if (n <= 0) { *u_off = (int64_t*)calloc(1, 8); *b_off = (int64_t*)calloc(1, 8); return 0; }
	const int64_t tot = a_off[n];
	dptr d_a, d_aoff, d_u, d_b, d_nu, d_nb, d_ws, d_qoff, d_flag;
	const size_t wsb = mga_dev_lchain_ws_bytes(tot);
	if (!d_a.alloc((size_t)tot * 16 + 16) || !d_aoff.alloc((n + 1) * 8) || !d_u.alloc((size_t)tot * 8 + 8) || !d_b.alloc((size_t)tot * 16 + 16) ||
		!d_nu.alloc(n * 4) || !d_nb.alloc(n * 4) || !d_ws.alloc(wsb)) return -1;
	if (mga_h2d(d_a.p, a, (size_t)tot * 16) < 0 || mga_h2d(d_aoff.p, a_off, (n + 1) * 8) < 0) return -1;
	if (resc) { // the pipeline's d_q_off: the reads' lengths as a prefix array
		std::vector<int64_t> q_off((size_t)n + 1);
		q_off[0] = 0;
		for (int i = 0; i < n; ++i) q_off[i + 1] = q_off[i] + qlen[i];
		if (!d_qoff.alloc((n + 1) * 8) || !d_flag.alloc(n * 4) || mga_h2d(d_qoff.p, q_off.data(), (n + 1) * 8) < 0) return -1;
	}
	if (mga_dev_lchain(SC, n, d_a.as<mg128_t>(), d_aoff.as<int64_t>(), par, resc, d_qoff.as<int64_t>(), d_u.as<uint64_t>(), d_b.as<mg128_t>(), d_nu.as<int32_t>(), d_nb.as<int32_t>(),
					   d_flag.as<int32_t>(), d_ws.p, wsb, tot) < 0) return -1;
	std::vector<int32_t> nu(n), nb(n);
	std::vector<uint64_t> hu((size_t)tot + 1);
	std::vector<mg128_t> hb((size_t)tot + 1);
	if (mga_ssync(SC) < 0 || mga_d2h(nu.data(), d_nu.p, n * 4) < 0 || mga_d2h(nb.data(), d_nb.p, n * 4) < 0 ||
		mga_d2h(hu.data(), d_u.p, (size_t)tot * 8) < 0 || mga_d2h(hb.data(), d_b.p, (size_t)tot * 16) < 0) return -1;
	if (resc && mga_d2h(flag, d_flag.p, n * 4) < 0) return -1;
	int64_t *uo = (int64_t*)malloc((n + 1) * 8), *bo = (int64_t*)malloc((n + 1) * 8);
	int64_t tu = 0, tb = 0;
	for (int i = 0; i < n; ++i) { uo[i] = tu, bo[i] = tb; tu += nu[i], tb += nb[i]; }
	uo[n] = tu, bo[n] = tb;
	uint64_t *ou = (uint64_t*)malloc((size_t)tu * 8 + 8);
	mg128_t *ob = (mg128_t*)malloc((size_t)tb * 16 + 16);
	for (int i = 0; i < n; ++i) {
		memcpy(ou + uo[i], hu.data() + a_off[i], (size_t)nu[i] * 8);
		memcpy(ob + bo[i], hb.data() + a_off[i], (size_t)nb[i] * 16);
	}
	*u = ou, *u_off = uo, *b = ob, *b_off = bo;
	return 0;
}

extern "C" int mga_lchain_batch(int n, const mg128_t *a, const int64_t *a_off, const mga_lchain_par_t *par,
								uint64_t **u, int64_t **u_off, mg128_t **b, int64_t **b_off)
{
	return lchain_batch_impl(n, a, a_off, par, 0, 0, u, u_off, b, b_off, 0);
}

// stage test of the long-join rescue inside k_lchain (lc_dp_rmq_lds / lc_dp_rmq and what lc_read_finish does when they hand a read back): tests/test_gpu_rmq.py
extern "C" int mga_lchain_rescue_batch(int n, const mg128_t *a, const int64_t *a_off, const mga_lchain_par_t *par, const mga_rescue_par_t *resc, const int32_t *qlen,
									   uint64_t **u, int64_t **u_off, mg128_t **b, int64_t **b_off, int32_t *flag)
{
	if (resc == 0 || qlen == 0 || flag == 0) { mga_set_error("lchain_rescue_batch: rescue parameters, query lengths and the flag array are required"); return -1; }
	for (int i = 0; i < n; ++i) if (qlen[i] < 0) { mga_set_error("lchain_rescue_batch: read %d has a negative length", i); return -1; }
	return lchain_batch_impl(n, a, a_off, par, resc, qlen, u, u_off, b, b_off, flag);
}

// stage test of the RMQ chainer's forward pass (k_rmq.hip): what rq_dev_fwd_hook (chunk.c) allocates and uploads for a chunk, one launch on the default stage stream, f / p / v
// and the runs' status back.  A status the kernel never wrote stays 4, as in the pipeline.  tests/test_gpu_rmq.py
extern "C" int mga_rmq_fwd_batch(int64_t n_total, const mg128_t *a, int n_runs, const int64_t *runs, int n_order, const int32_t *order, int max_dist, int max_dist_inner, int bw,
								 int max_skip, int cap, float pen_gap, float pen_skip, int32_t *f, int64_t *p, int32_t *v, int32_t *status)
{
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	if (n_total < 0 || n_runs < 0 || n_total >= 0x7fffffffLL) { mga_set_error("rmq_fwd_batch: bad sizes"); return -1; }
	if (order == 0) n_order = n_runs;
	for (int r = 0; r < n_runs; ++r) { // the kernel trusts its table
		const int64_t beg = runs[3 * r], end = runs[3 * r + 1], base = runs[3 * r + 2];
		if (!(0 <= base && base <= beg && beg <= end && end <= n_total)) { mga_set_error("rmq_fwd_batch: run %d lies outside the %ld anchors", r, (long)n_total); return -1; }
	}
	if (n_order < 0 || n_order > n_runs) { mga_set_error("rmq_fwd_batch: more work items than runs"); return -1; }
	for (int k = 0; order && k < n_order; ++k)
		if (order[k] < 0 || order[k] >= n_runs) { mga_set_error("rmq_fwd_batch: order[%d] names no run", k); return -1; }
	for (int r = 0; r < n_runs; ++r) status[r] = 4;
	if (n_total > 0) { memset(f, 0, (size_t)n_total * 4); memset(p, 0, (size_t)n_total * 8); memset(v, 0, (size_t)n_total * 4); }
	if (n_total == 0 || n_order == 0) return 0;
	const size_t n = (size_t)n_total;
	dptr d_a, d_f, d_p, d_v, d_t, d_pri, d_ys, d_runs, d_ord, d_stat, d_cnt;
	if (!d_a.alloc(n * 16 + 64) || !d_f.alloc(n * 4 + 64) || !d_p.alloc(n * 8 + 64) || !d_v.alloc(n * 4 + 64) || !d_t.alloc(n * 4 + 64) || !d_pri.alloc(n * 8 + 64) ||
		!d_ys.alloc(n * 4 + 64) || !d_runs.alloc((size_t)n_runs * 24 + 64) || !d_ord.alloc((size_t)n_runs * 4 + 64) || !d_stat.alloc((size_t)n_runs * 4 + 64) || !d_cnt.alloc(64)) return -1;
	if (mga_h2d(d_a.p, a, n * 16) < 0 || mga_h2d(d_runs.p, runs, (size_t)n_runs * 24) < 0 || mga_h2d(d_stat.p, status, (size_t)n_runs * 4) < 0) return -1;
	if (order && mga_h2d(d_ord.p, order, (size_t)n_order * 4) < 0) return -1;
	if (mga_dmemset_s(SC, d_t.p, 0, n * 4) < 0 || mga_dmemset_s(SC, d_f.p, 0, n * 4) < 0 || mga_dmemset_s(SC, d_p.p, 0, n * 8) < 0 || mga_dmemset_s(SC, d_v.p, 0, n * 4) < 0) return -1;
	if (mga_dev_rmq_fwd(SC, n_total, d_a.as<mg128_t>(), n_order, d_runs.p, order ? d_ord.as<int32_t>() : 0, max_dist, max_dist_inner, bw, max_skip, cap, pen_gap, pen_skip,
						d_f.as<int32_t>(), d_p.as<int64_t>(), d_v.as<int32_t>(), d_t.as<int32_t>(), d_pri.as<double>(), d_ys.as<int32_t>(), d_stat.as<int32_t>(), (int*)d_cnt.p) < 0) return -1;
	if (mga_ssync(SC) < 0 || mga_d2h(f, d_f.p, n * 4) < 0 || mga_d2h(p, d_p.p, n * 8) < 0 || mga_d2h(v, d_v.p, n * 4) < 0 || mga_d2h(status, d_stat.p, (size_t)n_runs * 4) < 0) return -1;
	return 0;
}

// mg_cov_map (cal_cov.c:8-53) for flat chain records through k_cov.hip against gi's graph replica; ADDS into seg_bases[n_seg] / link_cnt[n_arc] / *st
extern "C" int mga_cov_batch(const mg_idx_t *gi, int n_chain, const mga_cov_chain_t *chain, int64_t n_vert, const uint32_t *vert, int32_t min_mapq, int32_t min_blen,
							 int64_t *seg_bases, int64_t *link_cnt, mga_cov_stats_t *st)
{
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	const mga_didx_t *ix = &((const mg_idx_bucket_s_view*)gi->B)->dev;
	const int64_t n_seg = gi->g->n_seg, n_arc = (int64_t)gi->g->n_arc;
	for (int i = 0; i < n_chain; ++i) // the kernel does not follow such a record either; here the caller hears about it
		if (chain[i].vert_cnt < 0 || chain[i].vert_beg < 0 || chain[i].vert_beg + chain[i].vert_cnt > n_vert) { mga_set_error("cov: chain %d points outside the %ld walk vertices", i, (long)n_vert); return -1; }
	dptr d_chain, d_vert, d_seg, d_link, d_cnt;
	if (!d_chain.alloc((size_t)(n_chain > 0 ? n_chain : 1) * sizeof(mga_cov_chain_t)) || !d_vert.alloc((size_t)n_vert * 4 + 16) || !d_seg.alloc((size_t)(n_seg + 1) * 8) ||
		!d_link.alloc((size_t)(n_arc + 1) * 8) || !d_cnt.alloc(64)) return -1;
	if (mga_dmemset_s(SC, d_seg.p, 0, (size_t)(n_seg + 1) * 8) < 0 || mga_dmemset_s(SC, d_link.p, 0, (size_t)(n_arc + 1) * 8) < 0 || mga_dmemset_s(SC, d_cnt.p, 0, 64) < 0) return -1;
	if (n_chain > 0 && (mga_h2d(d_chain.p, chain, (size_t)n_chain * sizeof(mga_cov_chain_t)) < 0 || (n_vert > 0 && mga_h2d(d_vert.p, vert, (size_t)n_vert * 4) < 0))) return -1;
	if (mga_dev_cov(SC, ix, n_chain, d_chain.as<mga_cov_chain_t>(), d_vert.as<uint32_t>(), n_vert, min_mapq, min_blen, d_seg.as<int64_t>(), d_link.as<int64_t>(), d_cnt.as<int64_t>()) < 0) return -1;
	std::vector<int64_t> hs((size_t)n_seg + 1), hl((size_t)n_arc + 1);
	int64_t cnt[8];
	if (mga_ssync(SC) < 0 || mga_d2h(hs.data(), d_seg.p, (size_t)n_seg * 8) < 0 || mga_d2h(hl.data(), d_link.p, (size_t)n_arc * 8) < 0 || mga_d2h(cnt, d_cnt.p, 64) < 0) return -1;
	for (int64_t i = 0; i < n_seg; ++i) seg_bases[i] += hs[i];
	for (int64_t k = 0; k < n_arc; ++k) link_cnt[k] += hl[k];
	if (st) st->chains_counted += cnt[MGA_COV_CHAINS], st->links_counted += cnt[MGA_COV_LINKS], st->links_skipped += cnt[MGA_COV_SKIPPED];
	return 0;
}

// mg_call_asm's scan (asm-call.c:47-115) for flat records through k_call.hip: win[n_bb] = the surviving candidate of largest key per bubble, *warn = the warnings by key
extern "C" int mga_call_batch(int n_chain, const mga_call_chain_t *chain, int64_t n_pos, const mga_call_pos_t *pos, uint32_t n_seg, const mga_call_seg_t *seg, const int32_t *seg_len,
							  int n_seq, const int64_t *q_off, const mga_call_intv_t *qintv, int32_t n_bb, mga_call_cand_t *win, mga_call_warn_t **warn, int64_t *n_warn)
{
	*warn = 0, *n_warn = 0;
	if (mga_dev_init() < 0) return -1;
	mga_sctx_t *SC = mga_sctx_default();
	if (SC == 0) return -1;
	if (mga_call_batch_check(n_chain, chain, n_pos, pos, n_seg, seg, n_seq, q_off, n_bb) < 0) return -1; // the kernel does not follow such a record either; here the caller hears about it
	const int64_t n_q = n_seq > 0 ? q_off[n_seq] : 0;
	const size_t cap = (size_t)n_pos + 1;
	dptr d_chain, d_pos, d_seg, d_len, d_qoff, d_q, d_best, d_cand, d_warn, d_cnt;
	if (!d_chain.alloc((size_t)(n_chain + 1) * sizeof *chain) || !d_pos.alloc(cap * sizeof *pos) || !d_seg.alloc((size_t)(n_seg + 1) * sizeof *seg) || !d_len.alloc((size_t)(n_seg + 1) * 4) ||
		!d_qoff.alloc((size_t)(n_seq + 2) * 8) || !d_q.alloc((size_t)(n_q + 1) * sizeof *qintv) || !d_best.alloc((size_t)(n_bb + 1) * 8) || !d_cand.alloc(cap * sizeof(mga_call_cand_t)) ||
		!d_warn.alloc(cap * sizeof(mga_call_warn_t)) || !d_cnt.alloc(64)) return -1;
	if (mga_dmemset_s(SC, d_best.p, 0, (size_t)(n_bb + 1) * 8) < 0 || mga_dmemset_s(SC, d_cnt.p, 0, 64) < 0) return -1;
	if ((n_chain > 0 && mga_h2d(d_chain.p, chain, (size_t)n_chain * sizeof *chain) < 0) || (n_pos > 0 && mga_h2d(d_pos.p, pos, (size_t)n_pos * sizeof *pos) < 0) ||
		(n_seg > 0 && (mga_h2d(d_seg.p, seg, (size_t)n_seg * sizeof *seg) < 0 || mga_h2d(d_len.p, seg_len, (size_t)n_seg * 4) < 0)) ||
		(n_seq > 0 && mga_h2d(d_qoff.p, q_off, (size_t)(n_seq + 1) * 8) < 0) || (n_q > 0 && mga_h2d(d_q.p, qintv, (size_t)n_q * sizeof *qintv) < 0)) return -1;
	if (mga_dev_call(SC, n_chain, d_chain.as<mga_call_chain_t>(), n_pos, d_pos.as<mga_call_pos_t>(), n_seg, d_seg.as<mga_call_seg_t>(), d_len.as<int32_t>(), n_seq, d_qoff.as<int64_t>(),
					 d_q.as<mga_call_intv_t>(), n_bb, d_best.as<uint64_t>(), d_cand.as<mga_call_cand_t>(), (int64_t)n_pos, d_warn.as<mga_call_warn_t>(), (int64_t)n_pos, d_cnt.as<uint64_t>()) < 0) return -1;
	uint64_t cnt[8];
	if (mga_ssync(SC) < 0 || mga_d2h(cnt, d_cnt.p, 64) < 0) return -1;
	if ((int64_t)cnt[0] > n_pos || (int64_t)cnt[1] > n_pos) { mga_set_error("call: the kernel reports more candidates than walk positions"); return -1; }
	std::vector<uint64_t> best((size_t)n_bb + 1);
	std::vector<mga_call_cand_t> hc((size_t)cnt[0] + 1);
	mga_call_warn_t *hw = (mga_call_warn_t*)malloc(((size_t)cnt[1] + 1) * sizeof(mga_call_warn_t));
	if ((n_bb > 0 && mga_d2h(best.data(), d_best.p, (size_t)n_bb * 8) < 0) || (cnt[0] > 0 && mga_d2h(hc.data(), d_cand.p, (size_t)cnt[0] * sizeof(mga_call_cand_t)) < 0) ||
		(cnt[1] > 0 && mga_d2h(hw, d_warn.p, (size_t)cnt[1] * sizeof(mga_call_warn_t)) < 0)) { free(hw); return -1; }
	if (mga_call_pick(n_bb, (int64_t)cnt[0], hc.data(), best.data(), win) < 0) { free(hw); mga_set_error("call: a bubble's largest key has no candidate record"); return -1; }
	mga_call_sort_warn((int64_t)cnt[1], hw);
	*warn = hw, *n_warn = (int64_t)cnt[1];
	return 0;
}
