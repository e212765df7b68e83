// The Moreschi supermomentum on a supertranslated cut and the alpha perturbation of the super-rest-frame iteration
// (scri/asymptotic_bondi_data/map_to_superrest_frame.py:108-224): bms_supermomentum_on_cut, bms_alpha_perturbation
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI; kernels_cut.hip: the kernels)
#include "engine.h"

namespace {

constexpr int64_t CUT_REACH = 64;  // knots kept on either side of the cut's times: a cubic spline forgets its far data like 0.268^n

inline size_t n_pix_of(int ell_max) { return (size_t)(2 * ell_max + 1) * (2 * ell_max + 1); }

// one row of modes -> the grid, as bms_salm2map runs it (the two-kernel form: the one-kernel form wants padded rows)
int synthesise_row(bms_ctx* c, const SynthesisPlan& syn, const double* d_modes, int ell_max, double* d_grid) {
  SynthesisPlan two = syn;
  two.nt = 0;
  return run_synthesis(c, two, d_modes, 2LL * LM_total_size(0, ell_max), 1, nullptr, d_grid, 2LL * (long long)n_pix_of(ell_max));
}

// the synthesis tables (their lambda_lm(theta_i) feed cut_kernel) and, with `ana`, the analysis plan of the (2L+1)^2 grid
int cut_plans(bms_ctx* c, const char* who, int ell_max, SynthesisPlan& syn, AnalysisPlan* ana) {
  const int N = 2 * ell_max + 1;
  if (int rc = build_synthesis(c, N, N, 0, 0, ell_max, syn)) return rc;
  if (!syn.large || !syn.d_T) return fail(c, BMS_ERR_UNSUPPORTED, "%s: the separable synthesis is switched off on this context", who);
  return ana ? build_analysis(c, "cut", N, N, 0, 0, ell_max, *ana) : BMS_OK;
}

}  // namespace

// rows [*lo, *hi) of the axis t[n] whose spline the cut's times amin .. amax are evaluated on (_rows_near of map_to_superrest_frame.py)
BMS_INTERNAL void cut_window(const double* t, int64_t n, double amin, double amax, int64_t* lo, int64_t* hi) {
  const int64_t a = std::upper_bound(t, t + n, amin) - t;  // searchsorted(t, amin, "right")
  const int64_t b = std::lower_bound(t, t + n, amax) - t;  // searchsorted(t, amax, "left")
  *lo = std::max<int64_t>(a - 1 - CUT_REACH, 0);
  *hi = std::min<int64_t>(b + 1 + CUT_REACH, n);
}

// what bms_supermomentum_on_cut refuses before it selects a device; the window on success
BMS_INTERNAL int cut_checks(bms_ctx* c, const double* t, int64_t n, const void* psi, int64_t ld, int mem, int ell_max, const double* alpha,
                            const void* modes_out, const double* psi_at_alpha, const double* k_at_alpha, int64_t* lo, int64_t* hi) {
  const char* who = "bms_supermomentum_on_cut";
  if (!t || !psi || !alpha) return fail(c, BMS_ERR_INVALID, "%s: NULL times, modes or alpha", who);
  if (!modes_out && !psi_at_alpha && !k_at_alpha) return fail(c, BMS_ERR_INVALID, "%s: every output is NULL", who);
  if (n < 0 || ld < 0 || ell_max < 0) return fail(c, BMS_ERR_INVALID, "%s: negative size", who);
  if (ell_max < 2) return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max = %d: the supertranslation term starts at ell = 2", who, ell_max);
  if (ell_max > CUT_MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max = %d is beyond %d", who, ell_max, CUT_MAX_ELL);
  if (ld < LM_total_size(0, ell_max)) return fail(c, BMS_ERR_INVALID, "%s: row stride smaller than the number of modes (%d)", who, LM_total_size(0, ell_max));
  if (mem == BMS_DEVICE && ((uintptr_t)psi & 15)) return fail(c, BMS_ERR_INVALID, "%s: device arrays must be aligned to their elements", who);
  for (int64_t i = 1; i < n; ++i)
    if (!(t[i] > t[i - 1])) return fail(c, BMS_ERR_INVALID, "%s: time array must be strictly increasing (index %lld)", who, (long long)i);
  double amin = INFINITY, amax = -INFINITY;
  for (size_t p = 0; p < n_pix_of(ell_max); ++p) {
    if (!std::isfinite(alpha[p])) return fail(c, BMS_ERR_INVALID, "%s: alpha is not finite at pixel %zu", who, p);
    amin = std::min(amin, alpha[p]), amax = std::max(amax, alpha[p]);
  }
  cut_window(t, n, amin, amax, lo, hi);
  if (*hi - *lo < 4) return fail(c, BMS_ERR_UNSUPPORTED, "%s: the cubic spline needs at least 4 rows, the window has %lld", who, (long long)(*hi - *lo));
  return BMS_OK;
}

extern "C" int bms_supermomentum_on_cut(bms_ctx* c, const double* t, int64_t n, const void* psi, int64_t ld, int mem, int ell_max,
                                        const double* alpha, void* modes_out, double* psi_at_alpha, double* k_at_alpha) try {
  if (!c) return BMS_ERR_INVALID;
  const char* who = "bms_supermomentum_on_cut";
  if (int rc0 = entry_mem(c, mem, who, false)) return rc0;  // (the argument checks come before the device is selected)
  int rc;
  int64_t lo, hi;
  if ((rc = cut_checks(c, t, n, psi, ld, mem, ell_max, alpha, modes_out, psi_at_alpha, k_at_alpha, &lo, &hi))) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t nw = hi - lo;
  const int nm = LM_total_size(0, ell_max), with_k = (modes_out || k_at_alpha) ? 1 : 0;
  const size_t n_pix = n_pix_of(ell_max);
  if (cut_lds_bytes(ell_max, nw, with_k) > (size_t)lds_per_workgroup(c->device))
    return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max %d on a window of %lld rows: the sweep of a ring (%zu bytes) does not fit in LDS", who, ell_max,
                (long long)nw, cut_lds_bytes(ell_max, nw, with_k));
  SynthesisPlan syn;
  AnalysisPlan ana;
  if ((rc = cut_plans(c, who, ell_max, syn, modes_out ? &ana : nullptr))) return rc;
  hipStream_t S = c->stream;
  CallIO io(c, mem);
  void* vp;
  if ((rc = upload(c, "cut_alpha", alpha, 8 * n_pix, &vp))) return rc;
  const double* d_alpha = (const double*)vp;
  // the window is an axis of its own: its tables, sweeps and results are those of a call on rows [lo, hi) alone
  double* d_x;
  SplineTable* d_tab;
  if ((rc = upload_times(c, t + lo, nw, 0, nw, 0, nw, &d_x, &d_tab))) return rc;
  const double* d_W = (const double*)psi + 2 * lo * ld;
  if (io.host() || ld != nm) {  // dense rows of the window in a block of the context's
    double* d_rows;
    if ((rc = dev_buf_t(c, "cut_W", (size_t)nw * nm * 2, &d_rows))) return rc;
    if (io.host()) c->host_copy_queued = true;
    HIP_TRY(c, hipMemcpy2DAsync(d_rows, 16 * (size_t)nm, (const char*)psi + 16 * (size_t)lo * ld, 16 * (size_t)ld, 16 * (size_t)nm, (size_t)nw,
                                io.host() ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, S));
    d_W = d_rows;
  }
  double *d_R, *d_S, *d_out;
  if ((rc = dev_buf_t(c, "cut_R", (size_t)nw * nm * 2, &d_R))) return rc;
  if ((rc = dev_buf_t(c, "cut_S", (size_t)nw * nm * 2, &d_S))) return rc;
  if ((rc = dev_buf_t(c, "cut_out", 2 * n_pix, &d_out))) return rc;
  double *d_grid = nullptr, *d_modes = nullptr;  // with modes_out: c16 grids alpha, D alpha, combined; modes of alpha, of the result
  if (modes_out) {
    if ((rc = dev_buf_t(c, "cut_grid", 6 * n_pix, &d_grid))) return rc;
    if ((rc = dev_buf_t(c, "cut_modes", (size_t)4 * nm, &d_modes))) return rc;
  }
  double *d_Dalpha = d_grid ? d_grid + 2 * n_pix : nullptr, *d_comb = d_grid ? d_grid + 4 * n_pix : nullptr;
  const int tile = spline_tile_for(t + lo, nw);
  TIMED(c, BMS_TAG_SPLINE_FORWARD, launch_spline_forward(S, d_W, d_R, 2LL * nm, nm, 0, nw, nw, d_x, d_tab, tile, SPLINE_HALO));
  TIMED(c, BMS_TAG_SPLINE_BACKWARD, launch_spline_slopes(S, d_R, d_S, 2LL * nm, nm, nw, d_tab, tile, SPLINE_HALO));
  if (modes_out) {  // D alpha on the grid
    TIMED(c, BMS_TAG_CUT, launch_cut_real_to_complex(S, d_alpha, d_grid, (int)n_pix));
    if ((rc = run_analysis(c, ana, d_grid, 1, d_modes, 2LL * nm))) return rc;
    TIMED(c, BMS_TAG_CUT, launch_cut_scale_modes(S, d_modes, ell_max, 0));
    if ((rc = synthesise_row(c, syn, d_modes, ell_max, d_Dalpha))) return rc;
  }
  TIMED(c, BMS_TAG_CUT, launch_cut(S, d_W, d_S, nm, nw, d_x, d_tab, syn.d_T, d_alpha, d_Dalpha, ell_max, with_k, d_out, with_k ? d_out + n_pix : nullptr, d_comb));
  if (modes_out) {
    if ((rc = run_analysis(c, ana, d_comb, 1, d_modes + 2 * nm, 2LL * nm))) return rc;
    if ((rc = io.copy_back(modes_out, d_modes + 2 * nm, 16 * (size_t)nm))) return rc;
  }
  if ((rc = io.copy_back(psi_at_alpha, d_out, 8 * n_pix))) return rc;
  if ((rc = io.copy_back(k_at_alpha, d_out + n_pix, 8 * n_pix))) return rc;
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_alpha_perturbation(bms_ctx* c, const void* psi_modes, int ell_max, const double* m_grid, const double* k_grid,
                                      double* alpha_out) try {
  if (!c) return BMS_ERR_INVALID;
  const char* who = "bms_alpha_perturbation";
  if (!psi_modes || !alpha_out) return fail(c, BMS_ERR_INVALID, "%s: NULL modes or output", who);
  if (ell_max < 0) return fail(c, BMS_ERR_INVALID, "%s: negative ell_max", who);
  if (ell_max < 2) return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max = %d: the supertranslation term starts at ell = 2", who, ell_max);
  if (ell_max > CUT_MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max = %d is beyond %d", who, ell_max, CUT_MAX_ELL);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  SynthesisPlan syn;
  AnalysisPlan ana;
  if ((rc = cut_plans(c, who, ell_max, syn, &ana))) return rc;
  const int nm = LM_total_size(0, ell_max);
  const size_t n_pix = n_pix_of(ell_max);
  hipStream_t S = c->stream;
  CallIO io(c, BMS_HOST);
  const double *d_in, *d_m = nullptr, *d_k = nullptr;
  if ((rc = io.in("cut_modes_in", psi_modes, 16 * (size_t)nm, &d_in))) return rc;
  if (m_grid && (rc = io.in("cut_m_grid", m_grid, 8 * n_pix, &d_m))) return rc;
  if (k_grid && (rc = io.in("cut_k_grid", k_grid, 8 * n_pix, &d_k))) return rc;
  double *d_grid, *d_modes, *d_out;
  if ((rc = dev_buf_t(c, "cut_grid", 6 * n_pix, &d_grid))) return rc;
  if ((rc = dev_buf_t(c, "cut_modes", (size_t)4 * nm, &d_modes))) return rc;
  if ((rc = dev_buf_t(c, "cut_out", 2 * n_pix, &d_out))) return rc;
  if ((rc = synthesise_row(c, syn, d_in, ell_max, d_grid))) return rc;
  TIMED(c, BMS_TAG_CUT, launch_cut_mass_term(S, d_grid, d_in, d_m, d_k, ell_max));
  if ((rc = run_analysis(c, ana, d_grid, 1, d_modes, 2LL * nm))) return rc;
  TIMED(c, BMS_TAG_CUT, launch_cut_scale_modes(S, d_modes, ell_max, 1));
  if ((rc = synthesise_row(c, syn, d_modes, ell_max, d_grid + 2 * n_pix))) return rc;
  TIMED(c, BMS_TAG_CUT, launch_cut_real_part(S, d_grid + 2 * n_pix, d_out, (int)n_pix));
  if ((rc = io.copy_back(alpha_out, d_out, 8 * n_pix))) return rc;
  return io.finish();
} BMS_CATCH(c)
