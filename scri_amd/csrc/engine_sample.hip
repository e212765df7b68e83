// The precessing sample waveform and its finite-radius family: bms_precessing_waveform, bms_radius_terms
// (scri/sample_waveforms.py:383-755; kernels_sample.hip and sample_math.h: the arithmetic)
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI)
#include "engine.h"
#include "sample_math.h"

namespace {

constexpr int64_t SAMPLE_MIN_MERGER_STEP = 20;  // sample_waveforms.py:453
constexpr int64_t SAMPLE_MIN_KNOTS = 4;         // of a not-a-knot cubic spline

// np.argmin(np.abs(t - v)) on a strictly increasing axis: the two neighbours of v, the earlier one on a tie
int64_t nearest_step(const double* t, int64_t n, double v) {
  const int64_t j = std::lower_bound(t, t + n, v) - t;
  int64_t best = std::max<int64_t>(j - 1, 0);
  for (int64_t k = best + 1; k <= std::min(j, n - 1); ++k)
    if (std::fabs(t[k] - v) < std::fabs(t[best] - v)) best = k;
  return best;
}

// first index in [0, n) at which pred holds (pred false then true along the axis), n if none
template <class Pred>
int64_t first_step(int64_t n, Pred pred) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (pred(mid))
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// The argument checks of bms_precessing_waveform that need no device, and the steps at which the definitions of the waveform change:
// the reference's argmin searches (sample_waveforms.py:452, 467-468, 480-481), each over the two candidates a bisection leaves.
int plan_precessing(bms_ctx* c, const double* t, int64_t n, int ell_max, const bms_precessing_params* p, SamplePlan& P) {
  if (!t || !p) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (n < SAMPLE_MIN_MERGER_STEP + SAMPLE_MIN_KNOTS) return fail(c, BMS_ERR_INVALID, "%lld time steps are too few for the merger to be %lld steps in", (long long)n, (long long)SAMPLE_MIN_MERGER_STEP);
  if (ell_max < 2) return fail(c, BMS_ERR_INVALID, "ell_max = %d: the strain starts at l = 2", ell_max);
  if (ell_max > MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "ell_max = %d is beyond %d", ell_max, MAX_ELL);
  if (!p->coef || !p->power) return fail(c, BMS_ERR_INVALID, "NULL amplitude tables");
  const bool finite = std::isfinite(p->mass_ratio) && std::isfinite(p->t_merger) && std::isfinite(p->opening_angle) &&
                      std::isfinite(p->relative_rate) && (p->derive_opening_angle_dot || std::isfinite(p->opening_angle_dot)) &&
                      (p->derive_nutation_angle || std::isfinite(p->nutation_angle));
  if (!finite) return fail(c, BMS_ERR_INVALID, "the parameters of the waveform must be finite");
  if (!(p->mass_ratio > 0)) return fail(c, BMS_ERR_INVALID, "mass_ratio must be positive, got %g", p->mass_ratio);
  if (p->relative_rate == 0) return fail(c, BMS_ERR_INVALID, "precession_relative_rate must not be zero");
  if (!std::isfinite(t[0])) return fail(c, BMS_ERR_INVALID, "time array must be finite");
  for (int64_t i = 1; i < n; ++i)
    if (!(t[i] > t[i - 1]) || !std::isfinite(t[i])) return fail(c, BMS_ERR_INVALID, "time array must be finite and strictly increasing (index %lld)", (long long)i);
  const double q = p->mass_ratio < 1.0 ? 1.0 / p->mass_ratio : p->mass_ratio;
  P = SamplePlan{};
  P.n = n;
  P.nu = q / ((1 + q) * (1 + q));
  P.t_merger = p->t_merger;
  P.im = nearest_step(t, n, P.t_merger);
  if (P.im < SAMPLE_MIN_MERGER_STEP)
    return fail(c, BMS_ERR_INVALID, "the merger (t = %g) is step %lld of the time axis: it must be at least %lld steps in", P.t_merger, (long long)P.im,
                (long long)SAMPLE_MIN_MERGER_STEP);
  // omega = (nu / 2) tau^(-3/8) rises with t and is NaN once tau < 0: the step nearest to omega = 0.25 among those before that
  auto tau = [&](int64_t i) { return P.nu * (P.t_merger - t[i]) / 5; };
  auto omega_pn = [&](int64_t i) { return (P.nu / 2) * std::pow(tau(i), -3.0 / 8); };
  const int64_t n_valid = first_step(n, [&](int64_t i) { return !(tau(i) >= 0); });
  if (n_valid == 0) return fail(c, BMS_ERR_INVALID, "the time axis starts after the merger");
  const int64_t k = first_step(n_valid, [&](int64_t i) { return omega_pn(i) >= SAMPLE_OMEGA_MERGER; });
  P.i1 = std::max<int64_t>(k - 1, 0);
  if (k < n_valid && std::fabs(omega_pn(k) - SAMPLE_OMEGA_MERGER) < std::fabs(omega_pn(P.i1) - SAMPLE_OMEGA_MERGER)) P.i1 = k;
  P.tb1 = t[P.i1];
  P.i0 = nearest_step(t, n, P.tb1 - 5.0);
  P.tb0 = t[P.i0];
  P.tr0 = t[P.im];
  P.ir = nearest_step(t, n, P.tr0 + 20);
  P.tr1 = t[P.ir];
  if (n - P.i0 < SAMPLE_MIN_KNOTS || P.ib() - P.ia() < SAMPLE_MIN_KNOTS)
    return fail(c, BMS_ERR_UNSUPPORTED, "the spline integrals need at least %lld steps: there are %lld from the frequency transition on and %lld inside the ringdown transition",
                (long long)SAMPLE_MIN_KNOTS, (long long)(n - P.i0), (long long)(P.ib() - P.ia()));
  P.opening = p->opening_angle;
  P.opening_dot = p->derive_opening_angle_dot ? 2.0 * p->opening_angle / (P.tr1 - t[0]) : p->opening_angle_dot;
  P.rate = p->relative_rate;
  P.nutation = p->derive_nutation_angle ? p->opening_angle / 10.0 : p->nutation_angle;
  return BMS_OK;
}

// the per-column table of the mode kernel from the caller's amplitude tables
int sample_mode_table(bms_ctx* c, int ell_max, const bms_precessing_params* p, std::vector<SampleMode>& modes) {
  const cplx* coef = (const cplx*)p->coef;
  modes.resize((size_t)LM_total_size(2, ell_max));
  size_t k = 0;
  for (int ell = 2; ell <= ell_max; ++ell)
    for (int m = -ell; m <= ell; ++m, ++k) {
      const double twice = 2 * p->power[k];
      if (!std::isfinite(coef[k].re) || !std::isfinite(coef[k].im) || !(twice >= 0 && twice <= (1 << 20)) || twice != std::floor(twice))
        return fail(c, BMS_ERR_INVALID, "amplitude table of mode (%d, %d): a finite coefficient and a power that is a multiple of 1/2 in [0, 2^19]", ell, m);
      modes[k] = {coef[k].re, coef[k].im, (int)twice, (m > 0) - (m < 0)};
    }
  return BMS_OK;
}

}  // namespace

extern "C" int bms_precessing_waveform(bms_ctx* c, const double* t, int64_t n, int ell_max, const bms_precessing_params* params, int inertial,
                                       void* data_out, int64_t ld, int mem, double* frame_out) try {
  if (!c) return BMS_ERR_INVALID;
  if (!data_out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (!valid_mem(mem)) return fail(c, BMS_ERR_INVALID, "mem is BMS_HOST or BMS_DEVICE, got %d", mem);
  int rc;
  SamplePlan P;
  if ((rc = plan_precessing(c, t, n, ell_max, params, P))) return rc;
  const int n_modes = LM_total_size(2, ell_max);
  if (ld < n_modes) return fail(c, BMS_ERR_INVALID, "row stride %lld smaller than %d modes", (long long)ld, n_modes);
  std::vector<SampleMode> modes;
  if ((rc = sample_mode_table(c, ell_max, params, modes))) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t n_om = n - P.i0, n_win = P.ib() - P.ia();
  void *d_t, *d_modes;
  double *d_phi, *d_omega, *d_frame, *d_left, *d_sp = nullptr;
  double2 *d_col, *d_Iom, *d_wcol, *d_Iwin, *d_data = (double2*)data_out;
  int64_t ld_dev = ld;
  if ((rc = upload(c, "smp_t", t, 8 * (size_t)n, &d_t))) return rc;
  if ((rc = upload(c, "smp_modes", modes.data(), sizeof(SampleMode) * modes.size(), &d_modes))) return rc;
  if ((rc = dev_buf_t(c, "smp_phi", (size_t)n, &d_phi))) return rc;
  if ((rc = dev_buf_t(c, "smp_omega", (size_t)n, &d_omega))) return rc;
  if ((rc = dev_buf_t(c, "smp_frame", (size_t)n * 4, &d_frame))) return rc;
  if ((rc = dev_buf_t(c, "smp_left", (size_t)4, &d_left))) return rc;
  if ((rc = dev_buf_t(c, "smp_col", (size_t)n_om, &d_col))) return rc;
  if ((rc = dev_buf_t(c, "smp_Iom", (size_t)n_om, &d_Iom))) return rc;
  if ((rc = dev_buf_t(c, "smp_wcol", (size_t)n_win, &d_wcol))) return rc;
  if ((rc = dev_buf_t(c, "smp_Iwin", (size_t)n_win, &d_Iwin))) return rc;
  if (inertial && (rc = dev_buf_t(c, "smp_spinors", (size_t)n * 4, &d_sp))) return rc;
  if (mem == BMS_HOST) {
    ld_dev = n_modes;
    if ((rc = dev_buf_t(c, "smp_data", (size_t)n * n_modes, &d_data))) return rc;
  }
  hipStream_t S = c->stream;
  const double* dt = (const double*)d_t;
  TIMED(c, BMS_TAG_POINTWISE, launch_sample_phase(S, P, dt, d_phi, d_omega, d_col));
  // phi from step i0 on: phi[i0] + the antiderivative of the spline through omega there (:475)
  if ((rc = bms_spline_derivative(c, t + P.i0, n_om, d_col, 1, 1, BMS_DEVICE, t + P.i0, n_om, -1, d_Iom))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_sample_window(S, P, dt, d_phi, d_Iom, d_wcol));
  // the two integrals of transition_to_constant (utilities.py:189) as the real and imaginary part of one column
  if ((rc = bms_spline_derivative(c, t + P.ia(), n_win, d_wcol, 1, 1, BMS_DEVICE, t + P.ia(), n_win, -1, d_Iwin))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_sample_waveform(S, P, dt, d_phi, d_omega, d_Iom, d_Iwin, d_left, (const SampleMode*)d_modes, n_modes, d_data,
                                                     ld_dev, d_frame, d_sp));
  if (frame_out) HIP_TRY(c, hipMemcpyAsync(frame_out, d_frame, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, S));
  // to the inertial frame as to_inertial_frame goes: the time-series rotation by the conjugate frame, on the device
  if (inertial && (rc = rotate_impl(c, d_data, BMS_DEVICE, n, ld_dev, 2, ell_max, d_sp, true))) return rc;
  if (mem == BMS_HOST)
    HIP_TRY(c, hipMemcpy2DAsync(data_out, (size_t)ld * 16, d_data, (size_t)n_modes * 16, (size_t)n_modes * 16, (size_t)n, hipMemcpyDeviceToHost, S));
  HIP_TRY(c, hipStreamSynchronize(S));
  return BMS_OK;
} BMS_CATCH(c)

extern "C" int bms_radius_terms(bms_ctx* c, const double* t, int64_t n, const void* h0, int64_t ld_h0, int64_t n_cols, int n_terms, double amp,
                                double radius, void* out, int64_t ld_out, int mem) try {
  if (!c) return BMS_ERR_INVALID;
  if (!t || !h0 || !out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (!valid_mem(mem)) return fail(c, BMS_ERR_INVALID, "mem is BMS_HOST or BMS_DEVICE, got %d", mem);
  if (n < 0 || n_cols < 0 || n_cols > (1 << 26) || ld_h0 < n_cols || ld_out < n_cols) return fail(c, BMS_ERR_INVALID, "bad sizes");
  if (n_terms < 0 || n_terms > RADIUS_TERMS_MAX) return fail(c, BMS_ERR_INVALID, "n_terms = %d outside [0, %d]", n_terms, RADIUS_TERMS_MAX);
  if (!std::isfinite(amp) || !std::isfinite(radius) || radius == 0) return fail(c, BMS_ERR_INVALID, "amp and radius must be finite, the radius not zero");
  if (n == 0 || n_cols == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  RadiusTerms terms{};
  terms.n = n_terms;
  for (int k = 1; k <= n_terms; ++k) terms.coef[k - 1] = amp * std::pow(radius, -k);
  int rc;
  void* d_t;
  if ((rc = upload(c, "smp_t", t, 8 * (size_t)n, &d_t))) return rc;
  const double* d_h0;
  if ((rc = stage_in(c, "in_data", h0, mem, ((size_t)(n - 1) * ld_h0 + n_cols) * 16, &d_h0))) return rc;
  double2* d_out = (double2*)out;
  int64_t ld_dev = ld_out;
  if (mem == BMS_HOST) {
    ld_dev = n_cols;
    if ((rc = dev_buf_t(c, "out_data", (size_t)n * n_cols, &d_out))) return rc;
  }
  hipStream_t S = c->stream;
  TIMED(c, BMS_TAG_POINTWISE, launch_radius_terms(S, (const double*)d_t, n, (const double2*)d_h0, ld_h0, (int)n_cols, terms, d_out, ld_dev));
  if (mem == BMS_HOST)
    HIP_TRY(c, hipMemcpy2DAsync(out, (size_t)ld_out * 16, d_out, (size_t)n_cols * 16, (size_t)n_cols * 16, (size_t)n, hipMemcpyDeviceToHost, S));
  HIP_TRY(c, hipStreamSynchronize(S));
  return BMS_OK;
} BMS_CATCH(c)
