// Fluxes of energy, momentum, angular momentum and boost in one pass over the modes, and the general sparse expectation value
// (kernels_flux.hip): the coefficient image of an l range, built on the host in long double and kept per context, and the two entries
// behind scri_amd/flux.py; the brackets of two waveforms <f|g>, <f|L_a|g>, <f|L_a L_b|g> in one pass (bms_pair_brackets); the Bondi
// charges P, J, N, G of AsymptoticBondiData rows in one pass (bms_bondi_charges) with a coefficient image of their own
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI)
#include "engine.h"

namespace {

// <l, m; 1, mu | J, m + mu> (Condon-Shortley), the closed forms for coupling with j = 1; zero outside the triangle and the m ranges
long double cg_one(int l, int m, int mu, int J) {
  const int M = m + mu;
  if (l < 0 || J < 0 || std::abs(J - l) > 1 || std::abs(m) > l || std::abs(M) > J || std::abs(mu) > 1) return 0.0L;
  const long double L = l, Md = M;
  if (J == l + 1) {
    if (mu == 1) return sqrtl((L + Md) * (L + Md + 1) / ((2 * L + 1) * (2 * L + 2)));
    if (mu == 0) return sqrtl((L - Md + 1) * (L + Md + 1) / ((2 * L + 1) * (L + 1)));
    return sqrtl((L - Md) * (L - Md + 1) / ((2 * L + 1) * (2 * L + 2)));
  }
  if (J == l) {
    if (l == 0) return 0.0L;
    if (mu == 1) return -sqrtl((L + Md) * (L - Md + 1) / (2 * L * (L + 1)));
    if (mu == 0) return Md / sqrtl(L * (L + 1));
    return sqrtl((L - Md) * (L + Md + 1) / (2 * L * (L + 1)));
  }
  if (mu == 1) return sqrtl((L - Md) * (L - Md + 1) / (2 * L * (2 * L + 1)));
  if (mu == 0) return -sqrtl((L - Md) * (L + Md) / (L * (2 * L + 1)));
  return sqrtl((L + Md + 1) * (L + Md) / (2 * L * (2 * L + 1)));
}

// <s, lp, m + mu| chi_mu |s, l, m>, chi_0 = cos(theta), chi_+-1 = sin(theta) e^{+-i phi} (the reference's p_z, p_plus, p_minus,
// scri/flux.py:213-300; the factors of pi of its two prefactors cancel)
long double chi_element(int s, int lp, int l, int m, int mu) {
  const long double ratio = (2.0L * l + 1) / (2.0L * lp + 1), spin = cg_one(l, -s, 0, lp);
  if (mu == 0) return sqrtl(ratio) * cg_one(l, m, 0, lp) * spin;
  return -mu * sqrtl(2 * ratio) * cg_one(l, m, mu, lp) * spin;
}
// <lp, m + mu| (eth chi)_mu |l, m> between spin -1 and spin -2 (raise = true, scri/flux.py:480-500, 526-560) and
// <lp, m + mu| (ethbar chi)_mu |l, m> between spin -2 and spin -1 (:501-521, 566-598), as the reference's generators give them
long double ladder_chi_element(bool raise, int lp, int l, int m, int mu) {
  const long double ratio = (2.0L * l + 1) / (2.0L * lp + 1), spin = raise ? cg_one(l, 2, -1, lp) : cg_one(l, 1, 1, lp);
  if (mu == 0) return sqrtl(2 * ratio) * cg_one(l, m, 0, lp) * spin;
  return -mu * 2 * sqrtl(ratio) * cg_one(l, m, mu, lp) * spin;
}


// (l1 l2 L; m1 m2 m3) for L = 0, 1, from the couplings with j = 1 above:
//     (l1 l2 1; m1 m2 m3) = (-1)^(l1 + l2 + 1) (l1 1 l2; m1 m3 m2),   (j1 j2 j3; m1 m2 m3) = (-1)^(j1 - j2 - m3) <j1 m1; j2 m2|j3, -m3> / sqrt(2 j3 + 1)
long double w3j_low(int l1, int l2, int L, int m1, int m2, int m3) {
  if (m1 + m2 + m3 != 0 || std::abs(m1) > l1 || std::abs(m2) > l2 || std::abs(m3) > L || std::abs(l1 - l2) > L) return 0.0L;
  if (L == 0) return (((l1 - m1) & 1) ? -1.0L : 1.0L) / sqrtl(2.0L * l1 + 1);
  const long double sign = ((l1 + l2 + 1 + l1 - 1 - m2) & 1) ? -1.0L : 1.0L;
  return sign * cg_one(l1, m1, m3, l2) / sqrtl(2.0L * l2 + 1);
}

// C of sum C sigma_{l1 m1} conj(x_{l2, m1 + mu}), l2 = l1 + dl, for the mode (L, M = -mu) of sigma times a spin s2 field built from
// bar(x)_{l2 m2} = (-1)^m2 conj(x_{l2, -m2}), m2 = M - m1:  s2 = -2: sigma x-bar;  s2 = -1: sigma eth x-bar, with the GHP ladder factor
// sqrt((l2 + 2)(l2 - 1) / 2) of eth on the spin -2 field folded in.  Zero where the neighbour does not exist or either l is below 2.
long double charge_coefficient(int L, int s2, int l1, int m1, int dl, int mu) {
  const int l2 = l1 + dl, M = -mu, m2 = M - m1, S = 2 + s2;
  if (l1 < 2 || l2 < 2 || std::abs(m1) > l1 || std::abs(m2) > l2 || std::abs(M) > L || std::abs(dl) > L) return 0.0L;
  const long double pi = 3.14159265358979323846264338327950288L;
  long double c = sqrtl((2.0L * l1 + 1) * (2.0L * l2 + 1) * (2.0L * L + 1) / (4 * pi)) * w3j_low(l1, l2, L, m1, m2, -M) * w3j_low(l1, l2, L, -2, -s2, S);
  if ((M + S + m2) & 1) c = -c;
  if (s2 == -1) c *= sqrtl((long double)(l2 + 2) * (l2 - 1) / 2);
  return c;
}

}  // namespace

// The coefficient image of l = ell_min .. ell_max (layout: kernels_flux.hip), every entry computed in long double and rounded once.
// eth and ethbar of a spin -2 field multiply its mode l by E_l = sqrt((l + 2)(l - 1)) and Eb_l = -sqrt((l - 2)(l + 3))
// (Newman-Penrose convention, scri/waveform_modes.py:478-572).  Signs of the eth chi / ethbar chi terms as scri/flux.py:704-707, 740-741.
BMS_INTERNAL void build_flux_image(int ell_min, int ell_max, std::vector<double>& image) {
  const int n = LM_total_size(ell_min, ell_max);
  image.assign((size_t)flux_image_doubles(n), 0.0);
  auto E = [](int l) { return sqrtl((long double)(l + 2) * (l - 1)); };
  auto Eb = [](int l) { return -sqrtl((long double)(l - 2) * (l + 3)); };
  for (int l = ell_min; l <= ell_max; ++l)
    for (int m = -l; m <= l; ++m) {
      const int c = LM_index(l, m, ell_min);
      for (int dl = -1; dl <= 1; ++dl)
        for (int mu = -1; mu <= 1; ++mu) {
          const int lp = l + dl, k = 3 * (dl + 1) + (mu + 1);
          if (lp < ell_min || lp > ell_max || std::abs(m + mu) > lp) continue;
          const long double chi2 = chi_element(-2, lp, l, m, mu);
          const long double bracket = (Eb(lp) * chi_element(-3, lp, l, m, mu) * Eb(l) - E(lp) * chi_element(-1, lp, l, m, mu) * E(l) + 6 * chi2) / 8;
          image[(size_t)(3 * k + 0) * n + c] = (double)chi2;
          image[(size_t)(3 * k + 1) * n + c] = (double)(bracket - E(lp) * ladder_chi_element(true, lp, l, m, mu) / 4);
          image[(size_t)(3 * k + 2) * n + c] = (double)(bracket + ladder_chi_element(false, lp, l, m, mu) * E(l) / 4);
        }
      image[(size_t)27 * n + c] = (double)sqrtl((long double)(l - m) * (l + m + 1));
      image[(size_t)28 * n + c] = (double)sqrtl((long double)(l + m) * (l - m + 1));
      image[(size_t)29 * n + c] = (double)l;
    }
}

// the first triplet with an index outside [0, n_cols): -1 if there is none
BMS_INTERNAL int64_t first_bad_triplet(const int32_t* rows, const int32_t* cols, int64_t n_el, int n_cols) {
  for (int64_t e = 0; e < n_el; ++e)
    if (rows[e] < 0 || rows[e] >= n_cols || cols[e] < 0 || cols[e] >= n_cols) return e;
  return -1;
}

// what bms_poincare_fluxes refuses before it selects a device; *n_modes on success
BMS_INTERNAL int flux_checks(bms_ctx* c, const double* t, const void* h, int64_t ld_h, const void* hdot, int64_t ld_hdot, int64_t n_times,
                             int ell_min, int ell_max, int mem, const double* energy, const double* momentum, const double* angular,
                             const double* boost, int* n_modes) {
  if (!hdot) return fail(c, BMS_ERR_INVALID, "bms_poincare_fluxes: NULL hdot");
  if (!energy && !momentum && !angular && !boost) return fail(c, BMS_ERR_INVALID, "bms_poincare_fluxes: every output is NULL");
  if ((angular || boost) && !h) return fail(c, BMS_ERR_INVALID, "bms_poincare_fluxes: the angular-momentum and boost fluxes need h, which is NULL");
  if (boost && !t) return fail(c, BMS_ERR_INVALID, "bms_poincare_fluxes: the boost flux needs the times, which are NULL");
  if (n_times < 0) return fail(c, BMS_ERR_INVALID, "bms_poincare_fluxes: negative n_times");
  if (ell_max < ell_min) return fail(c, BMS_ERR_INVALID, "bms_poincare_fluxes: bad ell range [%d, %d]", ell_min, ell_max);
  if (ell_min < 2) return fail(c, BMS_ERR_UNSUPPORTED, "bms_poincare_fluxes: ell_min = %d: the fused fluxes take spin -2 modes from ell_min >= 2", ell_min);
  if (ell_max > MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "bms_poincare_fluxes: ell_max = %d is beyond %d", ell_max, MAX_ELL);
  *n_modes = LM_total_size(ell_min, ell_max);
  if (ld_hdot < *n_modes || (h && ld_h < *n_modes)) return fail(c, BMS_ERR_INVALID, "bms_poincare_fluxes: row stride smaller than the number of modes (%d)", *n_modes);
  if (mem == BMS_DEVICE && ((((uintptr_t)h | (uintptr_t)hdot) & 15) || (((uintptr_t)energy | (uintptr_t)momentum | (uintptr_t)angular | (uintptr_t)boost) & 7)))
    return fail(c, BMS_ERR_INVALID, "bms_poincare_fluxes: device arrays must be aligned to their elements");
  return BMS_OK;
}

// the image of (ell_min, ell_max) on the device, built once per context and range (as the rotation's resident tables are)
static int ensure_flux_image(bms_ctx* c, int ell_min, int ell_max, const double** d_image) {
  char name[64];
  snprintf(name, sizeof name, "flux_image_%d_%d", ell_min, ell_max);
  const int n = LM_total_size(ell_min, ell_max);
  double* d = nullptr;
  if (int rc = dev_buf_t(c, name, (size_t)flux_image_doubles(n), &d)) return rc;
  *d_image = d;
  if (c->flux_images.count({ell_min, ell_max})) return BMS_OK;
  std::vector<double> image;
  build_flux_image(ell_min, ell_max, image);
  HIP_TRY(c, hipMemcpyAsync(d, image.data(), sizeof(double) * image.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host vector goes out of scope
  c->flux_images[{ell_min, ell_max}] = true;
  return BMS_OK;
}

// (sizes, not statuses) how the fused kernel would run n_modes columns on the current device: shape[0] time steps per pass of one
// workgroup (returned as well), shape[1] workgroups at most, shape[2] != 0 if the coefficient image is held in LDS; returns 0 if the range is not supported
extern "C" int64_t bms_flux_launch_shape(int n_modes, int64_t shape[3]) {
  FluxShape S;
  if (!shape || !flux_launch_shape(n_modes, &S)) return 0;
  shape[0] = S.waves, shape[1] = S.groups, shape[2] = S.tables_in_lds ? 1 : 0;
  return S.waves;
}

// pure host routine: the coefficient image the fused kernel reads, [30][n_modes] doubles (kernels_flux.hip states the layout)
extern "C" int bms_flux_coefficients(int ell_min, int ell_max, double* image_out) try {
  if (!image_out || ell_min < 2 || ell_max < ell_min || ell_max > MAX_ELL) return BMS_ERR_INVALID;
  std::vector<double> image;
  build_flux_image(ell_min, ell_max, image);
  std::memcpy(image_out, image.data(), sizeof(double) * image.size());
  return BMS_OK;
} BMS_CATCH(nullptr)

extern "C" int bms_poincare_fluxes(bms_ctx* c, const double* t, const void* h, int64_t ld_h, const void* hdot, int64_t ld_hdot, int64_t n_times,
                                   int ell_min, int ell_max, int mem, double* energy, double* momentum, double* angular, double* boost) try {
  if (!c) return BMS_ERR_INVALID;
  if (int rc0 = entry_mem(c, mem, "bms_poincare_fluxes", false)) return rc0;  // (the argument checks come before the device is selected)
  int rc, n_modes = 0;
  if ((rc = flux_checks(c, t, h, ld_h, hdot, ld_hdot, n_times, ell_min, ell_max, mem, energy, momentum, angular, boost, &n_modes))) return rc;
  if (n_times == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  FluxShape S;
  if (!flux_launch_shape(n_modes, &S))
    return fail(c, BMS_ERR_UNSUPPORTED, "bms_poincare_fluxes: %d modes (ell = %d .. %d): one time step's rows of h and hdot do not fit in LDS", n_modes, ell_min, ell_max);
  const double* d_image;
  if ((rc = ensure_flux_image(c, ell_min, ell_max, &d_image))) return rc;
  const bool with_h = angular || boost;
  CallIO io(c, mem);
  const double *d_t = nullptr, *d_h = nullptr, *d_n;
  if ((rc = io.in("in_data", hdot, ((size_t)(n_times - 1) * ld_hdot + n_modes) * 16, &d_n))) return rc;
  if (with_h && (rc = io.in("in_aux0", h, ((size_t)(n_times - 1) * ld_h + n_modes) * 16, &d_h))) return rc;
  if (boost) {  // (the times are a host array whatever `mem` is, as everywhere in this interface)
    void* vp;
    if ((rc = upload(c, "times", t, 8 * (size_t)n_times, &vp))) return rc;
    d_t = (const double*)vp;
  }
  double *d_e, *d_p, *d_j, *d_b;
  if ((rc = io.out("flux_e", energy, (size_t)n_times, &d_e))) return rc;
  if ((rc = io.out("flux_p", momentum, (size_t)3 * n_times, &d_p))) return rc;
  if ((rc = io.out("flux_j", angular, (size_t)3 * n_times, &d_j))) return rc;
  if ((rc = io.out("flux_b", boost, (size_t)3 * n_times, &d_b))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_poincare_fluxes(c->stream, d_t, d_h, ld_h, d_n, ld_hdot, n_times, ell_min, ell_max, d_image, d_e, d_p, d_j, d_b));
  return io.finish();
} BMS_CATCH(c)

// what bms_expectation_values refuses before it selects a device
BMS_INTERNAL int expectation_checks(bms_ctx* c, const void* a, int64_t ld_a, const void* b, int64_t ld_b, int64_t n_times, int n_cols,
                                    const int32_t* rows, const int32_t* cols, const void* values, int64_t n_el, int mem, const void* out) {
  if (!a || !b || !out || (n_el > 0 && (!rows || !cols || !values))) return fail(c, BMS_ERR_INVALID, "bms_expectation_values: NULL argument");
  if (n_times < 0 || n_el < 0 || n_cols < 1) return fail(c, BMS_ERR_INVALID, "bms_expectation_values: bad sizes");
  if (ld_a < n_cols || ld_b < n_cols) return fail(c, BMS_ERR_INVALID, "bms_expectation_values: row stride smaller than the number of columns (%d)", n_cols);
  const int64_t bad = first_bad_triplet(rows, cols, n_el, n_cols);
  if (bad >= 0)
    return fail(c, BMS_ERR_INVALID, "bms_expectation_values: element %lld couples row %d and column %d, outside [0, %d)", (long long)bad, (int)rows[bad],
                (int)cols[bad], n_cols);
  if (mem == BMS_DEVICE && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15))
    return fail(c, BMS_ERR_INVALID, "bms_expectation_values: device arrays must be aligned to their elements");
  return BMS_OK;
}

extern "C" int bms_expectation_values(bms_ctx* c, const void* a, int64_t ld_a, int conj_a, const void* b, int64_t ld_b, int64_t n_times, int n_cols,
                                      const int32_t* rows, const int32_t* cols, const void* values, int64_t n_el, int mem, void* out) try {
  if (!c) return BMS_ERR_INVALID;
  if (int rc0 = entry_mem(c, mem, "bms_expectation_values", false)) return rc0;
  int rc;
  if ((rc = expectation_checks(c, a, ld_a, b, ld_b, n_times, n_cols, rows, cols, values, n_el, mem, out))) return rc;
  if (n_times == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (n_cols > expectation_max_cols())
    return fail(c, BMS_ERR_UNSUPPORTED, "bms_expectation_values: %d columns: one time step's row pair does not fit in LDS (at most %d)", n_cols, expectation_max_cols());
  CallIO io(c, mem);
  void *d_rows, *d_cols, *d_vals;
  const size_t ne = (size_t)std::max<int64_t>(n_el, 1);
  if ((rc = dev_buf(c, "ev_rows", 4 * ne, &d_rows)) || (rc = dev_buf(c, "ev_cols", 4 * ne, &d_cols)) || (rc = dev_buf(c, "ev_values", 16 * ne, &d_vals))) return rc;
  if (n_el > 0) {
    if ((rc = upload(c, "ev_rows", rows, 4 * (size_t)n_el, &d_rows))) return rc;
    if ((rc = upload(c, "ev_cols", cols, 4 * (size_t)n_el, &d_cols))) return rc;
    if ((rc = upload(c, "ev_values", values, 16 * (size_t)n_el, &d_vals))) return rc;
  }
  const double *d_a, *d_b;
  if ((rc = io.in("in_data", a, ((size_t)(n_times - 1) * ld_a + n_cols) * 16, &d_a))) return rc;
  if ((rc = io.in("in_aux0", b, ((size_t)(n_times - 1) * ld_b + n_cols) * 16, &d_b))) return rc;
  double* d_out;
  if ((rc = io.out("ev_out", out, (size_t)2 * n_times, &d_out))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_expectation_values(c->stream, d_a, ld_a, conj_a != 0, d_b, ld_b, n_times, n_cols, (const int*)d_rows, (const int*)d_cols,
                                                        (const double*)d_vals, n_el, d_out));
  return io.finish();
} BMS_CATCH(c)

// what bms_pair_brackets refuses before it selects a device; on success *n_modes of the common range and the columns at which it starts
// in the rows of a and b
BMS_INTERNAL int pair_checks(bms_ctx* c, const void* a, int64_t ld_a, int ell_min_a, const void* b, int64_t ld_b, int ell_min_b, int64_t n_times,
                             int ell_min, int ell_max, int mem, const void* inner, const void* l_out, const void* ll_out, int* n_modes,
                             int64_t* off_a, int64_t* off_b) {
  if (!a || !b) return fail(c, BMS_ERR_INVALID, "bms_pair_brackets: NULL waveform");
  if (!inner && !l_out && !ll_out) return fail(c, BMS_ERR_INVALID, "bms_pair_brackets: every output is NULL");
  if (n_times < 0) return fail(c, BMS_ERR_INVALID, "bms_pair_brackets: negative n_times");
  if (ell_max < ell_min) return fail(c, BMS_ERR_INVALID, "bms_pair_brackets: bad ell range [%d, %d]", ell_min, ell_max);
  if (ell_min_a < 0 || ell_min_b < 0 || ell_min < ell_min_a || ell_min < ell_min_b)
    return fail(c, BMS_ERR_INVALID, "bms_pair_brackets: the common range starts at ell = %d, below a row's first ell (%d, %d)", ell_min, ell_min_a, ell_min_b);
  if (ell_max > MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "bms_pair_brackets: ell_max = %d is beyond %d", ell_max, MAX_ELL);
  *n_modes = LM_total_size(ell_min, ell_max);
  *off_a = (int64_t)ell_min * ell_min - (int64_t)ell_min_a * ell_min_a;
  *off_b = (int64_t)ell_min * ell_min - (int64_t)ell_min_b * ell_min_b;
  if (ld_a < *off_a + *n_modes || ld_b < *off_b + *n_modes)
    return fail(c, BMS_ERR_INVALID, "bms_pair_brackets: row stride smaller than the columns up to ell_max (%lld, %lld)", (long long)(*off_a + *n_modes),
                (long long)(*off_b + *n_modes));
  if (mem == BMS_DEVICE && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)inner | (uintptr_t)l_out | (uintptr_t)ll_out) & 15))
    return fail(c, BMS_ERR_INVALID, "bms_pair_brackets: device arrays must be aligned to their elements");
  return BMS_OK;
}

// (sizes, not statuses) how the bracket kernel would run n_modes columns on the current device: shape[0] time steps per pass of one
// workgroup (returned as well), shape[1] workgroups at most, shape[2] = 0 (it reads no tables); returns 0 if a row does not fit in LDS
extern "C" int64_t bms_pair_launch_shape(int n_modes, int64_t shape[3]) {
  FluxShape S;
  if (!shape || !pair_launch_shape(n_modes, &S)) return 0;
  shape[0] = S.waves, shape[1] = S.groups, shape[2] = 0;
  return S.waves;
}

extern "C" int bms_pair_brackets(bms_ctx* c, const void* a, int64_t ld_a, int ell_min_a, const void* b, int64_t ld_b, int ell_min_b, int64_t n_times,
                                 int ell_min, int ell_max, int mem, void* inner, void* l_out, void* ll_out) try {
  if (!c) return BMS_ERR_INVALID;
  if (int rc0 = entry_mem(c, mem, "bms_pair_brackets", false)) return rc0;  // (the argument checks come before the device is selected)
  int rc, n_modes = 0;
  int64_t off_a = 0, off_b = 0;
  if ((rc = pair_checks(c, a, ld_a, ell_min_a, b, ld_b, ell_min_b, n_times, ell_min, ell_max, mem, inner, l_out, ll_out, &n_modes, &off_a, &off_b))) return rc;
  if (n_times == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  FluxShape S;
  if (!pair_launch_shape(n_modes, &S))
    return fail(c, BMS_ERR_UNSUPPORTED, "bms_pair_brackets: %d modes (ell = %d .. %d): one time step's row does not fit in LDS", n_modes, ell_min, ell_max);
  CallIO io(c, mem);
  // (host rows go up whole, from their first column to the last of the common range: the kernel reads the range where it lies)
  const double *d_a, *d_b;
  if ((rc = io.in("in_data", a, ((size_t)(n_times - 1) * ld_a + off_a + n_modes) * 16, &d_a))) return rc;
  if ((rc = io.in("in_aux0", b, ((size_t)(n_times - 1) * ld_b + off_b + n_modes) * 16, &d_b))) return rc;
  double *d_i, *d_l, *d_ll;
  if ((rc = io.out("pair_i", inner, (size_t)2 * n_times, &d_i))) return rc;
  if ((rc = io.out("pair_l", l_out, (size_t)6 * n_times, &d_l))) return rc;
  if ((rc = io.out("pair_ll", ll_out, (size_t)18 * n_times, &d_ll))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_pair_brackets(c->stream, d_a + 2 * off_a, ld_a, d_b + 2 * off_b, ld_b, n_times, ell_min, ell_max, d_i, d_l, d_ll));
  return io.finish();
} BMS_CATCH(c)

// ---- Bondi charges (scri/asymptotic_bondi_data/bms_charges.py:14-200) of rows stored from l = 0 -------------------------------------
// The coefficient image of l = 0 .. ell_max (layout: kernels_flux.hip, charge_kernel), every entry computed in long double and rounded once
BMS_INTERNAL void build_charge_image(int ell_max, std::vector<double>& image) {
  const int n = LM_total_size(0, ell_max);
  image.assign((size_t)charge_image_doubles(n), 0.0);
  for (int l = 0; l <= ell_max; ++l)
    for (int m = -l; m <= l; ++m) {
      const int c = LM_index(l, m, 0);
      for (int dl = -1; dl <= 1; ++dl)
        for (int mu = -1; mu <= 1; ++mu) {
          const int k = 3 * (dl + 1) + (mu + 1);
          if (l + dl > ell_max) continue;
          image[(size_t)(2 * k + 0) * n + c] = (double)charge_coefficient(1, -2, l, m, dl, mu);
          image[(size_t)(2 * k + 1) * n + c] = (double)charge_coefficient(1, -1, l, m, dl, mu);
        }
      image[(size_t)18 * n + c] = (double)charge_coefficient(0, -2, l, m, 0, 0);
      image[(size_t)19 * n + c] = (double)l;
    }
}

// what bms_bondi_charges refuses before it selects a device; *n_modes on success
BMS_INTERNAL int charge_checks(bms_ctx* c, const double* t, const void* psi1, int64_t ld_psi1, const void* psi2, int64_t ld_psi2, const void* sigma,
                               int64_t ld_sigma, const void* sigma_dot, int64_t ld_sigma_dot, int64_t n_times, int ell_max, int mem,
                               const double* four_momentum, const double* angular, const double* boost, const double* com, int* n_modes) {
  if (!four_momentum && !angular && !boost && !com) return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: every output is NULL");
  if (!sigma) return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: NULL sigma");
  if ((four_momentum || boost) && !sigma_dot)
    return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: the four-momentum and the boost charge need sigma_dot, which is NULL");
  if ((four_momentum || boost) && !psi2) return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: the four-momentum and the boost charge need psi2, which is NULL");
  if ((angular || boost || com) && !psi1)
    return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: the angular momentum, the boost charge and the centre-of-mass charge need psi1, which is NULL");
  if (boost && !t) return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: the boost charge needs the times, which are NULL");
  if (n_times < 0) return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: negative n_times");
  if (ell_max < 0) return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: negative ell_max");
  if (ell_max < 2) return fail(c, BMS_ERR_UNSUPPORTED, "bms_bondi_charges: ell_max = %d: the shear starts at ell = 2", ell_max);
  if (ell_max > MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "bms_bondi_charges: ell_max = %d is beyond %d", ell_max, MAX_ELL);
  *n_modes = LM_total_size(0, ell_max);
  if (ld_sigma < *n_modes || (sigma_dot && ld_sigma_dot < *n_modes))
    return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: row stride smaller than the number of modes (%d)", *n_modes);
  if ((psi1 && ld_psi1 < 4) || (psi2 && ld_psi2 < 4)) return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: row stride of psi1 or psi2 smaller than its four columns read");
  if (mem == BMS_DEVICE && ((((uintptr_t)psi1 | (uintptr_t)psi2 | (uintptr_t)sigma | (uintptr_t)sigma_dot) & 15) ||
                            (((uintptr_t)four_momentum | (uintptr_t)angular | (uintptr_t)boost | (uintptr_t)com) & 7)))
    return fail(c, BMS_ERR_INVALID, "bms_bondi_charges: device arrays must be aligned to their elements");
  return BMS_OK;
}

// the image of ell_max on the device, built once per context and ell_max (as the fluxes' is)
static int ensure_charge_image(bms_ctx* c, int ell_max, const double** d_image) {
  char name[64];
  snprintf(name, sizeof name, "charge_image_%d", ell_max);
  const int n = LM_total_size(0, ell_max);
  double* d = nullptr;
  if (int rc = dev_buf_t(c, name, (size_t)charge_image_doubles(n), &d)) return rc;
  *d_image = d;
  if (c->charge_images.count(ell_max)) return BMS_OK;
  std::vector<double> image;
  build_charge_image(ell_max, image);
  HIP_TRY(c, hipMemcpyAsync(d, image.data(), sizeof(double) * image.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host vector goes out of scope
  c->charge_images[ell_max] = true;
  return BMS_OK;
}

// (sizes, not statuses) as bms_flux_launch_shape, for the charge kernel and n_modes = (ell_max + 1)^2 columns
extern "C" int64_t bms_charge_launch_shape(int n_modes, int64_t shape[3]) {
  FluxShape S;
  if (!shape || !charge_launch_shape(n_modes, &S)) return 0;
  shape[0] = S.waves, shape[1] = S.groups, shape[2] = S.tables_in_lds ? 1 : 0;
  return S.waves;
}

// pure host routine: the coefficient image the charge kernel reads, [20][(ell_max + 1)^2] doubles (kernels_flux.hip states the layout)
extern "C" int bms_charge_coefficients(int ell_max, double* image_out) try {
  if (!image_out || ell_max < 2 || ell_max > MAX_ELL) return BMS_ERR_INVALID;
  std::vector<double> image;
  build_charge_image(ell_max, image);
  std::memcpy(image_out, image.data(), sizeof(double) * image.size());
  return BMS_OK;
} BMS_CATCH(nullptr)

extern "C" int bms_bondi_charges(bms_ctx* c, const double* t, const void* psi1, int64_t ld_psi1, const void* psi2, int64_t ld_psi2, const void* sigma,
                                 int64_t ld_sigma, const void* sigma_dot, int64_t ld_sigma_dot, int64_t n_times, int ell_max, int mem,
                                 double* four_momentum, double* angular, double* boost, double* com) try {
  if (!c) return BMS_ERR_INVALID;
  if (int rc0 = entry_mem(c, mem, "bms_bondi_charges", false)) return rc0;  // (the argument checks come before the device is selected)
  int rc, n_modes = 0;
  if ((rc = charge_checks(c, t, psi1, ld_psi1, psi2, ld_psi2, sigma, ld_sigma, sigma_dot, ld_sigma_dot, n_times, ell_max, mem, four_momentum, angular, boost,
                          com, &n_modes)))
    return rc;
  if (n_times == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  FluxShape S;
  if (!charge_launch_shape(n_modes, &S))
    return fail(c, BMS_ERR_UNSUPPORTED, "bms_bondi_charges: %d modes (ell_max = %d): one time step's rows of sigma and sigma_dot do not fit in LDS", n_modes, ell_max);
  const double* d_image;
  if ((rc = ensure_charge_image(c, ell_max, &d_image))) return rc;
  const bool with_dot = four_momentum || boost, with_psi1 = angular || boost || com;
  CallIO io(c, mem);
  const double *d_t = nullptr, *d_p1 = nullptr, *d_p2 = nullptr, *d_s, *d_sd = nullptr;
  if ((rc = io.in("in_data", sigma, ((size_t)(n_times - 1) * ld_sigma + n_modes) * 16, &d_s))) return rc;
  if (with_dot && (rc = io.in("in_aux0", sigma_dot, ((size_t)(n_times - 1) * ld_sigma_dot + n_modes) * 16, &d_sd))) return rc;
  if (with_psi1 && (rc = io.in("in_aux1", psi1, ((size_t)(n_times - 1) * ld_psi1 + 4) * 16, &d_p1))) return rc;
  if (with_dot && (rc = io.in("in_aux2", psi2, ((size_t)(n_times - 1) * ld_psi2 + 4) * 16, &d_p2))) return rc;
  if (boost) {  // (the times are a host array whatever `mem` is, as everywhere in this interface)
    void* vp;
    if ((rc = upload(c, "times", t, 8 * (size_t)n_times, &vp))) return rc;
    d_t = (const double*)vp;
  }
  double *d_p, *d_j, *d_n, *d_g;
  if ((rc = io.out("charge_p", four_momentum, (size_t)4 * n_times, &d_p))) return rc;
  if ((rc = io.out("charge_j", angular, (size_t)3 * n_times, &d_j))) return rc;
  if ((rc = io.out("charge_n", boost, (size_t)3 * n_times, &d_n))) return rc;
  if ((rc = io.out("charge_g", com, (size_t)3 * n_times, &d_g))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_bondi_charges(c->stream, d_t, d_p1, ld_psi1, d_p2, ld_psi2, d_s, ld_sigma, d_sd, ld_sigma_dot, n_times, ell_max, d_image,
                                                   d_p, d_j, d_n, d_g));
  return io.finish();
} BMS_CATCH(c)
