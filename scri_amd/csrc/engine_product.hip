// Products of spin-weighted functions on Gauss-Legendre rows (kernels_product.hip): the nodes and weights (Newton iteration on P_n) and the
// tables lambda^s_lm(theta_j) = sYlm(theta_j, 0), built on the host in long double and rounded once, kept on the device per context and
// (spin, ell_max, n_nodes); the entries bms_mode_product, bms_supermomenta, bms_bondi_constraints and bms_bianchi_rhs, their launch shape and the pure host export of the tables
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI)
#include "engine.h"

namespace {

constexpr int PRODUCT_MAX_SPIN = 4;
const long double PI_L = 3.14159265358979323846264338327950288L;

// nodes x_j = cos(theta_j), theta ascending, and weights of the n-point Gauss-Legendre rule: Newton iteration on P_n from the Chebyshev
// guess for the upper half, mirrored (the middle node of an odd rule is exactly zero)
void gauss_legendre(int n, std::vector<long double>& x, std::vector<long double>& w) {
  x.assign((size_t)n, 0.0L);
  w.assign((size_t)n, 0.0L);
  for (int i = 0; i < (n + 1) / 2; ++i) {
    long double z = (2 * i + 1 == n) ? 0.0L : cosl(PI_L * (i + 0.75L) / (n + 0.5L)), dp = 0.0L;
    for (int it = 0; it < 100; ++it) {
      long double p0 = 1.0L, p1 = z;  // P_0, P_1
      for (int k = 2; k <= n; ++k) {
        const long double p2 = ((2 * k - 1) * z * p1 - (k - 1) * p0) / k;
        p0 = p1, p1 = p2;
      }
      if (n == 1) p0 = 1.0L, p1 = z;
      dp = n * (z * p1 - p0) / (z * z - 1.0L);
      if (2 * i + 1 == n) break;  // (z = 0 is the root; dp is what the weight needs)
      const long double dz = p1 / dp;
      z -= dz;
      if (fabsl(dz) <= 1e-18L * fabsl(z)) {  // one more evaluation of dp at the converged node
        p0 = 1.0L, p1 = z;
        for (int k = 2; k <= n; ++k) {
          const long double p2 = ((2 * k - 1) * z * p1 - (k - 1) * p0) / k;
          p0 = p1, p1 = p2;
        }
        dp = n * (z * p1 - p0) / (z * z - 1.0L);
        break;
      }
    }
    x[(size_t)i] = z, x[(size_t)(n - 1 - i)] = -z;
    w[(size_t)i] = w[(size_t)(n - 1 - i)] = 2.0L / ((1.0L - z * z) * dp * dp);
  }
}

long double ipow_l(long double v, int k) {
  long double r = 1.0L;
  for (; k > 0; k >>= 1, v *= v)
    if (k & 1) r *= v;
  return r;
}

long double sqrt_binom_l(int l0, int k) {  // sqrt(C(2 l0, k))
  const int nn = 2 * l0;
  if (k > nn - k) k = nn - k;
  long double c = 1.0L;
  for (int i = 1; i <= k; ++i) c = c * (nn - k + i) / i;
  return sqrtl(c);
}

// d^{l0}_{mp, m}(ra, rb), l0 = max(|mp|, |m|)  (wigner.h, d_start)
long double d_start_l(int l0, int mp, int m, long double ra, long double rb) {
  if (l0 == mp) {
    const long double v = sqrt_binom_l(l0, l0 - m) * ipow_l(ra, l0 + m) * ipow_l(rb, l0 - m);
    return ((l0 - m) & 1) ? -v : v;
  }
  if (l0 == -mp) return sqrt_binom_l(l0, l0 + m) * ipow_l(ra, l0 - m) * ipow_l(rb, l0 + m);
  if (l0 == m) return sqrt_binom_l(l0, l0 - mp) * ipow_l(ra, l0 + mp) * ipow_l(rb, l0 - mp);
  const long double v = sqrt_binom_l(l0, l0 + mp) * ipow_l(ra, l0 - mp) * ipow_l(rb, l0 + mp);
  return ((l0 + mp) & 1) ? -v : v;
}

// row[(l, m)] = lambda^s_lm = (-1)^s sqrt((2 l + 1) / 4 pi) d^l_{m, -s}(theta), cos(theta) = x, for l = 0 .. ell_max (zero below |s|): the
// three-term recurrence in l of wigner.h (DChain) carried in long double
void lambda_row(int spin, int ell_max, long double x, long double* row) {
  const long double ra = sqrtl((1.0L + x) / 2), rb = sqrtl((1.0L - x) / 2);
  const long double sig = ra >= rb ? 1.0L : -1.0L, t = ra >= rb ? rb * rb : ra * ra;
  const int mq = -spin;
  for (int m = -ell_max; m <= ell_max; ++m) {
    int l = std::max(std::abs(m), std::abs(mq));
    if (l > ell_max) continue;
    long double dm1 = 0.0L, d0 = d_start_l(l, m, mq, ra, rb);
    for (;; ++l) {
      const long double v = sqrtl((2.0L * l + 1) / (4 * PI_L)) * d0;
      row[l * (l + 1) + m] = (spin & 1) ? -v : v;
      if (l == ell_max) break;
      long double d1;
      if (l == 0) {
        d1 = sig * (1.0L - 2.0L * t) * d0;
      } else {
        const long double L = l, L1 = l + 1, mm = (long double)(m * mq);
        const long double c1 = (2 * L + 1) * sig * ((L * L1 - sig * mm) - (2 * L * L1) * t);
        const long double c2 = L1 * sqrtl((L * L - (long double)(m * m)) * (L * L - (long double)(mq * mq)));
        const long double den = L * sqrtl((L1 * L1 - (long double)(m * m)) * (L1 * L1 - (long double)(mq * mq)));
        d1 = (c1 * d0 - c2 * dm1) / den;
      }
      dm1 = d0, d0 = d1;
    }
  }
}

}  // namespace

// cos(theta_j), w_j and table[j][(l, m)] = lambda^spin_lm(theta_j) (times 2 pi w_j if `weighted`) of the n_nodes-point rule, l = 0 .. ell_max:
// every value computed in long double and rounded once.  cos_theta / weights may be null
BMS_INTERNAL void build_product_table(int spin, int ell_max, int n_nodes, bool weighted, double* cos_theta, double* weights, std::vector<double>& table) {
  const size_t n_cols = (size_t)(ell_max + 1) * (ell_max + 1);
  std::vector<long double> x, w, row(n_cols);
  gauss_legendre(n_nodes, x, w);
  table.assign((size_t)n_nodes * n_cols, 0.0);
  for (int j = 0; j < n_nodes; ++j) {
    std::fill(row.begin(), row.end(), 0.0L);
    lambda_row(spin, ell_max, x[(size_t)j], row.data());
    const long double scale = weighted ? 2 * PI_L * w[(size_t)j] : 1.0L;
    for (size_t c = 0; c < n_cols; ++c) table[(size_t)j * n_cols + c] = (double)(scale * row[c]);
    if (cos_theta) cos_theta[j] = (double)x[(size_t)j];
    if (weights) weights[j] = (double)w[(size_t)j];
  }
}

// what both entries refuse of the sizes of a product before a device is selected; *n_nodes on success
static int product_size_checks(bms_ctx* c, const char* who, int s_a, int l_a, int s_b, int l_b, int l_out, int64_t n_times, int* n_nodes) {
  if (n_times < 0) return fail(c, BMS_ERR_INVALID, "%s: negative n_times", who);
  if (l_a < 0 || l_b < 0 || l_out < 0) return fail(c, BMS_ERR_INVALID, "%s: negative ell_max", who);
  if (l_a > MAX_ELL || l_b > MAX_ELL || l_out > MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "%s: an ell_max beyond %d", who, MAX_ELL);
  if (l_out > l_a + l_b)
    return fail(c, BMS_ERR_INVALID, "%s: ell_max_out = %d is beyond ell_max_a + ell_max_b = %d, where the product ends", who, l_out, l_a + l_b);
  if (std::abs(s_a) > PRODUCT_MAX_SPIN || std::abs(s_b) > PRODUCT_MAX_SPIN || std::abs(s_a + s_b) > PRODUCT_MAX_SPIN)
    return fail(c, BMS_ERR_UNSUPPORTED, "%s: spins %d and %d: spins and their sum are carried up to |s| = %d", who, s_a, s_b, PRODUCT_MAX_SPIN);
  *n_nodes = product_nodes(l_a, l_b, l_out);
  return BMS_OK;
}

BMS_INTERNAL int product_checks(bms_ctx* c, const void* a, int64_t ld_a, int spin_a, int ell_max_a, int conj_a, const void* b, int64_t ld_b, int spin_b,
                                int ell_max_b, int conj_b, int64_t n_times, int ell_max_out, int mem, const void* out, int64_t ld_out, int* n_nodes) {
  const char* who = "bms_mode_product";
  if (!a || !b || !out) return fail(c, BMS_ERR_INVALID, "%s: NULL a, b or out", who);
  if (int rc = product_size_checks(c, who, conj_a ? -spin_a : spin_a, ell_max_a, conj_b ? -spin_b : spin_b, ell_max_b, ell_max_out, n_times, n_nodes)) return rc;
  if (ld_a < (int64_t)LM_total_size(0, ell_max_a) || ld_b < (int64_t)LM_total_size(0, ell_max_b))
    return fail(c, BMS_ERR_INVALID, "%s: row stride of a or b smaller than its (ell_max + 1)^2 columns read", who);
  if (ld_out < (int64_t)LM_total_size(0, ell_max_out))
    return fail(c, BMS_ERR_INVALID, "%s: row stride of out smaller than the (ell_max_out + 1)^2 = %d columns written", who, LM_total_size(0, ell_max_out));
  if (mem == BMS_DEVICE && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15))
    return fail(c, BMS_ERR_INVALID, "%s: device arrays must be aligned to their elements", who);
  return BMS_OK;
}

BMS_INTERNAL int supermomenta_checks(bms_ctx* c, const void* psi2, int64_t ld_psi2, const void* sigma, int64_t ld_sigma, const void* sigma_dot,
                                     int64_t ld_sigma_dot, int64_t n_times, int ell_max, int ell_max_out, int mem, const void* bondi_sachs,
                                     const void* moreschi, const void* geroch, const void* geroch_winicour, const void* mass_aspect, int64_t ld_out,
                                     int* n_nodes) {
  const char* who = "bms_supermomenta";
  if (!bondi_sachs && !moreschi && !geroch && !geroch_winicour && !mass_aspect) return fail(c, BMS_ERR_INVALID, "%s: every output is NULL", who);
  if (!psi2 || !sigma || !sigma_dot) return fail(c, BMS_ERR_INVALID, "%s: NULL psi2, sigma or sigma_dot", who);
  if (n_times < 0) return fail(c, BMS_ERR_INVALID, "%s: negative n_times", who);
  if (ell_max < 0 || ell_max_out < 0) return fail(c, BMS_ERR_INVALID, "%s: negative ell_max", who);
  if (ell_max_out > ell_max) return fail(c, BMS_ERR_INVALID, "%s: ell_max_out = %d is beyond ell_max = %d", who, ell_max_out, ell_max);
  if (ell_max < 2) return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max = %d: the shear starts at ell = 2", who, ell_max);
  if (int rc = product_size_checks(c, who, 2, ell_max, -2, ell_max, ell_max_out, n_times, n_nodes)) return rc;
  const int64_t n_in = LM_total_size(0, ell_max), n_out = LM_total_size(0, ell_max_out);
  if (ld_sigma < n_in || ld_sigma_dot < n_in) return fail(c, BMS_ERR_INVALID, "%s: row stride of sigma or sigma_dot smaller than the number of modes (%d)", who, (int)n_in);
  if (ld_psi2 < n_out || ld_out < n_out)
    return fail(c, BMS_ERR_INVALID, "%s: row stride of psi2 or of the outputs smaller than the (ell_max_out + 1)^2 = %d columns", who, (int)n_out);
  if (mem == BMS_DEVICE && (((uintptr_t)psi2 | (uintptr_t)sigma | (uintptr_t)sigma_dot | (uintptr_t)bondi_sachs | (uintptr_t)moreschi | (uintptr_t)geroch |
                             (uintptr_t)geroch_winicour | (uintptr_t)mass_aspect) & 15))
    return fail(c, BMS_ERR_INVALID, "%s: device arrays must be aligned to their elements", who);
  return BMS_OK;
}

// the table of (spin, ell_max, n_nodes, weighted) on the device, built once per context (as the charge image is)
static int ensure_product_table(bms_ctx* c, int spin, int ell_max, int n_nodes, bool weighted, const double** d_table) {
  char name[96];
  snprintf(name, sizeof name, "product_table_%d_%d_%d_%d", spin, ell_max, n_nodes, weighted ? 1 : 0);
  const size_t count = (size_t)n_nodes * LM_total_size(0, ell_max);
  double* d = nullptr;
  if (int rc = dev_buf_t(c, name, count, &d)) return rc;
  *d_table = d;
  const std::array<int, 4> key{spin, ell_max, n_nodes, weighted ? 1 : 0};
  if (c->product_tables.count(key)) return BMS_OK;
  std::vector<double> table;
  build_product_table(spin, ell_max, n_nodes, weighted, nullptr, nullptr, table);
  HIP_TRY(c, hipMemcpyAsync(d, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host vector goes out of scope
  c->product_tables[key] = true;
  return BMS_OK;
}

// (sizes, not statuses) shape[0] time steps per pass of a workgroup (returned as well; 0: a step does not fit in LDS), shape[1] workgroups
// at most, shape[2] != 0 if the tables sit in LDS
extern "C" int64_t bms_product_launch_shape(int ell_max_a, int ell_max_b, int ell_max_out, int64_t shape[3]) {
  ProductShape S;
  if (!shape || ell_max_out > ell_max_a + ell_max_b || !product_launch_shape(ell_max_a, ell_max_b, ell_max_out, &S)) return 0;
  shape[0] = S.steps, shape[1] = S.groups, shape[2] = S.tables_in_lds ? 1 : 0;
  return S.steps;
}

// pure host routine: nodes, weights and the UNWEIGHTED table of one spin as the kernel reads it
extern "C" int bms_product_tables(int spin, int ell_max, int n_nodes, double* cos_theta, double* weights, double* table) try {
  if (!cos_theta || !weights || !table || ell_max < 0 || ell_max > MAX_ELL || n_nodes < 1 || n_nodes > 2 * MAX_ELL || std::abs(spin) > PRODUCT_MAX_SPIN)
    return BMS_ERR_INVALID;
  std::vector<double> image;
  build_product_table(spin, ell_max, n_nodes, false, cos_theta, weights, image);
  std::memcpy(table, image.data(), sizeof(double) * image.size());
  return BMS_OK;
} BMS_CATCH(nullptr)

extern "C" int bms_mode_product(bms_ctx* c, const void* a, int64_t ld_a, int spin_a, int ell_max_a, int conj_a, const void* b, int64_t ld_b, int spin_b,
                                int ell_max_b, int conj_b, int64_t n_times, int ell_max_out, int mem, void* out, int64_t ld_out) try {
  if (!c) return BMS_ERR_INVALID;
  if (int rc0 = entry_mem(c, mem, "bms_mode_product", false)) return rc0;  // (the argument checks come before the device is selected)
  int rc, n_nodes = 0;
  if ((rc = product_checks(c, a, ld_a, spin_a, ell_max_a, conj_a, b, ld_b, spin_b, ell_max_b, conj_b, n_times, ell_max_out, mem, out, ld_out, &n_nodes))) return rc;
  if (n_times == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  ProductShape S;
  if (!product_launch_shape(ell_max_a, ell_max_b, ell_max_out, &S))
    return fail(c, BMS_ERR_UNSUPPORTED, "bms_mode_product: ell_max %d and %d to %d on %d rows: the rows and panels of one time step do not fit in LDS",
                ell_max_a, ell_max_b, ell_max_out, n_nodes);
  const int s_a = conj_a ? -spin_a : spin_a, s_b = conj_b ? -spin_b : spin_b;
  const double *t_a, *t_b, *t_o;
  if ((rc = ensure_product_table(c, s_a, ell_max_a, n_nodes, false, &t_a))) return rc;
  if ((rc = ensure_product_table(c, s_b, ell_max_b, n_nodes, false, &t_b))) return rc;
  if ((rc = ensure_product_table(c, s_a + s_b, ell_max_out, n_nodes, true, &t_o))) return rc;
  const int n_a = LM_total_size(0, ell_max_a), n_b = LM_total_size(0, ell_max_b), n_o = LM_total_size(0, ell_max_out);
  CallIO io(c, mem);
  const double *d_a, *d_b;
  double* d_o;
  if ((rc = io.in("in_data", a, ((size_t)(n_times - 1) * ld_a + n_a) * 16, &d_a))) return rc;
  if ((rc = io.in("in_aux0", b, ((size_t)(n_times - 1) * ld_b + n_b) * 16, &d_b))) return rc;
  if ((rc = io.out_rows("product_out", out, (size_t)n_times, (size_t)2 * n_o, (size_t)2 * ld_out, &d_o))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_mode_product(c->stream, d_a, ld_a, spin_a, ell_max_a, conj_a, d_b, ld_b, spin_b, ell_max_b, conj_b, n_times, ell_max_out,
                                                  t_a, t_b, t_o, d_o, io.host() ? n_o : ld_out));
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_supermomenta(bms_ctx* c, const void* psi2, int64_t ld_psi2, const void* sigma, int64_t ld_sigma, const void* sigma_dot,
                                int64_t ld_sigma_dot, int64_t n_times, int ell_max, int ell_max_out, int mem, int integrated, void* bondi_sachs,
                                void* moreschi, void* geroch, void* geroch_winicour, void* mass_aspect, int64_t ld_out) try {
  if (!c) return BMS_ERR_INVALID;
  if (int rc0 = entry_mem(c, mem, "bms_supermomenta", false)) return rc0;  // (the argument checks come before the device is selected)
  int rc, n_nodes = 0;
  if ((rc = supermomenta_checks(c, psi2, ld_psi2, sigma, ld_sigma, sigma_dot, ld_sigma_dot, n_times, ell_max, ell_max_out, mem, bondi_sachs, moreschi, geroch,
                                geroch_winicour, mass_aspect, ld_out, &n_nodes)))
    return rc;
  if (n_times == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  ProductShape S;
  if (!product_launch_shape(ell_max, ell_max, ell_max_out, &S))
    return fail(c, BMS_ERR_UNSUPPORTED, "bms_supermomenta: ell_max %d to %d on %d rows: the rows and panels of one time step do not fit in LDS", ell_max,
                ell_max_out, n_nodes);
  const double *t_p, *t_m, *t_o;
  if ((rc = ensure_product_table(c, 2, ell_max, n_nodes, false, &t_p))) return rc;
  if ((rc = ensure_product_table(c, -2, ell_max, n_nodes, false, &t_m))) return rc;
  if ((rc = ensure_product_table(c, 0, ell_max_out, n_nodes, true, &t_o))) return rc;
  const int n_in = LM_total_size(0, ell_max), n_o = LM_total_size(0, ell_max_out);
  CallIO io(c, mem);
  const double *d_p, *d_s, *d_d;
  if ((rc = io.in("in_data", sigma, ((size_t)(n_times - 1) * ld_sigma + n_in) * 16, &d_s))) return rc;
  if ((rc = io.in("in_aux0", sigma_dot, ((size_t)(n_times - 1) * ld_sigma_dot + n_in) * 16, &d_d))) return rc;
  if ((rc = io.in("in_aux1", psi2, ((size_t)(n_times - 1) * ld_psi2 + n_o) * 16, &d_p))) return rc;
  void* const home[5] = {bondi_sachs, moreschi, geroch, geroch_winicour, mass_aspect};
  const char* const block[5] = {"super_bs", "super_m", "super_g", "super_gw", "super_mass"};
  double* d_out[5];
  for (int k = 0; k < 5; ++k)
    if ((rc = io.out_rows(block[k], home[k], (size_t)n_times, (size_t)2 * n_o, (size_t)2 * ld_out, &d_out[k]))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_supermomenta(c->stream, d_p, ld_psi2, d_s, ld_sigma, d_d, ld_sigma_dot, n_times, ell_max, ell_max_out, integrated, t_p, t_m,
                                                  t_o, d_out[0], d_out[1], d_out[2], d_out[3], d_out[4], io.host() ? n_o : ld_out));
  return io.finish();
} BMS_CATCH(c)

// ---- the six Bondi-gauge violations and their norms (constraint_kernel)
namespace {

constexpr int N_VIOLATIONS = 6;
const char* const CONSTRAINT_INPUT_NAME[CONSTRAINT_INPUTS] = {"psi0", "psi1", "psi2", "psi3", "psi4", "sigma", "psi0_dot", "psi1_dot", "psi2_dot", "sigma_dot", "sigma_ddot"};
// bit i: violation k reads input i (kernels.h: psi0 .. psi4, sigma, the three psi_dot, sigma_dot, sigma_ddot)
constexpr unsigned CONSTRAINT_READS[N_VIOLATIONS] = {
    1u << 1 | 1u << 2 | 1u << 5 | 1u << 6, 1u << 2 | 1u << 3 | 1u << 5 | 1u << 7, 1u << 3 | 1u << 4 | 1u << 5 | 1u << 8,
    1u << 3 | 1u << 9,                     1u << 4 | 1u << 10,                    1u << 2 | 1u << 5 | 1u << 9};

}  // namespace

// what bms_bondi_constraints refuses before it selects a device; in[] / ld[] in the order of kernels.h.  *reads: the inputs the outputs asked for read
BMS_INTERNAL int constraint_checks(bms_ctx* c, const void* const in[CONSTRAINT_INPUTS], const int64_t ld[CONSTRAINT_INPUTS], int64_t n_times, int ell_max,
                                   int mem, const void* const violations[6], int64_t ld_out, const double* norms, unsigned* reads, int* n_nodes) {
  const char* who = "bms_bondi_constraints";
  unsigned need = 0;
  bool any = norms != nullptr;
  for (int k = 0; k < N_VIOLATIONS; ++k)
    if (norms || violations[k]) need |= CONSTRAINT_READS[k], any = any || violations[k];
  if (!any) return fail(c, BMS_ERR_INVALID, "%s: every output is NULL", who);
  for (int i = 0; i < CONSTRAINT_INPUTS; ++i)
    if ((need >> i & 1) && !in[i]) return fail(c, BMS_ERR_INVALID, "%s: NULL %s, which an output asked for reads", who, CONSTRAINT_INPUT_NAME[i]);
  if (n_times < 0) return fail(c, BMS_ERR_INVALID, "%s: negative n_times", who);
  if (ell_max < 0) return fail(c, BMS_ERR_INVALID, "%s: negative ell_max", who);
  if (ell_max < 2) return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max = %d: the shear starts at ell = 2", who, ell_max);
  if (int rc = product_size_checks(c, who, 2, ell_max, -2, ell_max, ell_max, n_times, n_nodes)) return rc;
  const int64_t n_modes = LM_total_size(0, ell_max);
  uintptr_t bits = (uintptr_t)norms & 7 ? 15 : 0;  // (norms are doubles; the rest complex)
  for (int i = 0; i < CONSTRAINT_INPUTS; ++i)
    if (need >> i & 1) {
      if (ld[i] < n_modes) return fail(c, BMS_ERR_INVALID, "%s: row stride of %s smaller than the number of modes (%d)", who, CONSTRAINT_INPUT_NAME[i], (int)n_modes);
      bits |= (uintptr_t)in[i];
    }
  for (int k = 0; k < N_VIOLATIONS; ++k)
    if (violations[k]) {
      if (ld_out < n_modes) return fail(c, BMS_ERR_INVALID, "%s: row stride of the violations smaller than the (ell_max + 1)^2 = %d columns written", who, (int)n_modes);
      bits |= (uintptr_t)violations[k];
    }
  if (mem == BMS_DEVICE && (bits & 15)) return fail(c, BMS_ERR_INVALID, "%s: device arrays must be aligned to their elements", who);
  *reads = need;
  return BMS_OK;
}

extern "C" int bms_bondi_constraints(bms_ctx* c, const void* const fields[6], const int64_t ld_fields[6], const void* const psi_dot[3],
                                     const int64_t ld_psi_dot[3], const void* sigma_dot, int64_t ld_sigma_dot, const void* sigma_ddot,
                                     int64_t ld_sigma_ddot, int64_t n_times, int ell_max, int mem, void* const violations[6], int64_t ld_out,
                                     double* norms) try {
  if (!c) return BMS_ERR_INVALID;
  const char* who = "bms_bondi_constraints";
  if (int rc0 = entry_mem(c, mem, who, false)) return rc0;  // (the argument checks come before the device is selected)
  if (!fields || !ld_fields || !psi_dot || !ld_psi_dot) return fail(c, BMS_ERR_INVALID, "%s: NULL list of fields, of psi_dot or of their row strides", who);
  const void* in[CONSTRAINT_INPUTS];
  int64_t ld[CONSTRAINT_INPUTS];
  for (int i = 0; i < 6; ++i) in[i] = fields[i], ld[i] = ld_fields[i];
  for (int i = 0; i < 3; ++i) in[CONSTRAINT_PSI_DOT + i] = psi_dot[i], ld[CONSTRAINT_PSI_DOT + i] = ld_psi_dot[i];
  in[CONSTRAINT_SIGMA_DOT] = sigma_dot, ld[CONSTRAINT_SIGMA_DOT] = ld_sigma_dot;
  in[CONSTRAINT_SIGMA_DDOT] = sigma_ddot, ld[CONSTRAINT_SIGMA_DDOT] = ld_sigma_ddot;
  void* const none[N_VIOLATIONS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  void* const* home = violations ? violations : none;
  int rc, n_nodes = 0;
  unsigned reads = 0;
  if ((rc = constraint_checks(c, in, ld, n_times, ell_max, mem, home, ld_out, norms, &reads, &n_nodes))) return rc;
  if (n_times == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  ProductShape S;
  if (!product_launch_shape(ell_max, ell_max, ell_max, &S))
    return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max %d on %d rows: the rows and panels of one time step do not fit in LDS", who, ell_max, n_nodes);
  ConstraintArgs Q{};
  Q.l_max = ell_max, Q.n_nodes = n_nodes;
  // sigma's table and, for each product an output asked for needs, its operand's (spins 0, -1, -2) and its own (spins 2, 1, 0, weighted)
  const bool product[3] = {norms || home[0], norms || home[1], norms || home[2] || home[5]};
  if (product[0] || product[1] || product[2])
    if ((rc = ensure_product_table(c, 2, ell_max, n_nodes, false, &Q.tab_sigma))) return rc;
  for (int t = 0; t < 3; ++t)
    if (product[t]) {
      if ((rc = ensure_product_table(c, -t, ell_max, n_nodes, false, &Q.tab_in[t]))) return rc;
      if ((rc = ensure_product_table(c, 2 - t, ell_max, n_nodes, true, &Q.tab_out[t]))) return rc;
    }
  const int n_modes = LM_total_size(0, ell_max);
  CallIO io(c, mem);
  for (int i = 0; i < CONSTRAINT_INPUTS; ++i)
    if (reads >> i & 1) {
      char block[32];
      snprintf(block, sizeof block, "constraint_in%d", i);
      if ((rc = io.in(block, in[i], ((size_t)(n_times - 1) * ld[i] + n_modes) * 16, &Q.in[i]))) return rc;
      Q.ld[i] = ld[i];
    }
  for (int k = 0; k < N_VIOLATIONS; ++k) {
    char block[32];
    snprintf(block, sizeof block, "constraint_v%d", k);
    if ((rc = io.out_rows(block, home[k], (size_t)n_times, (size_t)2 * n_modes, (size_t)2 * ld_out, &Q.v[k]))) return rc;
  }
  if ((rc = io.out("constraint_norms", norms, (size_t)n_times * N_VIOLATIONS, &Q.norms))) return rc;
  Q.ld_out = io.host() ? n_modes : ld_out;
  TIMED(c, BMS_TAG_CONSTRAINTS, launch_bondi_constraints(c->stream, Q, n_times));
  return io.finish();
} BMS_CATCH(c)

// ---- one stage of the Bianchi identities run forwards (bianchi_kernel)
// what bms_bianchi_rhs refuses before it selects a device
BMS_INTERNAL int bianchi_checks(bms_ctx* c, int k, const void* sigma, int64_t ld_sigma, const void* a, int64_t ld_a, const void* b, int64_t ld_b,
                                int64_t n_times, int ell_max, int mem, const void* rhs, int64_t ld_rhs, const void* psi3, const void* psi4, int64_t ld_psi,
                                int* n_nodes) {
  const char* who = "bms_bianchi_rhs";
  if (k < 0 || k > 2) return fail(c, BMS_ERR_INVALID, "%s: k = %d names no stage (2: the head, then 1, then 0)", who, k);
  if (!sigma || !a || !b || !rhs) return fail(c, BMS_ERR_INVALID, "%s: NULL sigma, a, b or rhs", who);
  if (k == 2 && (!psi3 || !psi4)) return fail(c, BMS_ERR_INVALID, "%s: NULL psi3 or psi4, which the head (k = 2) writes", who);
  if (k != 2 && (psi3 || psi4)) return fail(c, BMS_ERR_INVALID, "%s: psi3 and psi4 are written by the head (k = 2) alone and must be NULL at k = %d", who, k);
  if (n_times < 0) return fail(c, BMS_ERR_INVALID, "%s: negative n_times", who);
  if (ell_max < 0) return fail(c, BMS_ERR_INVALID, "%s: negative ell_max", who);
  if (ell_max < 2) return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max = %d: the shear starts at ell = 2", who, ell_max);
  if (int rc = product_size_checks(c, who, 2, ell_max, -k, ell_max, ell_max, n_times, n_nodes)) return rc;
  const int64_t n_modes = LM_total_size(0, ell_max);
  if (ld_sigma < n_modes || ld_a < n_modes || ld_b < n_modes)
    return fail(c, BMS_ERR_INVALID, "%s: row stride of sigma, a or b smaller than the (ell_max + 1)^2 = %lld columns read", who, (long long)n_modes);
  if (ld_rhs < n_modes || (k == 2 && ld_psi < n_modes))
    return fail(c, BMS_ERR_INVALID, "%s: row stride of rhs or of psi3 and psi4 smaller than the (ell_max + 1)^2 = %lld columns written", who, (long long)n_modes);
  if (mem == BMS_DEVICE && (((uintptr_t)sigma | (uintptr_t)a | (uintptr_t)b | (uintptr_t)rhs | (uintptr_t)psi3 | (uintptr_t)psi4) & 15))
    return fail(c, BMS_ERR_INVALID, "%s: device arrays must be aligned to their elements", who);
  return BMS_OK;
}

extern "C" int bms_bianchi_rhs(bms_ctx* c, int k, const void* sigma, int64_t ld_sigma, const void* a, int64_t ld_a, const void* b, int64_t ld_b,
                               int64_t n_times, int ell_max, int mem, void* rhs, int64_t ld_rhs, void* psi3, void* psi4, int64_t ld_psi) try {
  if (!c) return BMS_ERR_INVALID;
  const char* who = "bms_bianchi_rhs";
  if (int rc0 = entry_mem(c, mem, who, false)) return rc0;  // (the argument checks come before the device is selected)
  int rc, n_nodes = 0;
  if ((rc = bianchi_checks(c, k, sigma, ld_sigma, a, ld_a, b, ld_b, n_times, ell_max, mem, rhs, ld_rhs, psi3, psi4, ld_psi, &n_nodes))) return rc;
  if (n_times == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  ProductShape S;
  if (!product_launch_shape(ell_max, ell_max, ell_max, &S))
    return fail(c, BMS_ERR_UNSUPPORTED, "%s: ell_max %d on %d rows: the rows and panels of one time step do not fit in LDS", who, ell_max, n_nodes);
  BianchiArgs Q{};
  Q.k = k, Q.l_max = ell_max, Q.n_nodes = n_nodes;
  if ((rc = ensure_product_table(c, 2, ell_max, n_nodes, false, &Q.tab_sigma))) return rc;
  if ((rc = ensure_product_table(c, -k, ell_max, n_nodes, false, &Q.tab_b))) return rc;
  if ((rc = ensure_product_table(c, 2 - k, ell_max, n_nodes, true, &Q.tab_out))) return rc;
  const int n_modes = LM_total_size(0, ell_max);
  CallIO io(c, mem);
  if ((rc = io.in("in_data", sigma, ((size_t)(n_times - 1) * ld_sigma + n_modes) * 16, &Q.sigma))) return rc;
  if ((rc = io.in("in_aux0", a, ((size_t)(n_times - 1) * ld_a + n_modes) * 16, &Q.a))) return rc;
  if ((rc = io.in("in_aux1", b, ((size_t)(n_times - 1) * ld_b + n_modes) * 16, &Q.b))) return rc;
  if ((rc = io.out_rows("bianchi_rhs", rhs, (size_t)n_times, (size_t)2 * n_modes, (size_t)2 * ld_rhs, &Q.rhs))) return rc;
  if ((rc = io.out_rows("bianchi_psi3", psi3, (size_t)n_times, (size_t)2 * n_modes, (size_t)2 * ld_psi, &Q.psi3))) return rc;
  if ((rc = io.out_rows("bianchi_psi4", psi4, (size_t)n_times, (size_t)2 * n_modes, (size_t)2 * ld_psi, &Q.psi4))) return rc;
  Q.ld_sigma = ld_sigma, Q.ld_a = ld_a, Q.ld_b = ld_b;
  Q.ld_rhs = io.host() ? n_modes : ld_rhs, Q.ld_psi = io.host() ? n_modes : ld_psi;
  TIMED(c, BMS_TAG_CONSTRAINTS, launch_bianchi_rhs(c->stream, Q, n_times));
  return io.finish();
} BMS_CATCH(c)
