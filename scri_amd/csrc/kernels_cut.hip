// A real series of modes and its conformal factor on a supertranslated cut u = alpha(theta, phi): the kernels behind
// bms_supermomentum_on_cut and bms_alpha_perturbation (scri/asymptotic_bondi_data/map_to_superrest_frame.py:108-224).
//
// The reference synthesises every row of the series on the (2L+1)^2 grid, takes the real part and fits one not-a-knot spline per
// pixel to evaluate it at that pixel's own time.  Synthesis and spline are both linear with real coefficients on the same knots,
// so they commute: the spline is solved on the MODES (the forward sweep and slopes of kernels_spline.hip / kernels_series.hip) and
// cut_kernel evaluates, per pixel, the Hermite value of every mode column at alpha_p inside the synthesis sum.  No grid of the
// window exists.  The conformal factor K_r(p) = M_r / (P0_r - P_r . r(p)) is not linear in the modes: its spline is per pixel,
// through the window's rows, with the factors of the shared matrix (SplineTable) and the forward sweep of a ring parked in LDS.
#include "kernels.h"

namespace bms {

namespace {

constexpr int CUT_WAVES = 4;  // waves of a workgroup: the mode columns k = w (mod 4) are wave w's share of the synthesis sum

// value at t = u - x_j of the cubic through (y0, s0) at x_j and (y1, s1) at x_j + h, in the form spline_hermite_eval_kernel uses
__device__ __forceinline__ double hermite_value(double y0, double y1, double s0, double s1, double h, double t) {
  const double ih = 1.0 / h;
  const double d = (y1 - y0) * ih;
  const double q = (s0 + s1 - 2.0 * d) * ih;
  const double c3 = q * ih, c2 = (d - s0) * ih - q;
  return y0 + t * (s0 + t * (c2 + t * c3));
}

// four-momentum P = -charge_vector_from_aspect(row) and rest mass of one row of modes (its four l <= 1 columns):
// out = (P0, Px, Py, Pz, M), M = sqrt(P0^2 - |P|^2) (NaN where that is negative, as the reference's sqrt)
__device__ __forceinline__ void row_four_momentum(const double2* __restrict__ row, double out[5]) {
  const double c0 = 0.28209479177387814;   // 1 / sqrt(4 pi)
  const double c1 = 0.11516471649044517;   // 1 / sqrt(6) / sqrt(4 pi)
  const double c3 = 0.16286750396763996;   // 1 / sqrt(3) / sqrt(4 pi)
  const double2 a0 = row[0], a1 = row[1], a2 = row[2], a3 = row[3];
  const double p0 = -(c0 * a0.x), px = -(c1 * a1.x - c1 * a3.x), py = -(c1 * a1.y + c1 * a3.y), pz = -(c3 * a2.x);
  out[0] = p0, out[1] = px, out[2] = py, out[3] = pz;
  out[4] = sqrt(p0 * p0 - (px * px + py * py + pz * pz));
}

__device__ __forceinline__ double conformal_factor(const double* __restrict__ P5, double rx, double ry, double rz) {
  return P5[4] / (P5[0] - (P5[1] * rx + P5[2] * ry + P5[3] * rz));
}

}  // namespace

// One workgroup per theta ring i, lane j of every wave = pixel (i, j); CUT_WAVES waves.
// LDS: lam[nm] = lambda_lm(theta_i), root[N] = e^{2 pi i j / N}, part[CUT_WAVES][64], and with K: P5[nw][5], sweep[nw][N].
__global__ __launch_bounds__(64 * CUT_WAVES) void cut_kernel(const double2* __restrict__ W, const double2* __restrict__ S, long long ldw, int nw,
                                                              const double* __restrict__ x, const SplineTable* __restrict__ table,
                                                              const double* __restrict__ lambda, const double* __restrict__ alpha,
                                                              const double2* __restrict__ d_alpha, int L, int with_k,
                                                              double* __restrict__ psi_out, double* __restrict__ k_out,
                                                              double2* __restrict__ comb_out) {
  extern __shared__ double cut_lds[];
  const int N = 2 * L + 1, nm = (L + 1) * (L + 1);
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* lam = cut_lds;
  double2* root = reinterpret_cast<double2*>(lam + nm + (nm & 1));
  double* part = reinterpret_cast<double*>(root + N);
  double* P5 = part + 64 * CUT_WAVES;
  double* sweep = P5 + 5 * (size_t)nw;
  for (int k = threadIdx.x; k < nm; k += blockDim.x) lam[k] = lambda[(long long)k * N + i];
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    double sn, cs;
    sincospi(2.0 * j / N, &sn, &cs);
    root[j] = {cs, sn};
  }
  if (with_k)
    for (int r = threadIdx.x; r < nw; r += blockDim.x) row_four_momentum(W + (long long)r * ldw, P5 + 5 * r);
  __syncthreads();

  // the lanes beyond the ring repeat pixel (i, 0) and store nothing
  const int j = lane < N ? lane : 0;
  const int p = i * N + j;
  const double u = alpha[p];
  int lo = 0, hi = nw - 1;  // last knot <= u, clamped to [0, nw - 2]: the end intervals extrapolate, as spline_hermite_eval_kernel
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (x[mid] <= u)
      lo = mid;
    else
      hi = mid;
  }
  const int jp = lo;
  const double xj = x[jp], h = x[jp + 1] - xj, t = u - xj;

  // Psi(p) = Re sum_lm lambda_lm(theta_i) e^{i m phi_j} S_lm(u): wave w adds its columns in ascending order
  {
    const double2* w0 = W + (long long)jp * ldw;
    const double2* w1 = w0 + ldw;
    const double2* s0 = S + (long long)jp * ldw;
    const double2* s1 = s0 + ldw;
    double acc = 0.0;
    int ell = 0;
    for (int k = wave; k < nm; k += CUT_WAVES) {
      while ((ell + 1) * (ell + 1) <= k) ++ell;
      const int m = k - ell * (ell + 1);
      const double2 ya = w0[k], yb = w1[k], sa = s0[k], sb = s1[k];
      const double vx = hermite_value(ya.x, yb.x, sa.x, sb.x, h, t), vy = hermite_value(ya.y, yb.y, sa.y, sb.y, h, t);
      int e = (m * j) % N;
      if (e < 0) e += N;
      const double2 ph = root[e];
      acc += lam[k] * (ph.x * vx - ph.y * vy);
    }
    part[wave * 64 + lane] = acc;
  }
  __syncthreads();
  if (wave != 0) return;
  double psi = part[lane];
#pragma unroll
  for (int w = 1; w < CUT_WAVES; ++w) psi += part[w * 64 + lane];

  double K = 1.0;
  if (with_k) {
    double st, ct;
    sincospi((double)i / (N - 1), &st, &ct);
    const double2 ph = root[j];
    const double rx = st * ph.x, ry = -(st * ph.y), rz = ct;  // (4 pi times the charge vector of the unit-mode grids: its y carries the sign of Im(a_1-1 + a_11))
    auto kr = [&](int r) { return conformal_factor(P5 + 5 * r, rx, ry, rz); };
    double* sw = sweep + lane;  // sw[r * N]: this lane's r'_r (lanes beyond the ring are masked below)
    if (lane < N) {
      // forward sweep of the shared system over the whole window (kernels_spline.hip, spline_forward_kernel)
      double ym = kr(0), y0 = kr(1), y1 = kr(2);
      SplineTable e = table[0];
      double rp = e.P * (y0 - ym) + e.Q * (y1 - y0);
      sw[0] = rp;
      for (int r = 1; r < nw - 1; ++r) {
        e = table[r];
        rp = e.P * (y0 - ym) + e.Q * (y1 - y0) - e.A * rp;
        sw[(size_t)r * N] = rp;
        if (r + 2 < nw) ym = y0, y0 = y1, y1 = kr(r + 2);
      }
      // last row: D_{n-3} and D_{n-2} (ym, y0, y1 still hold rows nw - 3 .. nw - 1)
      e = table[nw - 1];
      rp = e.P * (y0 - ym) + e.Q * (y1 - y0) - e.A * rp;
      // back substitution down to the pixel's interval
      double s_hi = rp, s_lo = rp;
      for (int r = nw - 2; r >= jp; --r) {
        s_hi = s_lo;
        s_lo = sw[(size_t)r * N] - table[r].C * s_hi;
      }
      K = hermite_value(kr(jp), kr(jp + 1), s_lo, s_hi, h, t);
    }
  }
  if (lane >= N) return;
  if (psi_out) psi_out[p] = psi;
  if (k_out) k_out[p] = K;
  if (comb_out) {
    const double2 d = d_alpha[p];
    const double k3 = K * K * K;
    comb_out[p] = {(psi - d.x) / k3, (0.0 - d.y) / k3};
  }
}

size_t cut_lds_bytes(int ell_max, long long n_window, int with_k) {
  const size_t N = 2 * (size_t)ell_max + 1, nm = ((size_t)ell_max + 1) * (ell_max + 1);
  size_t doubles = nm + (nm & 1) + 2 * N + 64 * CUT_WAVES;
  if (with_k) doubles += 5 * (size_t)n_window + (size_t)n_window * N;
  return 8 * doubles;
}

hipError_t launch_cut(hipStream_t stream, const double* W, const double* S, long long ldw, long long n_window, const double* x,
                      const SplineTable* table, const double* lambda, const double* alpha, const double* d_alpha, int ell_max, int with_k,
                      double* psi_out, double* k_out, double* comb_out) {
  const int N = 2 * ell_max + 1;
  if (ell_max < 1 || N > 64 || n_window < 4 || n_window > 0x7fffffff || (comb_out && !d_alpha)) return hipErrorInvalidValue;
  const size_t lds = cut_lds_bytes(ell_max, n_window, with_k);
  if (lds > 64 * 1024) {
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(cut_kernel));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(cut_kernel, dim3(N), dim3(64 * CUT_WAVES), lds, stream, reinterpret_cast<const double2*>(W),
                     reinterpret_cast<const double2*>(S), ldw, (int)n_window, x, table, lambda, alpha,
                     reinterpret_cast<const double2*>(d_alpha), ell_max, with_k, psi_out, k_out, reinterpret_cast<double2*>(comb_out));
  return hipGetLastError();
}

// ---- the small pointwise steps around it: all of (2L+1)^2 pixels or (L+1)^2 modes
// op 0: grid c16[n] = (real f8[n], 0);  op 1: real f8[n] = Re grid c16[n]
__global__ __launch_bounds__(256) void cut_real_complex_kernel(const double* __restrict__ in, double* __restrict__ out, int n, int op) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  if (op == 0)
    reinterpret_cast<double2*>(out)[p] = {in[p], 0.0};
  else
    out[p] = in[2 * p];
}

// modes c16[(L+1)^2] times D_l = (l+2)(l+1)l(l-1)/4 (inverse: 4 / ((l+2)(l+1)l(l-1))), zero below l = 2
__global__ __launch_bounds__(256) void cut_scale_modes_kernel(double2* __restrict__ modes, int L, int inverse) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (L + 1) * (L + 1)) return;
  int ell = 0;
  while ((ell + 1) * (ell + 1) <= k) ++ell;
  const double prod = (double)(ell + 2) * (ell + 1) * ell * (ell - 1);
  const double f = ell < 2 ? 0.0 : (inverse ? 4.0 / prod : prod / 4.0);
  const double2 a = modes[k];
  modes[k] = {a.x * f, a.y * f};
}

// grid[p] += M(p) K(p)^3 on the real part.  m_grid / k_grid: f8 per pixel, or null: the rest mass and the conformal factor of `modes`
__global__ __launch_bounds__(256) void cut_mass_term_kernel(double2* __restrict__ grid, const double2* __restrict__ modes,
                                                            const double* __restrict__ m_grid, const double* __restrict__ k_grid, int L) {
  const int N = 2 * L + 1;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= N * N) return;
  double P5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (!m_grid || !k_grid) row_four_momentum(modes, P5);
  double K;
  if (k_grid) {
    K = k_grid[p];
  } else {
    const int i = p / N, j = p % N;
    double st, ct, sp, cp;
    sincospi((double)i / (N - 1), &st, &ct);
    sincospi(2.0 * j / N, &sp, &cp);
    K = conformal_factor(P5, st * cp, -(st * sp), ct);
  }
  const double M = m_grid ? m_grid[p] : P5[4];
  grid[p].x += M * (K * K * K);
}

hipError_t launch_cut_real_to_complex(hipStream_t stream, const double* in, double* out, int n) {
  hipLaunchKernelGGL(cut_real_complex_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, in, out, n, 0);
  return hipGetLastError();
}
hipError_t launch_cut_real_part(hipStream_t stream, const double* in, double* out, int n) {
  hipLaunchKernelGGL(cut_real_complex_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, in, out, n, 1);
  return hipGetLastError();
}
hipError_t launch_cut_scale_modes(hipStream_t stream, double* modes, int ell_max, int inverse) {
  const int nm = (ell_max + 1) * (ell_max + 1);
  hipLaunchKernelGGL(cut_scale_modes_kernel, dim3((nm + 255) / 256), dim3(256), 0, stream, reinterpret_cast<double2*>(modes), ell_max, inverse);
  return hipGetLastError();
}
hipError_t launch_cut_mass_term(hipStream_t stream, double* grid, const double* modes, const double* m_grid, const double* k_grid, int ell_max) {
  const int n = (2 * ell_max + 1) * (2 * ell_max + 1);
  hipLaunchKernelGGL(cut_mass_term_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, reinterpret_cast<double2*>(grid),
                     reinterpret_cast<const double2*>(modes), m_grid, k_grid, ell_max);
  return hipGetLastError();
}

}  // namespace bms
