// Extrapolation of finite-radius waveforms to null infinity: the per-time-step least-squares fit of scri/extrapolation.py:1394-1434,
//     extrapolated[N][t][m] = polyfit(1 / r_i(t), y_i[t][m], N)[0]      (numpy.polynomial.polynomial.polyfit, i = 0 .. n_radii - 1)
// for every order N of a list, in one pass over the data.
//
// The fit (numpy/polynomial/polyutils.py `_fit`): Vandermonde columns x^k (k = 0 .. N, x = 1 / r), each scaled by its 2-norm,
// least squares on the scaled matrix A, the coefficients divided by the scales.  The column norms do not depend on N, so the
// Householder QR of the scaled n_radii x (N_max + 1) matrix, built column by column, holds the QR of every lower order as its leading
// block: A[:, :N+1] = Q R[:N+1, :N+1].  The constant term is a LINEAR functional of the data, the same for every mode of the step:
//     c_0 = e_0^T R_N^-1 (Q^T y)[:N+1] / s_0 = g_N^T y,      g_N = H_0 H_1 ... H_N [u_N; 0] / s_0,   R_N^T u_N = e_0,
// and u_N is the leading part of ONE forward substitution (R^T is lower triangular).  So a step costs one factorisation and one
// reflector sweep per order on n_radii numbers, and every mode then costs one dot product of length n_radii per order: each input
// value is read once and serves all orders.
//
// One workgroup takes EXTRAP_TILE consecutive time steps.  Phase 1: each wavefront factors steps of the tile, lane = radius (the
// reductions are butterflies, whose result is the same to the bit in every lane), and leaves g_N of each order in the LDS.  Phase 2:
// the threads walk (step, mode) pairs of the tile -- a row of modes is read coalesced -- and accumulate all orders at once.  The
// arithmetic of a (step, mode) pair depends on neither the tile nor the launch, so any split of the time axis gives the same bits.
//
// Rank deficiency: numpy's lstsq drops singular values below rcond = n_radii * eps of the largest (and warns).  Here an order whose
// leading diagonal of R has min |R_kk| <= n_radii * eps * max |R_kk|, or an entry that is not finite (a radius of 0, infinity or
// NaN), gets NaN weights -- so NaN outputs -- and the step is counted in deficient[order].
//
// Where the time goes (24 radii, 77 modes, orders [2, 3, 4], 1e5 steps): split into a weights kernel (one wavefront per step) and a
// streaming kernel, the factorisations took about 0.5 ms and the dot products 0.65 ms (5.1 TB/s); fused, the two overlap in part
// and the whole takes 1.09 ms, so the fused form is kept.  The factorisations are bound by the latency of the cross-lane
// reductions (butterflies of __shfl_xor), not by memory.
#include "kernels.h"

namespace bms {

constexpr int EXTRAP_TILE = 16;
constexpr int EXTRAP_THREADS = 256;
constexpr int EXTRAP_ORDERS_PER_LAUNCH = 8;

struct ExtrapOrders {
  int n;
  int N[EXTRAP_ORDERS_PER_LAUNCH];
};

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Phase 1 for time step t of a wavefront: g[o][i] (o < ord.n, i < R) in the LDS
template <int KM>
__device__ inline void extrapolation_weights(const double* __restrict__ radii, long long r_ld, long long t, int R, int K,
                                             const ExtrapOrders& ord, double* g, unsigned long long* __restrict__ deficient) {
  const int lane = threadIdx.x & 63;
  const bool on = lane < R;
  const double x = on ? 1.0 / radii[(long long)lane * r_ld + t] : 0.0;
  // row `lane` of the Vandermonde matrix (polyvander: v_k = v_{k-1} x), scaled by the column norms
  double a[KM], scl[KM];
  double p = on ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    a[k] = p;
    p *= x;
  }
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    if (k < K) {
      double s = sqrt(wave_sum(a[k] * a[k]));
      if (s == 0.0) s = 1.0;
      scl[k] = s;
      a[k] /= s;
    }
  }
  // Householder QR (LAPACK dgeqr2 conventions): reflector j is I - tau_j v_j v_j^T, v_j[j] = 1; this lane keeps its component of v_j
  double v[KM], tau[KM], diag[KM];
#pragma unroll
  for (int j = 0; j < KM; ++j) {
    if (j < K) {
      const double alpha = __shfl(a[j], j, 64);
      const double below = lane > j ? a[j] : 0.0;
      const double xn2 = wave_sum(below * below);
      const double beta = xn2 == 0.0 ? alpha : -copysign(sqrt(alpha * alpha + xn2), alpha);
      tau[j] = xn2 == 0.0 ? 0.0 : (beta - alpha) / beta;
      const double scale = xn2 == 0.0 ? 0.0 : 1.0 / (alpha - beta);
      v[j] = lane == j ? 1.0 : below * scale;
      diag[j] = beta;
#pragma unroll
      for (int col = j + 1; col < KM; ++col) {
        if (col < K) {
          const double w = wave_sum(v[j] * a[col]);
          a[col] -= tau[j] * w * v[j];
        }
      }
    }
  }
  // R^T u = e_0 (row j of R: a[k] of lane j, k > j), redundantly in every lane
  double u[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    if (k < K) {
      double s = k == 0 ? 1.0 : 0.0;
#pragma unroll
      for (int j = 0; j < k; ++j) s -= __shfl(a[k], j, 64) * u[j];
      u[k] = s / diag[k];
    }
  }
  const double rcond = R * 2.220446049250313e-16;
#pragma unroll
  for (int o = 0; o < EXTRAP_ORDERS_PER_LAUNCH; ++o) {
    if (o < ord.n) {
      const int N = ord.N[o];
      double dmin = INFINITY, dmax = 0.0, z = 0.0;
      bool finite = true;  // (fmin / fmax pass NaN over: a diagonal of NaN -- a radius of 0 or NaN -- is caught here)
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        if (k <= N) {
          finite = finite && isfinite(diag[k]);
          dmin = fmin(dmin, fabs(diag[k]));
          dmax = fmax(dmax, fabs(diag[k]));
          if (lane == k) z = u[k];
        }
      }
      // H_0 ... H_N [u_N; 0]: the reflectors beyond N leave a vector with no component past N alone
#pragma unroll
      for (int j = KM - 1; j >= 0; --j) {
        if (j <= N) {
          const double w = wave_sum(v[j] * z);
          z -= tau[j] * w * v[j];
        }
      }
      const bool bad = !finite || !(dmin > rcond * dmax);
      if (on) g[o * R + lane] = bad ? NAN : z / scl[0];
      if (bad && lane == 0) atomicAdd(deficient + o, 1ull);
    }
  }
}

template <int KM>
__global__ __launch_bounds__(EXTRAP_THREADS) void extrapolate_kernel(const ExtrapSource* __restrict__ src, int R,
                                                                   const double* __restrict__ radii, long long r_ld,
                                                                   long long n_times, int n_modes, int K, ExtrapOrders ord,
                                                                   double2* __restrict__ out, long long out_order_stride,
                                                                   unsigned long long* __restrict__ deficient) {
  extern __shared__ double g_lds[];  // [EXTRAP_TILE][ord.n][R]
  const long long t0 = (long long)blockIdx.x * EXTRAP_TILE;
  const int rows = (int)min((long long)EXTRAP_TILE, n_times - t0);
  const int wave = threadIdx.x >> 6, n_waves = EXTRAP_THREADS / 64;
  for (int tl = wave; tl < rows; tl += n_waves)
    extrapolation_weights<KM>(radii, r_ld, t0 + tl, R, K, ord, g_lds + (size_t)tl * ord.n * R, deficient);
  __syncthreads();
  const int items = rows * n_modes;
  for (int item = threadIdx.x; item < items; item += EXTRAP_THREADS) {
    const int tl = item / n_modes, m = item - tl * n_modes;
    const long long t = t0 + tl;
    const double* gw = g_lds + (size_t)tl * ord.n * R;
    double re[EXTRAP_ORDERS_PER_LAUNCH], im[EXTRAP_ORDERS_PER_LAUNCH];
#pragma unroll
    for (int o = 0; o < EXTRAP_ORDERS_PER_LAUNCH; ++o) re[o] = im[o] = 0.0;
#pragma unroll 4
    for (int i = 0; i < R; ++i) {
      const double2 y = src[i].p[t * src[i].ld + m];
#pragma unroll
      for (int o = 0; o < EXTRAP_ORDERS_PER_LAUNCH; ++o) {
        if (o < ord.n) {
          const double w = gw[o * R + i];
          re[o] += w * y.x;
          im[o] += w * y.y;
        }
      }
    }
#pragma unroll
    for (int o = 0; o < EXTRAP_ORDERS_PER_LAUNCH; ++o)
      if (o < ord.n) out[o * out_order_stride + t * n_modes + m] = make_double2(re[o], im[o]);
  }
}

template <int KM>
static hipError_t launch_extrapolate_km(hipStream_t stream, const ExtrapSource* src, int R, const double* radii, long long r_ld,
                                        long long n_times, int n_modes, int K, const ExtrapOrders& ord, double2* out,
                                        long long out_order_stride, unsigned long long* deficient) {
  const size_t lds = sizeof(double) * EXTRAP_TILE * ord.n * R;
  const long long n_blocks = (n_times + EXTRAP_TILE - 1) / EXTRAP_TILE;
  hipLaunchKernelGGL(extrapolate_kernel<KM>, dim3((unsigned)n_blocks), dim3(EXTRAP_THREADS), lds, stream, src, R, radii, r_ld, n_times,
                     n_modes, K, ord, out, out_order_stride, deficient);
  return hipGetLastError();
}

hipError_t launch_extrapolate(hipStream_t stream, const ExtrapSource* src, int n_radii, const double* radii, long long r_ld,
                              long long n_times, int n_modes, const int* orders, int n_orders, double2* out, long long out_order_stride,
                              unsigned long long* deficient) {
  if (n_times <= 0 || n_modes <= 0 || n_orders <= 0) return hipSuccess;
  if (n_radii < 1 || n_radii > EXTRAP_MAX_RADII || (n_times + EXTRAP_TILE - 1) / EXTRAP_TILE > 0x7fffffffLL) return hipErrorInvalidValue;
  // groups of up to EXTRAP_ORDERS_PER_LAUNCH orders; each group factors up to its own largest order (the leading blocks, and so the
  // results, do not depend on the grouping)
  for (int o0 = 0; o0 < n_orders; o0 += EXTRAP_ORDERS_PER_LAUNCH) {
    ExtrapOrders ord{};
    ord.n = std::min(EXTRAP_ORDERS_PER_LAUNCH, n_orders - o0);
    int K = 1;
    for (int o = 0; o < ord.n; ++o) {
      ord.N[o] = orders[o0 + o];
      if (ord.N[o] < 0 || ord.N[o] > EXTRAP_MAX_ORDER || ord.N[o] >= n_radii) return hipErrorInvalidValue;
      K = std::max(K, ord.N[o] + 1);
    }
    double2* o_out = out + o0 * out_order_stride;
    unsigned long long* o_def = deficient + o0;
    hipError_t e = K <= 4   ? launch_extrapolate_km<4>(stream, src, n_radii, radii, r_ld, n_times, n_modes, K, ord, o_out, out_order_stride, o_def)
                   : K <= 8 ? launch_extrapolate_km<8>(stream, src, n_radii, radii, r_ld, n_times, n_modes, K, ord, o_out, out_order_stride, o_def)
                            : launch_extrapolate_km<16>(stream, src, n_radii, radii, r_ld, n_times, n_modes, K, ord, o_out, out_order_stride, o_def);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace bms
