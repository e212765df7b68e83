// Centre-of-mass drift of the horizon (or star) trajectories: scri/SpEC/com_motion.py.
//
// com_track_kernel   CoM = (m_A x_A + m_B x_B) / (m_A + m_B), and with matter t / m and CoM / m (:59-60, :112-118): numpy's rounding
//                    steps in numpy's order, no contraction, so the track equals the numpy expression bit for bit.
// com_window_kernel  t_i, t_f from the two skip fractions (:206) and, per workgroup, the first index of the minimum of |t - t_i| and
//                    of |t - t_f| (numpy's argmin: the lowest index wins a tie, a NaN counts as the minimum).
// com_moments_kernel the composite Simpson rule of scipy.integrate.simpson(y, x) on the irregular axis, over samples i_i .. i_f, for
//                    the integrands com, fl(t com) and fl(fl(t t) com) (:210-213: fp64 products, inputs of the rule).  One thread per
//                    panel (two intervals): weights, products and sums in double-double (dd.h), the nine (six) sums of a thread reduced
//                    over the wavefront and then over the workgroup, one partial per tile of COM_FIT_TILE panels.
// com_fit_kernel     adds the partials in a fixed order, the correction of the last interval for an even number of samples (or the
//                    trapezoid for two), and evaluates the closed-form minimiser of the integrated squared distance from the origin
//                    in double-double; one rounding to fp64 at the end.
// The answer depends on the input alone: the tiles are a constant, the order of every sum is fixed, and the argmin does not depend on
// an order at all.  Divisions of the rule are guarded as scipy's are: a zero divisor gives a zero quotient (a repeated time).
#include "kernels.h"
#include "dd.h"

#pragma clang fp contract(off)

namespace bms {

namespace {

constexpr int CT = COM_FIT_TILE;
static_assert(CT == 256, "one panel per thread of a 256-thread workgroup");
constexpr int COM_WINDOW_BLOCKS_MAX = 1024;

struct ArgMin {
  double key;  // |t - target|, -1 for a NaN (numpy's argmin returns the first NaN)
  long long idx;
};
__device__ __forceinline__ ArgMin arg_better(ArgMin a, ArgMin b) { return (b.key < a.key || (b.key == a.key && b.idx < a.idx)) ? b : a; }
__device__ __forceinline__ double arg_key(double v) { return v != v ? -1.0 : v; }

// minimum over the workgroup (256 threads), known to every thread; lds[4]
__device__ __forceinline__ ArgMin block_argmin(ArgMin v, ArgMin* lds) {
  for (int o = 32; o; o >>= 1) {
    ArgMin w;
    w.key = __shfl_down(v.key, o);
    w.idx = __shfl_down(v.idx, o);
    v = arg_better(v, w);
  }
  __syncthreads();  // (the previous use of lds has been read)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  v = lds[0];
  for (int w = 1; w < 4; ++w) v = arg_better(v, lds[w]);
  return v;
}

struct ComWindow {
  double t_i, t_f;
  long long i_i, i_f;
};
__device__ __forceinline__ void com_window_times(const double* __restrict__ t, long long n, double skip_b, double skip_e, double& t_i, double& t_f) {
  const double t0 = t[0], t1 = t[n - 1], span = t1 - t0;
  t_i = t0 + span * skip_b;
  t_f = t1 - span * skip_e;
}

// sum of three weighted samples onto a double-double accumulator
__device__ __forceinline__ dd panel_sum(dd acc, dd w0, dd w1, dd w2, double y0, double y1, double y2) {
  acc = dd_add(acc, dd_mul_d(w0, y0));
  acc = dd_add(acc, dd_mul_d(w1, y1));
  return dd_add(acc, dd_mul_d(w2, y2));
}
__device__ __forceinline__ dd dd_div_guarded(dd a, dd b) { return b.hi == 0.0 ? dd{0.0, 0.0} : dd_div(a, b); }
__device__ __forceinline__ dd dd_shfl_down(dd a, int o) { return {__shfl_down(a.hi, o), __shfl_down(a.lo, o)}; }

}  // namespace

__global__ __launch_bounds__(256) void com_track_kernel(const double* __restrict__ t, const double* __restrict__ xa, const double* __restrict__ xb,
                                                        const double* __restrict__ ma, long long n_ma, const double* __restrict__ mb,
                                                        long long n_mb, long long n, int matter, double* __restrict__ t_out,
                                                        double* __restrict__ com_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double a = ma[n_ma > 1 ? i : 0], b = mb[n_mb > 1 ? i : 0];
  const double m = a + b;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double c = (a * xa[3 * i + k] + b * xb[3 * i + k]) / m;
    if (matter) c = c / m;
    com_out[3 * i + k] = c;
  }
  if (matter) t_out[i] = t[i] / m;
}

// partial[block] = {key_i, idx_i, key_f, idx_f} (indices stored as doubles' bit patterns of long long)
__global__ __launch_bounds__(256) void com_window_kernel(const double* __restrict__ t, long long n, double skip_b, double skip_e,
                                                         ArgMin* __restrict__ partial) {
  __shared__ ArgMin lds[4];
  double t_i, t_f;
  com_window_times(t, n, skip_b, skip_e, t_i, t_f);
  ArgMin bi = {INFINITY, 0x7fffffffffffffffLL}, bf = bi;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = t[i];
    bi = arg_better(bi, ArgMin{arg_key(fabs(x - t_i)), i});
    bf = arg_better(bf, ArgMin{arg_key(fabs(x - t_f)), i});
  }
  bi = block_argmin(bi, lds);
  bf = block_argmin(bf, lds);
  if (threadIdx.x == 0) partial[2 * blockIdx.x] = bi, partial[2 * blockIdx.x + 1] = bf;
}

// window[4] (written by workgroup 0): t_i, t_f and i_i, i_f as doubles; partial[tile][3 NM] double-double
template <int NM>
__global__ __launch_bounds__(256) void com_moments_kernel(const double* __restrict__ t, const double* __restrict__ com, long long n, double skip_b,
                                                          double skip_e, const ArgMin* __restrict__ win_partial, int n_win,
                                                          double* __restrict__ window, dd* __restrict__ partial) {
  __shared__ ArgMin lds[4];
  __shared__ double ts[2 * CT + 1];
  __shared__ double cs[3 * (2 * CT + 1)];
  __shared__ dd red[4][3 * NM];
  const int tid = threadIdx.x;
  // every workgroup finds the window for itself from the (at most 1024) partial minima
  ArgMin bi = {INFINITY, 0x7fffffffffffffffLL}, bf = bi;
  for (int e = tid; e < n_win; e += 256) bi = arg_better(bi, win_partial[2 * e]), bf = arg_better(bf, win_partial[2 * e + 1]);
  bi = block_argmin(bi, lds);
  bf = block_argmin(bf, lds);
  const long long i_i = bi.idx, i_f = bf.idx;
  if (blockIdx.x == 0 && tid == 0) {
    double t_i, t_f;
    com_window_times(t, n, skip_b, skip_e, t_i, t_f);
    window[0] = t_i, window[1] = t_f, window[2] = (double)i_i, window[3] = (double)i_f;
  }
  const long long N = i_f - i_i + 1;
  const long long n_panels = N >= 3 ? (N - 1) / 2 : 0;  // an even count leaves its last interval to com_fit_kernel
  const long long p0 = (long long)blockIdx.x * CT;
  if (p0 >= n_panels) return;
  const int np = (int)(n_panels - p0 < CT ? n_panels - p0 : CT);
  const long long s0 = i_i + 2 * p0;  // samples s0 .. s0 + 2 np <= i_f
  const int ns = 2 * np + 1;
  for (int e = tid; e < ns; e += 256) ts[e] = t[s0 + e];
  for (int e = tid; e < 3 * ns; e += 256) cs[e] = com[3 * s0 + e];
  __syncthreads();

  dd acc[3 * NM];
#pragma unroll
  for (int j = 0; j < 3 * NM; ++j) acc[j] = {0.0, 0.0};
  if (tid < np) {
    const double t0 = ts[2 * tid], t1 = ts[2 * tid + 1], t2 = ts[2 * tid + 2];
    const dd h0 = two_sum(t1, -t0), h1 = two_sum(t2, -t1);  // exact
    const dd hsum = dd_add(h0, h1), hs6 = dd_div(hsum, dd{6.0, 0.0});
    const bool flat = h0.hi == 0.0 || h1.hi == 0.0;
    const dd zero = {0.0, 0.0}, two = {2.0, 0.0};
    const dd r01 = dd_div_guarded(h0, h1);                   // h0 / h1
    const dd r10 = flat ? zero : dd_div(h1, h0);             // 1 / (h0 / h1), zero where h0 / h1 is
    const dd q = flat ? zero : dd_div(hsum, dd_mul(h0, h1));  // hsum / (h0 h1)
    const dd w0 = dd_mul(hs6, dd_sub(two, r10)), w1 = dd_mul(hs6, dd_mul(hsum, q)), w2 = dd_mul(hs6, dd_sub(two, r01));
    const double tt0 = t0 * t0, tt1 = t1 * t1, tt2 = t2 * t2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double y0 = cs[6 * tid + k], y1 = cs[6 * tid + 3 + k], y2 = cs[6 * tid + 6 + k];
      acc[k] = panel_sum(acc[k], w0, w1, w2, y0, y1, y2);
      acc[3 + k] = panel_sum(acc[3 + k], w0, w1, w2, t0 * y0, t1 * y1, t2 * y2);
      if (NM == 3) acc[6 + k] = panel_sum(acc[6 + k], w0, w1, w2, tt0 * y0, tt1 * y1, tt2 * y2);
    }
  }
  // over the wavefront, then over the workgroup: always the same tree
#pragma unroll
  for (int j = 0; j < 3 * NM; ++j)
    for (int o = 32; o; o >>= 1) acc[j] = dd_add(acc[j], dd_shfl_down(acc[j], o));
  if ((tid & 63) == 0)
#pragma unroll
    for (int j = 0; j < 3 * NM; ++j) red[tid >> 6][j] = acc[j];
  __syncthreads();
  if (tid < 3 * NM) {
    dd s = red[0][tid];
    for (int w = 1; w < 4; ++w) s = dd_add(s, red[w][tid]);
    partial[(long long)blockIdx.x * (3 * NM) + tid] = s;
  }
}

// out[COM_FIT_OUT]: x_i[3], v_i[3], a_i[3], t_i, t_f, i_i, i_f, moments[3][3], status (0 fine, 1 window of fewer than two samples,
// 2 t_f == t_i).  One wavefront.
template <int NM>
__global__ __launch_bounds__(64) void com_fit_kernel(const double* __restrict__ t, const double* __restrict__ com, const double* __restrict__ window,
                                                     const dd* __restrict__ partial, double* __restrict__ out) {
  const int lane = threadIdx.x;
  const double t_i = window[0], t_f = window[1];
  const long long i_i = (long long)window[2], i_f = (long long)window[3];
  const long long N = i_f - i_i + 1;
  const long long n_panels = N >= 3 ? (N - 1) / 2 : 0, n_tiles = (n_panels + CT - 1) / CT;
  dd M[3 * NM];
#pragma unroll
  for (int j = 0; j < 3 * NM; ++j) {
    dd s = {0.0, 0.0};
    if (N >= 2)
      for (long long b = lane; b < n_tiles; b += 64) s = dd_add(s, partial[b * (3 * NM) + j]);
    for (int o = 32; o; o >>= 1) s = dd_add(s, dd_shfl_down(s, o));
    M[j] = s;
  }
  if (lane != 0) return;
  for (int j = 0; j < COM_FIT_OUT; ++j) out[j] = 0.0;
  out[9] = t_i, out[10] = t_f, out[11] = (double)i_i, out[12] = (double)i_f;
  if (t_f == t_i) {
    out[22] = 2.0;
    return;
  }
  if (N < 2) {
    out[22] = 1.0;
    return;
  }
  if (N % 2 == 0) {  // the last interval: the trapezoid for two samples, else the correction from the last three
    const double tb = t[i_f - 1], tc = t[i_f];
    const dd h1 = two_sum(tc, -tb);
    dd wa, wb, wc = {0.0, 0.0};  // weights of samples i_f, i_f - 1, i_f - 2
    double ta = 0.0;
    if (N == 2) {
      wa = wb = dd_mul_d(h1, 0.5);
    } else {
      ta = t[i_f - 2];
      const dd h0 = two_sum(tb, -ta), hsum = dd_add(h0, h1), h01 = dd_mul(h0, h1), h11 = dd_mul(h1, h1);
      wa = dd_div_guarded(dd_add(dd_mul_d(h11, 2.0), dd_mul_d(h01, 3.0)), dd_mul_d(hsum, 6.0));
      wb = dd_div_guarded(dd_add(h11, dd_mul_d(h01, 3.0)), dd_mul_d(h0, 6.0));
      wc = dd_neg(dd_div_guarded(dd_mul(h11, h1), dd_mul_d(dd_mul(h0, hsum), 6.0)));
    }
    for (int k = 0; k < 3; ++k) {
      const double ya = com[3 * i_f + k], yb = com[3 * (i_f - 1) + k], yc = N == 2 ? 0.0 : com[3 * (i_f - 2) + k];
      M[k] = panel_sum(M[k], wa, wb, wc, ya, yb, yc);
      M[3 + k] = panel_sum(M[3 + k], wa, wb, wc, tc * ya, tb * yb, ta * yc);
      if (NM == 3) M[6 + k] = panel_sum(M[6 + k], wa, wb, wc, (tc * tc) * ya, (tb * tb) * yb, (ta * ta) * yc);
    }
  }
  // the minimiser of int |CoM - x - v t (- a t^2 / 2)|^2 dt over [t_i, t_f] from the moments C_k = int t^k CoM dt, with a = t_i, b = t_f:
  //   without acceleration   x = 2 [C0 (2 b^3 - 2 a^3) + C1 (3 a^2 - 3 b^2)] / (b - a)^4,   v = 6 [2 C1 - C0 (a + b)] / (b - a)^3
  //   with it                x = 3 [C0 (3 b^4 + 12 b^3 a + 30 b^2 a^2 + 12 b a^3 + 3 a^4) - 12 C1 (a + b) (b^2 + 3 a b + a^2)
  //                                 + C2 (10 b^2 + 40 a b + 10 a^2)] / (b - a)^5
  //                          v = 12 [-3 C0 (a + b) (b^2 + 3 a b + a^2) + C1 (16 b^2 + 28 a b + 16 a^2) - 15 C2 (a + b)] / (b - a)^5
  //                          acc = 60 [C0 (b^2 + 4 a b + a^2) - 6 C1 (a + b) + 6 C2] / (b - a)^5
  const dd a = dd_from(t_i), b = dd_from(t_f), d = two_sum(t_f, -t_i);
  const dd a2 = dd_mul(a, a), b2 = dd_mul(b, b), ab = dd_mul(a, b), s = dd_add(a, b);
  dd cx[3], cv[3], ca[3], den;
  if (NM == 2) {
    const dd a3 = dd_mul(a2, a), b3 = dd_mul(b2, b);
    cx[0] = dd_mul_d(dd_sub(b3, a3), 4.0), cx[1] = dd_mul_d(dd_sub(a2, b2), 6.0), cx[2] = {0.0, 0.0};
    cv[0] = dd_mul_d(s, -6.0), cv[1] = {12.0, 0.0}, cv[2] = {0.0, 0.0};
    ca[0] = ca[1] = ca[2] = {0.0, 0.0};
    den = dd_ipow(d, 3);
  } else {
    const dd quad = dd_add(dd_add(b2, dd_mul_d(ab, 3.0)), a2);  // b^2 + 3 a b + a^2
    const dd sq = dd_mul(s, quad);
    const dd p4 = dd_add(dd_add(dd_mul_d(dd_add(dd_mul(b2, b2), dd_mul(a2, a2)), 3.0), dd_mul_d(dd_mul(ab, dd_add(a2, b2)), 12.0)),
                         dd_mul_d(dd_mul(ab, ab), 30.0));
    cx[0] = dd_mul_d(p4, 3.0), cx[1] = dd_mul_d(sq, -36.0), cx[2] = dd_mul_d(dd_add(dd_add(b2, dd_mul_d(ab, 4.0)), a2), 30.0);
    cv[0] = dd_mul_d(sq, -36.0), cv[1] = dd_mul_d(dd_add(dd_mul_d(dd_add(a2, b2), 16.0), dd_mul_d(ab, 28.0)), 12.0), cv[2] = dd_mul_d(s, -180.0);
    ca[0] = dd_mul_d(dd_add(dd_add(b2, dd_mul_d(ab, 4.0)), a2), 60.0), ca[1] = dd_mul_d(s, -360.0), ca[2] = {360.0, 0.0};
    den = dd_ipow(d, 5);
  }
  for (int k = 0; k < 3; ++k) {
    dd x = {0.0, 0.0}, v = x, g = x;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      x = dd_add(x, dd_mul(cx[m], M[3 * m + k]));
      v = dd_add(v, dd_mul(cv[m], M[3 * m + k]));
      if (NM == 3) g = dd_add(g, dd_mul(ca[m], M[3 * m + k]));
    }
    out[k] = dd_to_double(dd_div(x, NM == 2 ? dd_mul(den, d) : den));
    out[3 + k] = dd_to_double(dd_div(v, den));
    out[6 + k] = NM == 3 ? dd_to_double(dd_div(g, den)) : 0.0;
#pragma unroll
    for (int m = 0; m < NM; ++m) out[13 + 3 * m + k] = dd_to_double(M[3 * m + k]);
  }
}

hipError_t launch_com_track(hipStream_t stream, const double* t, const double* xa, const double* xb, const double* ma, long long n_ma,
                            const double* mb, long long n_mb, long long n, int matter, double* t_out, double* com_out) {
  if (n <= 0) return hipSuccess;
  const long long blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(com_track_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, t, xa, xb, ma, n_ma, mb, n_mb, n, matter, t_out, com_out);
  return hipGetLastError();
}

long long com_fit_tiles(long long n) { return n >= 3 ? ((n - 1) / 2 + CT - 1) / CT : 1; }
// work space in doubles: window minima of the workgroups, the window, the tiles' double-double partials
long long com_fit_work_doubles(long long n) { return 4LL * COM_WINDOW_BLOCKS_MAX + 4 + 18 * com_fit_tiles(n); }

hipError_t launch_com_fit(hipStream_t stream, const double* t, const double* com, long long n, double skip_b, double skip_e, int accel,
                          double* work, double* out) {
  if (n < 2) return hipErrorInvalidValue;
  const long long tiles = com_fit_tiles(n);
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  ArgMin* win_partial = reinterpret_cast<ArgMin*>(work);
  double* window = work + 4LL * COM_WINDOW_BLOCKS_MAX;
  dd* partial = reinterpret_cast<dd*>(window + 4);
  const int n_win = (int)std::min<long long>((n + 255) / 256, COM_WINDOW_BLOCKS_MAX);
  hipLaunchKernelGGL(com_window_kernel, dim3(n_win), dim3(256), 0, stream, t, n, skip_b, skip_e, win_partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (accel)
    hipLaunchKernelGGL(com_moments_kernel<3>, dim3((unsigned)tiles), dim3(256), 0, stream, t, com, n, skip_b, skip_e, win_partial, n_win, window, partial);
  else
    hipLaunchKernelGGL(com_moments_kernel<2>, dim3((unsigned)tiles), dim3(256), 0, stream, t, com, n, skip_b, skip_e, win_partial, n_win, window, partial);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (accel)
    hipLaunchKernelGGL(com_fit_kernel<3>, dim3(1), dim3(64), 0, stream, t, com, window, partial, out);
  else
    hipLaunchKernelGGL(com_fit_kernel<2>, dim3(1), dim3(64), 0, stream, t, com, window, partial, out);
  return hipGetLastError();
}

}  // namespace bms
