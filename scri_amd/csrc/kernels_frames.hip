// Frame construction on the device: the corotating frame (scri/mode_calculations.py:435-491) and the coprecessing frame
// (scri/rotations.py:14-49, scri/mode_calculations.py:316-399) from per-step quantities that are already in HBM.
//
// Nothing here is sequential in time.  The frame R_j = E_{j-1} ... E_0 R_0 is a prefix product of interval rotors that depend on the
// spline of omega alone; the sign that makes the dominant axis continuous is a function of its neighbour's sign alone, and functions
// on {+1, -1} compose associatively; the minimal rotation is spline slopes, a spline antiderivative and pointwise products.  So the
// two scans below (one kernel family, parameterised by the operator) and a handful of one-thread-per-step kernels do all of it.
//
// The scans are the three-level kind: 64 lanes by __shfl_up, the waves of a block through LDS, the blocks by a second pass over the
// block totals (one block walks them in chunks) and a third that applies them.  No flags, no spinning, no atomics: the order of the
// operations is fixed by the indices, so a result is the same from run to run.
#include "kernels.h"
#include "pixel_math.h"

namespace bms {

namespace {

constexpr int SCAN_BLOCK = 256;

// combine(a, b): a covers the EARLIER steps, b the later ones
struct QuatProduct {
  using T = Quat;
  static __device__ __forceinline__ T identity() { return {1.0, 0.0, 0.0, 0.0}; }
  static __device__ __forceinline__ T combine(const T& a, const T& b) { return qmul(b, a); }
  static __device__ __forceinline__ T shfl_up(const T& a, int off) {
    return {__shfl_up(a.w, off, 64), __shfl_up(a.x, off, 64), __shfl_up(a.y, off, 64), __shfl_up(a.z, off, 64)};
  }
};
// a map s -> m(s) on {+1, -1}: bit 0 set when m(+1) = -1, bit 1 set when m(-1) = -1
struct SignMap {
  using T = unsigned;
  static __device__ __forceinline__ T identity() { return 2u; }
  static __device__ __forceinline__ T combine(T a, T b) {
    const T lo = b & 1u, hi = (b >> 1) & 1u;
    return ((a & 1u) ? hi : lo) | (((a & 2u) ? hi : lo) << 1);
  }
  static __device__ __forceinline__ T shfl_up(T a, int off) { return (T)__shfl_up((int)a, off, 64); }
};

// inclusive scan of the 256 values x of a block (every thread calls it); returns the scanned value of the caller
template <class Op>
__device__ __forceinline__ typename Op::T block_scan(typename Op::T x, typename Op::T* wave_tot /* LDS, 4 */) {
  using T = typename Op::T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T y = Op::shfl_up(x, off);
    if (lane >= off) x = Op::combine(y, x);
  }
  if (lane == 63) wave_tot[wave] = x;
  __syncthreads();
  if (wave > 0) {
    T p = wave_tot[0];
    for (int w = 1; w < wave; ++w) p = Op::combine(p, wave_tot[w]);
    x = Op::combine(p, x);
  }
  return x;
}

template <class Op>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_blocks_kernel(typename Op::T* __restrict__ data, long long n,
                                                                 typename Op::T* __restrict__ totals) {
  using T = typename Op::T;
  __shared__ T wave_tot[SCAN_BLOCK / 64];
  const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
  const T x = block_scan<Op>(i < n ? data[i] : Op::identity(), wave_tot);
  if (i < n) data[i] = x;
  if (threadIdx.x == SCAN_BLOCK - 1) totals[blockIdx.x] = x;
}

// one block: inclusive scan of the m block totals, a chunk of 256 at a time with the running value carried along
template <class Op>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_totals_kernel(typename Op::T* __restrict__ totals, long long m) {
  using T = typename Op::T;
  __shared__ T wave_tot[SCAN_BLOCK / 64];
  __shared__ T carry;
  for (long long base = 0; base < m; base += SCAN_BLOCK) {
    const long long i = base + threadIdx.x;
    T x = block_scan<Op>(i < m ? totals[i] : Op::identity(), wave_tot);
    if (base > 0) x = Op::combine(carry, x);
    if (i < m) totals[i] = x;
    __syncthreads();  // (every read of carry and wave_tot of this chunk is done)
    if (threadIdx.x == SCAN_BLOCK - 1) carry = x;
    __syncthreads();
  }
}

template <class Op>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_apply_kernel(typename Op::T* __restrict__ data, long long n,
                                                                const typename Op::T* __restrict__ totals) {
  if (blockIdx.x == 0) return;
  const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x;
  if (i < n) data[i] = Op::combine(totals[blockIdx.x - 1], data[i]);
}

template <class Op>
hipError_t launch_scan(hipStream_t stream, typename Op::T* data, long long n, typename Op::T* totals) {
  if (n <= 0) return hipSuccess;
  const long long blocks = frame_scan_blocks(n);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scan_blocks_kernel<Op>, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, stream, data, n, totals);
  if (blocks > 1) {
    hipLaunchKernelGGL(scan_totals_kernel<Op>, dim3(1), dim3(SCAN_BLOCK), 0, stream, totals, blocks);
    hipLaunchKernelGGL(scan_apply_kernel<Op>, dim3((unsigned)blocks), dim3(SCAN_BLOCK), 0, stream, data, n, totals);
  }
  return hipGetLastError();
}

__device__ __forceinline__ Quat load_quat(const double* p, long long j) { return {p[4 * j], p[4 * j + 1], p[4 * j + 2], p[4 * j + 3]}; }
__device__ __forceinline__ void store_quat(double* p, long long j, const Quat& q) {
  p[4 * j] = q.w, p[4 * j + 1] = q.x, p[4 * j + 2] = q.y, p[4 * j + 3] = q.z;
}
__device__ __forceinline__ Quat qconj(const Quat& q) { return {q.w, -q.x, -q.y, -q.z}; }
__device__ __forceinline__ Quat normalised(const Quat& q) {
  const double nr = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return nr > 0.0 ? Quat{q.w / nr, q.x / nr, q.y / nr, q.z / nr} : q;
}
inline unsigned grid_for(long long n) { return (unsigned)((n + 255) / 256); }

// ------------------------------------------------------------------------------------------------ corotating frame
__global__ __launch_bounds__(256) void pad_omega_kernel(const double* __restrict__ om3, double* __restrict__ w4, long long n) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  w4[4 * j] = om3[3 * j], w4[4 * j + 1] = om3[3 * j + 1], w4[4 * j + 2] = om3[3 * j + 2], w4[4 * j + 3] = 0.0;
}

// The rotor of sampling interval j by the rule of bms_integrate_angular_velocity (engine_blocks.hip): m sub-steps of bounded
// rotation angle, each one fourth-order Magnus step with two Gauss points applied as an exact exponential.  It depends on the cubic
// of omega over the interval only, so all intervals are formed side by side.  m is capped at MAX_SUBSTEPS (include/scri_amd.h says
// so): a thread must end whatever it is fed, and an interval that turns by more than 2e5 radians is not a sampled rotation anyway.
constexpr long long MAX_SUBSTEPS = 1 << 20;
__global__ __launch_bounds__(256) void interval_rotor_kernel(const double* __restrict__ w4, const double* __restrict__ s4,
                                                             const double* __restrict__ x, long long n, double amax,
                                                             double* __restrict__ Q) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  if (j == 0) store_quat(Q, 0, {1.0, 0.0, 0.0, 0.0});
  if (j + 1 >= n) return;
  const double h = x[j + 1] - x[j];
  double y0[3], y1[3], s0[3], c2[3], c3[3];
  for (int k = 0; k < 3; ++k) {
    y0[k] = w4[4 * j + k], y1[k] = w4[4 * (j + 1) + k], s0[k] = s4[4 * j + k];
    const double s1 = s4[4 * (j + 1) + k];
    const double dd = (y1[k] - y0[k]) / h, tt = (s0[k] + s1 - 2 * dd) / h;
    c3[k] = tt / h, c2[k] = (dd - s0[k]) / h - tt;
  }
  const double wmax = fmax(sqrt(y0[0] * y0[0] + y0[1] * y0[1] + y0[2] * y0[2]), sqrt(y1[0] * y1[0] + y1[1] * y1[1] + y1[2] * y1[2]));
  const double want = ceil(wmax * h / amax);
  const long long m = want >= (double)MAX_SUBSTEPS ? MAX_SUBSTEPS : (want > 1.0 ? (long long)want : 1);
  const double hs = h / m;
  const double g1 = 0.5 - sqrt(3.0) / 6.0, g2 = 0.5 + sqrt(3.0) / 6.0;
  const double k1 = hs / 4, k2 = sqrt(3.0) / 24 * hs * hs;
  Quat E = {1.0, 0.0, 0.0, 0.0};
  for (long long q = 0; q < m; ++q) {
    double wa[3], wb[3];
    const double ta = (q + g1) * hs, tb = (q + g2) * hs;
    for (int k = 0; k < 3; ++k) {
      wa[k] = y0[k] + ta * (s0[k] + ta * (c2[k] + ta * c3[k]));
      wb[k] = y0[k] + tb * (s0[k] + tb * (c2[k] + tb * c3[k]));
    }
    // rotation vector of the step (halved): h/4 (wa + wb) + (sqrt3/24) h^2 (wb x wa)
    const double cx = wb[1] * wa[2] - wb[2] * wa[1], cy = wb[2] * wa[0] - wb[0] * wa[2], cz = wb[0] * wa[1] - wb[1] * wa[0];
    const double vx = k1 * (wa[0] + wb[0]) + k2 * cx, vy = k1 * (wa[1] + wb[1]) + k2 * cy, vz = k1 * (wa[2] + wb[2]) + k2 * cz;
    const double vn = sqrt(vx * vx + vy * vy + vz * vz);
    const double sc = vn > 1e-300 ? sin(vn) / vn : 1.0;
    E = qmul(Quat{cos(vn), sc * vx, sc * vy, sc * vz}, E);
  }
  store_quat(Q, j + 1, E);
}

__global__ __launch_bounds__(256) void frame_finish_kernel(const double* P, long long n, Vec4 R0, double* out) {  // (out may be P: no restrict)
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const Quat r0 = {R0.v[0], R0.v[1], R0.v[2], R0.v[3]};
  store_quat(out, j, j == 0 ? r0 : normalised(qmul(load_quat(P, j), r0)));
}

// ------------------------------------------------------------------------------------------------ dominant axis
// Cyclic Jacobi on a symmetric 3 x 3 matrix: rotations in the (0,1), (0,2), (1,2) planes until the off-diagonal part is exactly
// zero (an element that no longer changes the diagonal it couples is set to zero), at most JACOBI_SWEEPS sweeps.  Accurate to
// rounding whatever the gaps between the eigenvalues, and exact on a diagonal matrix -- closed-form eigenvalue formulas are neither.
constexpr int JACOBI_SWEEPS = 24;
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& apr, double& aqr, double (&v)[3][3], int p,
                                              int q, bool late) {
  if (apq == 0.0) return;
  const double g = 100.0 * fabs(apq);
  if (late && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
    apq = 0.0;
    return;
  }
  const double d = aqq - app;
  double t;
  if (fabs(d) + g == fabs(d)) {
    t = apq / d;
  } else {
    const double theta = 0.5 * d / apq;
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  app -= t * apq, aqq += t * apq, apq = 0.0;
  const double xr = apr, yr = aqr;
  apr = xr - s * (yr + tau * xr), aqr = yr + s * (xr - tau * yr);
  for (int k = 0; k < 3; ++k) {
    const double xp = v[k][p], xq = v[k][q];
    v[k][p] = xp - s * (xq + tau * xp), v[k][q] = xq + s * (xp - tau * xq);
  }
}

__global__ __launch_bounds__(256) void dominant_axis_kernel(const double* __restrict__ ll, long long n, double* __restrict__ axis) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double* a = ll + 9 * j;
  // (the lower triangle, as numpy.linalg.eigh reads it)
  double a00 = a[0], a11 = a[4], a22 = a[8], a01 = a[3], a02 = a[6], a12 = a[7];
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    if (fabs(a01) + fabs(a02) + fabs(a12) == 0.0) break;
    const bool late = sweep >= 3;
    jacobi_rotate(a00, a11, a01, a02, a12, v, 0, 1, late);
    jacobi_rotate(a00, a22, a02, a01, a12, v, 0, 2, late);
    jacobi_rotate(a11, a22, a12, a01, a02, v, 1, 2, late);
  }
  int k = 0;
  double top = a00;
  if (a11 >= top) k = 1, top = a11;
  if (a22 >= top) k = 2;
  axis[3 * j] = v[0][k], axis[3 * j + 1] = v[1][k], axis[3 * j + 2] = v[2][k];
}

// the rule of scri/mode_calculations.py:316-363: v is flipped when |v - u|^2 > |v|^2, u its already fixed neighbour = s * (raw u)
__device__ __forceinline__ unsigned sign_map(const double* v, const double* u) {
  const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  unsigned bits = 0;
  for (int b = 0; b < 2; ++b) {
    const double s = b ? -1.0 : 1.0;
    const double dx = v[0] - s * u[0], dy = v[1] - s * u[1], dz = v[2] - s * u[2];
    if (dx * dx + dy * dy + dz * dz > vv) bits |= 1u << b;
  }
  return bits;
}

__global__ __launch_bounds__(256) void axis_sign_map_kernel(const double* __restrict__ axis, long long n, long long anchor, Vec4 rough,
                                                            unsigned* __restrict__ fwd, unsigned* __restrict__ bwd) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* v = axis + 3 * i;
  if (i == anchor) {
    const unsigned m = rough.v[0] * v[0] + rough.v[1] * v[1] + rough.v[2] * v[2] < 0.0 ? 3u : 0u;  // both signs -> the anchor's
    fwd[0] = m, bwd[0] = m;
  } else if (i > anchor) {
    fwd[i - anchor] = sign_map(v, v - 3);
  } else {
    bwd[anchor - i] = sign_map(v, v + 3);
  }
}

__global__ __launch_bounds__(256) void axis_apply_signs_kernel(const double* __restrict__ axis, long long n, long long anchor,
                                                               const unsigned* __restrict__ fwd, const unsigned* __restrict__ bwd,
                                                               double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned m = i >= anchor ? fwd[i - anchor] : bwd[anchor - i];
  const double s = (m & 1u) ? -1.0 : 1.0;
  double x = s * axis[3 * i], y = s * axis[3 * i + 1], z = s * axis[3 * i + 2];
  const double nr = sqrt(x * x + y * y + z * z);
  if (nr != 0.0) x /= nr, y /= nr, z /= nr;  // (zero vectors stay zero)
  out[3 * i] = x, out[3 * i + 1] = y, out[3 * i + 2] = z;
}

// ------------------------------------------------------------------------------------------------ pointwise rotor kernels
__global__ __launch_bounds__(256) void axis_rotor_kernel(const double* __restrict__ axis, long long n, double* __restrict__ R) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  // -v z = (v_z, -v_y, v_x, 0) and its square root (quaternions.sqrt: the half-angle rotor, -1 -> a rotation about x)
  const double vx = axis[3 * j], vy = axis[3 * j + 1], vz = axis[3 * j + 2];
  const double w = sqrt(fmax((1.0 + vz) / 2.0, 0.0));
  Quat q = {w, 1.0, 0.0, 0.0};
  if (w > 1e-150) q = {w, -vy / (2.0 * w), vx / (2.0 * w), 0.0};
  store_quat(R, j, q);
}

__global__ __launch_bounds__(256) void halfgammadot_kernel(const double* __restrict__ R, const double* __restrict__ Rdot, long long n,
                                                           double* __restrict__ h) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const Quat z = {0.0, 0.0, 0.0, 1.0};
  h[2 * j] = qmul(qmul(load_quat(Rdot, j), z), qconj(load_quat(R, j))).w;
  h[2 * j + 1] = 0.0;
}

__global__ __launch_bounds__(256) void spin_about_z_kernel(const double* R, const double* __restrict__ halfgamma, long long n,
                                                           double* out) {  // (out may be R: no restrict on the two)
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double g = halfgamma[2 * j];
  store_quat(out, j, qmul(load_quat(R, j), Quat{cos(g), 0.0, 0.0, sin(g)}));
}

__global__ __launch_bounds__(256) void rotor_omega_kernel(const double* __restrict__ R, const double* __restrict__ Rdot, long long n,
                                                          double* __restrict__ om3) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const Quat q = qmul(load_quat(Rdot, j), qconj(load_quat(R, j)));
  om3[3 * j] = 2.0 * q.x, om3[3 * j + 1] = 2.0 * q.y, om3[3 * j + 2] = 2.0 * q.z;
}

__global__ __launch_bounds__(256) void frame_adjust_kernel(double* __restrict__ frame, long long n, Vec4 right, int with_right, double pow2,
                                                           double* __restrict__ log_out, double* __restrict__ spinors) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  Quat q = load_quat(frame, j);
  if (with_right) q = qmul(q, Quat{right.v[0], right.v[1], right.v[2], right.v[3]});
  q = normalised(q);
  if (pow2 > 0.0) {
    // log, rounded to multiples of 1 / pow2, and exp of that (quaternions.log / quaternions.exp)
    double vn = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
    const double qn = sqrt(q.w * q.w + vn * vn);
    const double scale = vn > 1e-300 ? atan2(vn, q.w) / vn : 0.0;
    const Quat L = {rint(log(qn > 0.0 ? qn : 1.0) * pow2) / pow2, rint(q.x * scale * pow2) / pow2, rint(q.y * scale * pow2) / pow2,
                    rint(q.z * scale * pow2) / pow2};
    if (log_out) store_quat(log_out, j, L);
    vn = sqrt(L.x * L.x + L.y * L.y + L.z * L.z);
    const double e = exp(L.w), s = vn > 1e-300 ? sin(vn) / vn : 1.0;
    q = {e * cos(vn), e * s * L.x, e * s * L.y, e * s * L.z};
  }
  store_quat(frame, j, q);
  if (spinors) spinors[4 * j] = q.w, spinors[4 * j + 1] = q.z, spinors[4 * j + 2] = q.y, spinors[4 * j + 3] = q.x;
}

// ------------------------------------------------------------------------------------------------ rotor interpolation (squad)
// scri_amd.quaternions.squad, operation for operation (no contraction, the same order of every sum), so that the only difference from
// the numpy statement is the device's atan2 / sin / cos / log / exp.  Two kernels: the control points A_i, B_i depend on the knots
// alone (three logarithms and two exponentials per knot), so they are formed once per knot and not once per argument; an argument then
// costs a binary search of the knots and three slerps.  One thread per knot / per argument, nothing shared, no order among arguments.
__device__ __forceinline__ Quat quat_log(const Quat& q) {
#pragma clang fp contract(off)
  const double vn = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
  const double qn = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  const double scale = vn > 1e-300 ? atan2(vn, q.w) / vn : 0.0;
  return {log(qn > 0.0 ? qn : 1.0), q.x * scale, q.y * scale, q.z * scale};
}
__device__ __forceinline__ Quat quat_exp(const Quat& q) {
#pragma clang fp contract(off)
  const double vn = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
  const double e = exp(q.w);
  const double s = vn > 1e-300 ? sin(vn) / vn : 1.0;
  const double es = e * s;
  return {e * cos(vn), es * q.x, es * q.y, es * q.z};
}
__device__ __forceinline__ Quat quat_scaled(const Quat& q, double f) { return {q.w * f, q.x * f, q.y * f, q.z * f}; }
// q1 (q1^-1 q2)^tau
__device__ __forceinline__ Quat quat_slerp(const Quat& q1, const Quat& q2, double tau) {
  return qmul(q1, quat_exp(quat_scaled(quat_log(qmul(qconj(q1), q2)), tau)));
}

// AB f8[n][8] = (A_i, B_i).  The end rules in the statement's order: A[0] = R[0], A[-1] = R[-1], B[-2] = R[-1], B[-1] = R_n, the later
// one winning where they meet (n = 2, 3).  The knots the general rule reads (i - 1 .. i + 2) exist wherever an end rule does not apply.
__global__ __launch_bounds__(256) void squad_control_kernel(const double* __restrict__ R, const double* __restrict__ t, long long n,
                                                            double* __restrict__ AB) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Quat Ri = load_quat(R, i);
  Quat A, B;
  if (i == 0 || i == n - 1) {
    A = Ri;
  } else {
    const Quat step = quat_log(qmul(qconj(Ri), load_quat(R, i + 1)));
    const Quat back = quat_log(qmul(qconj(load_quat(R, i - 1)), Ri));
    const double r_next = (t[i + 1] - t[i]) / (t[i] - t[i - 1]);
    const Quat e = {(-step.w + back.w * r_next) * 0.25, (-step.x + back.x * r_next) * 0.25, (-step.y + back.y * r_next) * 0.25,
                    (-step.z + back.z * r_next) * 0.25};
    A = qmul(Ri, quat_exp(e));
  }
  if (i == n - 1) {
    B = qmul(qmul(Ri, qconj(load_quat(R, i - 1))), Ri);  // R_n, the mirrored value beyond the end
  } else if (i == n - 2) {
    B = load_quat(R, i + 1);
  } else {
    const Quat Rn = load_quat(R, i + 1);
    const Quat step = quat_log(qmul(qconj(Ri), Rn));
    const Quat ahead = quat_log(qmul(qconj(Rn), load_quat(R, i + 2)));
    const double r_after = (t[i + 1] - t[i]) / (t[i + 2] - t[i + 1]);
    const Quat e = {(ahead.w * r_after - step.w) * -0.25, (ahead.x * r_after - step.x) * -0.25, (ahead.y * r_after - step.y) * -0.25,
                    (ahead.z * r_after - step.z) * -0.25};
    B = qmul(Rn, quat_exp(e));
  }
  store_quat(AB, 2 * i, A);
  store_quat(AB, 2 * i + 1, B);
}

// out[j] = squad at t_out[j]: interval i = clip(searchsorted(t, t_out[j], "right") - 1, 0, n - 1); interval n - 1 runs to the mirrored
// knot 2 t[n-1] - t[n-2] with the mirrored rotor R_n = B[n-1]
__global__ __launch_bounds__(256) void squad_eval_kernel(const double* __restrict__ R, const double* __restrict__ t, long long n,
                                                         const double* __restrict__ AB, const double* __restrict__ t_out, long long m,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const double u = t_out[j];
  long long lo = 0, hi = n;  // the number of knots <= u
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (t[mid] <= u) lo = mid + 1; else hi = mid;
  }
  const long long i = lo > 0 ? lo - 1 : 0;
  const bool last = i == n - 1;
  const Quat Ri = load_quat(R, i);
  const Quat Rn = last ? load_quat(AB, 2 * i + 1) : load_quat(R, i + 1);
  const double t_next = last ? t[i] + (t[i] - t[i - 1]) : t[i + 1];
  const double tau = (u - t[i]) / (t_next - t[i]);
  const Quat a = quat_slerp(Ri, Rn, tau);
  const Quat b = quat_slerp(load_quat(AB, 2 * i), load_quat(AB, 2 * i + 1), tau);
  store_quat(out, j, quat_slerp(a, b, 2 * tau * (1 - tau)));
}

}  // namespace

long long frame_scan_blocks(long long n) { return (n + SCAN_BLOCK - 1) / SCAN_BLOCK; }

hipError_t launch_scan_quat(hipStream_t stream, double* q, long long n, double* totals) {
  return launch_scan<QuatProduct>(stream, reinterpret_cast<Quat*>(q), n, reinterpret_cast<Quat*>(totals));
}
hipError_t launch_scan_sign_maps(hipStream_t stream, unsigned* m, long long n, unsigned* totals) {
  return launch_scan<SignMap>(stream, m, n, totals);
}

#define FRAME_LAUNCH(kernel, n, ...)                                                                   \
  do {                                                                                                 \
    if ((n) <= 0) return hipSuccess;                                                                   \
    if (((n) + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;                                 \
    hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, stream, __VA_ARGS__);                  \
    return hipGetLastError();                                                                          \
  } while (0)

hipError_t launch_pad_omega(hipStream_t stream, const double* om3, double* w4, long long n) { FRAME_LAUNCH(pad_omega_kernel, n, om3, w4, n); }
hipError_t launch_interval_rotors(hipStream_t stream, const double* w4, const double* s4, const double* x, long long n, double amax,
                                  double* Q) {
  FRAME_LAUNCH(interval_rotor_kernel, n, w4, s4, x, n, amax, Q);
}
hipError_t launch_frame_finish(hipStream_t stream, const double* P, long long n, Vec4 R0, double* out) {
  FRAME_LAUNCH(frame_finish_kernel, n, P, n, R0, out);
}
hipError_t launch_dominant_axis(hipStream_t stream, const double* ll, long long n, double* axis) {
  FRAME_LAUNCH(dominant_axis_kernel, n, ll, n, axis);
}
hipError_t launch_axis_sign_maps(hipStream_t stream, const double* axis, long long n, long long anchor, Vec4 rough, unsigned* fwd,
                                 unsigned* bwd) {
  if (anchor < 0 || anchor >= n) return hipErrorInvalidValue;
  FRAME_LAUNCH(axis_sign_map_kernel, n, axis, n, anchor, rough, fwd, bwd);
}
hipError_t launch_axis_apply_signs(hipStream_t stream, const double* axis, long long n, long long anchor, const unsigned* fwd,
                                   const unsigned* bwd, double* out) {
  if (anchor < 0 || anchor >= n) return hipErrorInvalidValue;
  FRAME_LAUNCH(axis_apply_signs_kernel, n, axis, n, anchor, fwd, bwd, out);
}
hipError_t launch_axis_rotor(hipStream_t stream, const double* axis, long long n, double* R) { FRAME_LAUNCH(axis_rotor_kernel, n, axis, n, R); }
hipError_t launch_halfgammadot(hipStream_t stream, const double* R, const double* Rdot, long long n, double* h) {
  FRAME_LAUNCH(halfgammadot_kernel, n, R, Rdot, n, h);
}
hipError_t launch_spin_about_z(hipStream_t stream, const double* R, const double* halfgamma, long long n, double* out) {
  FRAME_LAUNCH(spin_about_z_kernel, n, R, halfgamma, n, out);
}
hipError_t launch_rotor_omega(hipStream_t stream, const double* R, const double* Rdot, long long n, double* om3) {
  FRAME_LAUNCH(rotor_omega_kernel, n, R, Rdot, n, om3);
}
hipError_t launch_frame_adjust(hipStream_t stream, double* frame, long long n, Vec4 right, int with_right, double pow2, double* log_out,
                               double* spinors) {
  FRAME_LAUNCH(frame_adjust_kernel, n, frame, n, right, with_right, pow2, log_out, spinors);
}
hipError_t launch_squad_control(hipStream_t stream, const double* R, const double* t, long long n, double* AB) {
  if (n < 2) return hipErrorInvalidValue;
  FRAME_LAUNCH(squad_control_kernel, n, R, t, n, AB);
}
hipError_t launch_squad_eval(hipStream_t stream, const double* R, const double* t, long long n, const double* AB, const double* t_out,
                             long long m, double* out) {
  if (n < 2) return hipErrorInvalidValue;
  FRAME_LAUNCH(squad_eval_kernel, m, R, t, n, AB, t_out, m, out);
}

}  // namespace bms
