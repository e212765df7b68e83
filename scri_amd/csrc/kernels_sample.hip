// The precessing sample waveform of scri/sample_waveforms.py:383-533 (`fake_precessing_waveform`) generated on the device, and the
// radius-dependent terms of the finite-radius family built on it (:596-755).  The per-step math is sample_math.h; the piecewise
// definitions change at a handful of steps the host planner finds (SamplePlan).
//
//   sample_phase_kernel      per step: PN phase and frequency, the frequency blended up to its merger value; the frequency from step
//                            i0 on also as one complex column (omega, 0), which the spline antiderivative turns into the phase there
//   sample_window_kernel     per step of the ringdown window: the integrands f transition' of the two transition_to_constant calls
//                            (opening angle, precession angle) as ONE complex column -- the spline is linear, one solve integrates both
//   sample_first_rotor_kernel  conj(sqrt(frame[0])), the constant every frame is multiplied by from the left
//   sample_waveform_kernel   per step: transitions, ringdown, modulation, the three precession angles, the chain of seven rotors; then
//                            the row of modes c_lm x^(p_lm) (1 + sign(m) modulation) ringdown.  A streaming kernel: it reads 8 to 40
//                            bytes per step and writes 32 (frame) + 16 n_modes (+ 32, the spinors of the inverse rotation).
//
// A workgroup takes SAMPLE_TILE consecutive steps.  Phase 1, one thread per step, does the transcendental work and leaves
// sqrt(x), the modulation and the ringdown factor in LDS; phase 2 writes the rows: a wavefront per row, lanes along the modes, so a row
// leaves as contiguous 1 KiB stores.  x^p with p a multiple of 1/2 is an integer power of sqrt(x) (binary powering, no pow per mode).
// A step's arithmetic depends on its index alone, never on the tile or the launch: the same bits from any split of the time axis.
#include "kernels.h"
#include "sample_math.h"

namespace bms {

namespace {

constexpr int SAMPLE_TILE = 256;

__device__ __forceinline__ double sample_phi(const SamplePlan& P, const double* __restrict__ phi_pn, const double2* __restrict__ I_omega,
                                             long long j) {
  return j < P.i0 ? phi_pn[j] : phi_pn[P.i0] + I_omega[j - P.i0].x;
}

// the two angles that pass through transition_to_constant, at step i: f transition - integral, frozen at their value of step ib - 1
__device__ __forceinline__ void sample_precession_angles(const SamplePlan& P, const double* __restrict__ t, const double* __restrict__ phi_pn,
                                                         const double2* __restrict__ I_omega, const double2* __restrict__ I_window,
                                                         long long i, double& opening, double& precession) {
  const long long j = i < P.ib() ? i : P.ib() - 1;
  const double tj = t[j];
  const double falling = sample_transition(tj, P.tr0, P.tr1, 1.0, 0.0);
  opening = (P.opening + P.opening_dot * tj) * falling;
  precession = sample_phi(P, phi_pn, I_omega, j) / P.rate * falling;
  if (j >= P.ia()) {
    const double2 I = I_window[j - P.ia()];
    opening -= I.x;
    precession -= I.y;
  }
}

__device__ __forceinline__ Quat sample_frame_of_step(const SamplePlan& P, const double* __restrict__ t, const double* __restrict__ phi_pn,
                                                     const double2* __restrict__ I_omega, const double2* __restrict__ I_window, long long i,
                                                     double phi, double rising) {
  double opening, precession;
  sample_precession_angles(P, t, phi_pn, I_omega, I_window, i, opening, precession);
  return sample_frame(phi, opening, precession, P.nutation * rising);
}

__global__ __launch_bounds__(256) void sample_phase_kernel(SamplePlan P, const double* __restrict__ t, double* __restrict__ phi_pn,
                                                           double* __restrict__ omega, double2* __restrict__ omega_col) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n) return;
  double phi, om;
  sample_pn_phase(P, t[i], phi, om);
  om = sample_omega(P, i, t[i], om);
  phi_pn[i] = phi;
  omega[i] = om;
  if (i >= P.i0) omega_col[i - P.i0] = make_double2(om, 0.0);
}

__global__ __launch_bounds__(256) void sample_window_kernel(SamplePlan P, const double* __restrict__ t, const double* __restrict__ phi_pn,
                                                            const double2* __restrict__ I_omega, double2* __restrict__ integrands) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= P.ib() - P.ia()) return;
  const long long j = P.ia() + k;
  const double slope = sample_transition_slope(t[j], P.tr0, P.tr1, 1.0, 0.0);
  integrands[k] = make_double2((P.opening + P.opening_dot * t[j]) * slope, sample_phi(P, phi_pn, I_omega, j) / P.rate * slope);
}

__global__ void sample_first_rotor_kernel(SamplePlan P, const double* __restrict__ t, const double* __restrict__ phi_pn,
                                          const double2* __restrict__ I_omega, const double2* __restrict__ I_window,
                                          double* __restrict__ left) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double rising = sample_transition(t[0], P.tr0, P.tr1, 0.0, 1.0);
  const Quat q = sample_conj_sqrt(sample_frame_of_step(P, t, phi_pn, I_omega, I_window, 0, sample_phi(P, phi_pn, I_omega, 0), rising));
  left[0] = q.w, left[1] = q.x, left[2] = q.y, left[3] = q.z;
}

__global__ __launch_bounds__(SAMPLE_TILE) void sample_waveform_kernel(SamplePlan P, const double* __restrict__ t,
                                                                      const double* __restrict__ phi_pn, const double* __restrict__ omega,
                                                                      const double2* __restrict__ I_omega, const double2* __restrict__ I_window,
                                                                      const double* __restrict__ left, const SampleMode* __restrict__ modes,
                                                                      int n_modes, double2* __restrict__ out, long long ld,
                                                                      double* __restrict__ frame, double* __restrict__ spinors) {
  __shared__ double s_root[SAMPLE_TILE], s_mod[SAMPLE_TILE], s_ring[SAMPLE_TILE];
  const long long row0 = (long long)blockIdx.x * SAMPLE_TILE;
  const long long i = row0 + threadIdx.x;
  if (i < P.n) {
    const double ti = t[i];
    const double phi = sample_phi(P, phi_pn, I_omega, i);
    const double rising = sample_transition(ti, P.tr0, P.tr1, 0.0, 1.0);
    const Quat L = {left[0], left[1], left[2], left[3]};
    const Quat q = qmul(L, sample_frame_of_step(P, t, phi_pn, I_omega, I_window, i, phi, rising));
    frame[4 * i] = q.w, frame[4 * i + 1] = q.x, frame[4 * i + 2] = q.y, frame[4 * i + 3] = q.z;
    // the inverse rotation as spinors (w + i z, y + i x) of conj(frame): what bms_rotate_series takes
    if (spinors) spinors[4 * i] = q.w, spinors[4 * i + 1] = -q.z, spinors[4 * i + 2] = -q.y, spinors[4 * i + 3] = -q.x;
    s_root[threadIdx.x] = sqrt(pow(omega[i], 2.0 / 3));  // sqrt(x), x = omega^(2/3) (:507)
    s_mod[threadIdx.x] = sample_transition(ti, P.tr0, P.tr1, 1.0, 0.0) * cos(phi) / 40.0;
    s_ring[threadIdx.x] = sample_ringdown(P, i, ti, rising);
  }
  __syncthreads();
  const int rows = (int)(P.n - row0 < SAMPLE_TILE ? P.n - row0 : SAMPLE_TILE);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int c = lane; c < n_modes; c += 64) {
    const SampleMode md = modes[c];
    for (int r = wave; r < rows; r += SAMPLE_TILE / 64) {
      const double a = ipow(s_root[r], md.twice_power) * (1 + md.sign_m * s_mod[r]) * s_ring[r];
      out[(row0 + r) * ld + c] = make_double2(md.re * a, md.im * a);
    }
  }
}

// out = h0 + |h0| sum_k coef_k exp(i k (50 pi / n) t)    (scri/sample_waveforms.py:740-742, one radius)
__global__ __launch_bounds__(SAMPLE_TILE) void radius_terms_kernel(const double* __restrict__ t, long long n, const double2* __restrict__ h0,
                                                                   long long ld0, int n_cols, RadiusTerms terms, double2* __restrict__ out,
                                                                   long long ld_out) {
  __shared__ double2 s_factor[SAMPLE_TILE];
  const long long row0 = (long long)blockIdx.x * SAMPLE_TILE;
  const long long i = row0 + threadIdx.x;
  if (i < n) {
    double2 f = make_double2(0.0, 0.0);
    for (int k = 1; k <= terms.n; ++k) {
      const double angle = (k * 50 * M_PI / (double)n) * t[i];
      f.x += terms.coef[k - 1] * cos(angle);
      f.y += terms.coef[k - 1] * sin(angle);
    }
    s_factor[threadIdx.x] = f;
  }
  __syncthreads();
  const int rows = (int)(n - row0 < SAMPLE_TILE ? n - row0 : SAMPLE_TILE);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r = wave; r < rows; r += SAMPLE_TILE / 64) {
    const double2 f = s_factor[r];
    for (int c = lane; c < n_cols; c += 64) {
      const double2 h = h0[(row0 + r) * ld0 + c];
      const double a = hypot(h.x, h.y);
      out[(row0 + r) * ld_out + c] = make_double2(h.x + f.x * a, h.y + f.y * a);
    }
  }
}

inline bool sample_grid(long long n, unsigned* blocks) {
  const long long b = (n + SAMPLE_TILE - 1) / SAMPLE_TILE;
  *blocks = (unsigned)b;
  return b <= 0x7fffffffLL;
}

}  // namespace

hipError_t launch_sample_phase(hipStream_t stream, const SamplePlan& P, const double* t, double* phi_pn, double* omega, double2* omega_col) {
  unsigned blocks;
  if (P.n <= 0) return hipSuccess;
  if (P.i0 < 0 || P.i0 >= P.n || !sample_grid(P.n, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sample_phase_kernel, dim3(blocks), dim3(256), 0, stream, P, t, phi_pn, omega, omega_col);
  return hipGetLastError();
}

hipError_t launch_sample_window(hipStream_t stream, const SamplePlan& P, const double* t, const double* phi_pn, const double2* I_omega,
                                double2* integrands) {
  unsigned blocks;
  const long long m = P.ib() - P.ia();
  if (m <= 0) return hipSuccess;
  if (P.ia() < 0 || P.ib() > P.n || P.i0 < 0 || P.i0 >= P.n || !sample_grid(m, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sample_window_kernel, dim3(blocks), dim3(256), 0, stream, P, t, phi_pn, I_omega, integrands);
  return hipGetLastError();
}

hipError_t launch_sample_waveform(hipStream_t stream, const SamplePlan& P, const double* t, const double* phi_pn, const double* omega,
                                  const double2* I_omega, const double2* I_window, double* left, const SampleMode* modes, int n_modes,
                                  double2* out, long long ld, double* frame, double* spinors) {
  unsigned blocks;
  if (P.n <= 0) return hipSuccess;
  // every index the kernels form from the plan lies inside the arrays of n, n - i0 and ib - ia elements
  if (P.i0 < 0 || P.i0 >= P.n || P.ia() < 1 || P.ib() <= P.ia() || P.ib() > P.n || n_modes < 1 || ld < n_modes || !sample_grid(P.n, &blocks))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sample_first_rotor_kernel, dim3(1), dim3(64), 0, stream, P, t, phi_pn, I_omega, I_window, left);
  hipLaunchKernelGGL(sample_waveform_kernel, dim3(blocks), dim3(SAMPLE_TILE), 0, stream, P, t, phi_pn, omega, I_omega, I_window, left, modes,
                     n_modes, out, ld, frame, spinors);
  return hipGetLastError();
}

hipError_t launch_radius_terms(hipStream_t stream, const double* t, long long n, const double2* h0, long long ld0, int n_cols,
                               const RadiusTerms& terms, double2* out, long long ld_out) {
  unsigned blocks;
  if (n <= 0 || n_cols <= 0) return hipSuccess;
  if (terms.n < 0 || terms.n > RADIUS_TERMS_MAX || ld0 < n_cols || ld_out < n_cols || !sample_grid(n, &blocks)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(radius_terms_kernel, dim3(blocks), dim3(SAMPLE_TILE), 0, stream, t, n, h0, ld0, n_cols, terms, out, ld_out);
  return hipGetLastError();
}

}  // namespace bms
