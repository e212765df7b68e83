// Per-time-step math of the precessing sample waveform (scri/sample_waveforms.py:449-516, scri/utilities.py:12-102, 162-190), shared by
// the kernels (kernels_sample.hip) and the host planner (engine_sample.hip): the transition function and its derivative, the
// leading-order PN phase and frequency with the blend up to the merger value, the ringdown factor, and the chain of seven rotors.
#pragma once
#include "pixel_math.h"

namespace bms {

// Where the piecewise definitions of one waveform change, found by the planner on the host time axis (plan_precessing).
struct SamplePlan {
  long long n;       // time steps
  long long i0, i1;  // omega is the PN value blended into 0.25 over (t[i0], t[i1]) and 0.25 from i1 on; phi is integrated from i0 (:466-475)
  long long im, ir;  // merger step and end of the ringdown transition, (t[im], t[ir]) (:480-483)
  double nu, t_merger;
  double tb0, tb1;  // t[i0], t[i1]
  double tr0, tr1;  // t[im], t[ir]
  double opening, opening_dot, rate, nutation;  // precession_opening_angle, its rate, precession_relative_rate, precession_nutation_angle
  // transition_to_constant (utilities.py:186-190) integrates over the steps strictly inside (t[im], t[ir]): [ia, ib)
  BMS_HD long long ia() const { return im + 1; }
  BMS_HD long long ib() const { return ir; }
};

constexpr double SAMPLE_MAXEXP = 1024 * 0.6931471805599453 * 0.99;  // utilities.py:8: np.finfo(float).maxexp * np.log(2) * 0.99
constexpr double SAMPLE_OMEGA_MERGER = 0.25;

// transition_function(x, x0, x1, y0, y1) at one point of a monotonic axis (utilities.py:12-30)
BMS_HD double sample_transition(double x, double x0, double x1, double y0, double y1) {
  if (x <= x0) return y0;
  if (!(x < x1)) return y1;
  const double tau = (x - x0) / (x1 - x0);
  const double exponent = 1.0 / tau - 1.0 / (1.0 - tau);
  if (exponent >= SAMPLE_MAXEXP) return y0;
  return y0 + (y1 - y0) / (1.0 + exp(exponent));
}
// transition_function_derivative (utilities.py:61-102)
BMS_HD double sample_transition_slope(double x, double x0, double x1, double y0, double y1) {
  if (x <= x0 || !(x < x1)) return 0.0;
  const double tau = (x - x0) / (x1 - x0);
  const double exponent = 1.0 / tau - 1.0 / (1.0 - tau);
  if (exponent >= SAMPLE_MAXEXP) return 0.0;
  const double e = exp(exponent);
  return -(y1 - y0) * e * (-1.0 / (tau * tau) - 1.0 / ((1.0 - tau) * (1.0 - tau))) * (1 / (x1 - x0)) / ((1.0 + e) * (1.0 + e));
}

// tau = nu (t_merger - t) / 5, phi = -4 tau^(5/8), omega = (nu / 2) tau^(-3/8): NaN after the merger, as in the reference (:459-463)
BMS_HD void sample_pn_phase(const SamplePlan& P, double t, double& phi, double& omega) {
  const double tau = P.nu * (P.t_merger - t) / 5;
  phi = -4 * pow(tau, 5.0 / 8);
  omega = (P.nu / 2) * pow(tau, -3.0 / 8);
}
// omega of step i after the blend (:466-472)
BMS_HD double sample_omega(const SamplePlan& P, long long i, double t, double omega_pn) {
  if (i >= P.i1) return SAMPLE_OMEGA_MERGER;
  const double tr = sample_transition(t, P.tb0, P.tb1, 0.0, 1.0);
  return omega_pn * (1 - tr) + SAMPLE_OMEGA_MERGER * tr;
}
// ringdown factor of step i (:478-486); rising = transition_function(t, t[im], t[ir]) at this step
BMS_HD double sample_ringdown(const SamplePlan& P, long long i, double t, double rising) {
  if (i < P.im) return 1.0;
  return 1.0 * (1 - rising) + 2.25 * exp(-(t - P.t_merger) / 11.5) * rising;
}

// exp(a e) for a unit basis quaternion e: (cos |a|, a sin |a| / |a|), the real unit below numpy-quaternion's threshold
BMS_HD void sample_exp(double a, double& c, double& s) {
  const double v = fabs(a);
  if (v > 1e-14) {
    c = cos(v);
    s = sin(v) / v * a;
  } else {
    c = 1.0;
    s = 0.0;
  }
}
// R_orbital R_nutation conj(R_orbital) R_precession R_opening conj(R_precession) R_orbital (:493-503), multiplied from the left
BMS_HD Quat sample_frame(double phi, double opening, double precession, double nutation) {
  double c, s;
  sample_exp(phi / 2, c, s);
  const Quat Ro = {c, 0.0, 0.0, s}, Roc = {c, -0.0, -0.0, -s};
  sample_exp(nutation / 2, c, s);
  const Quat Rn = {c, s, 0.0, 0.0};
  sample_exp(precession / 2, c, s);
  const Quat Rp = {c, 0.0, 0.0, s}, Rpc = {c, -0.0, -0.0, -s};
  sample_exp(opening / 2, c, s);
  const Quat Rop = {c, s, 0.0, 0.0};
  return qmul(qmul(qmul(qmul(qmul(qmul(Ro, Rn), Roc), Rp), Rop), Rpc), Ro);
}
// conj(sqrt(q)) (numpy-quaternion's sqrt; :504)
BMS_HD Quat sample_conj_sqrt(const Quat& q) {
  const double a = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  if (fabs(a + q.w) < 1e-14 * a) return {0.0, -sqrt(a), -0.0, -0.0};
  const double c = a > 0 ? sqrt(a / (2 + 2 * q.w / a)) : 0.0;
  return {(1.0 + q.w / a) * c, -(q.x * c / a), -(q.y * c / a), -(q.z * c / a)};
}

}  // namespace bms
