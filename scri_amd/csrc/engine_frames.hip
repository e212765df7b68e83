// Frame construction: the corotating and the coprecessing frame of a waveform, built on the device from modes that are already there
// (kernels_frames.hip; the spline solves are those of kernels_spline.hip / kernels_series.hip on series of one or two complex columns)
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI)
#include "engine.h"

namespace {

struct FrameAxis {  // the time axis of one call on the device, with the tables of its not-a-knot spline
  double* d_x = nullptr;
  SplineTable* d_tab = nullptr;
  int tile = SPLINE_TILE;
};

int check_time_axis(bms_ctx* c, const double* t, int64_t n) {
  if (n < 4) return fail(c, BMS_ERR_UNSUPPORTED, "the splines of the frame need at least 4 time steps, got %lld", (long long)n);
  for (int64_t i = 1; i < n; ++i)
    if (!(t[i] > t[i - 1])) return fail(c, BMS_ERR_INVALID, "time array must be strictly increasing (index %lld)", (long long)i);
  return BMS_OK;
}

int frame_axis(bms_ctx* c, const double* t, int64_t n, FrameAxis& ax) {
  int rc = upload_times(c, t, n, 0, n, 0, n, &ax.d_x, &ax.d_tab);
  ax.tile = spline_tile_for(t, n);
  return rc;
}

// knot slopes d_S of the series d_y f8[n][2 n_cols] (n_cols complex columns): the forward pass goes through `fw`
int knot_slopes(bms_ctx* c, const FrameAxis& ax, int64_t n, const double* d_y, int n_cols, const char* fw, double* d_S) {
  double* d_F;
  int rc = dev_buf_t(c, fw, (size_t)n * 2 * n_cols, &d_F);
  if (rc) return rc;
  TIMED(c, BMS_TAG_SPLINE_FORWARD, launch_spline_forward(c->stream, d_y, d_F, 2 * n_cols, n_cols, 0, n, n, ax.d_x, ax.d_tab, ax.tile, SPLINE_HALO));
  TIMED(c, BMS_TAG_SPLINE_BACKWARD, launch_spline_slopes(c->stream, d_F, d_S, 2 * n_cols, n_cols, n, ax.d_tab, ax.tile, SPLINE_HALO));
  return BMS_OK;
}

// d_R f8[n][4] from d_om f8[n][3] (both on the device): slopes of omega, interval rotors, prefix product, R0 and normalisation
int frame_from_omega(bms_ctx* c, const FrameAxis& ax, int64_t n, const double* d_om, const double R0[4], double tolerance, double* d_R) {
  if (!(tolerance > 0)) tolerance = 1e-12;
  const double amax = std::min(0.2, std::max(1e-3, 2.0 * std::pow(tolerance, 0.2)));  // as bms_integrate_angular_velocity
  int rc;
  double *d_w4, *d_s4, *d_Q, *d_tot;
  if ((rc = dev_buf_t(c, "fr_w4", (size_t)n * 4, &d_w4))) return rc;
  if ((rc = dev_buf_t(c, "fr_s4", (size_t)n * 4, &d_s4))) return rc;
  if ((rc = dev_buf_t(c, "fr_Q", (size_t)n * 4, &d_Q))) return rc;
  if ((rc = dev_buf_t(c, "fr_totals", (size_t)frame_scan_blocks(n) * 4, &d_tot))) return rc;
  hipStream_t S = c->stream;
  TIMED(c, BMS_TAG_POINTWISE, launch_pad_omega(S, d_om, d_w4, n));
  if ((rc = knot_slopes(c, ax, n, d_w4, 2, "fr_fw", d_s4))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_interval_rotors(S, d_w4, d_s4, ax.d_x, n, amax, d_Q));
  TIMED(c, BMS_TAG_POINTWISE, launch_scan_quat(S, d_Q, n, d_tot));
  Vec4 r0 = {{R0[0], R0[1], R0[2], R0[3]}};
  TIMED(c, BMS_TAG_POINTWISE, launch_frame_finish(S, d_Q, n, r0, d_R));
  return BMS_OK;
}

// d_axis f8[n][3] from d_ll f8[n][9] (device): Jacobi per step, the two scans of sign maps out of the anchor, normalisation
int dominant_axis(bms_ctx* c, int64_t n, const double* d_ll, const double rough[3], int64_t anchor, double* d_axis) {
  int rc;
  double* d_raw;
  unsigned *d_fwd, *d_bwd, *d_tot;
  if ((rc = dev_buf_t(c, "fr_axis_raw", (size_t)n * 3, &d_raw))) return rc;
  if ((rc = dev_buf_t(c, "fr_sign_fwd", (size_t)n, &d_fwd))) return rc;
  if ((rc = dev_buf_t(c, "fr_sign_bwd", (size_t)n, &d_bwd))) return rc;
  if ((rc = dev_buf_t(c, "fr_sign_totals", (size_t)frame_scan_blocks(n), &d_tot))) return rc;
  hipStream_t S = c->stream;
  Vec4 rg = {{rough[0], rough[1], rough[2], 0.0}};
  TIMED(c, BMS_TAG_POINTWISE, launch_dominant_axis(S, d_ll, n, d_raw));
  TIMED(c, BMS_TAG_POINTWISE, launch_axis_sign_maps(S, d_raw, n, anchor, rg, d_fwd, d_bwd));
  TIMED(c, BMS_TAG_POINTWISE, launch_scan_sign_maps(S, d_fwd, n - anchor, d_tot));
  TIMED(c, BMS_TAG_POINTWISE, launch_scan_sign_maps(S, d_bwd, anchor + 1, d_tot));
  TIMED(c, BMS_TAG_POINTWISE, launch_axis_apply_signs(S, d_raw, n, anchor, d_fwd, d_bwd, d_axis));
  return BMS_OK;
}

// in place on d_R f8[n][4] (device)
int minimal_rotation(bms_ctx* c, const FrameAxis& ax, int64_t n, double* d_R, int iterations) {
  int rc;
  double *d_Rdot, *d_h, *d_hs, *d_P1, *d_carry;
  if ((rc = dev_buf_t(c, "fr_Rdot", (size_t)n * 4, &d_Rdot))) return rc;
  if ((rc = dev_buf_t(c, "fr_h", (size_t)n * 2, &d_h))) return rc;
  if ((rc = dev_buf_t(c, "fr_hs", (size_t)n * 2, &d_hs))) return rc;
  if ((rc = dev_buf_t(c, "fr_P1", (size_t)n * 2, &d_P1))) return rc;
  if ((rc = dev_buf_t(c, "fr_carry", (size_t)spline_prefix_carry_size(n, 1), &d_carry))) return rc;
  hipStream_t S = c->stream;
  for (int it = 0; it < iterations; ++it) {
    if ((rc = knot_slopes(c, ax, n, d_R, 2, "fr_fw", d_Rdot))) return rc;
    TIMED(c, BMS_TAG_POINTWISE, launch_halfgammadot(S, d_R, d_Rdot, n, d_h));
    if ((rc = knot_slopes(c, ax, n, d_h, 1, "fr_fw", d_hs))) return rc;
    TIMED(c, BMS_TAG_POINTWISE, launch_spline_prefix(S, d_h, d_hs, 2, 1, n, ax.d_x, d_P1, nullptr, d_carry, 1));
    TIMED(c, BMS_TAG_POINTWISE, launch_spin_about_z(S, d_R, d_P1, n, d_R));
  }
  return BMS_OK;
}

int rotor_omega(bms_ctx* c, const FrameAxis& ax, int64_t n, const double* d_R, double* d_om) {
  int rc;
  double* d_Rdot;
  if ((rc = dev_buf_t(c, "fr_Rdot", (size_t)n * 4, &d_Rdot))) return rc;
  if ((rc = knot_slopes(c, ax, n, d_R, 2, "fr_fw", d_Rdot))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_rotor_omega(c->stream, d_R, d_Rdot, n, d_om));
  return BMS_OK;
}

// what bms_squad refuses in its two host arrays, before anything is staged
int squad_checks(bms_ctx* c, const double* t_in, int64_t n, const double* t_out, int64_t m) {
  if (n < 2) return fail(c, BMS_ERR_INVALID, "squad needs at least 2 rotors, got %lld", (long long)n);
  if (m < 0) return fail(c, BMS_ERR_INVALID, "negative number of arguments (%lld)", (long long)m);
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(t_in[i])) return fail(c, BMS_ERR_INVALID, "time array must be finite (index %lld)", (long long)i);
  for (int64_t i = 1; i < n; ++i)
    if (!(t_in[i] > t_in[i - 1])) return fail(c, BMS_ERR_INVALID, "time array must be strictly increasing (index %lld)", (long long)i);
  for (int64_t j = 0; j < m; ++j)
    if (!std::isfinite(t_out[j])) return fail(c, BMS_ERR_INVALID, "arguments must be finite (index %lld)", (long long)j);
  return BMS_OK;
}

}  // namespace

extern "C" int64_t bms_frame_scan_blocks(int64_t n) { return frame_scan_blocks(n); }

extern "C" int bms_squad(bms_ctx* c, const double* t_in, int64_t n, const void* R_in, int mem, const double* t_out, int64_t m,
                         void* out) try {
  if (!c || !t_in || !R_in || !t_out || !out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  int rc;
  if ((rc = entry_mem(c, mem)) || (rc = squad_checks(c, t_in, n, t_out, m))) return rc;
  if (m == 0) return BMS_OK;
  CallIO io(c, mem);
  void *d_t, *d_u;
  const double* d_R;
  double *d_AB, *d_out;
  if ((rc = upload(c, "times", t_in, 8 * (size_t)n, &d_t))) return rc;
  if ((rc = upload(c, "times_new", t_out, 8 * (size_t)m, &d_u))) return rc;
  if ((rc = io.in("fr_in", R_in, 8 * (size_t)n * 4, &d_R))) return rc;
  if ((rc = dev_buf_t(c, "fr_squad_AB", (size_t)n * 8, &d_AB))) return rc;
  if ((rc = io.out("fr_out", out, (size_t)m * 4, &d_out))) return rc;
  hipStream_t S = c->stream;
  TIMED(c, BMS_TAG_POINTWISE, launch_squad_control(S, d_R, (const double*)d_t, n, d_AB));
  TIMED(c, BMS_TAG_POINTWISE, launch_squad_eval(S, d_R, (const double*)d_t, n, d_AB, (const double*)d_u, m, d_out));
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_frame_from_angular_velocity(bms_ctx* c, const double* t, int64_t n, const double* omega, int mem, const double R0[4],
                                               double tolerance, double* R_out) try {
  if (!c || !t || !omega || !R0 || !R_out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  int rc;
  if ((rc = entry_mem(c, mem)) || (rc = check_time_axis(c, t, n))) return rc;
  CallIO io(c, mem);
  FrameAxis ax;
  if ((rc = frame_axis(c, t, n, ax))) return rc;
  const double* d_om;
  double* d_R;
  if ((rc = io.in("fr_in", omega, 8 * (size_t)n * 3, &d_om))) return rc;
  if ((rc = io.out("fr_out", R_out, (size_t)n * 4, &d_R))) return rc;
  if ((rc = frame_from_omega(c, ax, n, d_om, R0, tolerance, d_R))) return rc;
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_dominant_axis(bms_ctx* c, const double* ll, int64_t n, int mem, const double rough[3], int64_t rough_index,
                                 double* axis_out) try {
  if (!c || !ll || !rough || !axis_out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (int rc0 = entry_mem(c, mem)) return rc0;
  if (n < 1) return fail(c, BMS_ERR_INVALID, "need at least one time step, got %lld", (long long)n);
  if (rough_index < 0 || rough_index >= n) return fail(c, BMS_ERR_INVALID, "rough_index %lld outside [0, %lld)", (long long)rough_index, (long long)n);
  int rc;
  CallIO io(c, mem);
  const double* d_ll;
  double* d_axis;
  if ((rc = io.in("fr_in", ll, 8 * (size_t)n * 9, &d_ll))) return rc;
  if ((rc = io.out("fr_out", axis_out, (size_t)n * 3, &d_axis))) return rc;
  if ((rc = dominant_axis(c, n, d_ll, rough, rough_index, d_axis))) return rc;
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_minimal_rotation(bms_ctx* c, const double* t, int64_t n, const double* R, int mem, int iterations, double* R_out) try {
  if (!c || !t || !R || !R_out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (int rc0 = entry_mem(c, mem)) return rc0;
  if (iterations < 1) return fail(c, BMS_ERR_INVALID, "iterations must be positive, got %d", iterations);
  int rc;
  if ((rc = check_time_axis(c, t, n))) return rc;
  CallIO io(c, mem);
  FrameAxis ax;
  if ((rc = frame_axis(c, t, n, ax))) return rc;
  double* d_R;  // (R_out itself on the device, after a copy of R unless the two are one array)
  if ((rc = io.inout("fr_out", R, R_out, (size_t)n * 4, &d_R))) return rc;
  if ((rc = minimal_rotation(c, ax, n, d_R, iterations))) return rc;
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_rotor_angular_velocity(bms_ctx* c, const double* t, int64_t n, const double* R, int mem, double* omega_out) try {
  if (!c || !t || !R || !omega_out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  int rc;
  if ((rc = entry_mem(c, mem)) || (rc = check_time_axis(c, t, n))) return rc;
  CallIO io(c, mem);
  FrameAxis ax;
  if ((rc = frame_axis(c, t, n, ax))) return rc;
  const double* d_R;
  double* d_om;
  if ((rc = io.in("fr_in", R, 8 * (size_t)n * 4, &d_R))) return rc;
  if ((rc = io.out("fr_out", omega_out, (size_t)n * 3, &d_om))) return rc;
  if ((rc = rotor_omega(c, ax, n, d_R, d_om))) return rc;
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_frame_adjust(bms_ctx* c, double* frame, int64_t n, int mem, const double right[4], double truncate_tolerance,
                                double* log_out, void* spinors_out) try {
  if (!c || !frame) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (int rc0 = entry_mem(c, mem)) return rc0;
  if (n < 0) return fail(c, BMS_ERR_INVALID, "negative size");
  if (n == 0) return BMS_OK;
  double pow2 = 0.0;
  if (truncate_tolerance > 0) {
    if (!std::isfinite(truncate_tolerance)) return fail(c, BMS_ERR_INVALID, "truncate_tolerance must be finite");
    pow2 = std::exp2(-std::floor(std::log2(2 * truncate_tolerance)));
  }
  int rc;
  CallIO io(c, mem);
  double *d_frame, *d_log, *d_sp;
  if ((rc = io.inout("fr_in", frame, frame, (size_t)n * 4, &d_frame))) return rc;
  if ((rc = io.out("fr_out", log_out, (size_t)n * 4, &d_log))) return rc;
  if ((rc = io.out("fr_spinors", spinors_out, (size_t)n * 4, &d_sp))) return rc;
  Vec4 rt = {{1.0, 0.0, 0.0, 0.0}};
  if (right)
    for (int i = 0; i < 4; ++i) rt.v[i] = right[i];
  TIMED(c, BMS_TAG_POINTWISE, launch_frame_adjust(c->stream, d_frame, n, rt, right != nullptr, pow2, d_log, d_sp));
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_corotating_frame(bms_ctx* c, const double* t, int64_t n, const void* data, int64_t ld, int ell_min, int ell_max, int mem,
                                    const double R0[4], double tolerance, double* frame_dev, double* frame_out, double* omega_out) try {
  if (!c || !t || !data || !R0 || !frame_dev) return fail(c, BMS_ERR_INVALID, "NULL argument");
  int rc, n_modes;
  if ((rc = entry_mem(c, mem)) || (rc = check_time_axis(c, t, n))) return rc;
  if ((rc = modes_checks(c, ell_min, ell_max, ld, &n_modes))) return rc;
  CallIO io(c, mem);
  FrameAxis ax;
  if ((rc = frame_axis(c, t, n, ax))) return rc;
  const double* d_y;
  double* d_res;  // <Ldt>, <LL>, omega: the kernels of bms_angular_velocity, in its work space
  if ((rc = io.in("in_data", data, ((size_t)(n - 1) * ld + n_modes) * 16, &d_y))) return rc;
  if ((rc = angular_velocity_on_device(c, d_y, ld, n, ell_min, n_modes, ax.d_x, ax.d_tab, ax.tile, &d_res))) return rc;
  if ((rc = frame_from_omega(c, ax, n, d_res + 12 * n, R0, tolerance, frame_dev))) return rc;
  if ((rc = io.copy_back(frame_out, frame_dev, sizeof(double) * 4 * n))) return rc;
  if ((rc = io.copy_back(omega_out, d_res + 12 * n, sizeof(double) * 3 * n))) return rc;
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_coprecessing_frame(bms_ctx* c, const double* t, int64_t n, const void* data, int64_t ld, int ell_min, int ell_max,
                                      int mem, const double rough[3], int64_t rough_index, int iterations, double* frame_dev,
                                      double* frame_out, double* axis_out) try {
  if (!c || !data || !rough) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (int rc0 = entry_mem(c, mem)) return rc0;
  const bool want_frame = frame_dev || frame_out;
  int rc, n_modes;
  if (want_frame) {
    if (!t) return fail(c, BMS_ERR_INVALID, "NULL argument");
    if (iterations < 1) return fail(c, BMS_ERR_INVALID, "iterations must be positive, got %d", iterations);
    if ((rc = check_time_axis(c, t, n))) return rc;
  } else if (n < 1) {
    return fail(c, BMS_ERR_INVALID, "need at least one time step, got %lld", (long long)n);
  }
  if (rough_index < 0 || rough_index >= n) return fail(c, BMS_ERR_INVALID, "rough_index %lld outside [0, %lld)", (long long)rough_index, (long long)n);
  if ((rc = modes_checks(c, ell_min, ell_max, ld, &n_modes))) return rc;
  CallIO io(c, mem);
  const double* d_y;
  if ((rc = io.in("in_data", data, ((size_t)(n - 1) * ld + n_modes) * 16, &d_y))) return rc;
  double *d_ll, *d_axis;
  if ((rc = dev_buf_t(c, "av_out", (size_t)n * 15, &d_ll))) return rc;
  if ((rc = dev_buf_t(c, "fr_axis", (size_t)n * 3, &d_axis))) return rc;
  hipStream_t S = c->stream;
  // <LL> alone needs no time derivative: the kernel reads the modes in its place, and nothing of <Ldt> or omega is written
  TIMED(c, BMS_TAG_POINTWISE, launch_angular_velocity(S, d_y, d_y, 2 * ld, n, ell_min, n_modes, nullptr, d_ll, nullptr));
  if ((rc = dominant_axis(c, n, d_ll, rough, rough_index, d_axis))) return rc;
  if ((rc = io.copy_back(axis_out, d_axis, sizeof(double) * 3 * n))) return rc;
  if (want_frame) {
    FrameAxis ax;
    if ((rc = frame_axis(c, t, n, ax))) return rc;
    double* d_R = frame_dev;
    if (!d_R && (rc = dev_buf_t(c, "fr_out", (size_t)n * 4, &d_R))) return rc;
    TIMED(c, BMS_TAG_POINTWISE, launch_axis_rotor(S, d_axis, n, d_R));
    if ((rc = minimal_rotation(c, ax, n, d_R, iterations))) return rc;
    if ((rc = io.copy_back(frame_out, d_R, sizeof(double) * 4 * n))) return rc;
  }
  return io.finish();
} BMS_CATCH(c)
