// Centre-of-mass track of the horizon (or star) trajectories and the fit of its average drift (kernels_com.hip): the two entries behind
// scri_amd/com_motion.py
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI)
#include "engine.h"

// (a size, not a status: entries that return `int` return a status, negative on failure)
extern "C" int64_t bms_com_fit_tile_panels(void) { return COM_FIT_TILE; }

extern "C" int bms_com_motion(bms_ctx* c, const double* t, const double* x_a, const double* x_b, const double* m_a, int64_t n_m_a,
                              const double* m_b, int64_t n_m_b, int64_t n, int matter, int mem, double* t_out, double* com_out) try {
  if (!c) return BMS_ERR_INVALID;
  if (!x_a || !x_b || !m_a || !m_b || !com_out || (matter && (!t || !t_out))) return fail(c, BMS_ERR_INVALID, "bms_com_motion: NULL argument");
  if (int rc0 = entry_mem(c, mem, "bms_com_motion", false)) return rc0;  // (the size checks come before the device is selected)
  if (n < 1) return fail(c, BMS_ERR_INVALID, "bms_com_motion: need at least one sample, got %lld", (long long)n);
  if ((n_m_a != 1 && n_m_a != n) || (n_m_b != 1 && n_m_b != n))
    return fail(c, BMS_ERR_INVALID, "bms_com_motion: a mass is one value or one per sample (%lld), got %lld and %lld", (long long)n, (long long)n_m_a,
                (long long)n_m_b);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  CallIO io(c, mem);
  const double *d_t = t, *d_xa, *d_xb, *d_ma, *d_mb;
  if ((rc = io.in("com_xa", x_a, (size_t)n * 24, &d_xa))) return rc;
  if ((rc = io.in("com_xb", x_b, (size_t)n * 24, &d_xb))) return rc;
  if ((rc = io.in("com_ma", m_a, (size_t)n_m_a * 8, &d_ma))) return rc;
  if ((rc = io.in("com_mb", m_b, (size_t)n_m_b * 8, &d_mb))) return rc;
  if (matter && (rc = io.in("com_t", t, (size_t)n * 8, &d_t))) return rc;
  double *d_com, *d_tout = t_out;
  if ((rc = io.out("com_track", com_out, (size_t)n * 3, &d_com))) return rc;
  if (matter && (rc = io.out("com_tout", t_out, (size_t)n, &d_tout))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_com_track(c->stream, d_t, d_xa, d_xb, d_ma, n_m_a, d_mb, n_m_b, n, matter, d_tout, d_com));
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_com_fit(bms_ctx* c, const double* t, const double* com, int64_t n, int mem, double skip_beginning_fraction,
                           double skip_ending_fraction, int fit_acceleration, bms_com_fit_result* result) try {
  if (!c) return BMS_ERR_INVALID;
  if (!t || !com || !result) return fail(c, BMS_ERR_INVALID, "bms_com_fit: NULL argument");
  if (int rc0 = entry_mem(c, mem, "bms_com_fit", false)) return rc0;
  if (n < 2) return fail(c, BMS_ERR_INVALID, "bms_com_fit: need at least 2 samples, got %lld", (long long)n);
  if (!std::isfinite(skip_beginning_fraction) || !std::isfinite(skip_ending_fraction))
    return fail(c, BMS_ERR_INVALID, "bms_com_fit: the skip fractions must be finite, got %g and %g", skip_beginning_fraction, skip_ending_fraction);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  CallIO io(c, mem);
  const double *d_t, *d_com;
  if ((rc = io.in("com_t", t, (size_t)n * 8, &d_t))) return rc;
  if ((rc = io.in("com_track", com, (size_t)n * 24, &d_com))) return rc;
  double *d_work, *d_out;
  if ((rc = dev_buf_t(c, "com_work", (size_t)com_fit_work_doubles(n), &d_work))) return rc;
  if ((rc = dev_buf_t(c, "com_out", (size_t)COM_FIT_OUT, &d_out))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_com_fit(c->stream, d_t, d_com, n, skip_beginning_fraction, skip_ending_fraction, fit_acceleration != 0, d_work, d_out));
  double out[COM_FIT_OUT];
  if ((rc = io.copy_back(out, d_out, sizeof(out))) || (rc = io.finish())) return rc;
  for (int k = 0; k < 3; ++k) {
    result->x_i[k] = out[k], result->v_i[k] = out[3 + k], result->a_i[k] = out[6 + k];
    for (int m = 0; m < 3; ++m) result->moments[m][k] = out[13 + 3 * m + k];
  }
  result->t_i = out[9], result->t_f = out[10];
  result->i_i = (int64_t)out[11], result->i_f = (int64_t)out[12];
  if (out[22] == 1.0)
    return fail(c, BMS_ERR_INVALID, "bms_com_fit: the window [%lld, %lld] between t_i = %.17g and t_f = %.17g holds fewer than two samples",
                (long long)result->i_i, (long long)result->i_f, result->t_i, result->t_f);
  if (out[22] == 2.0) return fail(c, BMS_ERR_INVALID, "bms_com_fit: t_f equals t_i = %.17g: the fit divides by their difference", result->t_i);
  return BMS_OK;
} BMS_CATCH(c)
