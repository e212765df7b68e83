// One raw finite-radius series retarded to tortoise time and scaled by its masses and radii (scri/extrapolation.py:27-45, :356-402):
// bms_finite_radius_retard, bms_retard_tile
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI; kernels_retard.hip: the kernels)
#include "engine.h"

extern "C" int64_t bms_retard_tile(void) { return RETARD_TILE; }  // (a size, not a status: int64_t like the other tile sizes)

// what bms_finite_radius_retard refuses before it selects a device
BMS_INTERNAL int retard_checks(bms_ctx* c, const double* t, const double* areal_radius, const double* average_lapse, int64_t n_raw, const void* data,
                               int64_t ld, int n_cols, int mem, const double* frame, double coord_radius, double initial_adm_energy, double ch_mass,
                               double unit_scale, int radius_exponent, double min_time_step, const int64_t* n_kept, const double* t_out,
                               const double* radii_out, const void* data_out, int64_t ld_out, const double* frame_out) {
  const char* who = "bms_finite_radius_retard";
  if (!t || !areal_radius || !average_lapse || !data || !n_kept || !t_out || !radii_out || !data_out)
    return fail(c, BMS_ERR_INVALID, "%s: NULL series, modes or output", who);
  if (frame && !frame_out) return fail(c, BMS_ERR_INVALID, "%s: a frame without frame_out", who);
  if (n_raw < 1) return fail(c, BMS_ERR_INVALID, "%s: n_raw = %lld: at least one sample", who, (long long)n_raw);
  if (n_cols < 1 || n_cols > (1 << 26)) return fail(c, BMS_ERR_INVALID, "%s: n_cols = %d outside [1, 2^26]", who, n_cols);
  if (ld < n_cols || ld_out < n_cols)
    return fail(c, BMS_ERR_INVALID, "%s: row strides %lld and %lld smaller than the number of columns (%d)", who, (long long)ld, (long long)ld_out, n_cols);
  if (retard_tiles(n_raw) > 0x7fffffffLL) return fail(c, BMS_ERR_INVALID, "%s: n_raw = %lld is beyond 2^31 tiles", who, (long long)n_raw);
  if (radius_exponent < 1 || radius_exponent > 5) return fail(c, BMS_ERR_INVALID, "%s: radius_exponent = %d outside 1 .. 5", who, radius_exponent);
  if (ch_mass == 0 || std::isnan(ch_mass)) return fail(c, BMS_ERR_INVALID, "%s: ch_mass = %g is not a valid mass", who, ch_mass);
  if (!std::isfinite(coord_radius) || coord_radius <= 0) return fail(c, BMS_ERR_INVALID, "%s: coord_radius = %g must be finite and positive", who, coord_radius);
  if (!std::isfinite(initial_adm_energy) || initial_adm_energy <= 0)
    return fail(c, BMS_ERR_INVALID, "%s: initial_adm_energy = %g must be finite and positive", who, initial_adm_energy);
  if (!(min_time_step >= 0)) return fail(c, BMS_ERR_INVALID, "%s: min_time_step = %g is negative", who, min_time_step);
  if (std::isnan(unit_scale)) return fail(c, BMS_ERR_INVALID, "%s: unit_scale is NaN", who);
  if (mem == BMS_DEVICE && ((((uintptr_t)data | (uintptr_t)data_out | (uintptr_t)frame | (uintptr_t)frame_out)) & 15))
    return fail(c, BMS_ERR_INVALID, "%s: device arrays must be aligned to 16 bytes", who);
  for (int64_t k = 0; k < n_raw; ++k)  // (a time that is not finite would be kept or dropped by no rule of the reference's)
    if (!std::isfinite(t[k])) return fail(c, BMS_ERR_INVALID, "%s: t[%lld] is not finite", who, (long long)k);
  return BMS_OK;
}

extern "C" int bms_finite_radius_retard(bms_ctx* c, const double* t, const double* areal_radius, const double* average_lapse, int64_t n_raw,
                                        const void* data, int64_t ld, int n_cols, int mem, const double* frame, double coord_radius,
                                        double initial_adm_energy, double ch_mass, double unit_scale, int radius_exponent, double min_time_step,
                                        int64_t* n_kept, double* t_out, double* radii_out, void* data_out, int64_t ld_out, double* frame_out) try {
  if (!c) return BMS_ERR_INVALID;
  const char* who = "bms_finite_radius_retard";
  if (int rc0 = entry_mem(c, mem, who, false)) return rc0;  // (the argument checks come before the device is selected)
  int rc;
  if ((rc = retard_checks(c, t, areal_radius, average_lapse, n_raw, data, ld, n_cols, mem, frame, coord_radius, initial_adm_energy, ch_mass,
                          unit_scale, radius_exponent, min_time_step, n_kept, t_out, radii_out, data_out, ld_out, frame_out)))
    return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t S = c->stream;
  CallIO io(c, mem);
  const size_t n = (size_t)n_raw, tiles = (size_t)retard_tiles(n_raw);
  void *v_t, *v_r, *v_l;
  if ((rc = upload(c, "rt_t", t, 8 * n, &v_t))) return rc;
  if ((rc = upload(c, "rt_r", areal_radius, 8 * n, &v_r))) return rc;
  if ((rc = upload(c, "rt_l", average_lapse, 8 * n, &v_l))) return rc;
  const double *d_t = (const double*)v_t, *d_r = (const double*)v_r, *d_l = (const double*)v_l;
  const double2 *d_in, *d_fin = nullptr;  // (a host series goes up in one piece, with its row stride)
  if ((rc = io.in("rt_in", data, 16 * ((n - 1) * (size_t)ld + (size_t)n_cols), &d_in))) return rc;
  if (frame && (rc = io.in("rt_frame_in", frame, 32 * n, &d_fin))) return rc;
  double *d_tile, *d_tout, *d_rout, *d_f, *d_tot;
  int* d_rank;
  long long *d_count, *d_idx, *d_st;
  if ((rc = dev_buf_t(c, "rt_tile", tiles, &d_tile))) return rc;
  if ((rc = dev_buf_t(c, "rt_rank", n, &d_rank))) return rc;
  if ((rc = dev_buf_t(c, "rt_count", tiles, &d_count))) return rc;
  if ((rc = dev_buf_t(c, "rt_idx", n, &d_idx))) return rc;
  if ((rc = dev_buf_t(c, "rt_st", (size_t)4, &d_st))) return rc;
  if ((rc = dev_buf_t(c, "rt_tot", 2 * tiles, &d_tot))) return rc;
  if ((rc = dev_buf_t(c, "rt_tout", n, &d_tout))) return rc;
  if ((rc = dev_buf_t(c, "rt_rout", n, &d_rout))) return rc;
  if ((rc = dev_buf_t(c, "rt_f", n, &d_f))) return rc;
  double2 *d_out, *d_fout = nullptr;
  if ((rc = io.out_rows("rt_out", data_out, n, (size_t)n_cols, (size_t)ld_out, &d_out))) return rc;
  if (frame && (rc = io.out("rt_frame_out", frame_out, 2 * n, &d_fout))) return rc;
  const long long ld_dev = io.host() ? n_cols : ld_out;
  TIMED(c, BMS_TAG_POINTWISE, launch_retard_keep(S, d_t, n_raw, min_time_step, d_tile, d_rank, d_count, d_idx, d_st));
  TIMED(c, BMS_TAG_POINTWISE, launch_retard_time(S, d_t, d_r, d_l, n_raw, d_idx, d_st, initial_adm_energy, coord_radius, ch_mass, unit_scale,
                                                 radius_exponent, d_tot, d_tout, d_rout, d_f));
  TIMED(c, BMS_TAG_POINTWISE, launch_retard_gather(S, d_in, ld, n_cols, n_raw, d_idx, d_f, d_st, d_out, ld_dev));
  if (frame) TIMED(c, BMS_TAG_POINTWISE, launch_retard_gather(S, d_fin, 2, 2, n_raw, d_idx, nullptr, d_st, d_fout, 2));
  long long st[3] = {0, 0, 0};
  if ((rc = io.copy_back(st, d_st, sizeof(st)))) return rc;
  if ((rc = io.copy_back(t_out, d_tout, 8 * n))) return rc;
  if ((rc = io.copy_back(radii_out, d_rout, 8 * n))) return rc;
  if ((rc = io.finish())) return rc;
  *n_kept = st[0];
  if (st[1])
    return fail(c, BMS_ERR_INVALID, "%s: %lld kept radii are not finite or not beyond 2 E = %g: the first is areal_radius[%lld] = %g", who, st[1],
                2 * initial_adm_energy, st[2], areal_radius[st[2]]);
  return BMS_OK;
} BMS_CATCH(c)
