// Time-and-phase alignment of two waveforms from correlation moments (kernels_align.hip): the two stateless entries behind the
// device route of scri_amd/alignment.py
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI)
#include "engine.h"

namespace {

constexpr size_t ALIGN_PARTIAL_BYTES = 128u << 20;  // work space of one launch: longer offset lists go through in slices

struct AlignHost {  // the arguments the two entries share, as the caller gave them
  const double* ta;
  int64_t na;
  const void *ya, *sa;
  int64_t ld_a;
  const int32_t* col_a;
  const double *tw, *w;
  int64_t nw;
  const void* b;
  int64_t ld_b;
  const int32_t* col_b;
  int n_cols, mem;
};

int align_increasing(bms_ctx* c, const char* what, const double* t, int64_t n) {
  if (!std::isfinite(t[0])) return fail(c, BMS_ERR_INVALID, "%s must be finite (index 0)", what);
  for (int64_t i = 1; i < n; ++i)
    if (!std::isfinite(t[i]) || !(t[i] > t[i - 1])) return fail(c, BMS_ERR_INVALID, "%s must be finite and strictly increasing (index %lld)", what, (long long)i);
  return BMS_OK;
}

int align_checks(bms_ctx* c, const AlignHost& h) {
  if (!c || !h.ta || !h.ya || !h.sa || !h.col_a || !h.tw || !h.w || !h.b || !h.col_b) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (int rc0 = entry_mem(c, h.mem, nullptr, false)) return rc0;  // (the device is selected once every check has passed)
  if (h.n_cols <= 0) return fail(c, BMS_ERR_INVALID, "need at least one common column, got %d", h.n_cols);
  if (h.nw < 2) return fail(c, BMS_ERR_INVALID, "the window needs at least 2 rows, got %lld", (long long)h.nw);
  if (h.na < 4) return fail(c, BMS_ERR_INVALID, "the spline of the moving waveform needs at least 4 time steps, got %lld", (long long)h.na);
  if (h.na > ALIGN_MAX_KNOTS) return fail(c, BMS_ERR_UNSUPPORTED, "a moving waveform of %lld time steps is beyond %lld", (long long)h.na, (long long)ALIGN_MAX_KNOTS);
  if (h.ld_a < 1 || h.ld_b < 1) return fail(c, BMS_ERR_INVALID, "row strides must be positive");
  for (int k = 0; k < h.n_cols; ++k)
    if (h.col_a[k] < 0 || h.col_a[k] >= h.ld_a || h.col_b[k] < 0 || h.col_b[k] >= h.ld_b)
      return fail(c, BMS_ERR_INVALID, "column table entry %d lies outside its row", k);
  int rc;
  if ((rc = align_increasing(c, "the time axis of the moving waveform", h.ta, h.na))) return rc;
  if ((rc = align_increasing(c, "the window times", h.tw, h.nw))) return rc;
  for (int64_t i = 0; i < h.nw; ++i)
    if (!std::isfinite(h.w[i])) return fail(c, BMS_ERR_INVALID, "the weights must be finite (index %lld)", (long long)i);
  return BMS_OK;
}

// the small host arrays of a call, packed into one upload each: doubles (ta, tw, w, extra) and ints (col_a, col_b, extra)
int align_stage(bms_ctx* c, CallIO& io, const AlignHost& h, const double* extra_d, int64_t n_extra_d, const int32_t* extra_i, int n_extra_i,
                std::vector<double>& pack_d, std::vector<int32_t>& pack_i, AlignSeries& a, const double** d_extra_d, const int** d_extra_i) {
  pack_d.clear(), pack_i.clear();
  pack_d.insert(pack_d.end(), h.ta, h.ta + h.na);
  pack_d.insert(pack_d.end(), h.tw, h.tw + h.nw);
  pack_d.insert(pack_d.end(), h.w, h.w + h.nw);
  if (pack_d.size() & 1) pack_d.push_back(0.0);  // (the extra array may hold complex numbers: 16-byte aligned)
  const size_t extra_at = pack_d.size();
  if (n_extra_d) pack_d.insert(pack_d.end(), extra_d, extra_d + n_extra_d);
  pack_i.insert(pack_i.end(), h.col_a, h.col_a + h.n_cols);
  pack_i.insert(pack_i.end(), h.col_b, h.col_b + h.n_cols);
  if (n_extra_i) pack_i.insert(pack_i.end(), extra_i, extra_i + n_extra_i);
  int rc;
  void *vd, *vi;
  if ((rc = upload(c, "al_axes", pack_d.data(), sizeof(double) * pack_d.size(), &vd))) return rc;
  if ((rc = upload(c, "al_tables", pack_i.data(), sizeof(int32_t) * pack_i.size(), &vi))) return rc;
  const double* dd = (const double*)vd;
  const int* di = (const int*)vi;
  a.ta = dd, a.na = h.na, a.tw = dd + h.na, a.w = dd + h.na + h.nw, a.nw = h.nw;
  *d_extra_d = dd + extra_at;
  a.col_a = di, a.col_b = di + h.n_cols, a.n_cols = h.n_cols;
  *d_extra_i = di + 2 * h.n_cols;
  a.ld_a = h.ld_a, a.ld_b = h.ld_b;
  // the bulk buffers: only the columns up to the last one a table names are read
  int top_a = 0, top_b = 0;
  for (int k = 0; k < h.n_cols; ++k) top_a = std::max(top_a, (int)h.col_a[k]), top_b = std::max(top_b, (int)h.col_b[k]);
  const double *dy, *ds, *db;
  const size_t bytes_a = ((size_t)(h.na - 1) * h.ld_a + top_a + 1) * 16, bytes_b = ((size_t)(h.nw - 1) * h.ld_b + top_b + 1) * 16;
  if ((rc = io.in("al_values", h.ya, bytes_a, &dy))) return rc;
  if ((rc = io.in("al_slopes", h.sa, bytes_a, &ds))) return rc;
  if ((rc = io.in("al_fixed", h.b, bytes_b, &db))) return rc;
  a.Y = reinterpret_cast<const double2*>(dy), a.S = reinterpret_cast<const double2*>(ds), a.B = reinterpret_cast<const double2*>(db);
  return BMS_OK;
}

}  // namespace

extern "C" int bms_align_moments(bms_ctx* c, const double* ta, int64_t na, const void* ya, const void* sa, int64_t ld_a, const int32_t* col_a,
                                 const double* tw, const double* w, int64_t nw, const void* b, int64_t ld_b, const int32_t* col_b, int n_cols,
                                 const int32_t* m_slot, int n_slots, int mem, const double* dts, int64_t nd, int order, double* out) try {
  const AlignHost h = {ta, na, ya, sa, ld_a, col_a, tw, w, nw, b, ld_b, col_b, n_cols, mem};
  int rc;
  if ((rc = align_checks(c, h))) return rc;
  if (!m_slot || !dts || !out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (order < 0 || order > 2) return fail(c, BMS_ERR_INVALID, "order is 0, 1 or 2, got %d", order);
  if (n_slots < 1) return fail(c, BMS_ERR_INVALID, "need at least one slot, got %d", n_slots);
  if (n_slots > ALIGN_MAX_SLOTS) return fail(c, BMS_ERR_UNSUPPORTED, "%d slots are beyond %d", n_slots, ALIGN_MAX_SLOTS);
  for (int k = 0; k < n_cols; ++k)
    if (m_slot[k] < 0 || m_slot[k] >= n_slots) return fail(c, BMS_ERR_INVALID, "m_slot[%d] = %d outside [0, %d)", k, (int)m_slot[k], n_slots);
  if (nd < 0) return fail(c, BMS_ERR_INVALID, "negative size");
  for (int64_t k = 0; k < nd; ++k) {
    if (!std::isfinite(dts[k])) return fail(c, BMS_ERR_INVALID, "offsets must be finite (index %lld)", (long long)k);
    if (k && dts[k] < dts[k - 1]) return fail(c, BMS_ERR_INVALID, "offsets must be sorted (index %lld)", (long long)k);
  }
  if (nd == 0) return BMS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  CallIO io(c, mem);
  std::vector<double> pack_d;
  std::vector<int32_t> pack_i;
  AlignSeries a;
  const double* d_dts;
  const int* d_slot;
  if ((rc = align_stage(c, io, h, dts, nd, m_slot, n_cols, pack_d, pack_i, a, &d_dts, &d_slot))) return rc;
  const int nv = 1 + 2 * n_slots, n_ord = order + 1;
  // a launch covers as many offsets as its partial sums have room for; an offset's moments do not depend on the cut
  const size_t per_offset = (size_t)align_row_tiles(nw) * n_ord * nv * sizeof(double);
  int64_t slice = (int64_t)(ALIGN_PARTIAL_BYTES / per_offset) / ALIGN_TILE_OFFSETS * ALIGN_TILE_OFFSETS;
  slice = std::min<int64_t>(std::max<int64_t>(slice, ALIGN_TILE_OFFSETS), nd);
  double *d_partial, *d_out;
  if ((rc = dev_buf_t(c, "al_partial", per_offset / sizeof(double) * (size_t)slice, &d_partial))) return rc;
  if ((rc = dev_buf_t(c, "al_out", (size_t)n_ord * nd * nv, &d_out))) return rc;
  for (int64_t d0 = 0; d0 < nd; d0 += slice)
    TIMED(c, BMS_TAG_POINTWISE, launch_align_moments(c->stream, a, d_slot, n_slots, d_dts + d0, std::min(slice, nd - d0), d0, nd, order, d_partial, d_out));
  if ((rc = io.copy_back(out, d_out, sizeof(double) * n_ord * nd * nv))) return rc;
  return io.finish();
} BMS_CATCH(c)

extern "C" int bms_align_residual(bms_ctx* c, const double* ta, int64_t na, const void* ya, const void* sa, int64_t ld_a, const int32_t* col_a,
                                  const double* tw, const double* w, int64_t nw, const void* b, int64_t ld_b, const int32_t* col_b, int n_cols,
                                  const int32_t* m_of, int mem, double dt, double dphi, double out[2]) try {
  const AlignHost h = {ta, na, ya, sa, ld_a, col_a, tw, w, nw, b, ld_b, col_b, n_cols, mem};
  int rc;
  if ((rc = align_checks(c, h))) return rc;
  if (!m_of || !out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (!std::isfinite(dt) || !std::isfinite(dphi)) return fail(c, BMS_ERR_INVALID, "the offset and the turn must be finite");
  HIP_TRY(c, hipSetDevice(c->device));
  CallIO io(c, mem);
  std::vector<double> pack_d, phase(2 * (size_t)n_cols);
  std::vector<int32_t> pack_i;
  for (int k = 0; k < n_cols; ++k) phase[2 * k] = std::cos(m_of[k] * dphi), phase[2 * k + 1] = std::sin(m_of[k] * dphi);
  AlignSeries a;
  const double* d_phase;
  const int* d_none;
  if ((rc = align_stage(c, io, h, phase.data(), 2 * (int64_t)n_cols, nullptr, 0, pack_d, pack_i, a, &d_phase, &d_none))) return rc;
  double *d_partial, *d_out;
  if ((rc = dev_buf_t(c, "al_partial", (size_t)2 * align_row_tiles(nw), &d_partial))) return rc;
  if ((rc = dev_buf_t(c, "al_out", (size_t)2, &d_out))) return rc;
  TIMED(c, BMS_TAG_POINTWISE, launch_align_residual(c->stream, a, d_phase, dt, d_partial, d_out));
  if ((rc = io.copy_back(out, d_out, sizeof(double) * 2))) return rc;
  return io.finish();
} BMS_CATCH(c)
