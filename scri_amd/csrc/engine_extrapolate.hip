// Extrapolation to null infinity: bms_extrapolate, the per-time-step polynomial fit in 1/r of scri/extrapolation.py:1394-1434
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI; kernels_extrapolate.hip: the arithmetic)
#include "engine.h"

extern "C" int bms_extrapolate(bms_ctx* c, int n_radii, const void* const* series, const int64_t* ld, int mem, int64_t n_times,
                               int64_t n_modes, const double* radii, int n_orders, const int* orders, void* out, int blocks,
                               int64_t* n_deficient) try {
  if (!c) return BMS_ERR_INVALID;
  if (!valid_mem(mem)) return fail(c, BMS_ERR_INVALID, "mem is BMS_HOST or BMS_DEVICE, got %d", mem);
  HIP_TRY(c, hipSetDevice(c->device));
  if (n_radii < 1) return fail(c, BMS_ERR_INVALID, "n_radii = %d: need at least one radius", n_radii);
  if (n_radii > EXTRAP_MAX_RADII) return fail(c, BMS_ERR_UNSUPPORTED, "n_radii = %d is beyond %d", n_radii, EXTRAP_MAX_RADII);
  if (n_times < 0 || n_modes < 0 || n_modes > (1 << 26) || n_orders < 0) return fail(c, BMS_ERR_INVALID, "bad sizes");
  if (n_orders > 0 && !orders) return fail(c, BMS_ERR_INVALID, "NULL orders");
  for (int o = 0; o < n_orders; ++o) {
    if (orders[o] < 0 || orders[o] >= n_radii)
      return fail(c, BMS_ERR_INVALID, "order %d of the fit needs %d radii, got %d", orders[o], orders[o] + 1, n_radii);
    if (orders[o] > EXTRAP_MAX_ORDER) return fail(c, BMS_ERR_UNSUPPORTED, "order %d is beyond %d", orders[o], EXTRAP_MAX_ORDER);
  }
  if (!series || !ld) return fail(c, BMS_ERR_INVALID, "NULL series or row strides");
  for (int i = 0; i < n_radii; ++i)
    if (ld[i] < n_modes) return fail(c, BMS_ERR_INVALID, "row stride %lld of radius %d smaller than %lld modes", (long long)ld[i], i, (long long)n_modes);
  if (n_deficient)
    for (int o = 0; o < n_orders; ++o) n_deficient[o] = 0;
  if (n_times == 0 || n_modes == 0 || n_orders == 0) return BMS_OK;
  for (int i = 0; i < n_radii; ++i)
    if (!series[i]) return fail(c, BMS_ERR_INVALID, "NULL series of radius %d", i);
  if (!radii || !out) return fail(c, BMS_ERR_INVALID, "NULL radii or output");
  unsigned long long* d_def = nullptr;
  int rc = dev_buf_t(c, "extrap_deficient", (size_t)n_orders, &d_def);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(d_def, 0, sizeof(unsigned long long) * n_orders, c->stream));
  auto finish = [&]() -> int {  // the counts come home (and the staged source table may go)
    std::vector<unsigned long long> def(n_orders);
    HIP_TRY(c, hipMemcpyAsync(def.data(), d_def, sizeof(unsigned long long) * n_orders, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n_deficient)
      for (int o = 0; o < n_orders; ++o) n_deficient[o] = (int64_t)def[o];
    return BMS_OK;
  };
  if (mem == BMS_DEVICE) {
    std::vector<ExtrapSource> src(n_radii);
    for (int i = 0; i < n_radii; ++i) src[i] = {(const double2*)series[i], (long long)ld[i]};
    void* vp;
    if ((rc = upload(c, "extrap_src", src.data(), sizeof(ExtrapSource) * n_radii, &vp))) return rc;
    TIMED(c, BMS_TAG_POINTWISE, launch_extrapolate(c->stream, (const ExtrapSource*)vp, n_radii, radii, n_times, n_times, (int)n_modes, orders,
                                                   n_orders, (double2*)out, n_times * n_modes, d_def));
    return finish();
  }
  // Host memory: blocks of time steps go up, are fitted and come back on three streams (run_host_pipeline).  Every step is
  // independent -- no halo -- and a step's arithmetic does not depend on the block it is in, so any number of blocks gives the
  // one-block result to the bit.  blocks = 0: blocks of >= 12 MB of input, at most 16 of them, as the rotations of host series.
  const size_t in_bytes = (size_t)n_times * n_modes * 16 * n_radii;
  if (blocks <= 0) blocks = (int)std::max<size_t>(1, std::min<size_t>(16, in_bytes / (12u << 20)));
  blocks = (int)std::min<int64_t>(blocks, n_times);
  const int64_t rows_max = (n_times + blocks - 1) / blocks;
  const size_t slot_modes = (size_t)rows_max * n_modes;  // c16 per radius (input) or per order (output) in one slot
  double2 *d_in[2], *d_out[2];
  double* d_r[2];
  for (int s = 0; s < 2; ++s) {
    if ((rc = dev_buf_t(c, s ? "extrap_in1" : "extrap_in0", slot_modes * n_radii, &d_in[s]))) return rc;
    if ((rc = dev_buf_t(c, s ? "extrap_out1" : "extrap_out0", slot_modes * n_orders, &d_out[s]))) return rc;
    if ((rc = dev_buf_t(c, s ? "extrap_r1" : "extrap_r0", (size_t)rows_max * n_radii, &d_r[s]))) return rc;
  }
  std::vector<ExtrapSource> src(2 * (size_t)n_radii);
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < n_radii; ++i) src[(size_t)s * n_radii + i] = {d_in[s] + i * slot_modes, (long long)n_modes};
  void* vp;
  if ((rc = upload(c, "extrap_src", src.data(), sizeof(ExtrapSource) * src.size(), &vp))) return rc;
  const ExtrapSource* d_src = (const ExtrapSource*)vp;
  auto row0 = [&](int k) { return n_times * k / blocks; };
  const size_t row_bytes = (size_t)n_modes * 16;
  const char* err = "extrapolation of host series in blocks";
  rc = run_host_pipeline(
      c, 0, blocks, false, false, err, err,
      [&](int k, int slot) -> hipError_t {
        const int64_t r0 = row0(k), rows = row0(k + 1) - r0;
        for (int i = 0; i < n_radii; ++i) {
          hipError_t e = hipMemcpy2DAsync(d_in[slot] + i * slot_modes, row_bytes, (const char*)series[i] + (size_t)r0 * ld[i] * 16,
                                          (size_t)ld[i] * 16, row_bytes, (size_t)rows, hipMemcpyHostToDevice, c->pipe_up);
          if (e != hipSuccess) return e;
        }
        return hipMemcpy2DAsync(d_r[slot], (size_t)rows_max * 8, radii + r0, (size_t)n_times * 8, (size_t)rows * 8, (size_t)n_radii,
                                hipMemcpyHostToDevice, c->pipe_up);
      },
      [&](int k, int slot) -> int {
        const int64_t rows = row0(k + 1) - row0(k);
        TIMED(c, BMS_TAG_POINTWISE, launch_extrapolate(c->stream, d_src + (size_t)slot * n_radii, n_radii, d_r[slot], rows_max, rows,
                                                       (int)n_modes, orders, n_orders, d_out[slot], (long long)slot_modes, d_def));
        return BMS_OK;
      },
      [&](int k, int slot) -> hipError_t {
        const int64_t r0 = row0(k), rows = row0(k + 1) - r0;
        for (int o = 0; o < n_orders; ++o) {
          hipError_t e = hipMemcpyAsync((char*)out + ((size_t)o * n_times + r0) * row_bytes, d_out[slot] + o * slot_modes,
                                        (size_t)rows * row_bytes, hipMemcpyDeviceToHost, c->pipe_down);
          if (e != hipSuccess) return e;
        }
        return hipSuccess;
      });
  if (rc) return rc;
  return finish();
} BMS_CATCH(c)
