// Internal header of the engine (the host side of libscri_amd.so): the context, its work space and plans, the timing and error
// macros, the tables of one transformation, and the helpers the entry-point families share.  The C ABI is include/scri_amd.h; this
// file is not installed.  The engine is split by entry family:
//   engine_context.hip   context, work-space slab, route options, page-locked host memory, timing            (bms_ctx_*, bms_host_*)
//   engine_tables.hip    planners: per-direction tables, output window, shard plan, time-axis checks, analysis / synthesis plans; the set-up
//                        steps both transforms take (knot tables, chunk plan, rotation into the grid frame, evaluating product's arguments)
//   engine_rotate.hip    rotations of the decomposition basis                                               (bms_rotate_*, bms_wigner_D)
//   engine_modes.hip     WaveformModes transform: one call, shard, pipelined, series, grid                   (bms_transform_modes*, ...)
//   engine_abd.hip       AsymptoticBondiData transform                                                       (bms_transform_abd*)
//   engine_blocks.hip    building blocks, series and bit operators               (bms_rotor_grid ... bms_grid_multiply, bms_xor_timeseries ...)
//   engine_frames.hip    corotating / coprecessing frames built on the device, rotor interpolation           (bms_corotating_frame ..., bms_dominant_axis ..., bms_squad)
//   engine_align.hip     time-and-phase alignment from correlation moments                                   (bms_align_moments, bms_align_residual)
//   engine_sample.hip    the precessing sample waveform and its finite-radius family                         (bms_precessing_waveform, bms_radius_terms)
//   engine_com.hip       centre-of-mass track of the horizon trajectories and the fit of its drift           (bms_com_motion, bms_com_fit)
//   engine_flux.hip      the four fluxes in one pass over the modes, sparse expectation values, brackets of a pair, Bondi charges (bms_poincare_fluxes, bms_expectation_values, bms_pair_brackets, bms_bondi_charges)
//   engine_product.hip   products of two mode rows on Gauss-Legendre rows, mass aspect and supermomenta          (bms_mode_product, bms_supermomenta, bms_bondi_constraints, bms_bianchi_rhs, bms_product_tables)
//   engine_cut.hip       a series of modes and its conformal factor on a supertranslated cut, the alpha perturbation   (bms_supermomentum_on_cut, bms_alpha_perturbation)
//   engine_retard.hip    one raw finite-radius series retarded to tortoise time and scaled                      (bms_finite_radius_retard)
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/scri_amd.h"
#include "kernels.h"
#include "pixel_math.h"
#include "wigner.h"

using namespace bms;

#define BMS_INTERNAL __attribute__((visibility("hidden")))

// ====================================================================================================== context

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int slab = -1;  // >= 0: carved from that reserved slab (bms_ctx_reserve) at offset `slab_off`, not an allocation of its own
  size_t slab_off = 0;
};
struct Slab {  // one device allocation that the named work-space buffers are carved from (first fit, free regions coalesced)
  char* base = nullptr;
  size_t cap = 0;
  std::map<size_t, size_t> free;  // offset -> length
  bool take(size_t want, size_t* off) {
    for (auto it = free.begin(); it != free.end(); ++it)
      if (it->second >= want) {
        *off = it->first;
        const size_t rest = it->second - want;
        free.erase(it);
        if (rest) free[*off + want] = rest;
        return true;
      }
    return false;
  }
  void give(size_t off, size_t len) {
    auto nx = free.lower_bound(off);
    if (nx != free.end() && off + len == nx->first) {
      len += nx->second;
      nx = free.erase(nx);
    }
    if (nx != free.begin()) {
      auto pv = std::prev(nx);
      if (pv->first + pv->second == off) {
        pv->second += len;
        return;
      }
    }
    free[off] = len;
  }
};

// ---------------------------------------------------------------------------------------------- analysis plan
// Separable analysis (kernels_analysis.hip) when n_theta <= MAX_THETA_SEPARABLE, dense quadrature GEMM otherwise.
struct AnalysisPlan {
  bool separable = true;
  bool fused = false;  // single-kernel analysis (kernels_analysis.hip, analysis_fused_kernel)
  bool large = false;  // folded phi-DFT + MFMA theta quadrature for grids too large for the fused kernel
  int ell_min_out = 0;
  int spin = 0;
  double* d_dcs = nullptr;
  int n_theta = 0, n_phi = 0, n_pix = 0, n_out = 0, L = 0, nm = 0;
  // separable
  double* d_dft = nullptr;
  long long ld_dft = 0;
  double* d_T = nullptr;
  int* d_mindex = nullptr;
  // dense
  double* d_W = nullptr;
  long long ldw = 0;
};

// separable synthesis of boost-free transformations (kernels_synthesis.hip)
struct SynthesisPlan {
  SynGeom g;
  int nt = 0;          // != 0: the one-kernel form takes the shape (synthesis_split_kernel)
  bool large = false;  // the two-kernel form does (kernels_synthesis_large.hip)
  int n_theta = 0, n_phi = 0, ell_min = 0, ell_max = 0;
  size_t lds = 0;
  double* d_T = nullptr;  // [n_modes][n_theta] sLambda_lm(theta_j)
  int* d_meta = nullptr;
};

// ---------------------------------------------------------------------------------------------- set-up kept across calls
// What a transformation sets up before its first heavy kernel depends on the time axis and on the pair (transformation, field
// description) only, and a caller transforms h, Psi4 ... sigma with one transformation on one axis.  The context keeps
// ONE entry of each kind from the last call that built it, found again BY CONTENT (never by address), in device blocks of their own
// names ("tc_*", "pc_*") that no other route writes.  Route option NO_PLAN_CACHE switches both off; bms_ctx_set_option drops them.
constexpr int64_t TIME_CACHE_MAX_SAMPLES = 1 << 21;   // 16 MiB of samples on the host, 200 bytes per sample on the device
constexpr size_t SETUP_CACHE_MAX_BYTES = 256u << 20;  // per-direction block / synthesis matrices: larger ones are rebuilt by every call

struct PixelTables {
  int n_theta = 0, n_phi = 0, n_pix = 0;
  std::vector<Quat> R;
  std::vector<double> k, alpha, skew_a, skew_b;
  double beta = 0, gamma = 1, tt = 0;
  bool nontrivial = false;  // beta != 0 or any supertranslation mode beyond l = 0 nonzero
  double uprm_scale_min = 0, uprm_scale_max = 0;
};

struct DevPixel {
  double *rotors, *k, *alpha, *skew_a, *skew_b, *col_off, *col_scale, *xa, *xb, *ethk, *etha, *ethetha, *ik, *ik3;
  const int* col_of_pixel = nullptr;  // set when the grid is stored as a column plan (kernels_swsh.hip, pixel_sort_kernel)
};

struct TimeAxisCache {  // knots [lo, hi) of an axis of n samples with their B-spline tables for knots [j0, j1) (upload_times_bspline)
  bool valid = false;   // the device blocks hold the tables of `host`
  bool in_use = false;  // the running call reads the device blocks (found or built by it)
  bool hit = false;     // ... and found them
  uint64_t gen = 0;     // counts the builds
  int64_t n = 0, lo = 0, hi = 0, j0 = 0, j1 = 0;
  std::vector<double> host;         // t[lo, hi) as uploaded
  const double* pending = nullptr;  // built in the running call from these samples; copied to `host` where the host waits anyway (time_axis_commit)
  bool walked = false, regular = true;  // outcome of walk_time_axis over [lo, hi), once a call has walked them
  double* d_x = nullptr;                // all three indexed by GLOBAL knot number
  BsplineTable* d_tab = nullptr;
  BsplineForward* d_fwd = nullptr;
};
struct PixelCache {  // per-direction tables of one (transformation, field description) (device_pixel_tables)
  bool valid = false, in_use = false, hit = false;
  uint64_t gen = 0;
  std::string key;  // every input of device_pixel_tables, by value
  PixelTables T;
  DevPixel D;
  // the dense synthesis matrix of the WaveformModes route, built behind the tables (Bsyn0 with its offset row)
  bool B_valid = false;
  int B_spin = 0, B_ell_min = 0, B_ell_max = 0, B_cols = 0;
  double* d_B = nullptr;
  // the five of the AsymptoticBondiData route (with sigma's offset row in the spin-2 one when B_sigma)
  bool B5_valid = false, B5_sigma = false;
  int B5_ell_max = 0, B5_cols = 0;
  double* d_B5[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // output window of (axis entry, this entry): a function of the two alone
  bool win_valid = false, win_abd = false;
  uint64_t win_tgen = 0, win_pgen = 0;
  int64_t win_lo = 0, win_hi = 0;
};

struct bms_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t aux = nullptr;  // set-up kernels whose results the host waits for run here, beside the main stream's work
  std::string err;
  RouteOptions opt;  // route switches of THIS context: defaults from the environment at bms_ctx_create, then bms_ctx_set_option (env.h)
  // cap on the grids of one chunk of the time axis: min(96 GB, a third of the memory that was free when the context was created)
  // unless the caller sets one (one GPU's cfg5 rows -- 25 000 steps, six 99 x 99 grids, 76 GB -- are ONE chunk on an otherwise empty
  // MI355X); a call that still runs out of memory halves it and tries again (with_smaller_chunks)
  uint64_t ws_limit = 96ull << 30;
  bool ws_limit_set = false;  // by the caller: then it is kept as given
  uint64_t sticky_limit = 0;  // the reduced cap a call of this context last succeeded with after allocation failures (with_smaller_chunks) ...
  int sticky_left = 0;        // ... and for how many more calls it is tried first
  // evaluating product (kernels_gemm_eval.hip): how often its samples left the window of abscissae a tile stages in LDS
  unsigned long long* d_eval_stats = nullptr;  // device: [0] tiles / boundary blocks off the LDS path, [1] marches continued from global memory
  uint64_t eval_tiles = 0;                     // tiles + boundary blocks launched since the last reset
  bool alloc_failed = false;  // a device allocation of the running call failed (as opposed to a cap that is too small by plan)
  std::map<std::string, DevBuf> bufs;  // grow-only named work space
  std::vector<Slab> slabs;             // reserved by bms_ctx_reserve; the newest one with room serves the named buffers
  int delta_lmax = -1;                 // Delta tables cached up to this l
  int delta_mfma_lmax = -1;            // ... in the MFMA B-image packing
  // which rotation kernel served the calls since the last reset (bms_ctx_get_rotate_stats): launches of the resident, staged and VALU
  // kernels, and the waves per workgroup of the most recent VALU launch as its launcher reported them
  uint64_t rot_launches[3] = {0, 0, 0};
  // kernel launches of the back substitution + evaluation on the grid since the last reset (bms_ctx_get_backward_stats): of the
  // instance that reads its abscissae from the staged window, and of the one that gathers them (launch_bspline_backward_eval)
  unsigned long long bwd_launches[2] = {0, 0};
  int rot_valu_waves = 0;
  hipStream_t pipe_up = nullptr, pipe_down = nullptr;  // run_host_pipeline: uploads and downloads beside the kernels
  // set by SharedPieceTables around the per-piece calls of a pipelined call: the pieces share one transformation, so the
  // per-direction tables are computed (and read back) once, and a piece returns without waiting for its kernels
  bool async_pieces = false;
  // Stream-ordered return (option ASYNC_RETURN): a transformation of device-resident data on a stream the caller gave
  // leaves without waiting for it unless the call queued a copy out of host memory that does not outlive it (upload() and the other
  // staging copies raise host_copy_queued; the entry point lowers it).  async_pending: such a call may still be running -- whatever is
  // about to write the context's buffers from ANOTHER stream, or moves the context to another stream, drains c->stream first
  // (drain_async_return).
  bool host_copy_queued = false;
  bool async_pending = false;
  bool chunk_retry = false;  // with_smaller_chunks runs the call again after a failed allocation
  uint64_t async_returns = 0;  // calls that returned without waiting since the last reset (bms_ctx_get_async_stats)
  bool piece_tables_valid = false;
  void* piece_tables = nullptr;  // PieceTables*
  // constant rotors of internal rotations travel through a page-locked ring (a truly asynchronous copy: no stream
  // synchronisation to protect a stack copy); the ring is drained once per lap
  double* rot_ring_host = nullptr;
  // per-direction scalars on their way back to the host (device_pixel_tables): page-locked, so that the copy is asynchronous and what is
  // queued behind it starts without the host; two events order the host and the main stream behind the auxiliary one
  double* pix_back_host = nullptr;
  size_t pix_back_cap = 0;
  hipEvent_t ev_tables = nullptr, ev_aux_done = nullptr;
  double* rot_ring_dev = nullptr;
  int rot_ring_next = 0;
  std::map<std::pair<int, int>, RotResPlan> rot_res_plans;  // LDS-resident table images built so far, by (ell_min, ell_max)
  std::map<std::pair<int, int>, bool> flux_images;          // coefficient images of the fused fluxes on the device, by (ell_min, ell_max)
  std::map<int, bool> charge_images;                        // coefficient images of the Bondi charges on the device, by ell_max
  std::map<std::array<int, 4>, bool> product_tables;        // lambda tables of the Gauss-Legendre products on the device, by (spin, ell_max, n_nodes, weighted)
  int n_cu = 0;
  // analysis tables depend on the grid, the spin and the l range only: kept per tag until a call asks for other ones
  std::map<std::string, std::pair<std::array<int, 6>, AnalysisPlan>> plans;
  std::map<std::array<int, 5>, SynthesisPlan> syn_plans;  // by (n_theta, n_phi, spin, ell_min, ell_max)
  // the last answer of separable_rotor_grid (frame rotation, boost, grid): repeated transformations skip the walk over the rotors
  double ring_key[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int ring_verdict = -1;  // -1: nothing kept
  std::vector<double> ring_thetas;
  // the same behind a boost along the grid's axis: the tables belong to the ring colatitudes of the last such transformation
  std::map<std::array<int, 5>, std::pair<std::vector<double>, SynthesisPlan>> syn_plans_axis;
  // optional per-kernel timing with HIP events on the context's stream (bms_ctx_enable_timing)
  bool timing = false;
  struct Timed {
    int tag;
    hipEvent_t a, b;
  };
  std::vector<Timed> timed;
  std::vector<hipEvent_t> event_pool;
  double tag_ms[BMS_TAG_COUNT] = {0};
  long long tag_calls[BMS_TAG_COUNT] = {0};
  TimeAxisCache tcache;  // set-up kept across calls (above)
  PixelCache pcache;
};

static inline void note_alloc_failure(bms_ctx* c) {
  if (c) c->alloc_failed = true;
}

struct ScopedTimer {  // brackets one kernel launch with two events when timing is enabled
  bms_ctx* c;
  int tag;
  hipStream_t stream;  // the stream the bracketed kernel is launched on (events recorded elsewhere would bracket unrelated work)
  hipEvent_t a = nullptr, b = nullptr;
  static hipEvent_t get(bms_ctx* c) {
    if (!c->event_pool.empty()) {
      hipEvent_t e = c->event_pool.back();
      c->event_pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  ScopedTimer(bms_ctx* c_, int tag_, hipStream_t stream_ = nullptr) : c(c_), tag(tag_), stream(stream_ ? stream_ : c_->stream) {
    if (c->timing) {
      a = get(c);
      b = get(c);
      (void)hipEventRecord(a, stream);
    }
  }
  ~ScopedTimer() {
    if (c->timing) {
      (void)hipEventRecord(b, stream);
      c->timed.push_back({tag, a, b});
      // a context that never asks for its timings must not collect events for ever: pairs that have completed are folded
      // into the totals once a few thousand are pending (no synchronisation: unfinished pairs stay)
      if (c->timed.size() > 4096) {
        size_t keep = 0;
        for (auto& t : c->timed) {
          float f = 0.f;
          if (hipEventQuery(t.b) == hipSuccess && hipEventElapsedTime(&f, t.a, t.b) == hipSuccess) {
            c->tag_ms[t.tag] += f;
            c->tag_calls[t.tag] += 1;
            c->event_pool.push_back(t.a);
            c->event_pool.push_back(t.b);
          } else {
            c->timed[keep++] = t;
          }
        }
        c->timed.resize(keep);
        (void)hipGetLastError();
      }
    }
  }
};
#define TIMED(ctx, tag, expr)     \
  do {                            \
    ScopedTimer st__(ctx, tag);   \
    HIP_TRY(ctx, expr);           \
  } while (0)
// the same for a kernel launched on another stream than the context's main one
#define TIMED_ON(ctx, strm, tag, expr)  \
  do {                                  \
    ScopedTimer st__(ctx, tag, strm);   \
    HIP_TRY(ctx, expr);                 \
  } while (0)


// host-side phase timing of a call, printed when SCRI_AMD_TRACE is set (debugging aid)
struct HostTrace {
  bool on;
  std::chrono::steady_clock::time_point t0;
  explicit HostTrace(const bms_ctx* c) : on(c && c->opt.on(OPT_TRACE)), t0(std::chrono::steady_clock::now()) {}
  void mark(const char* what) {
    if (!on) return;
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[scri_amd] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(t1 - t0).count());
    t0 = t1;
  }
};

BMS_INTERNAL int fail(bms_ctx* c, int code, const char* fmt, ...);

// No C++ exception leaves the library: its callers are C, cgo, ctypes, and an exception that unwinds into them ends the process.  Every
// extern "C" entry that returns a status is a function-try-block closed by BMS_CATCH, which turns what was thrown -- std::bad_alloc
// from the host-side tables, std::system_error from a thread that could not start -- into a status and a message on the context.
BMS_INTERNAL int exception_status(bms_ctx* c) noexcept;
#define BMS_CATCH(ctx) \
  catch (...) { return exception_status(ctx); }

#define HIP_TRY(ctx, expr)                                                                                   \
  do {                                                                                                       \
    hipError_t e__ = (expr);                                                                                 \
    if (e__ != hipSuccess) {                                                                                 \
      if (e__ == hipErrorOutOfMemory) note_alloc_failure(ctx);                                               \
      return fail(ctx, e__ == hipErrorOutOfMemory ? BMS_ERR_NOMEM : BMS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                  hipGetErrorString(e__), __FILE__, __LINE__);                                               \
    }                                                                                                        \
  } while (0)

// Before work goes to a stream other than c->stream (the auxiliary stream's set-up kernels, the pipelines' transfers): a call that
// returned stream-ordered may still read the buffers that work writes.
inline int drain_async_return(bms_ctx* c) {
  if (!c->async_pending) return BMS_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->async_pending = false;
  return BMS_OK;
}

inline bool valid_mem(int mem) { return mem == BMS_HOST || mem == BMS_DEVICE; }
constexpr int MAX_ELL = 8192;  // 2 (l + 1)^2 fits an int with room; tables of such an l are far beyond any device's memory anyway

BMS_INTERNAL hipError_t create_download_stream(bms_ctx* c);
BMS_INTERNAL int dev_buf(bms_ctx* c, const char* name, size_t bytes, void** out);
template <class T>
inline int dev_buf_t(bms_ctx* c, const char* name, size_t count, T** out) {
  void* p = nullptr;
  int rc = dev_buf(c, name, count * sizeof(T), &p);
  *out = static_cast<T*>(p);
  return rc;
}

// Runs `call` again with half the work space cap while it fails because a device ALLOCATION failed (the buffer that failed was
// released before the attempt, so a smaller chunk finds room).  Not retried: a cap the caller set, and the planning error "the cap
// holds fewer than N rows" -- halving only makes that one worse.  The cap itself is restored after the call; the reduced value that
// worked is only REMEMBERED for a bounded number of calls (below), so one transient shortage (a temporary tensor of the caller) does
// not leave every later call of the context with chunks up to 32x smaller.  If every attempt fails the FIRST message is reported.
template <class F>
inline int with_smaller_chunks(bms_ctx* c, F call) {
  c->alloc_failed = false;
  const uint64_t tiles0 = c->eval_tiles;
  // A context that had to halve its cap keeps the reduced one for the next calls (sticky_left): under STEADY memory pressure (a
  // co-resident tensor of the caller) every call would otherwise free its grown buffers, fail the same multi-GB allocation and
  // re-allocate smaller ones -- seconds per call at 70-120 ms per GB.  The full cap is tried again after 16 calls, or as soon as
  // the device reports room for it.
  const uint64_t full = c->ws_limit;
  if (c->sticky_left > 0 && c->sticky_limit && !c->ws_limit_set) {
    size_t free_b = 0, total_b = 0;
    const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && (uint64_t)free_b > full + full / 2;
    (void)hipGetLastError();
    if (room || --c->sticky_left == 0)
      c->sticky_limit = 0;
    else
      c->ws_limit = std::min(full, c->sticky_limit);
  }
  int rc = call();
  if (rc != BMS_ERR_NOMEM || !c->alloc_failed || c->ws_limit_set) {
    c->ws_limit = full;
    return rc;
  }
  const std::string first = c->err;
  for (int attempt = 0; rc == BMS_ERR_NOMEM && c->alloc_failed && attempt < 5 && c->ws_limit > (512ull << 20); ++attempt) {
    c->ws_limit /= 2;
    c->alloc_failed = false;
    c->eval_tiles = tiles0;  // (diagnostic counter: the failed attempt's launches, if any, are not counted twice)
    c->chunk_retry = true;   // (an attempt after a failed allocation ends with the host-side wait)
    rc = call();
    c->chunk_retry = false;
  }
  if (rc == BMS_OK) c->sticky_limit = c->ws_limit, c->sticky_left = 16;
  c->ws_limit = full;
  if (rc == BMS_ERR_NOMEM) c->err = first;
  return rc;
}

// the dealing of the one-process multi-device entry points (bms_transform_modes_multi, bms_transform_abd_multi)
template <class PartCall>
inline int run_dealt_over_contexts(bms_ctx* const* ctxs, int n_ctx, int pieces, int64_t* n_times_out, PartCall part) {
  if (!ctxs || n_ctx < 1) return BMS_ERR_INVALID;
  for (int k = 0; k < n_ctx; ++k)
    if (!ctxs[k]) return BMS_ERR_INVALID;
  for (int k = 0; k < n_ctx; ++k)
    for (int j = 0; j < k; ++j)
      if (ctxs[j] == ctxs[k]) return fail(ctxs[0], BMS_ERR_INVALID, "context %d is listed twice: one context serves one host thread at a time", k);
  if (pieces < 1) pieces = 1;
  std::vector<int> rc(n_ctx, BMS_OK);
  std::vector<int64_t> got(n_ctx, -1);
  auto run = [&](int k) noexcept {
    const int p0 = (int)(((long long)pieces * k) / n_ctx), p1 = (int)(((long long)pieces * (k + 1)) / n_ctx);
    try {
      if (p1 > p0) rc[k] = part(ctxs[k], p0, p1, &got[k]);
    } catch (...) {
      rc[k] = exception_status(ctxs[k]);
    }
  };
  std::vector<std::thread> threads;
  threads.reserve(n_ctx);
  int started = 1;
  try {
    for (; started < n_ctx; ++started) threads.emplace_back(run, started);
  } catch (...) {  // a thread that could not start: the contexts without one report it, the others finish their share first
    for (int k = started; k < n_ctx; ++k) rc[k] = exception_status(ctxs[k]);
  }
  run(0);
  for (auto& th : threads) th.join();
  for (int k = 0; k < n_ctx; ++k)
    if (rc[k] != BMS_OK) {
      if (k != 0) {
        const std::string msg = ctxs[k]->err;
        return fail(ctxs[0], rc[k], "context %d (device %d): %s", k, ctxs[k]->device, msg.c_str());
      }
      return rc[k];
    }
  int64_t n_new = -1;
  for (int k = 0; k < n_ctx; ++k) {
    if (got[k] < 0) continue;  // (a context without a shard of its own)
    if (n_new >= 0 && got[k] != n_new)
      return fail(ctxs[0], BMS_ERR_HIP, "the output window has %lld rows on context %d and %lld on another", (long long)got[k], k, (long long)n_new);
    n_new = got[k];
  }
  if (n_times_out) *n_times_out = std::max<int64_t>(n_new, 0);
  return BMS_OK;
}


// A series in HOST memory through the device in pieces k0 .. k1 - 1 over three streams, so that its transfers run beside the kernels
// (the link is full duplex): piece k goes up on c->pipe_up (up(k, slot)), is computed on c->stream (compute(k, slot), a status) and
// comes home on c->pipe_down (down(k, slot)), through two staging slots, slot = (k - k0) & 1; the host thread only enqueues.  The
// transformations (bms_transform_*_pipelined_part) and the rotations of a host series in blocks (engine_rotate.hip) use it.
//   compute k waits for upload k and, out of place, for download k - 2 (its output slot has left);
//   upload k waits for download k - 2 in place (in_place: the download reads the upload's slot), for compute k - 2 otherwise;
//   download k follows compute k: with host_waits the host synchronises on it before it enqueues the download, else pipe_down waits.
//   (For the transformations stream waits instead of the host wait made no difference, three alternating runs: 14.9 / 15.1 / 13.7
//   against 14.9 / 15.1 / 16.2 ms -- the transfers, not the kernels' gaps, set the time.)
// Issue order: upload k0, compute k0, upload k0 + 1, download k0, then upload k + 1, compute k, download k -- the first piece of a
// transformation reads its per-direction tables back with a blocking copy, which would wait for an upload queued before it.
// In the rocprofv3 trace of the transformations the uploads run on a DMA engine beside the kernels; the downloads are executed by the
// runtime as shader copies (__amd_rocclr_copyBuffer) that take turns with the compute kernels.  Storing the results straight into the
// page-locked array from the analysis kernel (on a side stream, with a small grid) was tried: the stores leave at 42 GB/s instead of
// 57 and every memory-bound kernel running beside them crawls -- 19.8 ms against 15.7 ms per cfg3 transform.
// A HIP error fails the call with "<err_first>: ..." if the first upload could not be issued, "<err>: ..." otherwise.  Once anything is
// enqueued every exit synchronises the three streams and returns the events.
template <class Up, class Compute, class Down>
int run_host_pipeline(bms_ctx* c, int k0, int k1, bool in_place, bool host_waits, const char* err_first, const char* err, Up up,
                      Compute compute, Down down) {
  if (int rc0 = drain_async_return(c)) return rc0;
  if (!c->pipe_up) {
    HIP_TRY(c, hipStreamCreateWithFlags(&c->pipe_up, hipStreamNonBlocking));
    HIP_TRY(c, create_download_stream(c));
  }
  const int n = k1 - k0;
  std::vector<hipEvent_t> ev_up(n), ev_c(n), ev_dn(n);
  for (int i = 0; i < n; ++i) ev_up[i] = ScopedTimer::get(c), ev_c[i] = ScopedTimer::get(c), ev_dn[i] = ScopedTimer::get(c);
  auto send = [&](int i) -> hipError_t {  // upload of piece k0 + i
    if (i >= n) return hipSuccess;
    hipError_t e = i >= 2 ? hipStreamWaitEvent(c->pipe_up, in_place ? ev_dn[i - 2] : ev_c[i - 2], 0) : hipSuccess;
    if (e == hipSuccess) e = up(k0 + i, i & 1);
    return e == hipSuccess ? hipEventRecord(ev_up[i], c->pipe_up) : e;
  };
  int rc = BMS_OK;
  hipError_t he = send(0);
  const bool first_failed = he != hipSuccess;
  for (int i = 0; i < n && he == hipSuccess; ++i) {
    const int k = k0 + i, slot = i & 1;
    if (i > 0 && (he = send(i + 1)) != hipSuccess) break;
    if ((he = hipStreamWaitEvent(c->stream, ev_up[i], 0)) != hipSuccess) break;
    if (!in_place && i >= 2 && (he = hipStreamWaitEvent(c->stream, ev_dn[i - 2], 0)) != hipSuccess) break;
    if ((rc = compute(k, slot)) != BMS_OK) break;
    if (i == 0 && (he = send(1)) != hipSuccess) break;
    if ((he = hipEventRecord(ev_c[i], c->stream)) != hipSuccess) break;
    if ((he = host_waits ? hipEventSynchronize(ev_c[i]) : hipStreamWaitEvent(c->pipe_down, ev_c[i], 0)) != hipSuccess) break;
    if ((he = down(k, slot)) != hipSuccess) break;
    if ((he = hipEventRecord(ev_dn[i], c->pipe_down)) != hipSuccess) break;
  }
  (void)hipStreamSynchronize(c->pipe_up);
  (void)hipStreamSynchronize(c->stream);
  (void)hipStreamSynchronize(c->pipe_down);
  for (int i = 0; i < n; ++i) c->event_pool.push_back(ev_up[i]), c->event_pool.push_back(ev_c[i]), c->event_pool.push_back(ev_dn[i]);
  if (rc) return rc;
  if (he != hipSuccess) return fail(c, BMS_ERR_HIP, "%s: %s", first_failed ? err_first : err, hipGetErrorString(he));
  return BMS_OK;
}


// ====================================================================================================== tables of one transformation

constexpr int SPLINE_TILE = 320;  // knots per (pixel group, tile) wave: measured sweep 128..640 on cfg3, best at 320 (halo re-reads 10 %)
constexpr int SPLINE_HALO = 32;
// input rows an output range reads beyond its knots on either side: bms_shard_plan, the pieces of the pipelined calls and the chunk
// loops all take their rows from needed_rows (engine_tables.hip), so a shard planned by one holds what the others read
constexpr int ROW_MARGIN = SPLINE_HALO + 2;

inline long long round_up(long long a, long long b) { return (a + b - 1) / b * b; }

struct FieldPlan {  // one field to synthesise: input modes, its SWSH matrix
  const double* d_data = nullptr;  // device c16[n][ld]
  int64_t ld = 0;
  int ell_min = 0, ell_max = 0, spin = 0;
  double* d_B = nullptr;  // synthesis matrix
  long long ldb = 0;
  int K = 0;  // 2 * n_modes
};

// Time samples a call touches on the device: the rows it holds plus the spline-table warm-up margin.  A shard of an
// 8 x 1e5-step series uploads and checks 1e5 + 128 samples, not 8e5 (the host still sees the global array: window
// search and chunk planning are binary searches on it).
constexpr int64_t TIME_MARGIN = 64;

struct PieceTables {  // tables shared by the pieces of one pipelined call: per direction, and per knot of the WHOLE series
  PixelTables T;
  DevPixel DP;
  int col_plan = 0;  // the column order T / DP were built in
  bool times_valid = false;
  double* d_x = nullptr;
  BsplineTable* d_bstab = nullptr;
  BsplineForward* d_bsfwd = nullptr;
};

// For its lifetime the per-piece calls on `c` share one PieceTables (the pipelined calls, bms_transform_modes_series): the first piece
// builds the tables, the others read them, and a piece returns without waiting for its kernels
struct SharedPieceTables {
  bms_ctx* c;
  PieceTables tables;
  explicit SharedPieceTables(bms_ctx* c_) : c(c_) {
    c->piece_tables = &tables;
    c->piece_tables_valid = false;
    c->async_pieces = true;
  }
  ~SharedPieceTables() {
    c->async_pieces = false;
    c->piece_tables_valid = false;
    c->piece_tables = nullptr;
  }
  SharedPieceTables(const SharedPieceTables&) = delete;
  SharedPieceTables& operator=(const SharedPieceTables&) = delete;
};

// The time shards of a pipelined call (plan_pieces): the output window cut into `pieces` (clamped to at least 8 outputs each), of which
// this call runs [p0, p1); piece k produces outputs [cut[k], cut[k + 1]) from input rows [r0[k], r1[k]) -- what bms_shard_plan names for
// that output range.  (A clamped count keeps the pieces that exist: a caller that dealt a larger count over its contexts still covers
// every one once.)
struct PiecePlan {
  int pieces = 0, p0 = 0, p1 = 0;
  std::vector<int64_t> cut, r0, r1;
  int64_t max_rows = 0, max_out = 0;  // over the pieces [p0, p1)
  bms_shard shard(int k) const { return {r0[k], r1[k] - r0[k], cut[k], cut[k + 1], 0, 0}; }
  int64_t rows_out(int k) const { return cut[k + 1] - cut[k]; }
};

// ---- shared helpers (engine_tables.hip unless noted)
BMS_INTERNAL void build_rotor_grid(const double fr[4], const double v[3], int n_theta, int n_phi, std::vector<Quat>& R);
BMS_INTERNAL void theta_quadrature_weights(int n_theta, std::vector<double>& q);
BMS_INTERNAL int ensure_delta(bms_ctx* c, int lmax, const double** d_delta, const long long** d_off);
BMS_INTERNAL int ensure_delta_mfma(bms_ctx* c, int lmax, const double** d_tab, const long long** d_off);
BMS_INTERNAL int ensure_delta_resident(bms_ctx* c, int ell_min, int ell_max, bool* ok, RotResPlan* P, size_t* lds_bytes,
                                 const double** d_tab, unsigned int** d_counter);
BMS_INTERNAL void init_pixel_tables(const bms_transformation* tr, PixelTables& T);
BMS_INTERNAL PixelSpec base_pixel_spec(const bms_transformation* tr, const PixelTables& T);
BMS_INTERNAL void build_pixel_tables(const bms_transformation* tr, PixelTables& T);
BMS_INTERNAL void output_window(const PixelTables& T, const double* t, int64_t n, int64_t& i_lo, int64_t& i_hi);
BMS_INTERNAL void output_window_abd(const PixelTables& T, const double* u, int64_t n, int64_t& i_lo, int64_t& i_hi);
BMS_INTERNAL void needed_knots(const PixelTables& T, const double* t, int64_t n, int64_t c0, int64_t c1, int64_t& ja, int64_t& jb);
BMS_INTERNAL void needed_rows(const PixelTables& T, const double* t, int64_t n, int64_t c0, int64_t c1, int64_t& r0, int64_t& r1);
BMS_INTERNAL void plan_pieces(const PixelTables& T, const double* t, int64_t n, int64_t i_lo, int64_t i_hi, int pieces, int piece0, int piece1,
                              PiecePlan& P);
BMS_INTERNAL int piece_produced(bms_ctx* c, const PiecePlan& P, int k, int64_t got, int64_t first);
BMS_INTERNAL int build_analysis(bms_ctx* c, const char* tag, int n_theta, int n_phi, int spin, int ell_min_out, int ell_max_out,
                          AnalysisPlan& A);
inline bool analysis_reads_contiguous_rows(const AnalysisPlan& A) { return !A.fused && !A.large && A.separable; }
BMS_INTERNAL int run_analysis(bms_ctx* c, const AnalysisPlan& A, const double* d_G, long long rows, double* d_out, long long ldo,
                        const int* col_of_pixel = nullptr, long long ld_cols = 0);
BMS_INTERNAL int upload(bms_ctx* c, const char* name, const void* host, size_t bytes, void** dev);
BMS_INTERNAL int upload_times(bms_ctx* c, const double* t, int64_t n, int64_t lo, int64_t hi, int64_t j0, int64_t j1, double** d_x,
                        SplineTable** d_tab);
BMS_INTERNAL int upload_times_bspline(bms_ctx* c, const double* t, int64_t n, int64_t lo, int64_t hi, int64_t j0, int64_t j1, double** d_x,
                                BsplineTable** d_tab, BsplineForward** d_fwd);
// (the kept entries serve a call only once its own set-up has found or built them)
inline void begin_setup_reuse(bms_ctx* c) {
  c->tcache.in_use = c->tcache.hit = false;
  c->tcache.pending = nullptr;
  c->pcache.in_use = c->pcache.hit = false;
}
// the `reuse` argument of device_pixel_tables for a transformation under this shard description: never 0, one value per column part
inline int reuse_tag(const bms_shard* sh) { return 1 + ((sh && sh->col_parts > 1 && sh->col_part >= 0) ? 1 + (sh->col_part & 0x7fff) + ((sh->col_parts & 0x7fff) << 15) : 0); }
// ---- steps the two transform implementations share (transform_modes_impl, transform_abd_impl), each called where its block stood
struct KnotTables {  // the knot tables of one call: slope form (d_tab) or B-spline form (d_bstab, d_bsfwd), indexed by GLOBAL knot number
  double* d_x = nullptr;
  SplineTable* d_tab = nullptr;
  BsplineTable* d_bstab = nullptr;
  BsplineForward* d_bsfwd = nullptr;
  bool times_ahead = false;  // on their way since the top of the call (knot_tables_ahead)
  bool axis_known = false;   // the axis is one the context has tables for AND has walked: neither is done again
};
struct ChunkPlan {
  int64_t chunk = 0;  // output samples per pass of the chunk loop
  int spline_tile = SPLINE_TILE;
};
BMS_INTERNAL int knot_tables_ahead(bms_ctx* c, const double* t, int64_t n, const bms_shard* sh, int64_t t_lo, int64_t t_hi, KnotTables& kt);
BMS_INTERNAL int knot_tables_of_call(bms_ctx* c, const double* t, int64_t n, int64_t t_lo, int64_t t_hi, int64_t row0, int64_t rows_avail, bool bsg, PieceTables* shared, KnotTables& kt);
BMS_INTERNAL int refuse_sharded_graded_axis(bms_ctx* c, bool regular_mesh, const bms_shard* sh, int64_t n);
BMS_INTERNAL int plan_chunks(bms_ctx* c, uint64_t ws_limit, double bytes_per_row, int64_t n_new, bool regular_mesh, int64_t n, const char* how_many, int n_cols, ChunkPlan& P);
BMS_INTERNAL int chunk_rows(bms_ctx* c, const PixelTables& T, const double* t, int64_t n, bool regular_mesh, int64_t c0, int64_t c1, int64_t row0, int64_t rows_avail, int64_t& g0, int64_t& g1);
BMS_INTERNAL int rotate_into_grid_frame(bms_ctx* c, const bms_transformation* tr, double* data, int64_t rows, int64_t ld, int ell_min, int ell_max);
BMS_INTERNAL int rotated_input_in_grid_frame(bms_ctx* c, const bms_transformation* tr, const char* name, int mem, const double** d_data, int64_t rows, int64_t ld, int ell_min, int ell_max);
BMS_INTERNAL int spline_eval_args(bms_ctx* c, const KnotTables& kt, const PixelTables& T, int cA, int cB, const double* t, int64_t n, int64_t g0, int64_t g1, int64_t c0, int64_t c1,
                                  double* out, long long ldo, long long ldg, SplineEval& ev);
BMS_INTERNAL void time_axis_commit(bms_ctx* c, bool walked, bool regular);
BMS_INTERNAL void drop_setup_caches(bms_ctx* c);
BMS_INTERNAL bool cached_window(bms_ctx* c, bool abd, int64_t& i_lo, int64_t& i_hi);
BMS_INTERNAL void keep_window(bms_ctx* c, bool abd, int64_t i_lo, int64_t i_hi);
BMS_INTERNAL int stage_in(bms_ctx* c, const char* name, const void* src, int mem, size_t bytes, const double** dev);
// ---- the arguments of a building-block entry: `int mem` says whether the caller's arrays are host or device memory
// The refusal of a bad `mem` in the words every entry uses (`who`: the entries that prefix their messages with their name), then the
// context's device; select_device = false for the entries whose size checks stand between the two.
inline int entry_mem(bms_ctx* c, int mem, const char* who = nullptr, bool select_device = true) {
  if (!valid_mem(mem)) return who ? fail(c, BMS_ERR_INVALID, "%s: mem is BMS_HOST or BMS_DEVICE, got %d", who, mem)
                                  : fail(c, BMS_ERR_INVALID, "mem is BMS_HOST or BMS_DEVICE, got %d", mem);
  if (select_device) HIP_TRY(c, hipSetDevice(c->device));
  return BMS_OK;
}

// The staging of one call's arrays, for the entries of the shape "stage inputs, run kernels, copy outputs back, wait".  Device arrays
// pass through; host arrays go up into named work-space blocks and results come home from such blocks.  finish() queues the copies
// home in the order they were declared, waits ONCE on the context's stream (read then, as the entries always did) and returns the
// status.  If the call leaves before finish() -- a refusal or a HIP error after a copy was queued -- the destructor waits on the
// stream instead, so that no queued work still reads or writes the caller's arrays when the error is returned (before this struct
// such exits returned at once: the one change of behaviour it brings, on failure paths only).  No heap allocation: MAX_BACK records.
struct CallIO {
  static constexpr int MAX_BACK = 7;
  struct Back {
    void* dst;
    const void* dev;
    size_t bytes, rows, dst_pitch;  // rows != 0: `rows` rows of `bytes` bytes, dense on the device, `dst_pitch` bytes apart at home
    hipMemcpyKind kind;
  };
  bms_ctx* c;
  int mem;
  bool finished = false;
  Back back[MAX_BACK];
  int n_back = 0;
  CallIO(bms_ctx* c_, int mem_) : c(c_), mem(mem_) { c->host_copy_queued = false; }
  CallIO(const CallIO&) = delete;
  CallIO& operator=(const CallIO&) = delete;
  ~CallIO() {  // (host_copy_queued: raised by every copy the helper issues, and by upload() / upload_times() beside it)
    if (c->host_copy_queued && !finished) (void)hipStreamSynchronize(c->stream);
  }
  bool host() const { return mem == BMS_HOST; }
  // an input of `bytes` bytes: the caller's device pointer, or a copy of the host array in block `name` (of block_bytes, if larger)
  template <class T>
  int in(const char* name, const void* src, size_t bytes, const T** dev, size_t block_bytes = 0) {
    if (!host()) {
      *dev = static_cast<const T*>(src);
      return BMS_OK;
    }
    void* p;
    if (int rc = dev_buf(c, name, std::max(bytes, block_bytes), &p)) return rc;
    *dev = static_cast<const T*>(p);
    c->host_copy_queued = true;
    HIP_TRY(c, hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return BMS_OK;
  }
  // a copy of `bytes` bytes from the device to `dst` at finish(), whatever `mem` is: the outputs that always go to the host
  // (dst == NULL: an output the caller did not ask for), and with `kind` the result of an in-place entry on its way back
  int copy_back(void* dst, const void* dev, size_t bytes, hipMemcpyKind kind = hipMemcpyDeviceToHost, size_t rows = 0, size_t dst_pitch = 0) {
    if (!dst) return BMS_OK;
    if (n_back == MAX_BACK) return fail(c, BMS_ERR_INVALID, "internal: more than %d outputs in one call", MAX_BACK);
    back[n_back++] = {dst, dev, bytes, rows, dst_pitch, kind};
    return BMS_OK;
  }
  // an output of `count` elements: the caller's device pointer, or block `name`, which finish() copies to the host array
  template <class T>
  int out(const char* name, void* dst, size_t count, T** dev) {
    *dev = static_cast<T*>(dst);
    if (!host() || !dst) return BMS_OK;
    if (int rc = dev_buf_t(c, name, count, dev)) return rc;
    return copy_back(dst, *dev, count * sizeof(T));
  }
  // the same for `rows` rows of `cols` elements that lie `ld_dst` elements apart in a HOST array (dense in the block; a device
  // array is written in place, with its own pitch)
  template <class T>
  int out_rows(const char* name, void* dst, size_t rows, size_t cols, size_t ld_dst, T** dev) {
    *dev = static_cast<T*>(dst);
    if (!host() || !dst) return BMS_OK;
    if (int rc = dev_buf_t(c, name, rows * cols, dev)) return rc;
    return copy_back(dst, *dev, cols * sizeof(T), hipMemcpyDeviceToHost, rows, ld_dst * sizeof(T));
  }
  // an array the kernels work on in place: it starts as `src` and ends in `dst` (which may be `src`).  Device memory: `dst` itself,
  // after a copy of `src` unless the two are one array; host memory: block `name`, filled from `src` and copied to `dst` by finish()
  template <class T>
  int inout(const char* name, const void* src, void* dst, size_t count, T** dev) {
    *dev = static_cast<T*>(dst);
    if (host())
      if (int rc = dev_buf_t(c, name, count, dev)) return rc;
    if (host() || src != dst) c->host_copy_queued = true;  // (a copy out of or into one of the caller's arrays)
    if (host() || src != dst) HIP_TRY(c, hipMemcpyAsync(*dev, src, count * sizeof(T), host() ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    return host() ? copy_back(dst, *dev, count * sizeof(T)) : BMS_OK;
  }
  int finish() {
    hipStream_t S = c->stream;
    for (int i = 0; i < n_back; ++i) {
      const Back& b = back[i];
      if (b.rows)
        HIP_TRY(c, hipMemcpy2DAsync(b.dst, b.dst_pitch, b.dev, b.bytes, b.bytes, b.rows, b.kind, S));
      else
        HIP_TRY(c, hipMemcpyAsync(b.dst, b.dev, b.bytes, b.kind, S));
    }
    HIP_TRY(c, hipStreamSynchronize(S));
    finished = true;
    return BMS_OK;
  }
};

// what the entries that read modes c16[n][ld] of l = ell_min .. ell_max through the angular-velocity kernel refuse; *n_modes on success
BMS_INTERNAL int modes_checks(bms_ctx* c, int ell_min, int ell_max, int64_t ld, int* n_modes);
// <Ldt> f8[n][3], <LL> f8[n][9] and omega f8[n][3] of the modes d_y (knots and tables of their time axis: d_x, d_tab, tile) side by side
// in block "av_out", through blocks "R" and "S": the launches bms_angular_velocity and bms_corotating_frame share (engine_blocks.hip)
BMS_INTERNAL int angular_velocity_on_device(bms_ctx* c, const double* d_y, int64_t ld, int64_t n, int ell_min, int n_modes, const double* d_x,
                                            const SplineTable* d_tab, int tile, double** d_res);
// engine_flux.hip: the coefficient image of the fused fluxes (long double, rounded once), the walk over a triplet list, and what the two
// entries refuse before they select a device
BMS_INTERNAL void build_flux_image(int ell_min, int ell_max, std::vector<double>& image);
BMS_INTERNAL int64_t first_bad_triplet(const int32_t* rows, const int32_t* cols, int64_t n_el, int n_cols);
BMS_INTERNAL int flux_checks(bms_ctx* c, const double* t, const void* h, int64_t ld_h, const void* hdot, int64_t ld_hdot, int64_t n_times,
                             int ell_min, int ell_max, int mem, const double* energy, const double* momentum, const double* angular,
                             const double* boost, int* n_modes);
BMS_INTERNAL int expectation_checks(bms_ctx* c, const void* a, int64_t ld_a, const void* b, int64_t ld_b, int64_t n_times, int n_cols,
                                    const int32_t* rows, const int32_t* cols, const void* values, int64_t n_el, int mem, const void* out);
BMS_INTERNAL int pair_checks(bms_ctx* c, const void* a, int64_t ld_a, int ell_min_a, const void* b, int64_t ld_b, int ell_min_b, int64_t n_times,
                             int ell_min, int ell_max, int mem, const void* inner, const void* l_out, const void* ll_out, int* n_modes,
                             int64_t* off_a, int64_t* off_b);
BMS_INTERNAL void build_charge_image(int ell_max, std::vector<double>& image);
BMS_INTERNAL int charge_checks(bms_ctx* c, const double* t, const void* psi1, int64_t ld_psi1, const void* psi2, int64_t ld_psi2, const void* sigma,
                               int64_t ld_sigma, const void* sigma_dot, int64_t ld_sigma_dot, int64_t n_times, int ell_max, int mem,
                               const double* four_momentum, const double* angular, const double* boost, const double* com, int* n_modes);
// engine_product.hip: the Gauss-Legendre nodes and lambda tables of the products (long double, rounded once) and what the three entries refuse
// before they select a device
BMS_INTERNAL void build_product_table(int spin, int ell_max, int n_nodes, bool weighted, double* cos_theta, double* weights, std::vector<double>& table);
BMS_INTERNAL int product_checks(bms_ctx* c, const void* a, int64_t ld_a, int spin_a, int ell_max_a, int conj_a, const void* b, int64_t ld_b, int spin_b,
                                int ell_max_b, int conj_b, int64_t n_times, int ell_max_out, int mem, const void* out, int64_t ld_out, int* n_nodes);
BMS_INTERNAL int supermomenta_checks(bms_ctx* c, const void* psi2, int64_t ld_psi2, const void* sigma, int64_t ld_sigma, const void* sigma_dot,
                                     int64_t ld_sigma_dot, int64_t n_times, int ell_max, int ell_max_out, int mem, const void* bondi_sachs,
                                     const void* moreschi, const void* geroch, const void* geroch_winicour, const void* mass_aspect, int64_t ld_out,
                                     int* n_nodes);
BMS_INTERNAL int constraint_checks(bms_ctx* c, const void* const in[CONSTRAINT_INPUTS], const int64_t ld[CONSTRAINT_INPUTS], int64_t n_times, int ell_max,
                                   int mem, const void* const violations[6], int64_t ld_out, const double* norms, unsigned* reads, int* n_nodes);
BMS_INTERNAL int bianchi_checks(bms_ctx* c, int k, const void* sigma, int64_t ld_sigma, const void* a, int64_t ld_a, const void* b, int64_t ld_b,
                                int64_t n_times, int ell_max, int mem, const void* rhs, int64_t ld_rhs, const void* psi3, const void* psi4, int64_t ld_psi,
                                int* n_nodes);
// engine_cut.hip: the window rule of a cut's times and what bms_supermomentum_on_cut refuses before it selects a device
BMS_INTERNAL void cut_window(const double* t, int64_t n, double amin, double amax, int64_t* lo, int64_t* hi);
BMS_INTERNAL int cut_checks(bms_ctx* c, const double* t, int64_t n, const void* psi, int64_t ld, int mem, int ell_max, const double* alpha,
                            const void* modes_out, const double* psi_at_alpha, const double* k_at_alpha, int64_t* lo, int64_t* hi);
// engine_retard.hip: what bms_finite_radius_retard refuses before it selects a device
BMS_INTERNAL int retard_checks(bms_ctx* c, const double* t, const double* areal_radius, const double* average_lapse, int64_t n_raw, const void* data,
                               int64_t ld, int n_cols, int mem, const double* frame, double coord_radius, double initial_adm_energy, double ch_mass,
                               double unit_scale, int radius_exponent, double min_time_step, const int64_t* n_kept, const double* t_out,
                               const double* radii_out, const void* data_out, int64_t ld_out, const double* frame_out);
BMS_INTERNAL void time_window(int64_t n, const bms_shard* sh, int64_t& lo, int64_t& hi);
BMS_INTERNAL int validate_transformation(bms_ctx* c, int64_t n, const double* t, const bms_transformation* tr, int64_t n_min);
BMS_INTERNAL int walk_time_axis(bms_ctx* c, const double* t, int64_t lo, int64_t hi, bool* regular);
BMS_INTERNAL int validate_common(bms_ctx* c, int64_t n, const double* t, const bms_transformation* tr, int64_t lo = 0, int64_t hi = -1,
                           bool* regular = nullptr, int64_t n_min = 4);
BMS_INTERNAL int spline_tile_for(const double* x, int64_t n);
BMS_INTERNAL BsplineSpread skew_spread(const PixelTables& T, int cA, int cB, const double* x_host);
BMS_INTERNAL int eval_search_halfwidth(const PixelTables& T, int cA, int cB, const double* x_host, int64_t g0, int64_t g1);
BMS_INTERNAL bool large_synthesis_route(const bms_ctx* c, int n_theta, int n_phi, int ell_min, int ell_max);
BMS_INTERNAL bool axis_boost_pays(const bms_ctx* c, int n_modes, int n_theta, int n_phi);
BMS_INTERNAL bool separable_rotor_grid(const bms_transformation* tr, std::vector<double>& thetas, bool axis_boost_off = false);
BMS_INTERNAL bool separable_rotor_grid(bms_ctx* c, const bms_transformation* tr, std::vector<double>& thetas);
BMS_INTERNAL int build_synthesis(bms_ctx* c, int n_theta, int n_phi, int spin, int ell_min, int ell_max, SynthesisPlan& P,
                           const std::vector<double>* thetas = nullptr);
BMS_INTERNAL int run_synthesis(bms_ctx* c, const SynthesisPlan& P, const double* A, long long lda, long long rows, const double* off, double* Y,
                         long long ldy, const double* scale = nullptr);
BMS_INTERNAL int column_plan(const bms_ctx* c, const bms_transformation* tr, int n_out);
BMS_INTERNAL int device_pixel_tables(bms_ctx* c, const bms_transformation* tr, PixelTables& T, int mode, int spin, int cw,
                               const std::vector<cplx>* coef0, const std::vector<cplx>* coef1, const cplx cv[4], DevPixel& D,
                               int plan, hipStream_t PS = nullptr,
                               const std::function<int(hipStream_t, const DevPixel&, int)>& behind_tables = nullptr,
                               const std::function<void()>& while_waiting = nullptr, int reuse = 0);
BMS_INTERNAL int tables_and_window(bms_ctx* c, const bms_transformation* tr, const double* t, int64_t n, bool abd, PixelTables& T, int64_t& i_lo,
                                   int64_t& i_hi);
BMS_INTERNAL int column_range(bms_ctx* c, const bms_shard* sh, int n_cols, int& cA, int& cB);
BMS_INTERNAL int part_analysis_matrix(bms_ctx* c, const AnalysisPlan& A, const char* name, int n_cols, const int* col_of_pixel,
                                double** d_At, long long* ld_at);
BMS_INTERNAL uint64_t eval_tile_count(long long rows, int n_cols, int step);
// engine_rotate.hip: in-place rotation of resident or host modes by one rotor (series = false) or one per row; the transformations
// rotate the modes into the frame of the separable synthesis with it (sync_after = false: the caller's stream carries on)
BMS_INTERNAL int rotate_impl(bms_ctx* c, void* data, int mem, int64_t n_times, int64_t ld, int ell_min, int ell_max, const void* spinors, bool series,
                             bool sync_after = true);
