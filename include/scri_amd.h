/* scri_amd -- C ABI of the MI355X-native BMS-transformation engine.
 *
 * Drop-in boundary for the BMS hot path of moble/scri (reference scri 2024.0.13).  The reference has no FFI:
 * its seam is Python attribute grafting (scri/__init__.py:125-150, scri/waveform_modes.py:705-719,
 * scri/asymptotic_bondi_data/__init__.py:235-263).  Each entry point below replaces the arithmetic of the
 * cited reference function; argument parsing / validation / bookkeeping (kwargs precedence, history, frame
 * update) stays in the Python shim `scri_amd` which mirrors the reference's behaviour and binds these symbols
 * with ctypes (INTEGRATION.md shows the stub a scri maintainer would add).
 *
 * Conventions
 *   - complex data are interleaved (re, im) float64 = numpy complex128; "c16[N][ld]" means N rows with a
 *     row stride of `ld` complex elements (C-contiguous when ld == row length);
 *   - `mem` selects where the bulk buffers live: BMS_HOST (numpy memory; the library copies to the GPU and
 *     back) or BMS_DEVICE (HIP device pointers, e.g. torch.Tensor.data_ptr()); time arrays and all small
 *     parameter arrays are always host memory;
 *   - the caller owns every buffer; the library keeps no pointer after return.  Device work space is cached
 *     behind the opaque context and released by bms_ctx_destroy;
 *   - every function returns 0 on success or a negative bms_status; bms_last_error(ctx) gives the text;
 *   - a context is bound to one GPU and one HIP stream; calls on one context are serialised by the caller,
 *     different contexts are independent.  There is NO CPU fallback: without a gfx950 device
 *     bms_ctx_create fails.
 */
#ifndef SCRI_AMD_H
#define SCRI_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bms_ctx bms_ctx;

enum bms_status {
  BMS_OK = 0,
  BMS_ERR_INVALID = -1,     /* bad argument (maps to ValueError in the shim) */
  BMS_ERR_HIP = -2,         /* HIP runtime failure */
  BMS_ERR_NOMEM = -3,       /* device (or host) allocation failed */
  BMS_ERR_UNSUPPORTED = -4, /* valid request outside the implemented range */
  BMS_ERR_NODEVICE = -5,    /* no usable GPU */
  BMS_ERR_INTERNAL = -6     /* a C++ exception inside the library, caught at the boundary (none ever crosses it) */
};

enum bms_mem { BMS_HOST = 0, BMS_DEVICE = 1 };

/* type-specific inhomogeneous term of the WaveformModes path, scri/waveform_grid.py:485-557 */
enum bms_type_term {
  BMS_TERM_NONE = 0,  /* psi4, hdot, news (and unknown types, which the reference treats as psi4) */
  BMS_TERM_H = 1,     /* h:     f -= ethbar^2 alpha (NP normalisation), waveform_grid.py:486-494 */
  BMS_TERM_SIGMA = 2, /* sigma: f -= eth^2 alpha / 2 ... GHP,            waveform_grid.py:495-503 */
  BMS_TERM_PSI = 3    /* psi0..psi3: sum over higher Weyl scalars,       waveform_grid.py:504-550 */
};

int bms_version(void);

/* ---- context ------------------------------------------------------------------------------------------- */
int bms_ctx_create(int device, bms_ctx** ctx);
void bms_ctx_destroy(bms_ctx* ctx);
const char* bms_last_error(const bms_ctx* ctx); /* ctx may be NULL: error of the last failed bms_ctx_create */
/* run on a caller-provided hipStream_t (NULL: the context's own stream) */
int bms_ctx_set_stream(bms_ctx* ctx, void* hip_stream);
/* run on the device's default (null) stream -- handle 0, which bms_ctx_set_stream takes as "own stream" -- so that work a
 * caller queued there (torch's default stream: allocations, copies, memsets) is ordered before the engine's kernels */
int bms_ctx_use_default_stream(bms_ctx* ctx);
/* Route options of ONE context: choices between routes that give the same results to rounding (dense product vs separable
 * synthesis, evaluating product vs product + back substitution, fused vs two-pass boost-free route, ...; the list is
 * scri_amd/csrc/env.h, names with or without the SCRI_AMD_ prefix, e.g. "NO_GEMM_EVAL").  Flags take 0 / 1; AXIS_BOOST_MIN_WORK a
 * count of multiply-adds (< 0: built-in threshold, 0: always) and GEMM_EVAL_STEP 0 / 61 / 64.  A context takes its DEFAULTS from the
 * SCRI_AMD_<NAME> environment variables once, inside bms_ctx_create; no call reads the environment afterwards, so two contexts of
 * one process may run different routes concurrently ("re-entrant per ctx").  BMS_ERR_INVALID for an unknown name. */
int bms_ctx_set_option(bms_ctx* ctx, const char* name, int64_t value);
int bms_ctx_get_option(bms_ctx* ctx, const char* name, int64_t* value);
/* cap on the grid work space in bytes (time axis is processed in chunks that fit); 0 = default: min(96 GB, a third of the device
 * memory that is free at the time).  With the default a call that runs out of device memory halves the cap and tries again. */
int bms_ctx_set_workspace_limit(bms_ctx* ctx, uint64_t bytes);
/* For short-lived callers: ONE device allocation of `bytes` (0: one and a half times the work-space cap) from which the context carves
 * its work-space buffers afterwards, so that the first full-size call of the process allocates nothing (device allocations cost
 * 70 - 120 ms per GB on this platform: the first device-resident map_to_superrest_frame of a process took 2.45 - 3.3 s, the second
 * 0.92 s).  May be called again to add room.  No reference counterpart. */
int bms_ctx_reserve(bms_ctx* ctx, uint64_t bytes);
/* Diagnostics of the evaluating product (the dense route's synthesis + spline evaluation): out[0] = tiles launched since the last
 * reset, out[1] = tiles whose samples left the window of output times staged in LDS (non-uniform time axes, strong boosts: same
 * results through global memory, slower), out[2] = per-column marches continued from global memory.  No reference counterpart. */
int bms_ctx_get_eval_stats(bms_ctx* ctx, int64_t* out /* [3] */, int reset);
/* Which kernel served the rotations (bms_rotate_const / bms_rotate_series and the transforms' rotation of the modes): out[0], out[1],
 * out[2] = launches of the LDS-resident, the staged matrix-core and the VALU kernel since the last reset, out[3] = waves per
 * workgroup (4, 3, 2 or 1, by ell_max) of the most recent VALU launch, 0 if there was none.  Host counters; no reference counterpart. */
int bms_ctx_get_rotate_stats(bms_ctx* ctx, int64_t* out /* [4] */, int reset);
/* Which instance of the back substitution + evaluation on the grid served the transformations: out[0] = kernel launches that read the
 * output times from the window staged in LDS (the lanes of a wave within a few samples of each other), out[1] = launches of the
 * instance that gathers them (large supertranslations, strong boosts at large |t|), since the last reset.  One call of a
 * transformation makes one launch per run of time tiles of the same kind.  Host counters; no reference counterpart. */
int bms_ctx_get_backward_stats(bms_ctx* ctx, int64_t* out /* [2] */, int reset);
/* STREAM-ORDERED RETURN.  bms_transform_modes and bms_transform_modes_shard return WITHOUT waiting for the device when all of this
 * holds: the data is device-resident (mem == BMS_DEVICE, the result goes to a device pointer); the context runs on a stream the caller
 * named (bms_ctx_set_stream with a handle, or bms_ctx_use_default_stream -- with the context's own stream the caller has nothing to
 * order on, so those calls wait); the call is warm, i.e. every table it needs was kept by the context and nothing was copied out of
 * host memory for it (a first call, a call on a new time axis or transformation, a call that runs in several chunks or again after
 * a failed allocation all wait as before); and the context option ASYNC_RETURN is on (the default; bms_ctx_set_option(ctx,
 * "ASYNC_RETURN", 0) or the environment variable SCRI_AMD_NO_ASYNC_RETURN when the context is created switch it off).  The contract
 * of such a call: the result, and the moment the input may be overwritten or freed, are ORDERED ON THE CONTEXT'S STREAM -- work the
 * caller queues there afterwards sees the result, and further calls of the context follow in order; the host must not read the
 * result or reuse the input from another stream before bms_ctx_synchronize (the host-side wait) or a wait on that stream of its own.
 * t_out, *n_times_out and *first_index_out are host values and complete at the return.  Errors in the arguments still fail at the
 * call; an error of a kernel surfaces at the next wait.  Host-memory calls, grids sent to the host and every other entry point wait
 * as they always did.  out[0] = calls that returned without waiting since the last reset, out[1] = 1 while one may still be running.
 * Host counters; no reference counterpart. */
int bms_ctx_get_async_stats(bms_ctx* ctx, int64_t* out /* [2] */, int reset);
/* block until all work queued by this context has finished: the host-side wait of a stream-ordered return */
int bms_ctx_synchronize(bms_ctx* ctx);

/* Optional per-kernel timing: when enabled every kernel launch is bracketed by two HIP events on the
 * context's stream; bms_ctx_get_timing synchronises and returns the accumulated milliseconds and launch
 * counts per kernel class since the last reset. */
enum bms_kernel_tag {
  BMS_TAG_ROTATE = 0,          /* rotate_modes_resident_kernel (l <= 27), rotate_modes_mfma_kernel (l <= 33), rotate_modes_kernel */
  BMS_TAG_SETUP = 1,           /* pixel_sort_kernel, pixel_tables_kernel, swsh_kernel (synthesis matrix), bspline table kernels */
  BMS_TAG_GEMM_SYNTHESIS = 2,  /* modes -> grid: zgemm3m_mfma_kernel (with a boost), synthesis_split_kernel or
                                  theta_synthesis_mfma_kernel + phi_synthesis_folded_kernel (without one) */
  BMS_TAG_SPLINE_FORWARD = 3,  /* bspline_forward_modes_kernel, abd_mix_forward_kernel (slope form: spline_forward_kernel) */
  BMS_TAG_SPLINE_BACKWARD = 4, /* bspline_backward_eval_kernel (slope form: spline_backward_eval_kernel, spline_slopes_kernel) */
  BMS_TAG_GEMM_ANALYSIS = 5,   /* dgemm_mfma_kernel / zgemm3m_mfma_kernel, grid -> modes: phi-DFT of the unfused analysis, dense
                                  quadrature beyond n_theta = 104, a column part's analysis */
  BMS_TAG_POINTWISE = 6,       /* psi mixing / affine / Horner kernels, grid products, spline prefix sums and evaluation */
  BMS_TAG_THETA_QUADRATURE = 7, /* theta_quadrature_kernel (second step of the unfused separable analysis) */
  BMS_TAG_ANALYSIS_FUSED = 8,   /* analysis_split_kernel / analysis_fused_kernel (phi-DFT on MFMA + theta quadrature, one kernel) */
  BMS_TAG_ANALYSIS_LARGE = 9,   /* phi_dft_folded_kernel + theta_quadrature_mfma_kernel (grids with n_theta > 40) */
  BMS_TAG_CONSTRAINTS = 10,     /* constraint_kernel (bms_bondi_constraints), bianchi_kernel (bms_bianchi_rhs) */
  BMS_TAG_CUT = 11,             /* cut_kernel and the pointwise kernels around it (bms_supermomentum_on_cut, bms_alpha_perturbation) */
  BMS_TAG_COUNT = 12
};
int bms_ctx_enable_timing(bms_ctx* ctx, int on);
int bms_ctx_get_timing(bms_ctx* ctx, double ms[BMS_TAG_COUNT], int64_t calls[BMS_TAG_COUNT], int reset);

/* ---- rotation of modes ----------------------------------------------------------------------------------
 * replaces _rotate_decomposition_basis_by_constant (scri/rotations.py:346-367) and
 * _rotate_decomposition_basis_by_series (scri/rotations.py:370-392), including the Wigner-D evaluation
 * (sf._Wigner_D_matrices, rotations.py:327,381).  In place on data c16[n_times][ld], modes (l,m),
 * l = ell_min..ell_max at columns l(l+1) - ell_min^2 + m.
 */
int bms_rotate_const(bms_ctx* ctx, void* data, int mem, int64_t n_times, int64_t ld, int ell_min, int ell_max,
                     const double quaternion[4] /* w,x,y,z */);
int bms_rotate_series(bms_ctx* ctx, void* data, int mem, int64_t n_times, int64_t ld, int ell_min, int ell_max,
                      const void* spinors /* c16[n_times][2] = (w + i z, y + i x), same memory space as data */);
/* _rotate_decomposition_basis_by_constant at its own seam (scri/rotations.py:346-367): the caller hands the packed Wigner
 * matrices D (host c16, block l row-major (m', m) at sf._linear_matrix_offset(l, ell_min); rotations.py:327 fills it with
 * sf._Wigner_D_matrices), not the rotor.  data[t, l, m] <- sum_m' data[t, l, m'] D^l[m', m], in place. */
int bms_rotate_const_D(bms_ctx* ctx, void* data, int mem, int64_t n_times, int64_t ld, int ell_min, int ell_max,
                       const void* D_host);
/* packed Wigner-D matrices of one rotor, layout of sf.Wigner_D_matrices (tests/test_rotations.py:163-165):
 * host c16[(4 L^3 - L)/3 ...], block l at sf._linear_matrix_offset(l, ell_min), row-major (m', m) */
int bms_wigner_D(bms_ctx* ctx, const double quaternion[4], int ell_min, int ell_max, void* D_host);

/* ---- BMS transformation of WaveformModes ---------------------------------------------------------------
 * replaces WaveformGrid.from_modes + WaveformGrid.to_modes (scri/waveform_grid.py:331-613, 274-329), i.e.
 * WaveformModes.transform (scri/waveform_modes.py:705-719), after the kwargs have been parsed
 * (process_transformation_kwargs, scri/waveform_grid.py:20-127).
 */
typedef struct {
  int64_t n_times;
  const double* t;      /* host f8[n_times], strictly increasing */
  const void* data;     /* c16[n_times][ld] */
  int64_t ld;           /* row stride (complex elements) */
  int mem;              /* memory space of data, aux_data and of data_out */
  int ell_min, ell_max; /* modes present in data */
  int spin_weight;      /* SpinWeights[dataType], scri/__init__.py:81 */
  int conformal_weight; /* waveform_base.py:445-446 */
  int type_term;        /* enum bms_type_term */
  /* BMS_TERM_PSI only: the n_aux higher-index Weyl scalars psi_{n+1}..psi_4 (psi*_modes kwargs) */
  int n_aux;
  const void* aux_data[4]; /* c16[n_times][aux_ld[i]] */
  int64_t aux_ld[4];
  int aux_ell_min[4], aux_ell_max[4], aux_spin[4];
  double aux_coeff[4]; /* scipy.special.comb(5 - n, 5 - n_i), waveform_grid.py:547 */
  int aux_power[4];    /* n_i - n */
} bms_wm_input;

typedef struct {
  const void* supertranslation; /* host c16[(ell_max_supertranslation+1)^2], l from 0 */
  int ell_max_supertranslation; /* >= 1 (the reference pads to 4 modes) */
  double frame_rotation[4];     /* unit quaternion w,x,y,z */
  double boost_velocity[3];
  int n_theta, n_phi;           /* equiangular grid, theta includes both poles */
  int ell_max_out;              /* largest l of the output modes (smallest is |spin_weight|) */
} bms_transformation;

/* t_out: host f8[n_times]; data_out: c16[n_times][(ell_max_out+1)^2 - s^2] (caller allocates n_times rows);
 * the first *n_times_out rows are valid on return. */
int bms_transform_modes(bms_ctx* ctx, const bms_wm_input* in, const bms_transformation* tr, double* t_out,
                        void* data_out, int64_t* n_times_out);

/* Time-axis sharding (one process per GPU).  A rank holds rows [data_row0, data_row0 + data_rows) of the global
 * data (in->data / in->aux_data point at row data_row0; in->t and in->n_times stay GLOBAL) and produces the
 * output samples whose global input index lies in [out_i0, out_i1) (intersected with the valid window of
 * scri/waveform_grid.py:564-568).  bms_shard_plan returns the rows a rank must hold for that
 * (spline halo + boost/supertranslation time skew): need_rows = [first, one-past-last];
 * window = the global valid output index range [i_lo, i_hi). */
typedef struct {
  int64_t data_row0, data_rows;
  int64_t out_i0, out_i1;
  /* Pixel-column partition (SURVEY 8(e) plan B, for boosts whose time skew makes the row halo comparable to a time
   * shard): with col_parts > 1 the call synthesises, splines and analyses only part col_part of the grid columns and
   * data_out receives that part's CONTRIBUTION to every output sample (the analysis is linear in the grid columns):
   * the sum over the col_parts parts is the result, i.e. one reduce-scatter over ranks.  0 or 1: all columns. */
  int32_t col_part, col_parts;
} bms_shard;
int bms_shard_plan(bms_ctx* ctx, const double* t, int64_t n_times, const bms_transformation* tr, int64_t out_i0,
                   int64_t out_i1, int64_t need_rows[2], int64_t window[2]);
/* bms_transform_modes for HOST arrays as a three-stage pipeline over `pieces` time shards of the output range: upload of
 * shard k + 1, kernels of shard k and download of shard k - 1 run side by side on three streams (a long series in host memory
 * waits for PCIe, not for the kernels).  in->mem must be BMS_HOST; psi companions (n_aux 0..4, host rows like the data, any
 * aux_ld >= their number of modes) travel up with the rows of every shard.  data_out: host
 * c16[window rows][n_out], t_out f8[window rows] (size them with bms_output_window); full rate needs page-locked arrays
 * (bms_host_alloc for the result, bms_host_register for a caller's input).  Same results as the sharded path. */
int bms_transform_modes_pipelined(bms_ctx* ctx, const bms_wm_input* in, const bms_transformation* tr, int pieces, double* t_out,
                                  void* data_out, int64_t* n_times_out);

/* The same pipeline for AsymptoticBondiData.transform (scri/asymptotic_bondi_data/transformations.py:205-423): host arrays in and
 * out, raw = c16[6][n_times][(ell_max+1)^2], raw_out = c16[6][n_times_out][(ell_max_out+1)^2] (best page-locked: bms_host_alloc /
 * bms_host_register); the rows of the six fields of one time shard travel up while the previous shard is transformed and the one
 * before it travels down.  u_out must hold n_times doubles.  Results equal bms_transform_abd's to rounding. */
int bms_transform_abd_pipelined(bms_ctx* ctx, const double* u, const void* raw, int64_t n_times, int ell_max,
                                const bms_transformation* tr, int pieces, double* u_out, void* raw_out, int64_t* n_times_out);

/* One process, several GPUs, host arrays in and out (the callers the reference has: scri/waveform_modes.py:705-719 and
 * scri/asymptotic_bondi_data/transformations.py:391-412 take numpy arrays in one process).  The output window is cut into `pieces`
 * exactly as the two calls above cut it; these transform pieces [piece0, piece1) only and put them at their place in t_out / data_out,
 * which are the arrays of the WHOLE window (page-locked memory from bms_host_alloc / bms_host_register is visible to every device);
 * *n_times_out is the whole window's row count.  The caller deals the pieces over one context per device and calls from one host
 * thread per context (the library is re-entrant per context): every device receives its own rows + halo at upload time, so nothing
 * travels GPU to GPU, and the result equals the one-context call with the same `pieces` bit for bit. */
int bms_transform_modes_pipelined_part(bms_ctx* ctx, const bms_wm_input* in, const bms_transformation* tr, int pieces, int piece0,
                                       int piece1, double* t_out, void* data_out, int64_t* n_times_out);
int bms_transform_abd_pipelined_part(bms_ctx* ctx, const double* u, const void* raw, int64_t n_times, int ell_max,
                                     const bms_transformation* tr, int pieces, int piece0, int piece1, double* u_out, void* raw_out,
                                     int64_t* n_times_out);
/* The dealing itself, for bindings that do not want to manage threads: ONE call takes the n_ctx contexts (one per device; created
 * by the caller with bms_ctx_create, each listed once), deals the `pieces` time shards over them in contiguous runs and runs
 * bms_transform_*_pipelined_part on one host thread per context.  Host arrays in and out as above.  On failure the status of the first
 * failing context is returned and bms_last_error(ctxs[0]) names it ("context k (device d): ..."). */
int bms_transform_modes_multi(bms_ctx* const* ctxs, int n_ctx, const bms_wm_input* in, const bms_transformation* tr, int pieces,
                              double* t_out, void* data_out, int64_t* n_times_out);
int bms_transform_abd_multi(bms_ctx* const* ctxs, int n_ctx, const double* u, const void* raw, int64_t n_times, int ell_max,
                            const bms_transformation* tr, int pieces, double* u_out, void* raw_out, int64_t* n_times_out);
/* Several series under one transformation: the extra trailing data dimensions of the reference's waveform objects
 * (scri/waveform_grid.py:299-308 `final_dim`, :574-594): every trailing index is an independent series on the same time axis.
 * Arrays are in the REFERENCE'S layout -- the trailing index fastest, as numpy stores data[N, n_modes, F]: in->data is
 * c16[n_times][in->ld] with element (mode, j) of a row at column mode * n_series + j (in->ld >= n_modes n_series); psi companions
 * likewise.  Exactly one of data_out -- c16[n_times][n_out n_series] -- and grid_out -- c16[n_times][n_theta n_phi n_series],
 * WaveformGrid.from_modes -- is non-NULL, same convention, in the memory space in->mem; the first *n_times_out rows are written.
 * The block crosses PCIe once as it is (the permutation to one block of columns per series and back runs on the device); time axis,
 * spline tables, per-direction tables and window are set up once and shared by the series. */
int bms_transform_modes_series(bms_ctx* ctx, const bms_wm_input* in, int n_series, const bms_transformation* tr, double* t_out,
                               void* data_out, void* grid_out, int64_t* n_times_out);
/* WaveformGrid.from_modes on its own (scri/waveform_grid.py:331-613): the first half of bms_transform_modes -- the field on the
 * boost-distorted grid at the new time slices, grid_out c16[n_times][n_theta * n_phi] (only the first *n_times_out rows are
 * written; grid order, theta-major), in the memory space in->mem.  bms_map2salm of it is WaveformGrid.to_modes (:274-329). */
int bms_modes_to_grid(bms_ctx* ctx, const bms_wm_input* in, const bms_transformation* tr, double* t_out, void* grid_out,
                      int64_t* n_times_out);
/* The valid output window [i_lo, i_hi) of a transformation (scri/waveform_grid.py:564-568; abd != 0: the
 * AsymptoticBondiData flavour, transformations.py:391-396), from the same per-direction tables the transformations
 * compute on the GPU: output sample r of bms_transform_modes / bms_transform_abd has input index i_lo + r, so a caller
 * can size its (device) output buffers exactly: i_hi - i_lo rows. */
int bms_output_window(bms_ctx* ctx, const double* t, int64_t n_times, const bms_transformation* tr, int abd,
                      int64_t window[2]);
/* as bms_transform_modes; t_out/data_out receive only the rank's samples, *first_index_out their first global
 * input index (output row r corresponds to input index *first_index_out + r).  shard == NULL: whole series. */
int bms_transform_modes_shard(bms_ctx* ctx, const bms_wm_input* in, const bms_transformation* tr,
                              const bms_shard* shard, double* t_out, void* data_out, int64_t* n_times_out,
                              int64_t* first_index_out);

/* ---- page-locked host memory -----------------------------------------------------------------------------
 * Results that go back to host arrays (mem = BMS_HOST) cross PCIe at full rate only into page-locked memory; a caller
 * that lets the library allocate its result arrays gets that without a staging copy (scri_amd/_lib.py: pinned_empty).
 * NULL on failure. */
void* bms_host_alloc(uint64_t bytes);
void bms_host_free(void* p);
/* The other direction: page-lock a caller's INPUT array in place (and release it), so that repeated transformations of
 * the same host array upload at PCIe rate instead of through the runtime's staging copy.  Registration costs about one
 * upload; scri_amd/engine.py registers an array the second time it sees it and unregisters when it is freed. */
int bms_host_register(void* p, uint64_t bytes);
int bms_host_unregister(void* p);

/* ---- BMS transformation of AsymptoticBondiData ---------------------------------------------------------
 * replaces AsymptoticBondiData.transform (scri/asymptotic_bondi_data/transformations.py:199-431) after
 * _process_transformation_kwargs (:8-97).  raw: c16[6][n_times][(ell_max+1)^2] = psi0..psi4, sigma
 * (scri/asymptotic_bondi_data/__init__.py:36-75).  tr->n_theta = tr->n_phi = 2 working_ell_max + 1;
 * tr->ell_max_out = output_ell_max.  raw_out: c16[6][n_times][(ell_max_out+1)^2] (field stride n_times rows).
 */
int bms_transform_abd(bms_ctx* ctx, const double* u, const void* raw, int mem, int64_t n_times, int ell_max,
                      const bms_transformation* tr, double* u_out, void* raw_out, int64_t* n_times_out);

/* Time-axis shard of the same transformation (cfg5 of BASELINE.json: one shard per GPU).  u and n_times stay GLOBAL;
 * raw holds rows [shard->data_row0, +data_rows) of every field, c16[6][data_rows][(ell_max+1)^2]; the call produces the
 * output samples whose global input index lies in [out_i0, out_i1) (intersected with the valid window,
 * transformations.py:391-396): u_out[*n_times_out], raw_out c16[6][out_i1 - out_i0][(ell_max_out+1)^2] (only the first
 * *n_times_out rows of each field are written), *first_index_out = global input index of output row 0.
 * bms_shard_plan gives the rows a shard must hold.  shard == NULL: whole series (== bms_transform_abd). */
int bms_transform_abd_shard(bms_ctx* ctx, const double* u, const void* raw, int mem, int64_t n_times, int ell_max,
                            const bms_transformation* tr, const bms_shard* shard, double* u_out, void* raw_out,
                            int64_t* n_times_out, int64_t* first_index_out);

/* ---- building blocks (exported for the parity tests and for the "next" rows of the scope table) --------- */
/* boosted_grid / R_j_k (transformations.py:100-148, waveform_grid.py:130-174): host f8[n_theta][n_phi][4] */
int bms_rotor_grid(bms_ctx* ctx, const double frame_rotation[4], const double boost_velocity[3], int n_theta,
                   int n_phi, double* rotors_host);
/* Does that rotor grid keep its rings?  Returns 1 and the ring colatitudes Theta_j (thetas_out[n_theta]) when every rotor is
 * frame_rotation * R(Theta_j, phi'_k) -- no boost (Theta_j = theta'_j), or a boost along the polar axis of the rotated grid, whose
 * aberration (waveform_grid.py:141-161) only moves whole rings -- and 0 otherwise; < 0 on bad arguments.  Host only (no context):
 * the test the transformations use to pick the separable synthesis, made on the rotors themselves. */
int bms_ring_colatitudes(const double frame_rotation[4], const double boost_velocity[3], int n_theta, int n_phi,
                         double* thetas_out);
/* conformal_factors (transformations.py:151-196) on the given rotors (host f8[n][4]): k = 1 / (gamma (1 - v.r)) with r the
 * direction the rotor takes z to, eth k / k (spin weight 1, c16[n]), 1/k and 1/k^3.  Host evaluation with the code the
 * transformations run per direction on the GPU (pixel_math.h); ctx may be NULL. */
int bms_conformal_factors(bms_ctx* ctx, const double boost_velocity[3], const double* rotors_host, int64_t n_rotors,
                          double* k, void* ethk_over_k, double* one_over_k, double* one_over_k_cubed);
/* sf.SWSH_grid(R, s, ell_max)[..., ell_min^2:] : host c16[n_rotors][(ell_max+1)^2 - ell_min^2].  ctx = NULL: host
 * evaluation of the header the kernel compiles (wigner.h; double-double recurrence, correctly rounded values). */
int bms_swsh_grid(bms_ctx* ctx, const double* rotors_host /* f8[n][4] */, int64_t n_rotors, int spin, int ell_min,
                  int ell_max, void* Y_host);
/* spinsfast.map2salm(grid[n_maps][n_theta][n_phi], s, ell_max)[..., ell_min^2:] (waveform_grid.py:303-307) */
int bms_map2salm(bms_ctx* ctx, const void* grid, int mem, int64_t n_maps, int n_theta, int n_phi, int spin,
                 int ell_min, int ell_max, void* modes_out);
/* sf.Modes.evaluate(R): out[t][p] = sum_k modes[t][k] sY_k(R_p) at arbitrary rotors -- the dense contraction of
 * scri/asymptotic_bondi_data/transformations.py:312-334, waveform_grid.py:475-484, bms_transformations.py:179 on its own.
 * modes: c16[n_rows][ld] with l = ell_min..ell_max; rotors: host f8[n_rotors][4]; out: c16[n_rows][n_rotors] in `mem`. */
int bms_evaluate_modes(bms_ctx* ctx, const void* modes, int mem, int64_t n_rows, int64_t ld, int spin, int ell_min,
                       int ell_max, const double* rotors_host, int64_t n_rotors, void* out);
/* spinsfast.salm2map(modes[n_maps][(ell_max+1)^2], s, ell_max, n_theta, n_phi) -> c16[n_maps][n_theta][n_phi] */
int bms_salm2map(bms_ctx* ctx, const void* modes, int mem, int64_t n_maps, int spin, int ell_max, int n_theta, int n_phi,
                 void* grid_out);
/* not-a-knot cubic spline through (x[n], y c16[n][n_cols]) evaluated at x_new[n_new] (all x host; y/out in
 * `mem`): scipy CubicSpline(x, y)(x_new) of waveform_base.py:964 / modes_time_series.py:90 */
int bms_cubic_spline(bms_ctx* ctx, const double* x, int64_t n, const void* y, int64_t ld, int64_t n_cols, int mem,
                     const double* x_new, int64_t n_new, void* out);

/* ---- "next" rows of the scope table: time-series calculus and grid products ------------- */
/* scipy CubicSpline(x, y).derivative(order) (order 1..3), the spline itself (0) or .antiderivative(-order) (order -1 .. -16;
 * zero at x[0]) evaluated at x_new (any order of samples): ModesTimeSeries.interpolate(new_time, derivative_order) and
 * .dot / .ddot / .int / .iint (scri/modes_time_series.py:72-126).  y: c16[n][ld], out: c16[n_new][n_cols], both in `mem`. */
int bms_spline_derivative(bms_ctx* ctx, const double* x, int64_t n, const void* y, int64_t ld, int64_t n_cols, int mem,
                          const double* x_new, int64_t n_new, int order, void* out);
/* The mode-space operators of spherical_functions.Modes / scri.ModesTimeSeries (scri/modes_time_series.py:7-139 and the
 * algebra it inherits: eth, ethbar, bar, real, imag, +, -, scalar factors, truncate_ell) as ONE map along the mode axis,
 *     out[t][j] = r_t ( ca_j op_a(a[t][ia_j]) + cb_j op_b(b[t][ib_j]) ),   op = identity or complex conjugation,
 * with per-column tables the caller derives from (l, m, s) (scri_amd/device_series.py): idx_* int32[n_cols] (-1: zero),
 * coef_* c16[n_cols], host arrays.  a c16[n_rows][ld_a], b (may be NULL) and out c16[n_rows][ld_out] live in `mem`;
 * row_scale f8[n_rows] (may be NULL) too.  This is what keeps the charge and frame-fixing loops of
 * scri/asymptotic_bondi_data/bms_charges.py:14-286 resident in HBM between transformations. */
int bms_mode_map(bms_ctx* ctx, void* out, int64_t ld_out, int64_t n_rows, int n_cols, const void* a, int64_t ld_a,
                 const int32_t* idx_a, const void* coef_a, int conj_a, const void* b, int64_t ld_b, const int32_t* idx_b,
                 const void* coef_b, int conj_b, const double* row_scale, int mem);
/* WaveformBase.norm (scri/waveform_base.py:19-35,535-551): out[t] = sum_j |data[t][j]|^2, or its square root with take_sqrt
 * (complex_array_norm / complex_array_abs), the terms re^2 + im^2 added one at a time in column order, no fused multiply-adds --
 * the reference's loop, so the sums agree with it to the bit (and with them the parity-violation measures,
 * scri/waveform_modes.py:769-778 ...).  data c16[n_rows][ld] and out f8[n_rows] live in `mem`. */
int bms_row_norm(bms_ctx* ctx, const void* data, int64_t ld, int64_t n_rows, int n_cols, int mem, int take_sqrt, double* out);
/* Polar form of a series, WaveformBase.abs / arg / arg_unwrapped (scri/waveform_base.py:520-533): data c16[n_rows][ld] (the first n_cols
 * columns of a row) -> abs_out = hypot(re, im) and arg_out = atan2(im, re), f8[n_rows][ld_out] each, in `mem` like the data; either
 * (not both) may be NULL.  IEEE special cases: |inf + nan i| = inf, arg(+0 + 0i) = 0, arg(-1 + 0i) = pi, arg(-1 - 0i) = -pi, a NaN part
 * gives a NaN angle.  unwrap != 0: arg_out is the angle unwrapped down the rows, numpy.unwrap(numpy.angle(data), axis=0) stated as an
 * integer scan: with p the angle above and d = p[i][j] - p[i-1][j], k[i][j] = -1 if d > pi, +1 if d < -pi, else 0 (pi the double,
 * k[0][j] = 0), K = the running sum of k down column j, arg_out[i][j] = p[i][j] + 2 pi K[i][j] rounded once; row 0 is p[0].  From the
 * first NaN angle of a column on, that column is NaN (as numpy's cumsum leaves it); infinite parts give finite angles.  Where |d| is
 * within a rounding of pi numpy's rounded `mod` may decide the other way.  Host and device memory give the same
 * bits.  BMS_ERR_INVALID: NULL data, both outputs NULL, a bad mem, negative sizes, ld < n_cols, ld_out < n_cols; n_rows == 0 or
 * n_cols == 0 writes nothing. */
int bms_polar(bms_ctx* ctx, const void* data, int64_t ld, int64_t n_rows, int n_cols, int mem, int unwrap, double* abs_out,
              double* arg_out, int64_t ld_out);
/* rows per tile of the wrap-count scan behind bms_polar (series lengths around its multiples cross a tile edge) */
int64_t bms_polar_tile_rows(void);
/* *count = the elements of data c16[n_rows][ld] (first n_cols columns, in `mem`) with a non-finite real or imaginary part, *first_row =
 * the first row that holds one, -1 if none (both host integers): the "data must be finite" check of WaveformBase.ensure_validity
 * (scri/waveform_base.py:299-367).  n_rows == 0 or n_cols == 0 writes nothing. */
int bms_count_nonfinite(bms_ctx* ctx, const void* data, int64_t ld, int64_t n_rows, int n_cols, int mem, int64_t* count,
                        int64_t* first_row);
/* The library's dense products on operands of the caller: what every boosted synthesis, the dense and phi-DFT analysis, the psi fields of
 * AsymptoticBondiData and bms_rotate_const_D run through, callable by itself (and so testable against a reference).
 *   form BMS_PRODUCT_COMPLEX     A, B, C complex128 interleaved, three real matrix products per complex one ("3M")
 *        BMS_PRODUCT_COMPLEX_4M  the same operands, the plain four-product form (componentwise-accurate imaginary parts)
 *        BMS_PRODUCT_REAL        A, B, C fp64
 * Row-major, pitches lda / ldb / ldc in DOUBLES whatever the form.  With P = 64 complex columns and R = 8 rows (real form: P = 128
 * columns, R = 16 rows):
 *   read     of A: the K entries of rows 0 .. M-1 and nothing else -- not the rest of a pitch, not a row >= M;
 *            of B: R ceil(K / R) rows x P ceil(N / P) columns.  Rows >= K and columns >= N have to EXIST and be FINITE; their values
 *            reach no result (pad rows are multiplied by zeros, pad columns feed results nobody stores), so they need not be zero;
 *            of col_off / col_scale (either may be NULL: no offset / scale 1): 2N doubles, per real and imaginary column (real form: N).
 *   written  the 2N (real form: N) leading doubles of rows 0 .. M-1 of C, nothing else.
 *   refused  BMS_ERR_INVALID: a NULL ctx, A, B or C; form outside 0 .. 2; M < 0 or N < 0; K < 1; lda < 2K, ldc < 2N, ldb < 2 P ceil(N / P)
 *            (real form: K, N, P ceil(N / P)); A or B not 16-byte aligned, lda or ldb odd; complex forms: C not 16-byte aligned or ldc
 *            odd (real form: C not 8-byte aligned); col_off or col_scale not 8-byte aligned; real form: an odd K.  M == 0 or N == 0
 *            (with arguments that pass the above) is BMS_OK with nothing written.  BMS_ERR_UNSUPPORTED: N or K of 2^31, more than 2^30 tiles.
 * Nothing is launched by a refused call. */
enum { BMS_PRODUCT_COMPLEX = 0, BMS_PRODUCT_REAL = 1, BMS_PRODUCT_COMPLEX_4M = 2 };
/* C[M x N] = (A[M x K] . B[K x N] - col_off) * col_scale on the library's matrix-core kernels; all operands device memory of the
 * caller, pitches in doubles, stream-ordered on the context's stream (no host wait). */
int bms_dense_product(bms_ctx* ctx, int form, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                      int64_t M, int64_t N, int64_t K, const void* col_off, const void* col_scale);
/* ModesTimeSeries.grid_multiply (scri/modes_time_series.py:142-202): modes a (spin_a, l = 0..ell_max_a,
 * c16[n_times][(ell_max_a+1)^2]) and b likewise are evaluated on the (2 working_ell_max + 1)^2 equiangular grid
 * (spinsfast.salm2map), multiplied there, and the product is analysed (map2salm, spin spin_a + spin_b) into
 * out c16[n_times][(output_ell_max+1)^2].  Spin weights of the factors and of the product up to +-4 (the boost flux of
 * scri/flux.py multiplies ethbar h, s = -3, with its conjugate). */
int bms_grid_multiply(bms_ctx* ctx, const void* a, int spin_a, int ell_max_a, const void* b, int spin_b, int ell_max_b, int mem,
                      int64_t n_times, int working_ell_max, int output_ell_max, void* out);

/* ---- what feeds the rotation path -------------------------------------------------------- */
/* <Ldt> (f8[n][3]), <LL> (f8[n][3][3]) and the angular velocity omega = -<LL>^-1 <Ldt> (f8[n][3]) of a waveform from its
 * modes data c16[n][ld] (l = ell_min..ell_max) and their cubic-spline time derivative: LdtVector / LLMatrix /
 * angular_velocity of scri/mode_calculations.py:46-57, 298-313, 403-432.  Outputs are host arrays; any may be NULL.
 * A time step's modes and their derivatives are held in the LDS of one workgroup: a range of more modes than fit
 * (5120 with 160 KB: l = 0..70 is the largest range from 0) is BMS_ERR_UNSUPPORTED, here and in bms_corotating_frame /
 * bms_coprecessing_frame, before anything is launched. */
int bms_angular_velocity(bms_ctx* ctx, const double* t, int64_t n_times, const void* data, int64_t ld, int ell_min, int ell_max,
                         int mem, double* ldt_out, double* ll_out, double* omega_out);

/* Frame R[n][4] with R[0] = R0 and dR/dt = (1/2) Omega R, Omega(t) = not-a-knot cubic spline through omega[n][3]:
 * quaternion.integrate_angular_velocity as used by corotating_frame (scri/mode_calculations.py:435-491).  Host routine
 * (sequential in time); ctx may be NULL.  tolerance: absolute tolerance of the integration (<= 0: 1e-12). */
int bms_integrate_angular_velocity(bms_ctx* ctx, const double* t, int64_t n_times, const double* omega, const double R0[4],
                                   double tolerance, double* R_out);

/* ---- frame construction on the device (DESIGN: "Frames as scans") ---------------------------------------------------------
 * The chain behind to_corotating_frame / to_coprecessing_frame (scri/rotations.py:14-103, scri/mode_calculations.py:316-491) as GPU
 * kernels: every sequential step of the host versions is a prefix scan.  t is always a host array (n >= 4, strictly increasing);
 * the per-step arrays live in `mem`.  Rotors are f8[n][4] = (w, x, y, z). */
/* The frame of bms_integrate_angular_velocity -- same sub-step rule, same Magnus step -- with the interval rotors E_j formed
 * independently and R_j = E_{j-1} ... E_0 R0 as a prefix product; every R_j is normalised once (R_out[0] = R0 as given).
 * omega f8[n][3], R_out f8[n][4].  tolerance <= 0: 1e-12.  One difference from the host routine: an interval is cut into at most 2^20
 * sub-steps (the host routine has no cap), so a series that turns by more than about 2e5 radians between two samples is integrated
 * less accurately than the host routine would; no status reports it. */
int bms_frame_from_angular_velocity(bms_ctx* ctx, const double* t, int64_t n_times, const double* omega, int mem, const double R0[4],
                                    double tolerance, double* R_out);
/* Unit eigenvector of the largest eigenvalue of each symmetric matrix ll f8[n][9] (cyclic Jacobi), made continuous in time by the
 * rule of LLDominantEigenvector (scri/mode_calculations.py:316-363): at rough_index (0 <= rough_index < n) the axis points along
 * `rough`, and going outwards a vector is flipped when it is further from its neighbour than its own length.  axis_out f8[n][3].
 * n >= 1. */
int bms_dominant_axis(bms_ctx* ctx, const double* ll, int64_t n_times, int mem, const double rough[3], int64_t rough_index,
                      double* axis_out);
/* numpy-quaternion's minimal_rotation: R' = R exp(gamma z / 2) with gamma-dot / 2 = Re[Rdot z R^-1], derivative and integral by
 * not-a-knot cubic splines, `iterations` >= 1 times.  R_out may be R. */
int bms_minimal_rotation(bms_ctx* ctx, const double* t, int64_t n_times, const double* R, int mem, int iterations, double* R_out);
/* omega f8[n][3] = vector part of 2 Rdot R^-1, Rdot from the not-a-knot cubic spline through the components (quaternion.angular_velocity) */
int bms_rotor_angular_velocity(bms_ctx* ctx, const double* t, int64_t n_times, const double* R, int mem, double* omega_out);
/* In place on frame f8[n][4]: frame <- frame * right (right may be NULL), normalised; with truncate_tolerance > 0 then
 * frame <- exp(round(log(frame) 2^k) / 2^k), k = -floor(log2(2 truncate_tolerance)) (scri/rotations.py:86-90), the rounded logarithm
 * to log_out f8[n][4] (may be NULL).  spinors_out (may be NULL): c16[n][2] = (w + i z, y + i x), what bms_rotate_series takes.  All
 * arrays in `mem`. */
int bms_frame_adjust(bms_ctx* ctx, double* frame, int64_t n_times, int mem, const double right[4], double truncate_tolerance,
                     double* log_out, void* spinors_out);
/* corotating_frame (scri/mode_calculations.py:435-491) of modes data c16[n][ld] in `mem`: the kernels of bms_angular_velocity, the
 * spline of omega, the interval rotors and their prefix product, without leaving the device.  The frame goes to frame_dev (DEVICE
 * f8[n][4], whatever `mem` is), and to the host arrays frame_out f8[n][4] and omega_out f8[n][3] where those are not NULL. */
int bms_corotating_frame(bms_ctx* ctx, const double* t, int64_t n_times, const void* data, int64_t ld, int ell_min, int ell_max, int mem,
                         const double R0[4], double tolerance, double* frame_dev, double* frame_out, double* omega_out);
/* The coprecessing frame (scri/rotations.py:14-49) of modes data c16[n][ld] in `mem`: <LL>, its dominant axis v (as
 * bms_dominant_axis), the rotor sqrt(-v z) taking z to v and `iterations` >= 1 rounds of bms_minimal_rotation.  frame_dev (DEVICE
 * f8[n][4]) and the host arrays frame_out f8[n][4], axis_out f8[n][3] may be NULL; with neither frame asked for only the axis is
 * computed (LLDominantEigenvector), which needs no spline: then n >= 1 and t, iterations are not read. */
int bms_coprecessing_frame(bms_ctx* ctx, const double* t, int64_t n_times, const void* data, int64_t ld, int ell_min, int ell_max, int mem,
                           const double rough[3], int64_t rough_index, int iterations, double* frame_dev, double* frame_out,
                           double* axis_out);
/* quaternion.squad (scri/waveform_base.py:957 interpolates the frame of a waveform with it), as scri_amd.quaternions.squad states it:
 * the rotors R_in f8[n][4] at the times t_in[n] (host, finite, strictly increasing, n >= 2; the steps need not be uniform) interpolated
 * to the arguments t_out[m] (host, finite, in ANY order, m >= 0), out f8[m][4]; R_in and out live in `mem` and must not overlap.
 *     out = slerp( slerp(R_i, R_{i+1}, tau), slerp(A_i, B_i, tau), 2 tau (1 - tau) ),   slerp(p, q, tau) = p exp(tau log(p^-1 q)),
 *     A_i = R_i exp( (-log(R_i^-1 R_{i+1}) + log(R_{i-1}^-1 R_i) h_i / h_{i-1}) / 4 ),
 *     B_i = R_{i+1} exp( -(log(R_{i+1}^-1 R_{i+2}) h_i / h_{i+1} - log(R_i^-1 R_{i+1})) / 4 ),   h_i = t_{i+1} - t_i,
 * with the end rules A_0 = R_0, A_{n-1} = R_{n-1}, B_{n-2} = R_{n-1}, B_{n-1} = R_n applied in this order (they meet at n = 2 and 3).
 * Interval: i = clip(#{k: t_in[k] <= t} - 1, 0, n - 1), tau = (t - t_i) / (t_{i+1} - t_i); an argument below t_in[0] takes interval 0
 * with tau < 0, and interval n - 1 runs to the mirrored knot t_n = 2 t_{n-1} - t_{n-2} with R_n = R_{n-1} R_{n-2}^-1 R_{n-1}.  The
 * logarithm has a zero vector part where the vector norm is <= 1e-300.  Two launches: control points per knot, then one thread per
 * argument; every operation is in the order of the numpy statement, so host and device memory give the same bits and an argument's
 * value does not depend on the others.  A NULL pointer, a bad `mem`, n < 2, m < 0, non-finite or not strictly increasing t_in and
 * non-finite t_out are refused (BMS_ERR_INVALID) before anything is staged; the rotors themselves are not inspected. */
int bms_squad(bms_ctx* ctx, const double* t_in, int64_t n, const void* R_in, int mem, const double* t_out, int64_t m, void* out);
/* blocks the scans of the frame chain (the prefix product of rotors, the sign maps of the axis) cut a series of n steps into (tests
 * place series lengths around one block and around one chunk of block totals); a size, not a status */
int64_t bms_frame_scan_blocks(int64_t n);

/* ---- time-and-phase alignment of two waveforms from correlation moments (scri_amd/alignment.py; DESIGN: "Alignment as moments") ----
 * The moving waveform A: time axis ta[na] (host, na >= 4, strictly increasing), values ya and knot slopes sa of its not-a-knot cubic
 * spline, both c16[na][ld_a] in `mem` (the slopes are bms_spline_derivative(order = 1) evaluated at ta itself).  The fixed waveform B:
 * window times tw[nw] and quadrature weights w[nw] (host, nw >= 2), b = its first window row, c16[nw][ld_b] in `mem`.  Common column k
 * (k < n_cols) is column col_a[k] of A and col_b[k] of B (host int32 tables).  The spline is evaluated in the local Hermite form of
 * bms_spline_derivative; the interval of an argument is the last knot <= it (the last interval closed; an argument outside ta takes the
 * end interval's cubic).
 *
 * bms_align_moments: for every offset dts[k] (host, nd of them, finite, ascending) and derivative order o <= order (0, 1 or 2)
 *     out[o][k][0]             = (d/ddt)^o  sum_i w_i sum_c |A_c(tw_i + dt)|^2
 *     out[o][k][1 + 2 s, + 1]  = Re, Im of (d/ddt)^o  sum_i w_i sum_{c: m_slot[c] = s} A_c(tw_i + dt) conj(B_ic)
 * out: host f8[order + 1][nd][1 + 2 n_slots]; m_slot: host int32[n_cols] in [0, n_slots).  The sums are formed in a fixed order that
 * does not depend on the other offsets of the call, nor on `mem`: an offset's moments are the same bits scanned alone or among
 * thousands.  Limits (BMS_ERR_UNSUPPORTED): na <= 2^31, n_slots <= 16385; nothing else bounds the sizes (long offset lists and windows
 * run as several launches).
 *
 * bms_align_residual: out[0] = sum_i w_i sum_c |A_c(tw_i + dt) e^{i m_of[c] dphi} - B_ic|^2 and out[1] = sum_i w_i sum_c |B_ic|^2,
 * summed directly (non-negative, smooth at a perfect match); m_of: host int32[n_cols]. */
int bms_align_moments(bms_ctx* ctx, const double* ta, int64_t na, const void* ya, const void* sa, int64_t ld_a, const int32_t* col_a,
                      const double* tw, const double* w, int64_t nw, const void* b, int64_t ld_b, const int32_t* col_b, int n_cols,
                      const int32_t* m_slot, int n_slots, int mem, const double* dts, int64_t nd, int order, double* out);
int bms_align_residual(bms_ctx* ctx, const double* ta, int64_t na, const void* ya, const void* sa, int64_t ld_a, const int32_t* col_a,
                       const double* tw, const double* w, int64_t nw, const void* b, int64_t ld_b, const int32_t* col_b, int n_cols,
                       const int32_t* m_of, int mem, double dt, double dphi, double out[2]);

/* ---- bit transforms of the storage formats (scri/utilities.py:194-406), bit-exact ------------ */
/* xor_timeseries (reverse = 0) / xor_timeseries_reverse (reverse = 1), in place: data viewed as uint64[n_rows][words_per_row],
 * time along the rows; row 0 is unchanged, row i becomes row[i-1] ^ row[i] (forward) or the running XOR (reverse). */
int bms_xor_timeseries(bms_ctx* ctx, void* data, int mem, int64_t n_rows, int64_t words_per_row, int reverse);
/* multishuffle(shuffle_widths, forward)(a): n elements of sum(widths) in {8,16,32,64} bits; widths from the most significant
 * piece down.  in and out must not overlap. */
int bms_multishuffle(bms_ctx* ctx, const void* in, void* out, int mem, int64_t n, const int* widths, int n_widths, int forward);
/* fletcher32(data): 16-bit words, modulus 65535; returns c1 << 16 | c0 */
int bms_fletcher32(bms_ctx* ctx, const void* data, int mem, int64_t n_bytes, uint32_t* checksum);

/* ---- the corotating paired-XOR storage form (scri/SpEC/file_io/corotating_paired_xor.py: the in-memory core of save, :70-90, and
 * of load, :240,255), one fused kernel each way.  The files themselves (HDF5, JSON) are the caller's business.
 * pack: data c16[n_times][ld] (ld >= n_modes), modes l = ell_min .. ell_max of a waveform ALREADY in the corotating frame ->
 * words_out u64[n_times][2 n_modes].  Per time step: conjugate pairs s = (f[l,m] + conj f[l,-m]) / sqrt2 in column +m,
 * d = (f[l,m] - conj f[l,-m]) / sqrt2 in column -m (waveform_modes.py:659-685); every real and imaginary part rounded to a multiple
 * of 2^-e, e = floor(-log2(norm tolerance / sqrt(n_modes))) with the norm of that time step (:458-476); -0.0 replaced by +0.0; XOR with
 * the packed words of the previous time step (utilities.py:195-217).  The arithmetic is the reference's operation for operation, so
 * the words equal its own wherever the norm's exponent does not hinge on the order of the norm's sum.
 * A time step that cannot be packed -- a non-finite value, zero norm (the reference stores NaN there), 2^e outside the doubles -- fails
 * the call with BMS_ERR_INVALID; *first_bad_row (optional) is the first such row, -1 if there is none, and words_out is then not to be used.
 * BMS_ERR_INVALID also for tolerance <= 0, ld < n_modes and words_out overlapping data.  `mem` as everywhere: host arrays are staged
 * (in pieces under the work-space cap, each with the row before it; the words do not depend on the pieces), device arrays (16-byte
 * aligned) are used in place. */
int bms_pack_paired_xor(bms_ctx* ctx, const void* data, int64_t ld, int64_t n_times, int ell_min, int ell_max, int mem,
                        double tolerance, void* words_out, int64_t* first_bad_row);
/* unpack: words u64[n_times][2 n_modes] -> data_out c16[n_times][ld_out]: the running XOR down the time steps (utilities.py:220-232)
 * with f[l,m] = (s + d) / sqrt2, f[l,-m] = conj(s - d) / sqrt2 (waveform_modes.py:688-703) on the way out.  Pieces of a host array
 * pass the running XOR on.  data_out must not overlap words. */
int bms_unpack_paired_xor(bms_ctx* ctx, const void* words, int64_t n_times, int ell_min, int ell_max, int mem, void* data_out,
                          int64_t ld_out);
/* rows one tile of the pack kernel owns (tests place series lengths around it); a size, not a status */
int64_t bms_paired_xor_tile_rows(void);

/* ---- extrapolation of finite-radius waveforms to null infinity (scri/extrapolation.py:1270-1474, _Extrapolate) ------------
 * For every time step t and order N = orders[o]: the constant term of the least-squares polynomial of degree N in x = 1/r through
 * the n_radii points (1 / radii[i][t], series[i][t][m]), for each mode m -- numpy.polynomial.polynomial.polyfit(x, y, N)[0] of
 * extrapolation.py:1434 (columns x^k scaled by their norms, Householder QR; one factorisation per step serves every order).
 * series[i]: c16[n_times][ld[i]] (n_modes columns used); radii: f8[n_radii][n_times]; out: c16[n_orders][n_times][n_modes]; all three
 * in `mem` (series and ld themselves are host arrays).  0 <= orders[o] < n_radii <= 64, orders[o] <= 15; negative orders (copies of
 * one radius) are the caller's.  A step whose fit of order N is rank deficient (min |R_kk| <= n_radii eps max |R_kk|, numpy's rcond)
 * gets NaN in that order's row, and is counted in n_deficient[o] (host int64[n_orders], may be NULL).  Host memory goes through the
 * device in `blocks` pipelined blocks of time steps (0: chosen by size); the result does not depend on the number of blocks. */
int bms_extrapolate(bms_ctx* ctx, int n_radii, const void* const* series, const int64_t* ld, int mem, int64_t n_times,
                    int64_t n_modes, const double* radii, int n_orders, const int* orders, void* out, int blocks,
                    int64_t* n_deficient);

/* ---- the precessing sample waveform (scri/sample_waveforms.py:383-533, fake_precessing_waveform) and its finite-radius family -----
 * Strain modes l = 2 .. ell_max of a binary with leading-order PN phasing and amplitudes, a smooth merger and ringdown, in a frame that
 * precesses and nutates, generated per time step on the device.  t: host f8[n], the caller's time axis (np.arange(t_0, t_1 + 0.99 dt,
 * dt)), strictly increasing; the merger is at t_merger = t_1 - 100 and must be at least 20 steps in.  The amplitude of mode k is
 * coef[k] x^power[k] with x = omega^(2/3) (pn_leading_order_amplitude, :536-593: host tables c16[n_modes], f8[n_modes], powers
 * multiples of 1/2).  derive_*: take the reference's default for that parameter (:489-492) instead of the field.
 * data_out: c16[n][ld] in `mem` (n_modes columns are written, the rest of a row is left alone) -- the modes in the corotating frame, or
 * with inertial != 0 rotated back by the inverse of the frame (bms_rotate_series on the device).  frame_out: host f8[n][4], the
 * corotating frame whatever `inertial` is (may be NULL).  The steps at which the piecewise definitions change (the reference's argmin
 * searches) are found on the host; the three cumulative integrals are the spline antiderivatives of bms_spline_derivative(order = -1)
 * over windows near the merger, which need at least 4 steps each (BMS_ERR_UNSUPPORTED otherwise). */
typedef struct {
  double mass_ratio;        /* > 0; a ratio below 1 is inverted */
  double t_merger;
  double opening_angle;     /* precession_opening_angle */
  double opening_angle_dot; /* precession_opening_angle_dot */
  double relative_rate;     /* precession_relative_rate */
  double nutation_angle;    /* precession_nutation_angle */
  int derive_opening_angle_dot; /* != 0: 2 opening_angle / (end of the ringdown transition - t[0]) */
  int derive_nutation_angle;    /* != 0: opening_angle / 10 */
  const void* coef;         /* host c16[n_modes] */
  const double* power;      /* host f8[n_modes] */
} bms_precessing_params;
int bms_precessing_waveform(bms_ctx* ctx, const double* t, int64_t n, int ell_max, const bms_precessing_params* params, int inertial,
                            void* data_out, int64_t ld, int mem, double* frame_out);
/* One member of the finite-radius family built on it (:740-742, the docstring's model): out[t][c] = h0[t][c] + |h0[t][c]| sum_{k=1..n_terms}
 * amp R^-k exp(i k (50 pi / n) t[t]).  h0 c16[n][ld_h0] and out c16[n][ld_out] (n_cols columns used) live in `mem` and must not overlap;
 * t: host f8[n].  0 <= n_terms <= 16. */
int bms_radius_terms(bms_ctx* ctx, const double* t, int64_t n, const void* h0, int64_t ld_h0, int64_t n_cols, int n_terms, double amp,
                     double radius, void* out, int64_t ld_out, int mem);

/* ---- centre-of-mass drift of the horizon (or star) trajectories (scri/SpEC/com_motion.py) ---------------------------------------
 * bms_com_motion: the track (:59-60, :112-118).  x_a, x_b f8[n][3], masses f8[n_m_a], f8[n_m_b] of length n or 1:
 * com_out[n][3] = (m_A x_A + m_B x_B) / (m_A + m_B); with matter != 0 also t_out[n] = t / (m_A + m_B) and com_out / (m_A + m_B)
 * (t and t_out may be NULL otherwise).  numpy's rounding steps in numpy's order: the result equals the numpy expression bit for bit.
 * Every array lives in `mem`. */
int bms_com_motion(bms_ctx* ctx, const double* t, const double* x_a, const double* x_b, const double* m_a, int64_t n_m_a, const double* m_b,
                   int64_t n_m_b, int64_t n, int matter, int mem, double* t_out, double* com_out);
/* bms_com_fit: estimate_avg_com_motion's arithmetic (:206-241) on t f8[n], com f8[n][3] in `mem`.  t_i = t[0] + (t[n-1] - t[0])
 * skip_beginning_fraction, t_f = t[n-1] - (t[n-1] - t[0]) skip_ending_fraction; i_i, i_f the first index of the minimum of |t - t_i|,
 * |t - t_f| (found on the device); C_k = scipy.integrate.simpson(y_k[i_i .. i_f], t[i_i .. i_f]) for y_0 = com, y_1 = fl(t com) and, with
 * fit_acceleration, y_2 = fl(fl(t t) com) -- the irregular composite rule, the correction of the last interval for an even number of
 * samples, the trapezoid for two, a zero divisor giving a zero quotient; then the position, velocity (and acceleration) that bring the
 * track closest to the origin over [t_i, t_f].  Weights, sums and the closed form are carried in double-double and rounded to fp64 once:
 * the result is the correctly rounded value of the rule on the fp64 inputs, and depends on nothing but them (fixed tiles, fixed order).
 * BMS_ERR_INVALID for n < 2, a window of fewer than two samples (i_f <= i_i) and t_f == t_i; `result` then still names the window.
 * NaN in the input propagates. */
typedef struct {
  double x_i[3], v_i[3], a_i[3]; /* a_i zero without fit_acceleration */
  double t_i, t_f;
  int64_t i_i, i_f;
  double moments[3][3];          /* C_k[component] rounded to fp64; C_2 zero without fit_acceleration */
} bms_com_fit_result;
int bms_com_fit(bms_ctx* ctx, const double* t, const double* com, int64_t n, int mem, double skip_beginning_fraction,
                double skip_ending_fraction, int fit_acceleration, bms_com_fit_result* result);
/* panels (two intervals each) behind one partial sum of the moments (tests place window lengths around it); a size, not a status */
int64_t bms_com_fit_tile_panels(void);

/* ---- fluxes of energy, momentum, angular momentum and boost (scri/flux.py:182-798) in one pass over the modes ---------------------
 * bms_poincare_fluxes: energy f8[n] (:206-208), momentum f8[n][3] (:329-340), angular f8[n][3] (:428-439) and boost f8[n][3] (:652-745,
 * with the signs of its code, not of its docstring) of the strain h and its time derivative hdot, c16[n_times][ld_h] and
 * c16[n_times][ld_hdot] holding l = ell_min .. ell_max, ell_min >= 2.  h, hdot and the outputs live in `mem`; t is a host f8[n_times].
 * Any output may be NULL: it is neither computed nor written (at least one is asked for).  h may be NULL when neither `angular` nor
 * `boost` is asked for, t when `boost` is not.  Every sum <a|M|b> of the reference runs over a banded operator; with the ladder factors
 * of eth / ethbar folded into three real coefficient sets per (column, neighbour), built in long double and kept per context and l range,
 * only h and hdot are read, once.  The sum of a time step is taken in an order that depends on nothing but the l range: two calls give
 * the same bits, a slice of the time steps gives the bits of the whole call, and an output does not depend on which others are asked for.
 * BMS_ERR_INVALID: a NULL that is needed, ell_max < ell_min, a row stride below the number of modes, negative n_times, a bad mem,
 * misaligned device arrays; BMS_ERR_UNSUPPORTED: ell_min < 2, an l range whose rows do not fit in LDS.  n_times == 0 writes nothing. */
int bms_poincare_fluxes(bms_ctx* ctx, const double* t, const void* h, int64_t ld_h, const void* hdot, int64_t ld_hdot, int64_t n_times,
                        int ell_min, int ell_max, int mem, double* energy, double* momentum, double* angular, double* boost);
/* out[t] = sum_e op(a[t][rows_e]) values_e b[t][cols_e], op = complex conjugation if conj_a else the identity: the reference's
 * sparse_expectation_value (scri/flux.py:41-78) for any operator given as triplets.  rows, cols int32[n_el] and values c16[n_el] are
 * host arrays; a c16[n_times][ld_a], b c16[n_times][ld_b] (n_cols columns used) and out c16[n_times] live in `mem`.  The sum has a fixed
 * order (element e on lane e mod 64, lane sums in element order, a butterfly over the lanes).  BMS_ERR_INVALID: a NULL argument, a row
 * stride below n_cols, negative sizes, and an index outside [0, n_cols) -- found on the host before anything is launched. */
int bms_expectation_values(bms_ctx* ctx, const void* a, int64_t ld_a, int conj_a, const void* b, int64_t ld_b, int64_t n_times, int n_cols,
                           const int32_t* rows, const int32_t* cols, const void* values, int64_t n_el, int mem, void* out);
/* how bms_poincare_fluxes runs n_modes columns on the current device: shape[0] time steps per pass of one workgroup, shape[1] workgroups
 * at most, shape[2] != 0 if the coefficient tables are held in LDS (else they are read through L2).  Returns shape[0], or 0 if the rows of
 * one time step do not fit in LDS (tests place series lengths around these sizes); sizes, not a status */
int64_t bms_flux_launch_shape(int n_modes, int64_t shape[3]);
/* pure host routine: the coefficient tables of l = ell_min .. ell_max as the kernel reads them, image_out f8[30][n_modes]: row 3 k + set
 * for neighbour k = 3 (dl + 1) + (mu + 1) of a column (l, m) -- the row (l + dl, m + mu) -- and set 0 (chi at s = -2), 1 (the pair
 * hdot, h), 2 (the pair h, hdot); rows 27, 28: sqrt((l - m)(l + m + 1)), sqrt((l + m)(l - m + 1)); row 29: l. */
int bms_flux_coefficients(int ell_min, int ell_max, double* image_out);

/* ---- brackets of two waveforms (scri/mode_calculations.py:60-89, 106-180; scri/waveform_modes.py:574-656) in one pass over the modes --
 * For f = a and g = b on the common range l = ell_min .. ell_max, per time step and in the (+, -, z) basis:
 *   inner  c16[n]     sum conj(f[l,m]) g[l,m]                       (the integrand of WaveformModes.inner_product)
 *   l_out  c16[n][3]  sum conj(f[l,m']) <l,m'|L_a|l,m> g[l,m],      a = +, -, z
 *   ll_out c16[n][9]  sum conj(f[l,m']) <l,m'|L_a L_b|l,m> g[l,m],  ab = pp, pm, mp, mm, pz, zp, mz, zm, zz
 * with the reference's terms, clips and coefficients (products of sqrt((l -+ m)(l +- m + 1)) and m, formed on the device).
 * a c16[n_times][ld_a] holds l from ell_min_a on, b c16[n_times][ld_b] from ell_min_b on: the common range is read where it lies in
 * each row.  a, b and the outputs live in `mem`; a and b may be one array.  Any output may be NULL: it is neither computed nor written
 * (at least one is asked for).  The sum of a time step is taken in an order that depends on nothing but the common range: a slice of the
 * time steps gives the bits of the whole call, host memory those of device memory, and an output does not depend on which others are
 * asked for.  BMS_ERR_INVALID: a NULL that is needed, ell_max < ell_min, ell_min below ell_min_a or ell_min_b, a row stride that ends
 * before the column (ell_max, ell_max), negative n_times, a bad mem, device arrays not aligned to 16 bytes; BMS_ERR_UNSUPPORTED: a common
 * range whose row does not fit in LDS.  n_times == 0 writes nothing. */
int bms_pair_brackets(bms_ctx* ctx, const void* a, int64_t ld_a, int ell_min_a, const void* b, int64_t ld_b, int ell_min_b, int64_t n_times,
                      int ell_min, int ell_max, int mem, void* inner, void* l_out, void* ll_out);
/* how bms_pair_brackets runs n_modes columns on the current device: shape[0] time steps per pass of one workgroup, shape[1] workgroups at
 * most, shape[2] = 0 (the kernel reads no tables).  Returns shape[0], or 0 if a row does not fit in LDS; sizes, not a status */
int64_t bms_pair_launch_shape(int n_modes, int64_t shape[3]);

/* ---- Bondi charges of AsymptoticBondiData rows (scri/asymptotic_bondi_data/bms_charges.py:14-200) in one pass over the modes ---------
 * four_momentum f8[n][4] (:79-88), angular f8[n][3] (:91-106), boost f8[n][3] (:163-182) and com f8[n][3] (:185-200) of psi1, psi2, sigma
 * and sigma_dot = d sigma / dt, rows c16[n_times][ld] stored from l = 0 as AsymptoticBondiData stores them ((ell_max + 1)^2 columns of
 * sigma and sigma_dot are read, the first four of psi1 and psi2).  The fields and the outputs live in `mem`; t is a host f8[n_times].
 * Any output may be NULL: it is neither computed nor written (at least one is asked for).  sigma_dot and psi2 may be NULL when neither
 * `four_momentum` nor `boost` is asked for, psi1 when `four_momentum` alone is, t when `boost` is not.  The l <= 1 modes of the products
 * sigma sigma-bar-dot, sigma eth sigma-bar and sigma sigma-bar are sums over the columns of sigma and their nine neighbours with three
 * real coefficient sets, built in long double and kept per context and ell_max; nothing is synthesised on a grid.  The sum of a time step
 * is taken in an order that depends on nothing but ell_max: two calls give the same bits, a slice of the time steps gives the bits of the
 * whole call, row strides change no bit, and an output does not depend on which others are asked for.
 * BMS_ERR_INVALID: a NULL that is needed, a row stride below the columns read, negative n_times or ell_max, a bad mem, misaligned device
 * arrays; BMS_ERR_UNSUPPORTED: ell_max < 2 (no shear), rows that do not fit in LDS.  All of it is found on the host before anything is
 * launched.  n_times == 0 writes nothing. */
int bms_bondi_charges(bms_ctx* ctx, const double* t, const void* psi1, int64_t ld_psi1, const void* psi2, int64_t ld_psi2, const void* sigma,
                      int64_t ld_sigma, const void* sigma_dot, int64_t ld_sigma_dot, int64_t n_times, int ell_max, int mem,
                      double* four_momentum, double* angular, double* boost, double* com);
/* how bms_bondi_charges runs n_modes = (ell_max + 1)^2 columns on the current device, as bms_flux_launch_shape: shape[0] time steps per
 * pass of one workgroup (returned as well, 0 if the rows of one time step do not fit in LDS), shape[1] workgroups at most, shape[2] != 0
 * if the coefficient tables are held in LDS (they are while that costs no wave; else they are read through L2); sizes, not a status */
int64_t bms_charge_launch_shape(int n_modes, int64_t shape[3]);
/* pure host routine: the coefficient tables of l = 0 .. ell_max (ell_max >= 2) as the kernel reads them, image_out f8[20][(ell_max + 1)^2]:
 * row 2 k + set for the neighbour k = 3 (dl + 1) + (mu + 1) of a column (l, m) of sigma -- the column (l + dl, m + mu) of sigma or
 * sigma_dot, which contributes to the mode M = -mu -- and set 0 (A1: spins (2, -2) -> L = 1), 1 (B: spins (2, -1) -> L = 1 with the GHP
 * factor of eth on sigma-bar); row 18: A0 (spins (2, -2) -> L = 0, the column itself); row 19: l. */
int bms_charge_coefficients(int ell_max, double* image_out);

/* ---- Products of two spin-weighted functions on Gauss-Legendre rows: no grid ----------------------------------------------------------
 * out c16[n_times][ld_out] = the modes l = 0 .. ell_max_out of op(a) op(b), for rows a c16[n_times][ld_a] and b c16[n_times][ld_b] stored
 * from l = 0 ((ell_max + 1)^2 columns of each are read).  spin_* is the spin of the STORED row; with conj_* != 0 the operand is its bar,
 * bar(x)_lm = (-1)^(s + m) conj(x_{l, -m}), of spin -spin_*, applied as the row is loaded.  The output has the sum S of the effective spins
 * and (ell_max_out + 1)^2 columns; those with l < |S| are exact zeros, and input columns with l < |s| are never read.  a and b may be the
 * same array.  The product is taken as theta sums of both operands on n = floor((ell_max_a + ell_max_b + ell_max_out) / 2) + 1 Gauss-Legendre
 * nodes in cos(theta), a convolution in m and a quadrature: exact for the truncated product (the integrand has degree <= ell_max_a +
 * ell_max_b + ell_max_out), with no phi grid.  The nodes and the tables of sYlm(theta_j, 0) are built on the host in long double and kept
 * per context and (spin, ell_max, n).  Every sum is taken in a fixed order (l, then m1, then j ascending) that depends on nothing but the
 * sizes and the spins: two calls give the same bits, a slice of the time steps gives the bits of the whole call, row strides and the kind
 * of memory change no bit.
 * BMS_ERR_INVALID: a NULL, a row stride below the columns read or written, negative sizes, ell_max_out > ell_max_a + ell_max_b, a bad mem,
 * misaligned device arrays; BMS_ERR_UNSUPPORTED: an effective |spin| or |S| above 4, an ell_max beyond the library's, a time step whose
 * rows and panels do not fit in LDS.  All of it is found on the host before anything is launched.  n_times == 0 writes nothing. */
int bms_mode_product(bms_ctx* ctx, const void* a, int64_t ld_a, int spin_a, int ell_max_a, int conj_a, const void* b, int64_t ld_b, int spin_b,
                     int ell_max_b, int conj_b, int64_t n_times, int ell_max_out, int mem, void* out, int64_t ld_out);
/* mass aspect and supermomenta (scri/asymptotic_bondi_data/bms_charges.py:14-47, 203-286) of psi2, sigma and sigma_dot = d sigma / dt, rows
 * from l = 0 ((ell_max + 1)^2 columns of sigma and sigma_dot and (ell_max_out + 1)^2 of psi2 are read), 2 <= ell_max, ell_max_out <= ell_max:
 * the product body of bms_mode_product on sigma and bar(sigma_dot), and as the row is stored, mode by mode,
 *   bondi_sachs = psi2 + sigma sigma-bar-dot,   moreschi = bondi_sachs + eth^2 sigma-bar,   geroch = bondi_sachs + (eth^2 sigma-bar -
 *   ethbar^2 sigma) / 2,   geroch_winicour = bondi_sachs - ethbar^2 sigma,   mass_aspect = -(bondi_sachs + bar bondi_sachs) / 2
 * (GHP: eth^2 sigma-bar = bar(sigma) sqrt((l + 2)(l + 1) l (l - 1)) / 2, ethbar^2 sigma = sigma times the same factor).  Each output is
 * c16[n_times][ld_out] with (ell_max_out + 1)^2 columns written; any may be NULL, not all; an output does not depend on which others are
 * asked for.  integrated != 0: the four supermomenta are written as -bar(Psi) / (2 sqrt(pi)); the mass aspect is never altered.
 * Refusals and bit guarantees as bms_mode_product; ell_max < 2 is BMS_ERR_UNSUPPORTED, ell_max_out > ell_max BMS_ERR_INVALID. */
int bms_supermomenta(bms_ctx* ctx, const void* psi2, int64_t ld_psi2, const void* sigma, int64_t ld_sigma, const void* sigma_dot,
                     int64_t ld_sigma_dot, int64_t n_times, int ell_max, int ell_max_out, int mem, int integrated, void* bondi_sachs,
                     void* moreschi, void* geroch, void* geroch_winicour, void* mass_aspect, int64_t ld_out);
/* the violations of the six Bondi-gauge relations (scri/asymptotic_bondi_data/constraints.py) and their L2 norms over the sphere, in one
 * launch.  fields: psi0 .. psi4, sigma; psi_dot: d/du of psi0, psi1, psi2; sigma_dot, sigma_ddot: d sigma / du, d^2 sigma / du^2; every row
 * c16 with (ell_max + 1)^2 columns from l = 0 and its own row stride, 2 <= ell_max.  Mode by mode,
 *   v0 = psi0_dot - eth psi1 - 3 sigma psi2    v1 = psi1_dot - eth psi2 - 2 sigma psi3    v2 = psi2_dot - eth psi3 - sigma psi4
 *   v3 = psi3 + eth bar(sigma_dot)             v4 = psi4 + bar(sigma_ddot)                v5 = Im[psi2 + eth^2 bar(sigma) + sigma bar(sigma_dot)]
 * with the GHP eth (a row of spin s times sqrt((l - s)(l + s + 1) / 2), zero for l < |s| or l < |s + 1|), bar as in bms_mode_product and
 * Im(x) = -i (x - bar x) / 2; the products are those of bms_mode_product truncated at ell_max, sigma's theta sums taken once for all four.
 * The diagonal terms are read as stored, columns with l < |s| included; product columns with l < |S| are exact zeros.  violations[k]
 * c16[n_times][ld_out] and norms f8[n_times][6] (in the memory `mem` names; norms[t][k] = sqrt(sum_c |v_k[t][c]|^2), summed in a fixed
 * order) may each be NULL, not all; `violations` itself may be NULL.  An input that only outputs not asked for read may be NULL (psi0 is never
 * read); a product that no output asked for needs is not formed.  An output does not depend on which others are asked for; the bit
 * guarantees of bms_mode_product hold, and the norms of a norms-only call are the norms of a call that stores the violations too.
 * BMS_ERR_INVALID: a NULL that is needed, every output NULL, a row stride below (ell_max + 1)^2, negative sizes, a bad mem, misaligned
 * device arrays; BMS_ERR_UNSUPPORTED: ell_max < 2, an ell_max beyond the library's or a time step that does not fit in LDS (bms_product_launch_shape
 * of (ell_max, ell_max, ell_max)).  Found on the host before anything is launched.  n_times == 0 writes nothing and returns before the
 * device is asked for its LDS, as in bms_mode_product: an empty series is BMS_OK at any ell_max the library carries.  Timed as
 * BMS_TAG_CONSTRAINTS. */
int bms_bondi_constraints(bms_ctx* ctx, const void* const fields[6], const int64_t ld_fields[6], const void* const psi_dot[3],
                          const int64_t ld_psi_dot[3], const void* sigma_dot, int64_t ld_sigma_dot, const void* sigma_ddot,
                          int64_t ld_sigma_ddot, int64_t n_times, int ell_max, int mem, void* const violations[6], int64_t ld_out, double* norms);
/* one stage of the Bianchi identities run forwards (scri/asymptotic_bondi_data/from_initial_values.py:128-154): what the constraint
 * kernel subtracts from a given derivative, stored.  Rows c16 with (ell_max + 1)^2 columns from l = 0, each array with its own row stride,
 * 2 <= ell_max.  Mode by mode, with the GHP eth, bar and the truncated product of bms_bondi_constraints,
 *   rhs[c] = f(l, 1 - k) a[c] + (3 - k) (sigma b)[c],   f(l, s) = sqrt((l - s)(l + s + 1)) / sqrt(2), zero for l < |s| or l < |s + 1|,
 * evaluated as written per real and imaginary part (two products, one sum);
 *   k = 1: a = psi2 (spin 0), b = psi3 (spin -1)          k = 0: a = psi1 (spin 1), b = psi2 (spin 0)
 *   k = 2, the head: a = sigma_dot and b = sigma_ddot as stored (spin 2);  psi4 = -bar(b),  psi3 = -f(l, -2) bar(a),
 *                    rhs = f(l, -1) psi3 + sigma psi4;  psi3 and psi4 c16[n_times][ld_psi] are written as well
 * psi3 and psi4 are required at k = 2 and must be NULL at k = 1 and k = 0 (ld_psi is then not read).  The product is the one
 * bms_mode_product forms of sigma (spin 2) and b (spin -k) truncated at ell_max, bit for bit; its columns below l = |2 - k| are exact zeros
 * and input columns below the operand's spin are never read by it; the diagonal term reads `a` as stored.  The time integral between the
 * stages is the caller's (bms_spline_derivative of order -1).
 * BMS_ERR_INVALID: k outside 0 .. 2, a NULL that is needed, psi3 or psi4 given where it is not written, a row stride below (ell_max + 1)^2,
 * negative sizes, a bad mem, misaligned device arrays; BMS_ERR_UNSUPPORTED: ell_max < 2, an ell_max beyond the library's or a time step that
 * does not fit in LDS (bms_product_launch_shape of (ell_max, ell_max, ell_max)).  Found on the host before anything is launched.
 * n_times == 0 writes nothing and returns before the device is asked for its LDS.  The bit guarantees of bms_mode_product hold: two calls
 * give the same bits, a slice of the time steps gives the bits of the whole call, row strides and the kind of memory change no bit.  The
 * tables are those of the product family, kept per context.  Timed as BMS_TAG_CONSTRAINTS, beside the kernel whose inner step it is. */
int bms_bianchi_rhs(bms_ctx* ctx, int k, const void* sigma, int64_t ld_sigma, const void* a, int64_t ld_a, const void* b, int64_t ld_b,
                    int64_t n_times, int ell_max, int mem, void* rhs, int64_t ld_rhs, void* psi3, void* psi4, int64_t ld_psi);
/* how the product kernel runs on the current device: shape[0] time steps per pass of one workgroup (returned as well, 0 if the rows and
 * panels of one time step do not fit in LDS), shape[1] workgroups at most, shape[2] != 0 if the tables are held in LDS (they are read
 * through L2); sizes, not a status */
int64_t bms_product_launch_shape(int ell_max_a, int ell_max_b, int ell_max_out, int64_t shape[3]);
/* pure host routine: the n_nodes Gauss-Legendre nodes cos_theta f8[n_nodes] (theta ascending) and weights f8[n_nodes], and the table
 * f8[n_nodes][(ell_max + 1)^2] of sYlm(theta_j, 0) for spin s = `spin` (|spin| <= 4; zero for l < |s|) as the kernel reads it -- the
 * output spin's table is this one times 2 pi w_j, formed in long double before the one rounding */
int bms_product_tables(int spin, int ell_max, int n_nodes, double* cos_theta, double* weights, double* table);

/* ---- Cuts: a series of spin-0 modes on the supertranslated cut u = alpha(theta, phi) (scri/asymptotic_bondi_data/map_to_superrest_frame.py:108-224)
 * N = 2 ell_max + 1, the grid is the equiangular one of bms_salm2map (theta_i = pi i / (N - 1), phi_j = 2 pi j / N), nm = (ell_max + 1)^2.
 *
 * bms_supermomentum_on_cut: t host f8[n] strictly increasing; psi c16[n][ld] in `mem`, columns from l = 0 (the Moreschi supermomentum
 * Psi_M); alpha host f8[N][N], finite.  The window is rows [lo, hi), lo = (number of t <= min alpha) - 1 - 64, hi = (number of t < max alpha)
 * + 1 + 64, clipped to [0, n]: the not-a-knot cubic splines are taken through these rows only and nothing outside them is read.
 *   psi_at_alpha[p] = Re sum_lm Y_lm(p) S_lm(alpha_p), S_lm the spline through column lm -- the reference's per-pixel spline through the real
 *                     part of the synthesised rows, with the two linear steps in the other order;
 *   k_at_alpha[p]   = the per-pixel spline through K_r(p) = M_r / (P0_r - P_r . r(p)) at alpha_p, P_r = -(the charge vector of the four
 *                     l <= 1 columns of row r), M_r = sqrt(P0^2 - |P|^2), r(p) = (sin theta cos phi, -sin theta sin phi, cos theta): 4 pi times the same charge vector of
 *                     the four unit-mode grids, whose y component is Im(a_1-1 + a_11) / sqrt(24 pi);
 *   modes_out c16[nm] = map2salm((psi_at_alpha - salm2map(D map2salm(alpha))) / k_at_alpha^3), D_l = (l+2)(l+1)l(l-1)/4, 0 below l = 2.
 * All three are host arrays and each may be NULL, not all; with modes_out == NULL the entry is "a real series on a cut" (K is formed only
 * if k_at_alpha is asked for).  An output does not depend on which others are asked for.  A pixel whose alpha lies outside [t[0], t[n-1]] is
 * evaluated as bms_spline_derivative evaluates a point outside its knots: the cubic of the end interval is continued (scipy's
 * extrapolation), so the two agree there as well.  A row with P0^2 <= |P|^2 gives NaN or infinity in what depends on K, as the
 * reference's sqrt does, and raises nothing.
 * Bits: two calls give the same bits; a call on the rows [lo, hi) alone (with their times) gives the bits of the call on the whole
 * series; row stride and kind of memory change no bit.
 * BMS_ERR_INVALID: a NULL t, psi or alpha, every output NULL, ld < nm, negative sizes, a bad mem, a device array not aligned to 16 bytes,
 * times that are not strictly increasing, a non-finite alpha.  BMS_ERR_UNSUPPORTED: ell_max < 2, ell_max > 24, fewer than 4 window rows, or
 * (with K) a window whose forward sweep of one theta ring, 8 N (hi - lo) bytes, does not fit in LDS beside 8 (nm + 2 N + 5 (hi - lo)) + 2048
 * bytes of tables (160 KB: 398 rows at ell_max = 24, 795 at 12).  All of it is found on the host before anything is launched and leaves the
 * outputs untouched.  Stream-ordered on the context's stream up to the one wait behind the copies home.
 *
 * bms_alpha_perturbation: alpha_out f8[N][N] = Re salm2map(D^-1 map2salm(salm2map(psi_modes) + M K^3)) for one row psi_modes host c16[nm];
 * m_grid, k_grid host f8[N][N], or NULL: the rest mass M / the conformal factor K(p) of psi_modes itself, as above.  BMS_ERR_INVALID: a NULL
 * psi_modes or alpha_out, a negative ell_max; BMS_ERR_UNSUPPORTED: ell_max < 2 or > 24.  Both entries are timed as BMS_TAG_CUT (the grid <->
 * mode steps and the spline sweeps under their own tags). */
int bms_supermomentum_on_cut(bms_ctx* ctx, const double* t, int64_t n, const void* psi, int64_t ld, int mem, int ell_max, const double* alpha,
                             void* modes_out, double* psi_at_alpha, double* k_at_alpha);
int bms_alpha_perturbation(bms_ctx* ctx, const void* psi_modes, int ell_max, const double* m_grid, const double* k_grid, double* alpha_out);

/* ---- a raw finite-radius series retarded to tortoise time (scri/extrapolation.py:27-45 and :356-402), one radius per call -----------
 * bms_finite_radius_retard: t, areal_radius, average_lapse host f8[n_raw] as a simulation writes them (coordinate times with the repeated
 * stretches of restarts); data c16[n_raw][ld] (n_cols columns) and, if not NULL, frame f8[n_raw][4] in `mem`.
 *   kept samples: k is kept iff fl(t[k] + min_time_step) < min_{j > k} t[j] -- the indices of monotonic_indices, as a suffix minimum and
 *     an exclusive prefix sum of the mask; *n_kept is their number, K below, and k_0 < k_1 < ... are they;
 *   g_j = lapse[k_j] / sqrt((-2E / R[k_j]) + 1), term_j = ((t[k_j] - t[k_j-1]) (g_j + g_j-1)) / 2 in the operation order of
 *     scipy.integrate.cumulative_trapezoid, no fused multiply-add; their inclusive prefix sums are carried in double-double and rounded
 *     to fp64 once per sample;
 *   t_out[j] = (fl(sum_j + t[k_0]) - (R + 2E log(R / 2E - 1))) / ch_mass (t[k_0] itself for j = 0), radii_out[j] = R[k_j] / ch_mass;
 *   data_out[j][m] = data[k_j][m] f_j, both components, f_j = fl(fl((R[k_j] / coord_radius)^p) unit_scale), p = radius_exponent formed by
 *     repeated multiplication; frame_out[j] = frame[k_j].
 * t_out and radii_out are host f8[n_raw], data_out c16[n_raw][ld_out] and frame_out f8[n_raw][4] live in `mem`: the caller allocates n_raw
 * rows, the first K are the result.  Device rows from K on are not written; host entries from K on are unspecified.
 * Bits: two calls give the same bits; row strides and the kind of memory change no bit; an element's arithmetic depends on no tile.
 * BMS_ERR_INVALID, found on the host before anything is launched: a NULL series, data or output (frame_out with a frame), n_raw < 1,
 * n_cols < 1, radius_exponent outside 1 .. 5, ch_mass == 0, coord_radius or initial_adm_energy not finite or <= 0, min_time_step < 0,
 * ld or ld_out < n_cols, a time that is not finite, a bad mem, a device array not aligned to 16 bytes.  BMS_ERR_INVALID after the kernels:
 * a KEPT radius that is not finite or <= 2E (counted on the device; the message names the first) -- the reference returns a NaN time axis
 * there; the outputs are then written and not to be used.  A bad radius at a dropped sample is not read.
 * Stream-ordered on the context's stream up to the one wait behind the copies home.  Timed as BMS_TAG_POINTWISE. */
int bms_finite_radius_retard(bms_ctx* ctx, const double* t, const double* areal_radius, const double* average_lapse, int64_t n_raw,
                             const void* data, int64_t ld, int n_cols, int mem, const double* frame, double coord_radius,
                             double initial_adm_energy, double ch_mass, double unit_scale, int radius_exponent, double min_time_step,
                             int64_t* n_kept, double* t_out, double* radii_out, void* data_out, int64_t ld_out, double* frame_out);
/* samples per tile of the three scans (tests place restarts and lengths around it); a size, not a status */
int64_t bms_retard_tile(void);

#ifdef __cplusplus
}
#endif
#endif /* SCRI_AMD_H */
