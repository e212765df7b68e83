// Launchers of the gfx950 kernels (C++ internal interface between the engine and the kernels).
#pragma once
#include <algorithm>
#include <vector>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "env.h"

#include <map>
#include <mutex>
#include <utility>

namespace bms {

// y extent of a launch grid (HIP: 65 535); launchers whose y counts time tiles cut longer launches into slices or refuse them
constexpr long long GRID_Y_MAX = 65535;

// LDS one workgroup can have on device `dev`: asked of the device (the opt-in limit where the runtime reports one, else the per-block
// limit; this library only runs on gfx950, whose 160 KB is the floor assumed when neither query answers with more than the 64 KB
// default).
inline int lds_per_workgroup(int dev) {
  int lds = 0, v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, dev) == hipSuccess) lds = std::max(lds, v);
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess) lds = std::max(lds, v);
  (void)hipGetLastError();
  if (lds <= 64 * 1024) lds = 160 * 1024;
  return lds;
}

// Dynamic LDS beyond 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize on the kernel.  It is set ONCE per (kernel, device), to
// everything the CU has beyond the kernel's static LDS (lds_per_workgroup): a per-launch value is a race between host threads that
// launch the same kernel with different sizes (thread A sets 124 KB, thread B sets 60 KB, A's launch is refused) -- contexts are meant
// to be driven from several threads (include/scri_amd.h).  Only a SUCCESS is remembered: a transient failure is tried again by the
// next launch instead of failing that kernel for the life of the process.
inline hipError_t allow_dynamic_lds(const void* fn) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, bool> done;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> guard(mu);
  const auto key = std::make_pair(fn, dev);
  if (done.count(key)) return hipSuccess;
  const int lds = lds_per_workgroup(dev);
  hipFuncAttributes attr;
  hipError_t e = hipFuncGetAttributes(&attr, fn);
  if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds - (int)attr.sharedSizeBytes);
  if (e == hipSuccess)
    done[key] = true;
  else
    (void)hipGetLastError();
  return e;
}

constexpr int ROT_MB = 4;  // mu-block of the packed Delta tables (see kernels_rotate.hip)

// ---- rotation (scri/rotations.py:346-392)
int rotate_waves_per_block(int ell_max);
hipError_t launch_rotate_modes(hipStream_t stream, double* data, long long n_times, long long ld, int ell_min, int ell_max,
                               const double* RaRb, long long rotor_stride, const double* delta,
                               const long long* delta_off, int* waves_used = nullptr /* out: waves per workgroup of the launch */);

// MFMA formulation (kernels_rotate_mfma.hip), ell_max <= 33: btab = per-l packed B images, boff = offsets (doubles)
struct RotGeom;
void rotate_mfma_table_shape(int ell, int* kpad, int* pd);
int rotate_mfma_supported(int ell_max);
hipError_t launch_rotate_modes_mfma(hipStream_t stream, double* data, long long n_times, long long ld, int ell_min,
                                    int ell_max, const double* RaRb, long long rotor_stride, const double* btab,
                                    const long long* boff);

// Wave-autonomous formulation with all tables of the l range resident in the LDS (kernels_rotate_resident.hip)
constexpr int RR_MAXL = 24;
struct RotResPlan {
  int ell_min, ell_max, n_groups, kpad_max, tab_doubles, waves;
  int grp_lo[4], grp_hi[4];
  int tab_off[RR_MAXL];  // doubles, per l - ell_min
};
bool rotate_resident_plan(int ell_min, int ell_max, RotResPlan* P, size_t* lds_bytes);
void rotate_resident_pack(const RotResPlan& P, int ell, const double* Delta, double* image);
hipError_t launch_rotate_modes_resident(hipStream_t stream, double* data, long long n_times, long long ld, const double* RaRb,
                                        long long rotor_stride, const double* tab_global, const RotResPlan& P, size_t lds_bytes,
                                        unsigned int* counter, int n_cu);

// ---- mode-space operators on resident series (kernels_modes.hip)
struct ModeMapSide {
  const double* data;  // c16[n_rows][ld]; nullptr: side absent
  long long ld;        // row stride (complex)
  const int* idx;      // source column per output column, -1: zero
  const double* coef;  // c16 per output column
  int conj;            // conjugate the source
};
// s_t = sum_j |data[t][j]|^2 (or its square root), terms added in column order without contraction (waveform_base.py:19-35)
hipError_t launch_row_norm(hipStream_t stream, const double* data, long long ld, long long n_rows, int n_cols, int take_sqrt, double* out);
// trailing data dimensions: the reference's layout (trailing index fastest) <-> one block of unit-stride columns per series
hipError_t launch_series_to_blocks(hipStream_t stream, const double* in, long long ld_in, double* out, long long n_rows, int n_modes, int F);
hipError_t launch_blocks_to_series(hipStream_t stream, const double* in, long long block_rows, double* out, long long n_rows, int n_cols, int F);
hipError_t launch_mode_map(hipStream_t stream, double* out, long long ld_out, long long n_rows, int n_cols, const ModeMapSide& A,
                           const ModeMapSide& B, const double* row_scale);

// ---- SWSH matrices (sf.SWSH_grid, waveform_grid.py:470-484)
// Bmat[2k][2p] = Re Y_k(R_p), [2k][2p+1] = Im, [2k+1][2p] = -Im, [2k+1][2p+1] = Re;  k = LM_index(l,m,ell_min)
hipError_t launch_swsh_matrix(hipStream_t stream, const double* rotors /* f8[n_pix][4] */, int n_pix, int spin,
                              int ell_min, int ell_max, double* Bmat, long long ldb);
// the same harmonics as a plain complex matrix Y[k][p] (row pitch ldb doubles), the B operand of launch_zgemm3m
hipError_t launch_swsh_matrix_complex(hipStream_t stream, const double* rotors, int n_pix, int spin, int ell_min,
                                      int ell_max, double* Bmat, long long ldb);
// analysis (quadrature) matrix: W[p][k] = w_pix[p] conj(Y_k(R_p)) in the real layout with pixels as rows:
// Wmat[2p][2k] = Re W, [2p][2k+1] = Im W, [2p+1][2k] = -Im W, [2p+1][2k+1] = Re W
hipError_t launch_quadrature_matrix(hipStream_t stream, const double* rotors, const double* w_pix, int n_pix, int spin,
                                    int ell_min, int ell_max, double* Wmat, long long ldw);
// complex values Y[p][k] (row = pixel), for tests / small per-pixel tables
hipError_t launch_swsh_values(hipStream_t stream, const double* rotors, int n_pix, int spin, int ell_min, int ell_max,
                              double* Y /* c16[n_pix][n_modes] */);

// ---- per-pixel set-up tables on the device (pixel_math.h)
struct PixelSpec;
struct PixelOut;
// perm (device, may be null): column p holds grid pixel perm[p]
hipError_t launch_pixel_tables(hipStream_t stream, const PixelSpec& P, const PixelOut& O, int n_pix, const int* perm);
// Column plan of an n_theta x n_phi grid (n_theta n_phi <= pixel_sort_max(), n_theta >= 3): the pole rings contribute one
// column each (n_cols = n_pix - 2 (n_phi - 1)); perm[n_cols] = grid pixel of a column, in grid order (by_key = 0) or sorted by
// key (by_key = 1); inv[n_pix] = column of a grid pixel (pole pixels share their ring's column)
int pixel_sort_max();
hipError_t launch_pixel_sort(hipStream_t stream, const PixelSpec& P, int n_theta, int n_phi, int by_key, int* perm, int* inv);

// ---- separable analysis (kernels_analysis.hip): phi-DFT matrix for the GEMM, theta table, theta quadrature
hipError_t launch_dft_matrix(hipStream_t stream, int n_phi, int L, double* B, long long ldb);
hipError_t launch_theta_table(hipStream_t stream, const double* Y, const double* w_theta, int n_theta, int n_out, double* T);
hipError_t launch_theta_quadrature(hipStream_t stream, const double* F, long long n_rows, int n_theta, int nm, int n_out,
                                   const int* m_index, const double* T, double* out, long long ldo);
constexpr int MAX_THETA_SEPARABLE = 104;
// large grids (40 < n_theta <= 104): folded phi-DFT to F[t][m][jp] (jp = large_analysis_jp(n_theta) rings), then the theta
// quadrature as MFMA products batched over time; T from launch_theta_table; F: n_rows * (2L+1) * jp complex of work space
int large_analysis_supported(int n_theta, int n_phi, int L);
int large_analysis_jp(int n_theta);
hipError_t launch_analysis_large(hipStream_t stream, const double* G, long long ldg, long long n_rows, int n_theta, int n_phi,
                                 int L, int ell_min_out, const double* T, double* F, double* out, long long ldo);
// fused single-kernel analysis (n_theta <= 40, n_out <= 1024): D = cos|sin DFT matrix [4 ks][pd] from launch_dft_cs_matrix
struct FusedGeom;
int fused_analysis_supported(int n_theta, int n_phi, int L, int n_out);
size_t fused_dft_table_size(int n_phi, int L);  // doubles
hipError_t launch_dft_cs_matrix(hipStream_t stream, int n_phi, int L, double* D);
// col_of_pixel (device, may be null): grid pixel g is column col_of_pixel[g] of G; then the pixels k > 0 of the two pole
// rings are read from their ring's column times the spin phase e^{-+ i spin phi_k}
hipError_t launch_analysis_fused(hipStream_t stream, const double* G, long long ldg, long long n_rows, int n_theta, int n_phi,
                                 int L, int n_out, const int* m_index, const double* T, const double* D, double* out,
                                 long long ldo, const int* col_of_pixel, int spin, int n_cu, bool allow_split = true);

// series of 2 or 3 samples (ABD flavour): line / parabola through the samples, rows 0..n-1 of Y
hipError_t launch_short_series_eval(hipStream_t stream, const double* Y, long long ld, int n_cols, int n, const double* x,
                                    const double* base, const double* skew_a, const double* skew_b, double tt, long long i_lo,
                                    long long i_hi, double* out, long long ldo);

// ---- separable synthesis for boost-free transformations (kernels_synthesis.hip)
struct SynGeom {
  int n_theta, n_phi, L, n_modes, nk;
  int nth, nph;      // theta and phi waves
  int n_lists, len;  // lists of mode entries the theta threads walk, entries per list (8 .. 20)
};
int synthesis_split_plan(int n_theta, int n_phi, int ell_min, int ell_max, SynGeom& g, std::vector<int>& meta, size_t& lds_bytes,
                         int& nt, int& len);
// A: [n_rows][lda] modes (complex, n_modes + 1 per row: the last one multiplies `off`), Tsyn[n_modes][n_theta] = sLambda_lm(theta_j),
// off: complex per grid pixel or null; Y[n_rows][ldy] = grid rows in grid order; scale: null or 2 (equal) doubles per pixel
// multiplying the result -- it takes synthesis_split_scale_bytes more LDS than the plan's lds_bytes
size_t synthesis_split_scale_bytes(int n_theta, int n_phi);
hipError_t launch_synthesis_split(hipStream_t stream, const double* A, long long lda, long long n_rows, const SynGeom& g, int nt,
                                  const double* Tsyn, const int* meta, const double* off, double* Y, long long ldy, size_t lds_bytes,
                                  int n_cu, const double* scale = nullptr);

// the one-kernel form with the spline evaluation in it (kernels_synthesis_eval.hip): A = B-spline coefficients of the (rotated) modes
// over the knots e.g0 .. e.g0 + n_rows - 1 (n_modes per row), the output e.out = SAMPLES at the output rows [e.i_lo, e.i_hi) in grid
// order; e.skew_b per grid pixel (e.skew_a unused: no boost), s_min / s_max = its range.
// g, nt, Tsyn, meta: synthesis_split_plan's.
struct SplineEval;
int synthesis_eval_supported(const SynGeom& g, int nt, size_t* lds_bytes, int* nph, int* ring_rows, int* staged_abscissae);
hipError_t launch_synthesis_eval(hipStream_t stream, const double* A, long long lda, long long n_rows, const SynGeom& g, int nt,
                                 const double* Tsyn, const int* meta, const SplineEval& e, double s_min, double s_max, int n_cu);
// Y[k][col[j]] -= c[j] Y[k][one_col] (complex; c: n complex numbers, col: n column indices, all device memory): the h / sigma term
// subtracted on the modes
hipError_t launch_sub_const_modes(hipStream_t stream, double* Y, long long ld, long long n_rows, int n, const int* col, const double* c, int one_col);

// two-kernel form for the grids the one-kernel form does not take (kernels_synthesis_large.hip): n_theta <= 104, n_phi <= 127,
// l_max <= 33, any l_min; F = n_rows x (2 l_max + 1) x large_analysis_jp(n_theta) complex of work space.  With `off` the row has
// one more complex number at column n_modes (the eliminated constant series), which multiplies -off[pixel]; `scale` (2 doubles per
// pixel, equal) multiplies the result.
int large_synthesis_supported(int n_theta, int n_phi, int ell_min, int ell_max);
hipError_t launch_synthesis_large(hipStream_t stream, const double* A, long long lda, long long n_rows, int n_theta, int n_phi,
                                  int ell_min, int ell_max, const double* Tsyn, const double* off, double* F, double* Y,
                                  long long ldy, const double* scale = nullptr);

// AsymptoticBondiData without a boost: theta stage per field, then the phi stage of all six fields fused with their Horner mixing
// (time-independent without a boost: the elimination has moved onto the modes); per-pixel tables in grid order
hipError_t launch_theta_synthesis(hipStream_t stream, const double* A, long long lda, long long n_rows, int n_theta, int ell_min,
                                  int ell_max, const double* Tsyn, double* F);
int abd_mix6_supported(int n_theta, int n_phi, int ell_max);
hipError_t launch_phi_synthesis_mix6(hipStream_t stream, const double* const F6[6], long long n_rows, int n_theta, int n_phi,
                                     int ell_max, const double* eth_alpha, const double* etheth_alpha, const double* cst, long long ldc,
                                     double* const out6[6], long long ldo);

// ---- dense fp64 GEMM on MFMA: C[M x N] = (A[M x K] * B[K x N] - col_off[N]) * col_scale[N]
// A row-major (lda), B row-major (ldb), C row-major (ldc); col_off/col_scale N entries or null.
// Read: of A the K entries of rows 0 .. M-1 and nothing else (the kernel puts zeros for k >= K and rows >= M); of B
// 16 ceil(K / 16) rows x 128 ceil(N / 128) columns -- rows >= K and columns >= N have to exist and be finite, they need not be zero
// (pad rows meet the zeros of A, pad columns feed results nobody stores).  Written: the N leading doubles of rows 0 .. M-1 of C.
// Preconditions (hipErrorInvalidValue otherwise): K >= 2 and even (A is loaded two k at a time: with an odd K the load that holds
// A[row][K-1] would take A[row][K] along and multiply it by B's pad row); A and B 16-byte aligned with even lda and ldb, C 8-byte.
hipError_t launch_dgemm(hipStream_t stream, const double* A, long long lda, const double* B, long long ldb, double* C,
                        long long ldc, long long M, int N, int K, const double* col_off, const double* col_scale);

// ---- complex128 GEMM on MFMA with 3 real products per complex one: C = (A . B - col_off) * col_scale
// A[M x K], B[K x N], C[M x N] complex interleaved, row-major, pitches lda/ldb/ldc in DOUBLES; col_off/col_scale per real column
// (2N entries) or null.
// Read: of A the K entries of rows 0 .. M-1 and nothing else (not the rest of a pitch, not a row >= M: the kernel puts zeros there);
// of B 8 ceil(K / 8) rows x 64 ceil(N / 64) complex columns -- rows >= K and columns >= N have to exist and be FINITE, they need not
// be zero: pad rows meet the zeros of A (AsymptoticBondiData keeps sigma's offset row right behind the rows psi0 multiplies, the
// rotation hands over rows whose K entries are followed by the next l block), pad columns feed results nobody stores.
// Written: the 2N leading doubles of rows 0 .. M-1 of C.
// Preconditions (hipErrorInvalidValue otherwise): K >= 1; A, B and C 16-byte aligned with even lda, ldb and ldc (16-byte loads and
// stores).  four: the 4-product form (zgemm3m_mfma_kernel<true>, the accuracy yardstick) instead of the 3-product one; the probe
// switch SCRI_AMD_ZGEMM_4M asks for it on every call.
hipError_t launch_zgemm3m(hipStream_t stream, const double* A, long long lda, const double* B, long long ldb, double* C,
                          long long ldc, long long M, int N, int K, const double* col_off, const double* col_scale, bool four = false);

// ---- the same product with the spline evaluation in its epilogue (kernels_gemm_eval.hip): A holds B-spline coefficients of the
// modes (both sweeps of the collocation solve done on the modes), the product is the coefficient grid, and each 64-knot tile
// evaluates the output samples whose four coefficients it holds -- only the samples are written.
struct BsplineTable;
struct SplineEval {
  const BsplineTable* table;  // per knot (global index), as for launch_bspline_backward_eval
  const double* x;            // knots = output abscissae before the skew (global index)
  const double* skew_a;       // per column of the launch (may be null)
  const double* skew_b;
  double tt;
  long long g0;       // knot of row 0 of A
  long long n_knots;  // of the whole series
  long long i_lo, i_hi;  // output rows (indices into x); out row 0 = i_lo
  double* out;
  long long ldo;
  int search_halfwidth;  // bound on |row of a sample - knot of its window| (0: none known)
  double inv_dx;         // 1 / (mean step of the knots of this launch), or 0: row guesses allowed at all (the kernel uses each tile's own step)
  unsigned long long* stats;  // device, or null: [0] += tiles whose samples left the staged window, [1] += marches continued from global memory
  double* side;          // 6 rows of ldc doubles per 64-row tile (zgemm3m_eval_side_rows(M) rows), or null: overlapping tiles
  long long side_ld;
  int step = 0;          // rows a tile advances: 0 = automatic (64 with `side`, 61 without), 61 or 64 (the context's GEMM_EVAL_STEP option)
};
long long zgemm3m_eval_side_rows(long long M);
// Preconditions (hipErrorInvalidValue otherwise): M >= 4; lda >= 2 K (the rows of A do not overlap: the kernel's range check on A takes
// everything from a row's K entries to the next row for out of range); 64 rows of A and 8 rows + 64 columns of B span less than 2^31 bytes
// (32-bit byte offsets behind buffer descriptors).  B holds 8 ceil(K / 8) rows (the rows >= K are read, and multiplied by zeros of A).
hipError_t launch_zgemm3m_eval(hipStream_t stream, const double* A, long long lda, const double* B, long long ldb, long long M, int N,
                               int K, const double* col_scale, const SplineEval& e);

// ---- shared-matrix not-a-knot cubic spline along time (waveform_grid.py:574-588)
struct SplineTable {  // per knot j
  double P, Q, A, C;  // r'_j = P (y_j - y_{j-1}) + Q (y_{j+1} - y_j) - A r'_{j-1};  s_j = r'_j - C s_{j+1}
};
// entries [j0, j1) of the table; x / table are indexed by global knot number and touched on [j0 - 41, j1] only
hipError_t launch_spline_table(hipStream_t stream, const double* x, long long n, SplineTable* table, long long j0,
                               long long j1);
// forward elimination over rows [row_lo, row_hi) of the knot axis; Y, R are [rows][ld] doubles holding
// global rows g0.. (row index r maps to knot g0 + r)
hipError_t launch_spline_forward(hipStream_t stream, const double* Y, double* R, long long ld, int n_cols /* complex */,
                                 long long g0, long long n_rows, long long n_knots, const double* x,
                                 const SplineTable* table, int tile, int halo);
// back substitution + evaluation at u_eval(i) = base_i + skew_a[p] (base_i - tt) + skew_b[p] for output rows
// i in [i_lo, i_hi) (indices into base); out row index = i - i_lo.  skew_a/skew_b may be NULL (= 0).
hipError_t launch_spline_backward_eval(hipStream_t stream, const double* Y, const double* R, long long ld, int n_cols,
                                       long long g0, long long n_rows, long long n_knots, const double* x,
                                       const SplineTable* table, int tile, int halo, const double* base,
                                       const double* skew_a, const double* skew_b, double tt, long long i_lo,
                                       long long i_hi, double* out, long long ldo);

// ---- the same spline in B-spline form (kernels_bspline.hip): coefficients c with s(u) = sum_k c_k B_k(u) on the
// not-a-knot knot vector.  Forward elimination of the collocation system commutes with the synthesis contraction, so it
// runs on the MODES and the grid pass is the back substitution + evaluation alone.
struct BsplineTable {  // per knot j: what the back substitution + evaluation reads (20 words, staged through LDS)
  double m[16];        // m[4 d + q]: coefficient of t^d of B_{f_j + q} on [x_j, x_{j+1}], t = u - x_j, f_j = clamp(j-1, 0, n-4)
  double G, D;         // c_j = c'_j - G c_{j+1} - D c_{j+2}
  double x;            // x_j
  double pad;
};
struct BsplineForward {  // per knot j: c'_j = P y_j - A c'_{j-1} - E c'_{j-2}
  double P, A, E, x;     // x = x_j
};
hipError_t launch_bspline_table(hipStream_t stream, const double* x, long long n, BsplineTable* table, BsplineForward* fwd,
                                long long j_lo /* first knot the arrays are backed for */, long long j0, long long j1);
// Aout[r][0 .. n_modes] = forward-eliminated [A | 1] over rows r = knots g0 .. g0 + n_rows (complex; with_ones: the extra
// last column is the eliminated constant series, which carries the per-column offset through the contraction)
hipError_t launch_bspline_forward_modes(hipStream_t stream, const double* A, long long lda, int n_modes, double* Aout,
                                        long long ldo, long long g0, long long n_rows, long long n_knots,
                                        const BsplineForward* table, int tile, int halo, int with_ones);
// the back substitution on the eliminated modes: Aout = B-spline coefficients of the n_cols columns (out of place)
hipError_t launch_bspline_backward_modes(hipStream_t stream, const double* A, long long lda, int n_cols, double* Aout, long long ldo,
                                         long long g0, long long n_rows, const BsplineTable* table, int tile, int halo);
// both sweeps in one pass over memory (a thread keeps its column's tile + run-in rows in registers): Aout[r][0 .. n_modes] =
// B-spline coefficients of [A | 1]
hipError_t launch_bspline_solve_modes(hipStream_t stream, const double* A, long long lda, int n_modes, double* Aout, long long ldo,
                                      long long g0, long long n_rows, const BsplineForward* fwd, const BsplineTable* table, int with_ones);
// AsymptoticBondiData: Horner mixing of the six synthesised fields (as launch_abd_mix) fused with their elimination
struct AbdGrids;
hipError_t launch_abd_mix_forward(hipStream_t stream, const AbdGrids& Y, const AbdGrids& R, long long ld, int n_cols, long long g0,
                                  long long n_rows, const BsplineForward* table, int tile, int halo, const double* alpha,
                                  const double* ethk_over_k, const double* eth_alpha, const double* etheth_alpha,
                                  const double* inv_k, const double* inv_k3, int n_fields = 6 /* 5: without sigma */);
// B[row][0 .. 2 n_cols) = -off[0 .. 2 n_cols): the synthesis-matrix row that multiplies the constant column
hipError_t launch_negated_row(hipStream_t stream, const double* off, double* row, int n);
// back substitution + evaluation (arguments as launch_spline_backward_eval, C = eliminated grid coefficients)
// how far apart the lanes of a wave can stand (host side, optional): ranges of skew_a / skew_b within any block of 64 columns of the
// launch, and the time axis indexed by global knot number
struct BsplineSpread {
  double skew_rate_range, skew_offset_range;
  const double* x;
  unsigned long long* launches = nullptr;  // optional host counters: kernel launches [0] with the abscissa window, [1] of the gather instance
};
hipError_t launch_bspline_backward_eval(hipStream_t stream, const double* C, long long ld, int n_cols, long long g0,
                                        long long n_rows, long long n_knots, const double* x, const BsplineTable* table,
                                        int tile, int halo, const double* base, const double* skew_a, const double* skew_b,
                                        double tt, long long i_lo, long long i_hi, double* out, long long ldo, int n_cu,
                                        const BsplineSpread* spread = nullptr);

// ---- time-series calculus and grid products (kernels_series.hip; scri/modes_time_series.py:72-202)
// spline slopes s_j at all knots from the forward-pass result R (S != R)
hipError_t launch_spline_slopes(hipStream_t stream, const double* R, double* S, long long ld, int n_cols, long long n,
                                const SplineTable* table, int tile, int halo);
// running integrals at the knots: P1 = int f (order >= 1), P2 = int P1 (order 2); carry: spline_prefix_carry_size doubles
long long spline_prefix_carry_size(long long n, int n_cols);
// antiderivatives of order k >= 3: knot values of the levels 1..k in Pall + (r - 1) level_stride (doubles), then the evaluation
hipError_t launch_spline_prefix_levels(hipStream_t stream, const double* Y, const double* S, long long ld, int n_cols, long long n,
                                       const double* x, double* Pall, long long level_stride, double* carry, int levels);
hipError_t launch_spline_antiderivative_eval(hipStream_t stream, const double* Y, const double* S, const double* Pall, long long level_stride,
                                             long long ld, int n_cols, long long n, const double* x, const double* x_new, long long n_new,
                                             int k, double* out, long long ldo);
hipError_t launch_spline_prefix(hipStream_t stream, const double* Y, const double* S, long long ld, int n_cols, long long n,
                                const double* x, double* P1, double* P2, double* carry, int order);
// out[i][c] = (d/du)^order spline_c(x_new[i]), order in [-2, 3] (negative: antiderivatives vanishing at x[0])
hipError_t launch_spline_hermite_eval(hipStream_t stream, const double* Y, const double* S, const double* P1, const double* P2,
                                      long long ld, int n_cols, long long n, const double* x, const double* x_new,
                                      long long n_new, int order, double* out, long long ldo);
// c = a * b, n complex numbers
hipError_t launch_cmul(hipStream_t stream, const double* a, const double* b, double* c, long long n);

// <Ldt> f8[n][3], <LL> f8[n][9], omega = -<LL>^-1 <Ldt> f8[n][3] (any may be null) from modes F and their time
// derivative Fdot, both c16[n][ld/2] (scri/mode_calculations.py:14-57, 209-313, 403-432)
hipError_t launch_angular_velocity(hipStream_t stream, const double* F, const double* Fdot, long long ld, long long n_times,
                                   int ell_min, int n_modes, double* ldt_out, double* ll_out, double* omega_out);
// The kernel keeps the two rows of a time step in LDS, one wave per step: the launcher takes 4, 2 or 1 waves per workgroup, the most
// whose rows fit.  angular_velocity_max_modes: the most modes one wave's rows can hold on the current device (5120 with 160 KB);
// angular_velocity_supported: whether n_modes is within that.  The entries ask before they launch anything.
int angular_velocity_max_modes();
bool angular_velocity_supported(int n_modes);

// ---- frame construction (kernels_frames.hip): rotors f8[n][4] = (w, x, y, z)
struct Vec4 {
  double v[4];
};
// time-parallel inclusive scans in place (wave shuffles, LDS, a second pass over the block totals; totals: frame_scan_blocks(n) elements)
long long frame_scan_blocks(long long n);
// ordered quaternion product: q[j] <- q[j] q[j-1] ... q[0] (later elements multiply on the left)
hipError_t launch_scan_quat(hipStream_t stream, double* q, long long n, double* totals);
// composition of maps {+1, -1} -> {+1, -1} stored as 2 bits: m[j] <- m[j] o m[j-1] o ... o m[0]
hipError_t launch_scan_sign_maps(hipStream_t stream, unsigned* m, long long n, unsigned* totals);
// om3 f8[n][3] -> w4 f8[n][4] = (x, y, z, 0): two complex columns for the spline kernels
hipError_t launch_pad_omega(hipStream_t stream, const double* om3, double* w4, long long n);
// Q[0] = 1, Q[j + 1] = E_j: the rotor of sampling interval j from omega (w4) and its spline slopes (s4) at the knots
hipError_t launch_interval_rotors(hipStream_t stream, const double* w4, const double* s4, const double* x, long long n, double amax,
                                  double* Q);
// out[j] = P[j] R0 normalised (out[0] = R0 as given); out may be P
hipError_t launch_frame_finish(hipStream_t stream, const double* P, long long n, Vec4 R0, double* out);
// raw unit eigenvector of the largest eigenvalue of ll f8[n][9]
hipError_t launch_dominant_axis(hipStream_t stream, const double* ll, long long n, double* axis);
// the sign maps of the continuity rule in scan order: fwd[k] for step anchor + k (n - anchor maps), bwd[k] for step anchor - k
// (anchor + 1 maps); element 0 of both is the constant map to the anchor's sign
hipError_t launch_axis_sign_maps(hipStream_t stream, const double* axis, long long n, long long anchor, Vec4 rough, unsigned* fwd,
                                 unsigned* bwd);
hipError_t launch_axis_apply_signs(hipStream_t stream, const double* axis, long long n, long long anchor, const unsigned* fwd,
                                   const unsigned* bwd, double* out);
// R = sqrt(-v z): the rotor taking z to the unit vector v (-1 -> rotation about x, as quaternions.sqrt)
hipError_t launch_axis_rotor(hipStream_t stream, const double* axis, long long n, double* R);
// h[j] = ((Rdot z R^-1).w, 0): one complex column
hipError_t launch_halfgammadot(hipStream_t stream, const double* R, const double* Rdot, long long n, double* h);
// out = R (cos g + z sin g), g = halfgamma[j][0] (one complex column); out may be R
hipError_t launch_spin_about_z(hipStream_t stream, const double* R, const double* halfgamma, long long n, double* out);
// om3 = vector part of 2 Rdot R^-1
hipError_t launch_rotor_omega(hipStream_t stream, const double* R, const double* Rdot, long long n, double* om3);
// frame <- normalised frame * right (with_right), then exp(round(log frame * pow2) / pow2) (pow2 > 0), rounded log to log_out,
// (w + i z, y + i x) to spinors; log_out, spinors may be null
hipError_t launch_frame_adjust(hipStream_t stream, double* frame, long long n, Vec4 right, int with_right, double pow2, double* log_out,
                               double* spinors);
// quaternion.squad in two steps (n >= 2 knots t, rotors R f8[n][4]): the control points AB f8[n][8] = (A_i, B_i) with the statement's end
// rules, B[n-1] = the mirrored rotor beyond the end; then out f8[m][4] at the arguments t_out[m], in any order
hipError_t launch_squad_control(hipStream_t stream, const double* R, const double* t, long long n, double* AB);
hipError_t launch_squad_eval(hipStream_t stream, const double* R, const double* t, long long n, const double* AB, const double* t_out,
                             long long m, double* out);

// ---- time-and-phase alignment from correlation moments (kernels_align.hip; scri_amd/alignment.py)
constexpr int ALIGN_TILE_OFFSETS = 16;    // offsets x rows of a workgroup's tile; the row tiling fixes the order of every sum
constexpr int ALIGN_TILE_ROWS = 64;
constexpr int ALIGN_CHUNK_COLS = 16;      // columns staged at a time
constexpr int ALIGN_STRETCH_KNOTS = 112;  // knots of the moving waveform a tile stages in LDS; a longer stretch is read through L2
constexpr long long ALIGN_MAX_KNOTS = 1LL << 31;  // a tile keeps the intervals of its arguments as 32-bit offsets into its stretch
constexpr int ALIGN_MAX_SLOTS = 2 * 8192 + 1;     // one slot per m of the largest l the mode kernels carry (engine.h, MAX_ELL)
inline long long align_row_tiles(long long nw) { return (nw + ALIGN_TILE_ROWS - 1) / ALIGN_TILE_ROWS; }
struct AlignSeries {  // the two waveforms of one alignment, all device memory
  const double* ta;   // [na] time axis of the moving waveform, strictly increasing
  long long na;
  const double2* Y;   // c16[na][ld_a] its values ...
  const double2* S;   // ... and the slopes of its not-a-knot spline at the knots
  long long ld_a;
  const int* col_a;   // [n_cols] column of Y / S per common column
  const double* tw;   // [nw] window times of the fixed waveform, strictly increasing
  const double* w;    // [nw] quadrature weights
  long long nw;
  const double2* B;   // c16[nw][ld_b] window rows of the fixed waveform
  long long ld_b;
  const int* col_b;   // [n_cols]
  int n_cols;
};
// out[o][d0 + d][1 + 2 n_slots] (o <= order, rows of nd_total offsets) = (N_a, Re C_0, Im C_0, ...) of the offsets dts[0 .. nd) and their
// dt-derivatives; m_slot[n_cols] in [0, n_slots); dts ascending; partial: align_row_tiles(nw) (order + 1) nd (1 + 2 n_slots) doubles
hipError_t launch_align_moments(hipStream_t stream, const AlignSeries& a, const int* m_slot, int n_slots, const double* dts, long long nd,
                                long long d0, long long nd_total, int order, double* partial, double* out);
// out2 = (sum_i w_i sum_c |A_c(t_i + dt) phase_c - B_ic|^2, sum_i w_i sum_c |B_ic|^2); phase c16[n_cols]; partial: 2 align_row_tiles(nw) doubles
hipError_t launch_align_residual(hipStream_t stream, const AlignSeries& a, const double* phase, double dt, double* partial, double* out2);

// ---- bit transforms of the storage formats (kernels_bits.hip; scri/utilities.py:194-406)
// rows of n_cols 64-bit words; forward: out[i] = in[i-1] ^ in[i]; reverse: running XOR (carry: xor_carry_words words)
long long xor_carry_words(long long n_rows, long long n_cols);
hipError_t launch_xor_timeseries(hipStream_t stream, const void* in, void* out, void* carry, long long n_rows, long long n_cols,
                                 int reverse);
// n elements of bit_width bits; widths[n_widths] from the most significant piece down, summing to bit_width
hipError_t launch_multishuffle(hipStream_t stream, const void* in, void* out, long long n, const int* widths, int n_widths,
                               int bit_width, int forward);
// acc[0] += sum d_j mod 65535-ish, acc[1] += sum (N-j) d_j (both to be reduced mod 65535 by the caller); acc zeroed before
hipError_t launch_fletcher32(hipStream_t stream, const void* data, long long n_words, unsigned long long* acc);

// the corotating paired-XOR storage form (scri/SpEC/file_io/corotating_paired_xor.py:70-90, :240,255), one kernel each way.
// partner[n_modes]: column of (l, -m) for column (l, m); own[n_own]: the columns with m >= 0.  Pointers 16-byte aligned.
constexpr int PAIRED_PACK_TILE = 32;               // rows one wave packs in sequence (plus the halo row before them)
constexpr int PAIRED_UNPACK_TILE = 64;             // rows per tile of the running XOR
constexpr size_t PAIRED_PACK_MAX_LDS = 160 * 1024;  // the pack kernel stages 36 bytes per mode
size_t paired_pack_lds_bytes(int n_modes);
// in c16[n_out + halo][ld] -> out u64[n_out][2 n_modes]; halo = 1: row 0 of `in` is only the row before output row 0 (a piece of a
// longer series).  bad: min over the rows that could not be packed of row_base + output row (preset to all ones).
hipError_t launch_paired_pack(hipStream_t stream, const void* in, long long ld, long long n_out, int halo, const int* partner, int n_modes,
                              double tol_per_mode, long long row_base, void* out, unsigned long long* bad);
long long paired_unpack_carry_words(long long n_rows, int n_modes);
// words u64[n_rows][2 n_modes] -> out c16[n_rows][ld_out]; seed u64[2 n_modes]: running XOR before row 0 on entry, after the last row on exit
hipError_t launch_paired_unpack(hipStream_t stream, const void* words, long long n_rows, const int* own, int n_own, const int* partner,
                                int n_modes, void* carry, void* seed, void* out, long long ld_out);

// ---- polar form of a series (kernels_polar.hip; scri/waveform_base.py:520-533): abs = hypot(re, im), arg = atan2(im, re), and the angle
// unwrapped down the rows by an integer wrap count (p + 2 pi K, NaN from the first NaN angle of a column on)
constexpr int POLAR_TILE_ROWS = 64;  // rows per tile of the wrap-count scan
long long polar_carry_words(long long n_rows, int n_cols);  // 64-bit words of `carry`
// in c16[n_rows][ld] -> abs_out, arg_out f8[n_rows][ld_out] (one may be null); unwrap != 0: arg_out is the unwrapped angle (carry needed)
hipError_t launch_polar(hipStream_t stream, const void* in, long long ld, long long n_rows, int n_cols, int unwrap, double* abs_out,
                        double* arg_out, long long ld_out, void* carry);
// acc[0] += elements with a non-finite part, acc[1] = min(acc[1], first row holding one); acc preset to (0, all ones)
hipError_t launch_count_nonfinite(hipStream_t stream, const void* in, long long ld, long long n_rows, int n_cols, unsigned long long* acc);

// ---- fluxes of energy, momentum, angular momentum and boost in one pass over the modes (kernels_flux.hip; scri/flux.py:182-798)
// How the launcher runs a range of n_modes columns: one wave per time step, `waves` steps per pass of a workgroup, at most `groups`
// persistent workgroups; tables_in_lds: the coefficient image sits in LDS beside the rows, else it is read through L2.
struct FluxShape {
  int waves, groups;
  bool tables_in_lds;
  size_t lds_bytes;
};
int flux_image_doubles(int n_modes);                 // doubles of the coefficient image (engine_flux.hip builds it)
bool flux_launch_shape(int n_modes, FluxShape* S);  // false: not even one wave's row pair fits in LDS
// energy f8[n], momentum / angular / boost f8[n][3] (any may be null; h may be null without angular and boost, t without boost) of
// h, hdot c16[n][ld] holding l = ell_min .. ell_max, ell_min >= 2
hipError_t launch_poincare_fluxes(hipStream_t stream, const double* t, const double* h, long long ld_h, const double* hdot, long long ld_hdot,
                                  long long n_times, int ell_min, int ell_max, const double* image, double* energy, double* momentum,
                                  double* angular, double* boost);
// brackets of two waveforms (scri/mode_calculations.py:60-180): inner c16[n] = sum conj(f) g, l_out c16[n][3] = <f|L_a|g>, a = +, -, z,
// ll_out c16[n][9] = <f|L_a L_b|g>, ab = pp, pm, mp, mm, pz, zp, mz, zm, zz (any may be null, not all) of f c16[n][ld_f], g c16[n][ld_g],
// both pointing AT the column (ell_min, -ell_min) of rows that may hold more on either side.  One row of f per wave in LDS, no tables.
bool pair_launch_shape(int n_modes, FluxShape* S);  // false: a row does not fit in LDS (tables_in_lds is always false)
hipError_t launch_pair_brackets(hipStream_t stream, const double* f, long long ld_f, const double* g, long long ld_g, long long n_times,
                                int ell_min, int ell_max, double* inner, double* l_out, double* ll_out);
// Bondi charges (scri/asymptotic_bondi_data/bms_charges.py:14-200): four_momentum f8[n][4], angular / boost / com f8[n][3] (any may be
// null, not all) of sigma, sigma_dot c16[n][ld] holding l = 0 .. ell_max and the first four columns of psi1, psi2 c16[n][ld].  sigma_dot
// and psi2 may be null without four_momentum and boost, psi1 with four_momentum alone, t without boost.
int charge_image_doubles(int n_modes);                 // doubles of the coefficient image (engine_flux.hip builds it)
bool charge_launch_shape(int n_modes, FluxShape* S);  // false: not even one wave's row pair fits in LDS
hipError_t launch_bondi_charges(hipStream_t stream, const double* t, const double* psi1, long long ld_psi1, const double* psi2, long long ld_psi2,
                                const double* sigma, long long ld_sigma, const double* sigma_dot, long long ld_sigma_dot, long long n_times,
                                int ell_max, const double* image, double* four_momentum, double* angular, double* boost, double* com);
// Products on Gauss-Legendre rows (kernels_product.hip): out c16[n][ld_out] = the modes l = 0 .. l_out of op(a) op(b), rows c16[n][ld] from
// l = 0; op = bar where conj != 0.  tab_a, tab_b: lambda tables f8[n_nodes][(l + 1)^2] of the EFFECTIVE spins, tab_out the output spin's
// with 2 pi w_j folded (engine_product.hip builds them); n_nodes = product_nodes(l_a, l_b, l_out).
struct ProductShape {
  int steps, groups;  // time steps per pass of one workgroup, workgroups at most
  bool tables_in_lds;
  size_t lds_bytes;
};
int product_nodes(int l_a, int l_b, int l_out);
bool product_launch_shape(int l_a, int l_b, int l_out, ProductShape* S);  // false: the rows and panels of one time step do not fit in LDS
hipError_t launch_mode_product(hipStream_t stream, const double* a, long long ld_a, int spin_a, int l_a, int conj_a, const double* b, long long ld_b,
                               int spin_b, int l_b, int conj_b, long long n_times, int l_out, const double* tab_a, const double* tab_b,
                               const double* tab_out, double* out, long long ld_out);
// the same body on sigma and bar(sigma_dot) (tab_plus: spin 2, tab_minus: spin -2, both of ell_max; tab_out: spin 0 of l_out, weighted) with
// psi2 and the diagonal terms added as the row is stored; any output may be null, not all
hipError_t launch_supermomenta(hipStream_t stream, const double* psi2, long long ld_psi2, const double* sigma, long long ld_sigma,
                               const double* sigma_dot, long long ld_sigma_dot, long long n_times, int ell_max, int l_out, int integrated,
                               const double* tab_plus, const double* tab_minus, const double* tab_out, double* bondi_sachs, double* moreschi,
                               double* geroch, double* geroch_winicour, double* mass_aspect, long long ld_out);
// The six Bondi-gauge violations and their norms in one launch (constraint_kernel: the same stages, sigma's theta sums taken once).  Rows
// c16[n][ld] from l = 0; an input that no output asked for reads may be null.  v[k] c16[n][ld_out] and norms f8[n][6]: any may be null, not all.
enum { CONSTRAINT_SIGMA = 5, CONSTRAINT_PSI_DOT = 6, CONSTRAINT_SIGMA_DOT = 9, CONSTRAINT_SIGMA_DDOT = 10, CONSTRAINT_INPUTS = 11 };
struct ConstraintArgs {
  const double* in[CONSTRAINT_INPUTS];  // psi0 .. psi4, sigma; d/du of psi0, psi1, psi2; d/du and d2/du2 of sigma (psi0 itself is never read)
  long long ld[CONSTRAINT_INPUTS];
  int l_max, n_nodes;         // n_nodes = product_nodes(l_max, l_max, l_max)
  const double* tab_sigma;    // lambda table of spin 2
  const double* tab_in[3];    // of spins 0, -1, -2: psi2, psi3, psi4 and bar(sigma_dot)
  const double* tab_out[3];   // of spins 2, 1, 0 with 2 pi w_j folded
  double* v[6];
  long long ld_out;
  double* norms;
};
hipError_t launch_bondi_constraints(hipStream_t stream, const ConstraintArgs& Q, long long n_times);
// One stage of the Bianchi identities run forwards (bianchi_kernel: the inner step of constraint_kernel, stored instead of subtracted):
//     rhs_k = eth a + (3 - k) sigma b     k = 1: a = psi2, b = psi3     k = 0: a = psi1, b = psi2
//     k = 2 (the head): a = sigma_dot, b = sigma_ddot as stored;  psi4 = -bar(b), psi3 = -eth bar(a), rhs_2 = eth psi3 + sigma psi4
// Rows c16[n][ld] from l = 0.  psi3, psi4 c16[n][ld_psi]: written by the head alone, null otherwise.
struct BianchiArgs {
  const double *sigma, *a, *b;
  long long ld_sigma, ld_a, ld_b;
  int k, l_max, n_nodes;                    // n_nodes = product_nodes(l_max, l_max, l_max)
  const double *tab_sigma, *tab_b, *tab_out;  // lambda tables of spins 2, -k and 2 - k (the last with 2 pi w_j folded)
  double *rhs, *psi3, *psi4;
  long long ld_rhs, ld_psi;
};
hipError_t launch_bianchi_rhs(hipStream_t stream, const BianchiArgs& Q, long long n_times);
// out c16[n] = sum_e op(a[t][rows_e]) values_e b[t][cols_e] for triplets on the device, indices inside [0, n_cols) (the entry checks them)
int expectation_max_cols();
hipError_t launch_expectation_values(hipStream_t stream, const double* a, long long ld_a, int conj_a, const double* b, long long ld_b,
                                     long long n_times, int n_cols, const int* rows, const int* cols, const double* values, long long n_el,
                                     double* out);

// ---- a real series and its conformal factor on a supertranslated cut (kernels_cut.hip; map_to_superrest_frame.py:108-224)
// psi_out[p] = Re sum_k Y_k(p) spline_k(alpha[p]) over the (2 ell_max + 1)^2 pixels of the equiangular grid, from the window rows
// W c16[n_window][ldw] (columns from l = 0), their spline slopes S (same shape) and the knots x; with_k: k_out[p] = the per-pixel spline
// through K_r(p) = M_r / (P0_r - P_r . r(p)) at alpha[p] (1 otherwise); comb_out c16 = (psi - d_alpha) / K^3 (d_alpha c16 per pixel).
// lambda f8[(ell_max + 1)^2][2 ell_max + 1]: sYlm(theta_i, 0) of spin 0 (build_synthesis).  Any output may be null.  One workgroup per
// theta ring; cut_lds_bytes is its dynamic LDS (with K the forward sweep of a ring: 8 n_window (2 ell_max + 1) bytes of it).
constexpr int CUT_MAX_ELL = 24;
size_t cut_lds_bytes(int ell_max, long long n_window, int with_k);
hipError_t launch_cut(hipStream_t stream, const double* W, const double* S, long long ldw, long long n_window, const double* x,
                      const SplineTable* table, const double* lambda, const double* alpha, const double* d_alpha, int ell_max, int with_k,
                      double* psi_out, double* k_out, double* comb_out);
hipError_t launch_cut_real_to_complex(hipStream_t stream, const double* in, double* out, int n);  // c16 out = (in, 0)
hipError_t launch_cut_real_part(hipStream_t stream, const double* in, double* out, int n);        // f8 out = Re of c16 in
// modes c16[(ell_max + 1)^2] times (l+2)(l+1)l(l-1)/4, or with `inverse` its reciprocal; zero below l = 2
hipError_t launch_cut_scale_modes(hipStream_t stream, double* modes, int ell_max, int inverse);
// Re grid[p] += M(p) K(p)^3; m_grid / k_grid f8 per pixel, or null: the rest mass / conformal factor of the four l <= 1 columns of `modes`
hipError_t launch_cut_mass_term(hipStream_t stream, double* grid, const double* modes, const double* m_grid, const double* k_grid, int ell_max);

// centre-of-mass track and drift fit of the horizon trajectories (scri/SpEC/com_motion.py), kernels_com.hip
constexpr int COM_FIT_TILE = 256;  // panels (two intervals each) per partial of the moment sums: one per thread of a workgroup
constexpr int COM_FIT_OUT = 24;    // doubles of the fit's result block (com_fit_kernel)
// com_out[n][3] = (m_A x_A + m_B x_B) / (m_A + m_B), masses of length n or 1; matter != 0: also t_out = t / m and com_out / m
hipError_t launch_com_track(hipStream_t stream, const double* t, const double* xa, const double* xb, const double* ma, long long n_ma,
                            const double* mb, long long n_mb, long long n, int matter, double* t_out, double* com_out);
long long com_fit_work_doubles(long long n);
// window, Simpson moments in double-double and the closed-form fit of t[n], com[n][3] (n >= 2) into out[COM_FIT_OUT]
hipError_t launch_com_fit(hipStream_t stream, const double* t, const double* com, long long n, double skip_b, double skip_e, int accel,
                          double* work, double* out);

// ---- pointwise helpers
// Y[t][p] += coeff * Yaux[t][p] * X[t][p]^power,  X = (x_t - alpha_p) * xa_p - xb_p   (waveform_grid.py:516-550)
hipError_t launch_psi_mix(hipStream_t stream, double* Y, const double* Yaux, long long ld, int n_pix, long long n_rows,
                          const double* x /* times of the rows */, const double* alpha, const double* xa /* c16[n_pix] */,
                          const double* xb /* c16[n_pix] */, double coeff, int power);
// Horner mixing of the six ABD grids in place (transformations.py:340-385)
struct AbdGrids {
  double* y[6];
};
hipError_t launch_abd_mix(hipStream_t stream, const AbdGrids& g, long long ld, int n_pix, long long n_rows, const double* u,
                          const double* alpha, const double* ethk_over_k /* c16[n_pix] */,
                          const double* eth_alpha /* c16 */, const double* etheth_alpha /* c16 */, const double* inv_k,
                          const double* inv_k3);
// y[t][col] = (y[t][col] - off[col]) * scale[col]
hipError_t launch_affine_cols(hipStream_t stream, double* Y, long long ld, int n_cols, long long n_rows,
                              const double* off, const double* scale);

// ---- extrapolation to null infinity (scri/extrapolation.py:1394-1434; kernels_extrapolate.hip)
constexpr int EXTRAP_MAX_RADII = 64;  // one radius per lane of a wavefront
constexpr int EXTRAP_MAX_ORDER = 15;
struct ExtrapSource {  // the series of one radius: c16 rows of stride ld
  const double2* p;
  long long ld;
};
// out[o][t][m] (o stride out_order_stride, row stride n_modes) = constant term of the fit of order orders[o] of src[i].p[t][m] against
// 1 / radii[i * r_ld + t], i < n_radii; deficient[o] += the steps whose fit of order orders[o] is rank deficient (those rows are NaN)
hipError_t launch_extrapolate(hipStream_t stream, const ExtrapSource* src, int n_radii, const double* radii, long long r_ld,
                              long long n_times, int n_modes, const int* orders, int n_orders, double2* out, long long out_order_stride,
                              unsigned long long* deficient);

// ---- the precessing sample waveform and its finite-radius family (scri/sample_waveforms.py:383-755; kernels_sample.hip)
struct SamplePlan;   // sample_math.h: the steps at which the piecewise definitions change
struct SampleMode {  // one column of the corotating modes: c_lm x^(twice_power / 2) (1 + sign_m modulation) ringdown
  double re, im;
  int twice_power, sign_m;
};
// phi_pn f8[n], omega f8[n] (blended), omega_col c16[n - i0] = (omega, 0) from step i0 on
hipError_t launch_sample_phase(hipStream_t stream, const SamplePlan& P, const double* t, double* phi_pn, double* omega, double2* omega_col);
// integrands c16[ib - ia] = (opening-angle series, precession-angle series) times the slope of the falling transition; I_omega c16[n - i0]:
// the antiderivative of omega_col (zero at step i0)
hipError_t launch_sample_window(hipStream_t stream, const SamplePlan& P, const double* t, const double* phi_pn, const double2* I_omega,
                                double2* integrands);
// frame f8[n][4], out c16[n][ld] (n_modes columns written), spinors f8[n][4] of conj(frame) (may be null); I_window c16[ib - ia]: the
// antiderivative of the integrands (zero at step ia); left f8[4]: work space, receives conj(sqrt(frame[0]))
hipError_t launch_sample_waveform(hipStream_t stream, const SamplePlan& P, const double* t, const double* phi_pn, const double* omega,
                                  const double2* I_omega, const double2* I_window, double* left, const SampleMode* modes, int n_modes,
                                  double2* out, long long ld, double* frame, double* spinors);
constexpr int RADIUS_TERMS_MAX = 16;
struct RadiusTerms {  // coef[k - 1] = amp R^-k, k = 1 .. n
  int n;
  double coef[RADIUS_TERMS_MAX];
};
// out[t][c] = h0[t][c] + |h0[t][c]| sum_k coef[k - 1] exp(i k (50 pi / n) t_t); out and h0 must not overlap
hipError_t launch_radius_terms(hipStream_t stream, const double* t, long long n, const double2* h0, long long ld0, int n_cols,
                               const RadiusTerms& terms, double2* out, long long ld_out);

// ---- retardation of a raw finite-radius series to tortoise time (scri/extrapolation.py:27-45, :356-402; kernels_retard.hip)
constexpr int RETARD_TILE = 256;  // samples per tile of the three scans: one per thread of a workgroup
long long retard_tiles(long long n_raw);
// idx[j] = the raw index of kept sample j -- k is kept iff fl(T[k] + min_step) < min_{j > k} T[j] -- and st[0] = their number, st[1] = 0,
// st[2] = LLONG_MAX.  Work space: tile_min f8[tiles], rank i4[n_raw], count i8[tiles].  idx has n_raw entries, st three.
hipError_t launch_retard_keep(hipStream_t stream, const double* T, long long n_raw, double min_step, double* tile_min, int* rank,
                              long long* count, long long* idx, long long* st);
// for kept sample j < st[0]: t_out[j], radii_out[j] and factor[j] = fl(fl((R / coord_radius)^p) unit) (kernels_retard.hip states the
// arithmetic); st[1] += the kept radii that are not finite or not beyond 2 E, st[2] = the raw index of the first.  totals: 16 bytes per tile.
hipError_t launch_retard_time(hipStream_t stream, const double* T, const double* R, const double* lapse, long long n_raw, const long long* idx,
                              long long* st, double initial_adm_energy, double coord_radius, double ch_mass, double unit, int p, void* totals,
                              double* t_out, double* radii_out, double* factor);
// out c16[r][m] = in[idx[r]][m] * factor[r] for r < st[0], m < n_cols (factor == nullptr: the rows as they are); rows beyond are not written
hipError_t launch_retard_gather(hipStream_t stream, const void* in, long long ld, int n_cols, long long n_raw, const long long* idx,
                                const double* factor, const long long* st, void* out, long long ld_out);

}  // namespace bms
