// Time-and-phase alignment of two waveforms (scri_amd/alignment.py) from correlation moments.
//
// With window times t_i of the fixed waveform, trapezoid weights w_i, common columns c, A_c the not-a-knot cubic spline of the moving
// waveform's column and B_ic the rows of the fixed one, everything the cost needs at a time offset dt is
//     N_a(dt) = sum_i w_i sum_c |A_c(t_i + dt)|^2          C_m(dt) = sum_i w_i sum_{c: m_c = m} A_c(t_i + dt) conj(B_ic)
// and their dt-derivatives, which are the same sums over the spline's own derivatives: 1 + 2 n_slots numbers per offset and order.
// align_moments_kernel forms them for many offsets at once (the brute-force scan, order 0) or for one (a Newton step, orders 0..2).
//
// Evaluation: the local Hermite form of spline_hermite_eval_kernel (kernels_series.hip) from knot values Y and knot slopes S; the
// interval of x = t_i + dt is the last knot <= x clamped to [0, na - 2] (scipy: ta[j] <= x < ta[j + 1], the last interval closed, an
// argument outside the axis by rounding takes the end interval's cubic).
//
// Work shape: a workgroup takes ALIGN_TILE_OFFSETS consecutive offsets x ALIGN_TILE_ROWS consecutive window rows.  Offsets and rows
// are sorted, so the knots the tile reaches are one stretch [j_lo, j_hi + 1]; per chunk of ALIGN_CHUNK_COLS columns the tile stages
// that stretch of Y and S and its rows of B in LDS and every (offset, column) thread walks the rows of the tile in order.  A stretch
// beyond ALIGN_STRETCH_KNOTS (coarse offsets over a fine axis, graded axes) is read through L2 instead: the loads differ, the
// arithmetic does not.  LDS rows are ALIGN_CHUNK_COLS = 16 double2 = 256 B = one bank row, so the 16-lane groups of a ds_read_b128
// (which mix lanes of two offsets, i.e. two different rows) always land on 16 different 16-byte slots: no padding is needed.
//
// Reduction: a thread's sum over the rows of its tile, then the columns of a chunk in column order into the (offset, slot) running
// value of the tile (kept in the tile's block of the work space: always the same thread, no atomics), chunk after chunk; a second
// kernel adds the row tiles in order.  The row tiling is a constant, the offset tiling only decides which workgroup holds an offset:
// the moments of an offset are the same bits whether it is scanned alone or among thousands, staged or not.
//
// Contraction is switched off for this file and every fused multiply-add is written out: the staged and the unstaged instantiation
// of the loop must round alike whatever the optimiser does with them.
#include "kernels.h"

#pragma clang fp contract(off)

namespace bms {

namespace {

constexpr int AL_TD = ALIGN_TILE_OFFSETS, AL_TR = ALIGN_TILE_ROWS, AL_CW = ALIGN_CHUNK_COLS, AL_SK = ALIGN_STRETCH_KNOTS;
static_assert(AL_TD * AL_CW == 256 && AL_CW == 16 && AL_TR == 64, "the thread layout of align_moments_kernel");
// LDS: Y and S of the stretch, B of the tile, the stretch of the axis, the window times and weights, the interval of every (offset, row)
constexpr size_t AL_LDS = (size_t)(2 * AL_SK + AL_TR) * AL_CW * sizeof(double2) + (size_t)(AL_SK + 2 * AL_TR) * sizeof(double) +
                          (size_t)AL_TD * AL_TR * sizeof(int);
static_assert(2 * AL_LDS <= 160 * 1024, "two workgroups per CU");
static_assert(256 * 9 * sizeof(double) <= (size_t)AL_SK * AL_CW * sizeof(double2), "the column reduction reuses the Y stage");

// last knot <= x within [lo, hi], given ta[lo] <= x < ta[hi] or lo / hi the clamped ends of the axis
__device__ __forceinline__ long long align_interval(const double* __restrict__ ta, long long lo, long long hi, double x) {
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (ta[mid] <= x)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

struct AlignValue {  // the spline of one column and its first two derivatives at one argument
  double2 v0, v1, v2;
};

template <int ORDER>
__device__ __forceinline__ AlignValue align_eval(double2 y0, double2 y1, double2 s0, double2 s1, double h, double t) {
  // c3 = (s0 + s1 - 2 D) / h^2, c2 = (D - s0) / h - c3 h, D = (y1 - y0) / h: kernels_series.hip, hermite()
  const double ih = 1.0 / h;
  const double dx = (y1.x - y0.x) * ih, dy = (y1.y - y0.y) * ih;
  const double tx = ((s0.x + s1.x) - 2.0 * dx) * ih, ty = ((s0.y + s1.y) - 2.0 * dy) * ih;
  const double c3x = tx * ih, c3y = ty * ih;
  const double c2x = (dx - s0.x) * ih - tx, c2y = (dy - s0.y) * ih - ty;
  AlignValue V;
  V.v0.x = fma(t, fma(t, fma(t, c3x, c2x), s0.x), y0.x);
  V.v0.y = fma(t, fma(t, fma(t, c3y, c2y), s0.y), y0.y);
  if (ORDER >= 1) {
    V.v1.x = fma(t, fma(3.0 * t, c3x, 2.0 * c2x), s0.x);
    V.v1.y = fma(t, fma(3.0 * t, c3y, 2.0 * c2y), s0.y);
  }
  if (ORDER >= 2) {
    V.v2.x = fma(6.0 * t, c3x, 2.0 * c2x);
    V.v2.y = fma(6.0 * t, c3y, 2.0 * c2y);
  }
  return V;
}

// acc[o] = (N_a, Re C, Im C) of order o, one more row: weight w, fixed waveform b
template <int ORDER>
__device__ __forceinline__ void align_add(double (&acc)[ORDER + 1][3], const AlignValue& V, double w, double2 b) {
  acc[0][0] = fma(w, fma(V.v0.x, V.v0.x, V.v0.y * V.v0.y), acc[0][0]);
  acc[0][1] = fma(w, fma(V.v0.x, b.x, V.v0.y * b.y), acc[0][1]);
  acc[0][2] = fma(w, fma(V.v0.y, b.x, -(V.v0.x * b.y)), acc[0][2]);
  if (ORDER >= 1) {
    acc[1][0] = fma(2.0 * w, fma(V.v0.x, V.v1.x, V.v0.y * V.v1.y), acc[1][0]);
    acc[1][1] = fma(w, fma(V.v1.x, b.x, V.v1.y * b.y), acc[1][1]);
    acc[1][2] = fma(w, fma(V.v1.y, b.x, -(V.v1.x * b.y)), acc[1][2]);
  }
  if (ORDER >= 2) {
    const double q = fma(V.v1.x, V.v1.x, V.v1.y * V.v1.y) + fma(V.v0.x, V.v2.x, V.v0.y * V.v2.y);
    acc[2][0] = fma(2.0 * w, q, acc[2][0]);
    acc[2][1] = fma(w, fma(V.v2.x, b.x, V.v2.y * b.y), acc[2][1]);
    acc[2][2] = fma(w, fma(V.v2.y, b.x, -(V.v2.x * b.y)), acc[2][2]);
  }
}

}  // namespace

// partial: [row tile][ORDER + 1][nd][1 + 2 n_slots]; blockIdx.x = offset tile, blockIdx.y + row_tile0 = row tile
template <int ORDER>
__global__ __launch_bounds__(256) void align_moments_kernel(AlignSeries a, const int* __restrict__ m_slot, int n_slots,
                                                            const double* __restrict__ dts, long long nd, long long row_tile0,
                                                            double* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char al_lds[];
  double2* Ys = reinterpret_cast<double2*>(al_lds);
  double2* Ss = Ys + AL_SK * AL_CW;
  double2* Bs = Ss + AL_SK * AL_CW;
  double* tas = reinterpret_cast<double*>(Bs + AL_TR * AL_CW);
  double* tws = tas + AL_SK;
  double* wts = tws + AL_TR;
  int* jrel = reinterpret_cast<int*>(wts + AL_TR);
  double* red = reinterpret_cast<double*>(Ys);  // [256][9] between the row walk of a chunk and the staging of the next

  const int tid = threadIdx.x, cx = tid & (AL_CW - 1), dy = tid >> 4;
  const long long d_first = (long long)blockIdx.x * AL_TD;
  const long long tile_r = row_tile0 + blockIdx.y;
  const long long i0 = tile_r * AL_TR;
  const int n_r = (int)(a.nw - i0 < AL_TR ? a.nw - i0 : AL_TR);
  const int n_d = (int)(nd - d_first < AL_TD ? nd - d_first : AL_TD);
  const double* __restrict__ ta = a.ta;

  // rows and offsets ascend and the rounded sum is monotone in both: the first and the last pair bound every argument of the tile
  const double x_min = a.tw[i0] + dts[d_first], x_max = a.tw[i0 + n_r - 1] + dts[d_first + n_d - 1];
  const long long j_lo = align_interval(ta, 0, a.na - 1, x_min), j_hi = align_interval(ta, 0, a.na - 1, x_max);
  const long long n_j = j_hi - j_lo + 2;  // knots j_lo .. j_hi + 1
  const bool staged = n_j <= AL_SK;

  for (int e = tid; e < AL_TR; e += 256) {
    tws[e] = e < n_r ? a.tw[i0 + e] : 0.0;
    wts[e] = e < n_r ? a.w[i0 + e] : 0.0;
  }
  if (staged)
    for (int e = tid; e < (int)n_j; e += 256) tas[e] = ta[j_lo + e];
  for (int e = tid; e < AL_TD * AL_TR; e += 256) {
    const int r = e & (AL_TR - 1), q = e >> 6;
    if (r < n_r && q < n_d) jrel[e] = (int)(align_interval(ta, j_lo, j_hi + 1, a.tw[i0 + r] + dts[d_first + q]) - j_lo);
  }

  const int nv = 1 + 2 * n_slots;
  const long long d = d_first + dy;
  const double dt = dy < n_d ? dts[d] : 0.0;
  for (int cc = 0; cc < a.n_cols; cc += AL_CW) {
    __syncthreads();  // the stage is free: the reduction of the previous chunk has read it
    const int c = cc + cx;
    const bool c_ok = c < a.n_cols;
    const long long ca = c_ok ? a.col_a[c] : 0, cb = c_ok ? a.col_b[c] : 0;
    if (staged)
      for (int e = tid; e < (int)n_j * AL_CW; e += 256) {  // (256 is a multiple of the chunk width: e & 15 == cx)
        double2 y = {0.0, 0.0}, s = {0.0, 0.0};
        if (c_ok) {
          const long long at = (j_lo + (e >> 4)) * a.ld_a + ca;
          y = a.Y[at], s = a.S[at];
        }
        Ys[e] = y, Ss[e] = s;
      }
    for (int e = tid; e < n_r * AL_CW; e += 256) Bs[e] = c_ok ? a.B[(i0 + (e >> 4)) * a.ld_b + cb] : double2{0.0, 0.0};
    __syncthreads();

    double acc[ORDER + 1][3];
#pragma unroll
    for (int o = 0; o <= ORDER; ++o) acc[o][0] = acc[o][1] = acc[o][2] = 0.0;
    if (c_ok && dy < n_d) {
      const double2* __restrict__ yg = a.Y + ca;
      const double2* __restrict__ sg = a.S + ca;
      for (int r = 0; r < n_r; ++r) {
        const int jr = jrel[dy * AL_TR + r];
        double xj, xk;
        double2 y0, y1, s0, s1;
        if (staged) {
          xj = tas[jr], xk = tas[jr + 1];
          y0 = Ys[jr * AL_CW + cx], y1 = Ys[(jr + 1) * AL_CW + cx];
          s0 = Ss[jr * AL_CW + cx], s1 = Ss[(jr + 1) * AL_CW + cx];
        } else {
          const long long j = j_lo + jr;
          xj = ta[j], xk = ta[j + 1];
          y0 = yg[j * a.ld_a], y1 = yg[(j + 1) * a.ld_a];
          s0 = sg[j * a.ld_a], s1 = sg[(j + 1) * a.ld_a];
        }
        const double h = xk - xj, t = (tws[r] + dt) - xj;
        align_add<ORDER>(acc, align_eval<ORDER>(y0, y1, s0, s1, h, t), wts[r], Bs[r * AL_CW + cx]);
      }
    }
    __syncthreads();  // every thread has left the stage
#pragma unroll
    for (int o = 0; o <= ORDER; ++o)
#pragma unroll
      for (int k = 0; k < 3; ++k) red[tid * 9 + 3 * o + k] = acc[o][k];
    __syncthreads();
    if (dy < n_d) {
      const int n_q = a.n_cols - cc < AL_CW ? a.n_cols - cc : AL_CW;
      const double* mine = red + (size_t)dy * AL_CW * 9;
#pragma unroll
      for (int o = 0; o <= ORDER; ++o) {
        double* P = partial + (((tile_r * (ORDER + 1) + o) * nd + d) * nv);
        if (cx == 0) {
          double run = cc ? P[0] : 0.0;
          for (int q = 0; q < n_q; ++q) run += mine[q * 9 + 3 * o];
          P[0] = run;
        }
        for (int s = cx; s < n_slots; s += AL_CW) {
          double re = cc ? P[1 + 2 * s] : 0.0, im = cc ? P[2 + 2 * s] : 0.0;
          for (int q = 0; q < n_q; ++q)
            if (m_slot[cc + q] == s) re += mine[q * 9 + 3 * o + 1], im += mine[q * 9 + 3 * o + 2];
          P[1 + 2 * s] = re, P[2 + 2 * s] = im;
        }
      }
    }
  }
}

// out[(o nd_total + d0 + d) nv + v] = sum over the row tiles, in order, of partial[tile][o][d][v]
__global__ __launch_bounds__(256) void align_reduce_kernel(const double* __restrict__ partial, long long n_tiles, int n_ord, long long nd,
                                                           int nv, long long d0, long long nd_total, double* __restrict__ out) {
  const long long per_order = nd * nv, per_tile = per_order * n_ord;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < per_tile; e += (long long)gridDim.x * blockDim.x) {
    double sum = 0.0;
    for (long long t = 0; t < n_tiles; ++t) sum += partial[t * per_tile + e];
    const long long o = e / per_order, rem = e - o * per_order;
    out[(o * nd_total + d0) * nv + rem] = sum;
  }
}

hipError_t launch_align_moments(hipStream_t stream, const AlignSeries& a, const int* m_slot, int n_slots, const double* dts, long long nd,
                                long long d0, long long nd_total, int order, double* partial, double* out) {
  if (nd <= 0 || a.n_cols <= 0 || a.nw <= 0) return hipSuccess;
  if (order < 0 || order > 2) return hipErrorInvalidValue;
  const void* fn = order == 0 ? (const void*)align_moments_kernel<0> : order == 1 ? (const void*)align_moments_kernel<1> : (const void*)align_moments_kernel<2>;
  hipError_t e = allow_dynamic_lds(fn);
  if (e != hipSuccess) return e;
  const long long n_tiles = align_row_tiles(a.nw), d_tiles = (nd + AL_TD - 1) / AL_TD;
  if (d_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  for (long long t0 = 0; t0 < n_tiles; t0 += GRID_Y_MAX) {  // (the y extent of a grid ends at 65 535)
    const dim3 grid((unsigned)d_tiles, (unsigned)std::min(GRID_Y_MAX, n_tiles - t0));
    if (order == 0)
      hipLaunchKernelGGL(align_moments_kernel<0>, grid, dim3(256), AL_LDS, stream, a, m_slot, n_slots, dts, nd, t0, partial);
    else if (order == 1)
      hipLaunchKernelGGL(align_moments_kernel<1>, grid, dim3(256), AL_LDS, stream, a, m_slot, n_slots, dts, nd, t0, partial);
    else
      hipLaunchKernelGGL(align_moments_kernel<2>, grid, dim3(256), AL_LDS, stream, a, m_slot, n_slots, dts, nd, t0, partial);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const int nv = 1 + 2 * n_slots;
  const long long elems = (long long)(order + 1) * nd * nv, blocks = (elems + 255) / 256;
  hipLaunchKernelGGL(align_reduce_kernel, dim3((unsigned)std::min(blocks, 65536LL)), dim3(256), 0, stream, partial, n_tiles, order + 1, nd, nv, d0,
                     nd_total, out);
  return hipGetLastError();
}

// ---- the cost itself at one (dt, dphi): sum_i w_i sum_c |A_c(t_i + dt) e^{i m_c dphi} - B_ic|^2 and N_b = sum_i w_i sum_c |B_ic|^2,
// both summed directly (non-negative by construction, smooth at a perfect match, where the moment form cancels to +-1e-17).
// A workgroup takes the ALIGN_TILE_ROWS rows of a row tile, thread (row lane, column lane) its rows and columns in order; the 256
// sums of the workgroup are added in thread order, the tiles in tile order (align_reduce_kernel).
__global__ __launch_bounds__(256) void align_residual_kernel(AlignSeries a, const double2* __restrict__ phase, double dt,
                                                             double* __restrict__ partial /* [row tile][2] */) {
  __shared__ double red[256][2];
  const int tid = threadIdx.x, cx = tid & (AL_CW - 1), ry = tid >> 4;
  const long long i0 = (long long)blockIdx.x * AL_TR;
  const int n_r = (int)(a.nw - i0 < AL_TR ? a.nw - i0 : AL_TR);
  double res = 0.0, nb = 0.0;
  for (int r = ry; r < n_r; r += 256 / AL_CW) {
    const long long i = i0 + r;
    const double x = a.tw[i] + dt, w = a.w[i];
    const long long j = align_interval(a.ta, 0, a.na - 1, x);
    const double xj = a.ta[j], h = a.ta[j + 1] - xj, t = x - xj;
    for (int c = cx; c < a.n_cols; c += AL_CW) {
      const long long ca = a.col_a[c];
      const AlignValue V = align_eval<0>(a.Y[j * a.ld_a + ca], a.Y[(j + 1) * a.ld_a + ca], a.S[j * a.ld_a + ca], a.S[(j + 1) * a.ld_a + ca], h, t);
      const double2 b = a.B[i * a.ld_b + a.col_b[c]], p = phase[c];
      const double ex = fma(V.v0.x, p.x, -(V.v0.y * p.y)) - b.x, ey = fma(V.v0.x, p.y, V.v0.y * p.x) - b.y;
      res = fma(w, fma(ex, ex, ey * ey), res);
      nb = fma(w, fma(b.x, b.x, b.y * b.y), nb);
    }
  }
  red[tid][0] = res, red[tid][1] = nb;
  __syncthreads();
  if (tid < 2) {
    double sum = 0.0;
    for (int k = 0; k < 256; ++k) sum += red[k][tid];
    partial[2 * (long long)blockIdx.x + tid] = sum;
  }
}

hipError_t launch_align_residual(hipStream_t stream, const AlignSeries& a, const double* phase, double dt, double* partial, double* out2) {
  if (a.n_cols <= 0 || a.nw <= 0) return hipSuccess;
  const long long n_tiles = align_row_tiles(a.nw);
  if (n_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(align_residual_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, a, reinterpret_cast<const double2*>(phase), dt, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(align_reduce_kernel, dim3(1), dim3(256), 0, stream, partial, n_tiles, 1, 1LL, 2, 0LL, 1LL, out2);
  return hipGetLastError();
}

}  // namespace bms
