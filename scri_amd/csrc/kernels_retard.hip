// Retardation of one raw finite-radius series to tortoise time (scri/extrapolation.py:27-45, :356-402; bms_finite_radius_retard):
//   (1) the keep mask of monotonic_indices -- sample k stays iff fl(T[k] + MinTimeStep) < min_{j > k} T[j] -- as a suffix minimum, and
//       its compaction as an exclusive prefix sum of the mask;
//   (2) the retarded time of the kept samples: the cumulative trapezoid of lapse / sqrt(1 - 2E/R) in double-double, rounded once per
//       sample, minus the tortoise coordinate, over the mass;
//   (3) the gather of the kept rows, each times its real factor (R / CoordRadius)^p UnitScaleFactor: the one pass over the modes.
// Every scan is the three-launch form over tiles of RETARD_TILE samples, one thread each: tile totals, a scan of the totals by ONE
// workgroup that walks them in chunks of a tile (any number of tiles), then the scan inside each tile on top of its total.  No
// workgroup waits for another inside a launch.  The number of kept samples exists on the device only until the call's one wait, so
// every grid is sized by n_raw and reads the count from `st`.
#include "dd.h"
#include "kernels.h"

namespace bms {

namespace {

constexpr int RT = RETARD_TILE;

struct MinOp {
  __device__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct SumOp {
  __device__ long long operator()(long long a, long long b) const { return a + b; }
};
struct DdOp {
  __device__ dd operator()(dd a, dd b) const { return dd_add(a, b); }
};

// inclusive scan over the RT threads of a workgroup through sh[RT] (Hillis-Steele): forward, or with REVERSE from the last thread
// down.  On return sh[] holds the scanned values as well (the callers read their neighbour's and the total from it).
template <bool REVERSE, class T, class Op>
__device__ __forceinline__ T tile_scan(T v, T* sh, Op op) {
  const int i = threadIdx.x;
  sh[i] = v;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < RT; off <<= 1) {
    const bool has = REVERSE ? (i + off < RT) : (i >= off);
    const T other = sh[has ? (REVERSE ? i + off : i - off) : i];
    __syncthreads();
    if (has) v = REVERSE ? op(v, other) : op(other, v);
    sh[i] = v;
    __syncthreads();
  }
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- (1) keep mask
__global__ __launch_bounds__(RT) void retard_tile_min_kernel(const double* __restrict__ T, long long n, double* __restrict__ tile_min) {
  __shared__ double sh[RT];
  const long long k = (long long)blockIdx.x * RT + threadIdx.x;
  tile_scan<true>(k < n ? T[k] : INFINITY, sh, MinOp());
  if (threadIdx.x == 0) tile_min[blockIdx.x] = sh[0];
}

// tile_min[t] <- min over the tiles behind t (+inf behind the last), in place; one workgroup, chunks from the end
__global__ __launch_bounds__(RT) void retard_suffix_min_kernel(double* __restrict__ tile_min, long long n_tiles) {
  __shared__ double sh[RT];
  double carry = INFINITY;
  for (long long c0 = (n_tiles - 1) / RT * RT; c0 >= 0; c0 -= RT) {
    const long long t = c0 + threadIdx.x;
    tile_scan<true>(t < n_tiles ? tile_min[t] : INFINITY, sh, MinOp());
    const double behind = threadIdx.x + 1 < RT ? sh[threadIdx.x + 1] : INFINITY;
    if (t < n_tiles) tile_min[t] = fmin(behind, carry);
    carry = fmin(carry, sh[0]);
    __syncthreads();
  }
}

// rank[k] = the number of kept samples of k's tile before k, or -1 for a dropped sample; count[tile] = the kept ones of the tile
__global__ __launch_bounds__(RT) void retard_mask_kernel(const double* __restrict__ T, long long n, double min_step,
                                                         const double* __restrict__ behind_tile, int* __restrict__ rank,
                                                         long long* __restrict__ count) {
#pragma clang fp contract(off)
  __shared__ double sh[RT];
  __shared__ long long shc[RT];
  const int i = threadIdx.x;
  const long long k = (long long)blockIdx.x * RT + i;
  const double tk = k < n ? T[k] : INFINITY;
  tile_scan<true>(tk, sh, MinOp());
  const double later = fmin(i + 1 < RT ? sh[i + 1] : INFINITY, behind_tile[blockIdx.x]);
  const bool keep = k < n && tk + min_step < later;
  const long long incl = tile_scan<false>((long long)keep, shc, SumOp());
  if (k < n) rank[k] = keep ? (int)(incl - 1) : -1;
  if (i == RT - 1) count[blockIdx.x] = incl;
}

// count[t] <- the kept samples of the tiles before t, in place; st = (n_kept, bad radii = 0, first bad sample = none); one workgroup
__global__ __launch_bounds__(RT) void retard_count_scan_kernel(long long* __restrict__ count, long long n_tiles, long long* __restrict__ st) {
  __shared__ long long sh[RT];
  long long carry = 0;
  for (long long c0 = 0; c0 < n_tiles; c0 += RT) {
    const long long t = c0 + threadIdx.x;
    const long long v = t < n_tiles ? count[t] : 0;
    const long long incl = tile_scan<false>(v, sh, SumOp());
    if (t < n_tiles) count[t] = carry + incl - v;
    carry += sh[RT - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) st[0] = carry, st[1] = 0, st[2] = 0x7fffffffffffffffLL;
}

__global__ __launch_bounds__(RT) void retard_compact_kernel(const int* __restrict__ rank, const long long* __restrict__ base, long long n,
                                                            long long* __restrict__ idx) {
  const long long k = (long long)blockIdx.x * RT + threadIdx.x;
  if (k < n && rank[k] >= 0) idx[base[blockIdx.x] + rank[k]] = k;
}

// ---------------------------------------------------------------------------------------------------------------- (2) retarded time
struct RetardSeries {
  const double *T, *R, *lapse;  // raw, f8[n_raw]
  const long long* idx;         // kept sample j is raw sample idx[j]
  double minus_two_e, two_e;    // -2 E and 2 E
};

// the trapezoid that ends at kept sample j, in the operation order of scipy's cumulative_trapezoid on numpy's g; 0 for j = 0 and beyond
__device__ __forceinline__ double retard_term(const RetardSeries& s, long long j, long long nk) {
#pragma clang fp contract(off)
  if (j < 1 || j >= nk) return 0.0;
  const long long k1 = s.idx[j], k0 = s.idx[j - 1];
  const double g1 = s.lapse[k1] / sqrt((s.minus_two_e / s.R[k1]) + 1.0);
  const double g0 = s.lapse[k0] / sqrt((s.minus_two_e / s.R[k0]) + 1.0);
  const double d = s.T[k1] - s.T[k0];
  return (d * (g1 + g0)) / 2.0;
}

__global__ __launch_bounds__(RT) void retard_term_totals_kernel(RetardSeries s, const long long* __restrict__ st, dd* __restrict__ totals) {
  __shared__ dd sh[RT];
  const long long j = (long long)blockIdx.x * RT + threadIdx.x;
  tile_scan<false>(dd_from(retard_term(s, j, st[0])), sh, DdOp());
  if (threadIdx.x == 0) totals[blockIdx.x] = sh[RT - 1];
}

// totals[t] <- the sum of the tiles before t, in place; one workgroup
__global__ __launch_bounds__(RT) void retard_term_scan_kernel(dd* __restrict__ totals, long long n_tiles) {
  __shared__ dd sh[RT];
  dd carry = {0.0, 0.0};
  for (long long c0 = 0; c0 < n_tiles; c0 += RT) {
    const long long t = c0 + threadIdx.x;
    tile_scan<false>(t < n_tiles ? totals[t] : dd_from(0.0), sh, DdOp());
    if (t < n_tiles) totals[t] = threadIdx.x ? dd_add(carry, sh[threadIdx.x - 1]) : carry;
    carry = dd_add(carry, sh[RT - 1]);
    __syncthreads();
  }
}

// t_out[j] = (T[0] + sum - (R + 2E log(R / 2E - 1))) / ChMass, radii_out[j] = R / ChMass, factor[j] = fl(fl((R / CoordRadius)^p) unit);
// a kept radius that is not finite or not beyond 2E is counted in st[1] and the first one named in st[2] (by its raw index)
__global__ __launch_bounds__(RT) void retard_time_kernel(RetardSeries s, long long* __restrict__ st, const dd* __restrict__ before,
                                                         double coord_radius, double ch_mass, double unit, int p, double* __restrict__ t_out,
                                                         double* __restrict__ radii_out, double* __restrict__ factor) {
#pragma clang fp contract(off)
  __shared__ dd sh[RT];
  const long long nk = st[0];
  const long long j = (long long)blockIdx.x * RT + threadIdx.x;
  const dd in_tile = tile_scan<false>(dd_from(retard_term(s, j, nk)), sh, DdOp());
  if (j >= nk) return;
  const dd sum = dd_add(before[blockIdx.x], in_tile);
  const long long k = s.idx[j];
  const double R = s.R[k];
  const double t = j ? (sum.hi + sum.lo) + s.T[s.idx[0]] : s.T[k];
  const double r_star = R + s.two_e * log((R / s.two_e) - 1.0);
  t_out[j] = (t - r_star) / ch_mass;
  radii_out[j] = R / ch_mass;
  const double ratio = R / coord_radius;
  double pw = ratio;
  for (int q = 1; q < p; ++q) pw = pw * ratio;
  factor[j] = pw * unit;
  if (!(isfinite(R) && R > s.two_e)) {
    atomicAdd((unsigned long long*)&st[1], 1ULL);
    atomicMin((unsigned long long*)&st[2], (unsigned long long)k);
  }
}

// ---------------------------------------------------------------------------------------------------------------- (3) gather and scale
// out[r][m] = in[idx[r]][m] * factor[r] (both components; factor == nullptr: the plain gather), r < n_kept: a workgroup takes
// rows_per_block consecutive output rows and walks their elements in order, so that loads run along the modes of a source row and
// stores along the output
__global__ __launch_bounds__(256) void retard_gather_kernel(const double2* __restrict__ in, long long ld, int n_cols,
                                                            const long long* __restrict__ idx, const double* __restrict__ factor,
                                                            const long long* __restrict__ st, int rows_per_block, double2* __restrict__ out,
                                                            long long ld_out) {
#pragma clang fp contract(off)
  const long long nk = st[0];
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  if (r0 >= nk) return;
  const int rows = nk - r0 < rows_per_block ? (int)(nk - r0) : rows_per_block;
  const unsigned total = (unsigned)rows * (unsigned)n_cols;  // (rows_per_block n_cols <= max(4096, n_cols) <= 2^26)
#pragma unroll 4
  for (unsigned e = threadIdx.x; e < total; e += 256) {
    const unsigned r = e / (unsigned)n_cols, m = e - r * (unsigned)n_cols;
    const long long row = r0 + r;
    double2 v = in[idx[row] * ld + m];
    if (factor) {
      const double f = factor[row];
      v.x = v.x * f, v.y = v.y * f;
    }
    out[row * ld_out + m] = v;
  }
}

}  // namespace

long long retard_tiles(long long n_raw) { return (n_raw + RT - 1) / RT; }

hipError_t launch_retard_keep(hipStream_t stream, const double* T, long long n_raw, double min_step, double* tile_min, int* rank,
                              long long* count, long long* idx, long long* st) {
  const long long n_tiles = retard_tiles(n_raw);
  if (n_raw < 1 || n_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)n_tiles), block(RT);
  hipLaunchKernelGGL(retard_tile_min_kernel, grid, block, 0, stream, T, n_raw, tile_min);
  hipLaunchKernelGGL(retard_suffix_min_kernel, dim3(1), block, 0, stream, tile_min, n_tiles);
  hipLaunchKernelGGL(retard_mask_kernel, grid, block, 0, stream, T, n_raw, min_step, (const double*)tile_min, rank, count);
  hipLaunchKernelGGL(retard_count_scan_kernel, dim3(1), block, 0, stream, count, n_tiles, st);
  hipLaunchKernelGGL(retard_compact_kernel, grid, block, 0, stream, (const int*)rank, (const long long*)count, n_raw, idx);
  return hipGetLastError();
}

hipError_t launch_retard_time(hipStream_t stream, const double* T, const double* R, const double* lapse, long long n_raw, const long long* idx,
                              long long* st, double initial_adm_energy, double coord_radius, double ch_mass, double unit, int p, void* totals,
                              double* t_out, double* radii_out, double* factor) {
  const long long n_tiles = retard_tiles(n_raw);
  if (n_raw < 1 || n_tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const RetardSeries s{T, R, lapse, idx, -2.0 * initial_adm_energy, 2.0 * initial_adm_energy};
  const dim3 grid((unsigned)n_tiles), block(RT);
  hipLaunchKernelGGL(retard_term_totals_kernel, grid, block, 0, stream, s, (const long long*)st, (dd*)totals);
  hipLaunchKernelGGL(retard_term_scan_kernel, dim3(1), block, 0, stream, (dd*)totals, n_tiles);
  hipLaunchKernelGGL(retard_time_kernel, grid, block, 0, stream, s, st, (const dd*)totals, coord_radius, ch_mass, unit, p, t_out, radii_out,
                     factor);
  return hipGetLastError();
}

hipError_t launch_retard_gather(hipStream_t stream, const void* in, long long ld, int n_cols, long long n_raw, const long long* idx,
                                const double* factor, const long long* st, void* out, long long ld_out) {
  if (n_raw < 1 || n_cols < 1) return hipErrorInvalidValue;
  const int rows_per_block = n_cols >= 4096 ? 1 : 4096 / n_cols;  // about sixteen elements of 16 bytes per thread
  const long long blocks = (n_raw + rows_per_block - 1) / rows_per_block;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(retard_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const double2*)in, ld, n_cols, idx, factor, st,
                     rows_per_block, (double2*)out, ld_out);
  return hipGetLastError();
}

}  // namespace bms
