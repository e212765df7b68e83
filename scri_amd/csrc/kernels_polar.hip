// Polar form of a series of complex numbers (scri/waveform_base.py:520-533: abs, arg, arg_unwrapped) and the count of its non-finite
// elements (the "data must be finite" check of waveform_base.py:299-367).  Input c16[n_rows][ld], the first n_cols columns of a row used.
//
//   abs = hypot(re, im)   (no spurious overflow or underflow; |inf + nan i| = inf)
//   arg = atan2(im, re)   (IEEE special cases: arg(+0 + 0i) = 0, arg(-1 + 0i) = pi, arg(-1 - 0i) = -pi, a NaN part gives NaN)
//
// Unwrapped angle down the rows, np.unwrap(np.angle(data), axis=0) restated so that it scans exactly:
//   p[i][j] = arg, d = p[i][j] - p[i-1][j],  k[i][j] = -1 if d > pi, +1 if d < -pi, else 0 (pi the double; k[0][j] = 0),
//   K[i][j] = sum_{i' <= i} k[i'][j]  (an INTEGER sum: associative, any order),   out[i][j] = p[i][j] + 2 pi K[i][j]  (one rounding),
//   and out[i][j] = NaN once any p[i'][j], i' <= i, is NaN (numpy's cumsum poisons the same way); infinite parts give finite angles.
// Three phases over tiles of POLAR_TILE_ROWS rows, lanes along the columns (16-byte loads, 8-byte stores, both coalesced), as the
// running XOR of kernels_bits.hip: (1) the wrapped angle (and abs) of every element is stored, with the tile's (sum k, poison) per
// column; (2) exclusive scan of those per column; (3) 2 pi K is added in place.  The first row of a tile needs the angle of the row
// before it: both phases recompute it from the input with the same device function -- the stored one may already hold its unwrapped
// value -- so the tile and its neighbour see the same bits.  atan2 runs once per element (plus one row per tile, twice).
#include <cstdint>
#include "kernels.h"

namespace bms {

constexpr double POLAR_PI = 3.141592653589793, POLAR_TWO_PI = 6.283185307179586;

__device__ __forceinline__ double polar_abs(double2 z) { return hypot(z.x, z.y); }
__device__ __forceinline__ double polar_arg(double2 z) { return atan2(z.y, z.x); }
// the wrap count of one step (a NaN on either side: 0 -- the poison flag carries it)
__device__ __forceinline__ long long polar_step(double p, double prev) {
  const double d = p - prev;
  return d > POLAR_PI ? -1 : (d < -POLAR_PI ? 1 : 0);
}

// pointwise: (row, column) flattened over the lanes, so a wave is full whatever n_cols is and consecutive lanes read consecutive
// columns (a row's end continues with the next row's start)
__global__ __launch_bounds__(256) void polar_pointwise_kernel(const double2* __restrict__ in, long long ld, long long n_rows, int n_cols,
                                                              double* __restrict__ abs_out, double* __restrict__ arg_out, long long ld_out) {
  const long long total = n_rows * n_cols;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / n_cols;
    const long long c = e - r * n_cols;
    const double2 z = in[r * ld + c];
    if (abs_out) abs_out[r * ld_out + c] = polar_abs(z);
    if (arg_out) arg_out[r * ld_out + c] = polar_arg(z);
  }
}

// phase 1: wrapped angles (and abs) of a tile, and its totals carry[tile][col] = (sum of k over the tile's rows, any NaN angle in them)
__global__ __launch_bounds__(64) void polar_tile_kernel(const double2* __restrict__ in, long long ld, long long n_rows, int n_cols,
                                                        double* __restrict__ abs_out, double* __restrict__ arg_out, long long ld_out,
                                                        longlong2* __restrict__ carry) {
  const long long col = (long long)blockIdx.y * 64 + threadIdx.x;
  if (col >= n_cols) return;
  const long long r0 = (long long)blockIdx.x * POLAR_TILE_ROWS;
  const long long r1 = r0 + POLAR_TILE_ROWS < n_rows ? r0 + POLAR_TILE_ROWS : n_rows;
  double prev = r0 > 0 ? polar_arg(in[(r0 - 1) * ld + col]) : 0.0;
  long long sum = 0, poison = 0;
  for (long long r = r0; r < r1; ++r) {
    const double2 z = in[r * ld + col];
    const double p = polar_arg(z);
    arg_out[r * ld_out + col] = p;
    if (abs_out) abs_out[r * ld_out + col] = polar_abs(z);
    if (r > 0) sum += polar_step(p, prev);
    poison |= (long long)(p != p);
    prev = p;
  }
  carry[(long long)blockIdx.x * n_cols + col] = make_longlong2(sum, poison);
}

// phase 2: exclusive scan of the tile totals down each column
__global__ __launch_bounds__(64) void polar_scan_kernel(longlong2* __restrict__ carry, long long n_tiles, int n_cols) {
  const long long col = (long long)blockIdx.x * 64 + threadIdx.x;
  if (col >= n_cols) return;
  longlong2 run = make_longlong2(0, 0);
  long long t = 0;
  for (; t + 8 <= n_tiles; t += 8) {  // eight totals in flight: one wave per 64 columns walks every tile, so the loads' latency is its time
    longlong2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = carry[(t + u) * n_cols + col];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      carry[(t + u) * n_cols + col] = run;
      run.x += v[u].x;
      run.y |= v[u].y;
    }
  }
  for (; t < n_tiles; ++t) {
    const longlong2 v = carry[t * n_cols + col];
    carry[t * n_cols + col] = run;
    run.x += v.x;
    run.y |= v.y;
  }
}

// phase 3: the running count inside each tile, started from its carry; an element changes only where K != 0 or the column is poisoned
__global__ __launch_bounds__(64) void polar_unwrap_kernel(const double2* __restrict__ in, long long ld, long long n_rows, int n_cols,
                                                          const longlong2* __restrict__ carry, double* __restrict__ arg_out, long long ld_out) {
  const long long col = (long long)blockIdx.y * 64 + threadIdx.x;
  if (col >= n_cols) return;
  const long long r0 = (long long)blockIdx.x * POLAR_TILE_ROWS;
  const long long r1 = r0 + POLAR_TILE_ROWS < n_rows ? r0 + POLAR_TILE_ROWS : n_rows;
  longlong2 run = carry[(long long)blockIdx.x * n_cols + col];
  double prev = r0 > 0 ? polar_arg(in[(r0 - 1) * ld + col]) : 0.0;
  for (long long r = r0; r < r1; ++r) {
    const double p = arg_out[r * ld_out + col];
    if (r > 0) run.x += polar_step(p, prev);
    run.y |= (long long)(p != p);
    prev = p;
    if (run.y)
      arg_out[r * ld_out + col] = __builtin_nan("");
    else if (run.x != 0)
      arg_out[r * ld_out + col] = fma((double)run.x, POLAR_TWO_PI, p);  // K 2pi is exact inside the fma: one rounding
  }
}

long long polar_carry_words(long long n_rows, int n_cols) {
  return ((n_rows + POLAR_TILE_ROWS - 1) / POLAR_TILE_ROWS) * 2LL * n_cols;
}

hipError_t launch_polar(hipStream_t stream, const void* in, long long ld, long long n_rows, int n_cols, int unwrap, double* abs_out,
                        double* arg_out, long long ld_out, void* carry) {
  if (n_rows <= 0 || n_cols <= 0) return hipSuccess;
  if (!abs_out && !arg_out) return hipErrorInvalidValue;
  if (n_rows > (1LL << 62) / n_cols) return hipErrorInvalidValue;
  if (!unwrap || !arg_out) {
    const long long blocks = (n_rows * n_cols + 255) / 256;
    hipLaunchKernelGGL(polar_pointwise_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, (const double2*)in,
                       ld, n_rows, n_cols, abs_out, arg_out, ld_out);
    return hipGetLastError();
  }
  const long long n_tiles = (n_rows + POLAR_TILE_ROWS - 1) / POLAR_TILE_ROWS;
  const unsigned col_blocks = (unsigned)((n_cols + 63) / 64);
  if (n_tiles > 0x7fffffffLL || col_blocks > 65535u || !carry) return hipErrorInvalidValue;
  hipLaunchKernelGGL(polar_tile_kernel, dim3((unsigned)n_tiles, col_blocks), dim3(64), 0, stream, (const double2*)in, ld, n_rows, n_cols,
                     abs_out, arg_out, ld_out, (longlong2*)carry);
  hipLaunchKernelGGL(polar_scan_kernel, dim3(col_blocks), dim3(64), 0, stream, (longlong2*)carry, n_tiles, n_cols);
  hipLaunchKernelGGL(polar_unwrap_kernel, dim3((unsigned)n_tiles, col_blocks), dim3(64), 0, stream, (const double2*)in, ld, n_rows, n_cols,
                     (const longlong2*)carry, arg_out, ld_out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ non-finite elements
// acc[0] += the elements with a non-finite real or imaginary part, acc[1] = min(acc[1], the first row that holds one): integer
// reductions, so the order the workgroups arrive in does not matter.  Two atomics per workgroup that found one.
__global__ __launch_bounds__(256) void polar_count_kernel(const double2* __restrict__ in, long long ld, long long n_rows, int n_cols,
                                                          unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long s_n[256], s_r[256];
  const long long total = n_rows * n_cols;
  unsigned long long n = 0, first = ~0ull;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long r = e / n_cols;
    const double2 z = in[r * ld + (e - r * n_cols)];
    if (!(isfinite(z.x) && isfinite(z.y))) {
      ++n;
      if ((unsigned long long)r < first) first = (unsigned long long)r;
    }
  }
  s_n[threadIdx.x] = n;
  s_r[threadIdx.x] = first;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      s_n[threadIdx.x] += s_n[threadIdx.x + st];
      if (s_r[threadIdx.x + st] < s_r[threadIdx.x]) s_r[threadIdx.x] = s_r[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && s_n[0]) {
    atomicAdd(&acc[0], s_n[0]);
    atomicMin(&acc[1], s_r[0]);
  }
}

hipError_t launch_count_nonfinite(hipStream_t stream, const void* in, long long ld, long long n_rows, int n_cols,
                                  unsigned long long* acc /* [2] = (0, all ones) */) {
  if (n_rows <= 0 || n_cols <= 0) return hipSuccess;
  if (n_rows > (1LL << 62) / n_cols) return hipErrorInvalidValue;
  const long long blocks = (n_rows * n_cols + 255) / 256;
  hipLaunchKernelGGL(polar_count_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, (const double2*)in, ld, n_rows,
                     n_cols, acc);
  return hipGetLastError();
}

}  // namespace bms
