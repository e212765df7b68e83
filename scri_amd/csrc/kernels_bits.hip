// Bit transforms of the storage formats (scri/utilities.py:194-406): XOR differencing of a time
// series, the "multi-shuffle" bit transposition and the Fletcher-32 checksum.  Integer / byte work, HBM-bound, bit-exact.
// Behind them the corotating paired-XOR storage form built on the first (scri/SpEC/file_io/corotating_paired_xor.py): conjugate pairs,
// truncation and the XOR in one kernel each way.
#include <cstdint>
#include "kernels.h"

namespace bms {

// ------------------------------------------------------------------------------------------------ xor differencing
// forward (utilities.py:195-217): out[i] = in[i-1] ^ in[i] for i >= 1, out[0] = in[0]; rows of n_cols 64-bit words
__global__ __launch_bounds__(256) void xor_forward_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                          long long n_rows, long long n_cols) {
  const long long total = n_rows * n_cols;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    out[e] = e >= n_cols ? in[e] ^ in[e - n_cols] : in[e];
}

// reverse (utilities.py:220-232): running XOR down the rows.  Three phases over tiles of rows: tile totals, exclusive scan
// of the totals, running XOR inside each tile started from its carry.  Lanes across columns (coalesced 8-byte words).
__global__ __launch_bounds__(256) void xor_reverse_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                          uint64_t* __restrict__ carry, long long n_rows, long long n_cols,
                                                          int tile, int phase) {
  const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= n_cols) return;
  const long long n_tiles = (n_rows + tile - 1) / tile;
  if (phase == 2) {
    if (blockIdx.y != 0) return;
    uint64_t run = 0;
    for (long long t = 0; t < n_tiles; ++t) {
      const uint64_t v = carry[t * n_cols + col];
      carry[t * n_cols + col] = run;
      run ^= v;
    }
    return;
  }
  const long long r0 = (long long)blockIdx.y * tile;
  long long r1 = r0 + tile;
  if (r1 > n_rows) r1 = n_rows;
  uint64_t run = phase == 3 ? carry[blockIdx.y * n_cols + col] : 0;
  for (long long r = r0; r < r1; ++r) {
    run ^= in[r * n_cols + col];
    if (phase == 3) out[r * n_cols + col] = run;
  }
  if (phase == 1) carry[blockIdx.y * n_cols + col] = run;
}

hipError_t launch_xor_timeseries(hipStream_t stream, const void* in, void* out, void* carry, long long n_rows, long long n_cols,
                                 int reverse) {
  if (n_rows <= 0 || n_cols <= 0) return hipSuccess;
  if (!reverse) {
    const long long blocks = (n_rows * n_cols + 255) / 256;
    hipLaunchKernelGGL(xor_forward_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream,
                       (const uint64_t*)in, (uint64_t*)out, n_rows, n_cols);
    return hipGetLastError();
  }
  const int tile = 256;
  const long long n_tiles = (n_rows + tile - 1) / tile;
  const dim3 grid((unsigned)((n_cols + 255) / 256), (unsigned)n_tiles), one((unsigned)((n_cols + 255) / 256), 1);
  for (int phase = 1; phase <= 3; ++phase)
    hipLaunchKernelGGL(xor_reverse_kernel, phase == 2 ? one : grid, dim3(256), 0, stream, (const uint64_t*)in, (uint64_t*)out,
                       (uint64_t*)carry, n_rows, n_cols, tile, phase);
  return hipGetLastError();
}
long long xor_carry_words(long long n_rows, long long n_cols) { return ((n_rows + 255) / 256) * n_cols; }

// ------------------------------------------------------------------------------------------------ multi-shuffle
// The n elements of W bits are cut into pieces (widths listed from the most significant end); the output is the bit
// stream "piece k of element 0, of element 1, ..., of element n-1" for k from the LEAST significant piece upwards
// (utilities.py:271-406).  forward: one thread per output word gathers the W bits of its slot; reverse: one thread per
// element gathers its pieces back.
struct ShufflePieces {
  int n;             // number of pieces
  int width[64];     // piece widths, least significant piece first
  int shift[64];     // bit position of the piece inside an element
  long long off[65];  // first bit of the piece's section in the stream
};

template <typename T>
__global__ __launch_bounds__(256) void multishuffle_kernel(const T* __restrict__ a, T* __restrict__ b, long long n, ShufflePieces S) {
  constexpr int W = 8 * sizeof(T);
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
    long long P = j * W;
    int i = 0;
    while (i + 1 < S.n && S.off[i + 1] <= P) ++i;
    uint64_t val = 0;
    int filled = 0;
    while (filled < W) {
      const int w = S.width[i];
      const long long L = P - S.off[i];
      const long long e = L / w;
      const int r = (int)(L - e * w);
      int k = w - r;
      if (k > W - filled) k = W - filled;
      const uint64_t bits = ((uint64_t)a[e] >> (S.shift[i] + r)) & (k == 64 ? ~0ull : ((1ull << k) - 1));
      val |= bits << filled;
      filled += k;
      P += k;
      if (P == S.off[i + 1]) ++i;
    }
    b[j] = (T)val;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void multiunshuffle_kernel(const T* __restrict__ b, T* __restrict__ a, long long n, ShufflePieces S) {
  constexpr int W = 8 * sizeof(T);
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    uint64_t val = 0;
    for (int i = 0; i < S.n; ++i) {
      const int w = S.width[i];
      const long long P = S.off[i] + e * w;
      const long long word = P / W;
      const int be = (int)(P - word * W);
      const uint64_t mask = w == 64 ? ~0ull : ((1ull << w) - 1);
      uint64_t piece = ((uint64_t)b[word] >> be) & mask;
      if (be + w > W) piece |= ((uint64_t)b[word + 1] << (W - be)) & mask;
      val |= piece << S.shift[i];
    }
    a[e] = (T)val;
  }
}

hipError_t launch_multishuffle(hipStream_t stream, const void* in, void* out, long long n, const int* widths, int n_widths,
                               int bit_width, int forward) {
  if (n <= 0) return hipSuccess;
  if (n_widths < 1 || n_widths > 64) return hipErrorInvalidValue;
  ShufflePieces S;
  S.n = n_widths;
  int shift = 0;
  long long off = 0;
  for (int i = 0; i < n_widths; ++i) {
    const int w = widths[n_widths - 1 - i];  // least significant piece first
    if (w < 1) return hipErrorInvalidValue;
    S.width[i] = w;
    S.shift[i] = shift;
    S.off[i] = off;
    shift += w;
    off += (long long)w * n;
  }
  S.off[n_widths] = off;
  if (shift != bit_width) return hipErrorInvalidValue;
  const long long blocks = (n + 255) / 256;
  const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536)), block(256);
#define MS_GO(T)                                                                                        \
  if (forward)                                                                                          \
    hipLaunchKernelGGL(multishuffle_kernel<T>, grid, block, 0, stream, (const T*)in, (T*)out, n, S);     \
  else                                                                                                  \
    hipLaunchKernelGGL(multiunshuffle_kernel<T>, grid, block, 0, stream, (const T*)in, (T*)out, n, S);
  switch (bit_width) {
    case 8: MS_GO(uint8_t) break;
    case 16: MS_GO(uint16_t) break;
    case 32: MS_GO(uint32_t) break;
    case 64: MS_GO(uint64_t) break;
    default: return hipErrorInvalidValue;
  }
#undef MS_GO
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ Fletcher-32
// c0 = sum d_j mod 65535, c1 = sum (N - j) d_j mod 65535 over the N 16-bit words (utilities.py:235-268 reduces in blocks
// of 360, which leaves the same residues); partial sums in 64-bit accumulators, two atomics per workgroup.
__global__ __launch_bounds__(256) void fletcher32_kernel(const uint16_t* __restrict__ d, long long n, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long s0[256], s1[256];
  unsigned long long c0 = 0, c1 = 0;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
    const unsigned long long v = d[j];
    c0 += v;
    c1 += ((unsigned long long)((n - j) % 65535)) * v;
    if (c1 >= (1ull << 62)) c1 %= 65535;
  }
  s0[threadIdx.x] = c0 % 65535;
  s1[threadIdx.x] = c1 % 65535;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      s0[threadIdx.x] += s0[threadIdx.x + st];
      s1[threadIdx.x] += s1[threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicAdd(&acc[0], s0[0]);
    atomicAdd(&acc[1], s1[0]);
  }
}

hipError_t launch_fletcher32(hipStream_t stream, const void* data, long long n_words, unsigned long long* acc /* [2], zeroed */) {
  if (n_words <= 0) return hipSuccess;
  const long long blocks = (n_words + 256 * 8 - 1) / (256 * 8);
  hipLaunchKernelGGL(fletcher32_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream,
                     (const uint16_t*)data, n_words, acc);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ corotating paired-XOR storage form
// The in-memory core of scri/SpEC/file_io/corotating_paired_xor.py:70-90 (pack) and :240,255 (unpack) on modes already in the
// corotating frame: conjugate pairs -> precision truncation -> -0.0 to +0.0 -> XOR with the previous time step, one kernel each way.
//
// pack: a workgroup is ONE wave and owns PAIRED_PACK_TILE consecutive rows, which it packs in sequence.  A row is staged in LDS once
// (coalesced 16-byte loads), so the partner column (l, -m) is read from there and every input byte comes from HBM once -- apart from
// the one row before the tile, whose packed form the tile recomputes to XOR its first row with.  That halo row runs through exactly
// the statements its owner runs (same loop, same order of the norm's partial sums, same butterfly), so both get the same bits.
// The arithmetic is the reference's, operation for operation: (a + conj b) then times the double 1/sqrt(2) (what numpy's
// complex-by-real division does), the scale 2^e with e = floor(-log2(norm tol / sqrt(n_modes))) read off the exponent field,
// rint (half to even) of x 2^e, times 2^-e (exact, as the reference's division by 2^e is).  No contraction: a fused multiply-add
// rounds once where the reference rounds twice.
// LDS: raw row c16[n_modes] | packed previous row u64[2 n_modes] | partner column i32[n_modes]  = 36 n_modes bytes.
__device__ __forceinline__ double2 paired_value(const double2* __restrict__ row, int j, int p, double r) {
#pragma clang fp contract(off)
  if (p == j) return row[j];  // m = 0
  const double2 a = row[p < j ? j : p], b = row[p < j ? p : j];  // a = f[l, |m|], b = f[l, -|m|]
  double2 v;
  if (p < j) {  // column +m: s = (a + conj b) r
    v.x = (a.x + b.x) * r;
    v.y = (a.y - b.y) * r;
  } else {  // column -m: d = (a - conj b) r
    v.x = (a.x - b.x) * r;
    v.y = (a.y + b.y) * r;
  }
  return v;
}

__device__ __forceinline__ unsigned long long paired_truncated_bits(double x, double scale, double inv) {
#pragma clang fp contract(off)
  const unsigned long long u = (unsigned long long)__double_as_longlong(rint(x * scale) * inv);
  return u == 0x8000000000000000ull ? 0ull : u;  // -0.0 -> +0.0
}

__global__ __launch_bounds__(64) void paired_pack_kernel(const double2* __restrict__ in, long long ld, long long n_out, int halo,
                                                         const int* __restrict__ partner, int n_modes, double tol_per_mode, double r,
                                                         long long row_base, ulonglong2* __restrict__ out,
                                                         unsigned long long* __restrict__ bad) {
#pragma clang fp contract(off)
  extern __shared__ double2 paired_lds[];
  double2* raw = paired_lds;
  ulonglong2* prev = (ulonglong2*)(paired_lds + n_modes);
  int* part = (int*)(paired_lds + 2 * (size_t)n_modes);
  const int lane = threadIdx.x;
  for (int j = lane; j < n_modes; j += 64) part[j] = partner[j];
  const long long r0 = (long long)blockIdx.x * PAIRED_PACK_TILE;
  const long long r1 = r0 + PAIRED_PACK_TILE < n_out ? r0 + PAIRED_PACK_TILE : n_out;
  // output row i is input row i + halo (a piece of a longer series carries the row before it); the series' first row has no previous one
  for (long long i = (r0 + halo > 0) ? r0 - 1 : r0; i < r1; ++i) {
    const bool emit = i >= r0;
    const double2* __restrict__ src = in + (i + halo) * ld;
    __syncthreads();  // (the previous row's readers are done with `raw`; the first pass: `part` is written)
    for (int j = lane; j < n_modes; j += 64) raw[j] = src[j];
    __syncthreads();
    double sum = 0.0;
    for (int j = lane; j < n_modes; j += 64) {
      const double2 v = paired_value(raw, j, part[j], r);
      sum += v.x * v.x + v.y * v.y;
    }
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);  // a + b == b + a: every lane holds the same bits
    const double q = sqrt(sum) * tol_per_mode;
    // rows that cannot be packed: a non-finite value (the sum is inf or nan), zero norm, 2^e or 2^-e outside the normal doubles
    bool ok = isfinite(sum) && q > 0.0;
    int k = 0;
    const double f = frexp(ok ? q : 1.0, &k);         // q = f 2^k, f in [1/2, 1): -log2 q in (-k, 1 - k]
    const int e = f == 0.5 ? 1 - k : -k;              // floor(-log2 q)
    ok = ok && e >= -1022 && e <= 1022;
    const double scale = ldexp(1.0, ok ? e : 0), inv = ldexp(1.0, ok ? -e : 0);
    if (!ok && emit && lane == 0) atomicMin(bad, (unsigned long long)(row_base + i));
    for (int j = lane; j < n_modes; j += 64) {
      const double2 v = paired_value(raw, j, part[j], r);
      ulonglong2 w = make_ulonglong2(0ull, 0ull);  // (a refused row is reported, never packed: zeros keep the rest deterministic)
      if (ok) {
        w.x = paired_truncated_bits(v.x, scale, inv);
        w.y = paired_truncated_bits(v.y, scale, inv);
      }
      if (emit) {
        ulonglong2 x = w;
        if (i + halo > 0) {
          const ulonglong2 pv = prev[j];
          x.x ^= pv.x;
          x.y ^= pv.y;
        }
        out[i * n_modes + j] = x;
      }
      prev[j] = w;  // (column j of `prev` is this lane's alone)
    }
  }
}

size_t paired_pack_lds_bytes(int n_modes) { return (size_t)36 * (size_t)n_modes; }

hipError_t launch_paired_pack(hipStream_t stream, const void* in, long long ld, long long n_out, int halo, const int* partner, int n_modes,
                              double tol_per_mode, long long row_base, void* out, unsigned long long* bad) {
  if (n_out <= 0 || n_modes <= 0) return hipSuccess;
  const size_t lds = paired_pack_lds_bytes(n_modes);
  if (lds > PAIRED_PACK_MAX_LDS) return hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    hipError_t e = allow_dynamic_lds((const void*)paired_pack_kernel);
    if (e != hipSuccess) return e;
  }
  const long long tiles = (n_out + PAIRED_PACK_TILE - 1) / PAIRED_PACK_TILE;
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(paired_pack_kernel, dim3((unsigned)tiles), dim3(64), lds, stream, (const double2*)in, ld, n_out, halo, partner,
                     n_modes, tol_per_mode, 1.0 / sqrt(2.0), row_base, (ulonglong2*)out, bad);
  return hipGetLastError();
}

// unpack: the running XOR down the rows in the three phases of xor_reverse_kernel over tiles of PAIRED_UNPACK_TILE rows -- (1) tile
// totals, (2) exclusive scan of the totals, started from `seed` (the running value a previous piece of the series ended with) and
// leaving the new one there -- and (3) the running XOR inside each tile with the pairs undone on the way out: a lane owns one
// column (l, m >= 0) and carries the running words of s (column +m) and d (column -m) in registers, so
// f[l, m] = (s + d) r and f[l, -m] = conj(s - d) r leave without the un-XORed words ever being stored.
__global__ __launch_bounds__(256) void paired_unpack_scan_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ carry,
                                                                 uint64_t* __restrict__ seed, long long n_rows, long long n_cols, int phase) {
  const long long col = (long long)blockIdx.y * blockDim.x + threadIdx.x;
  if (col >= n_cols) return;
  if (phase == 2) {
    const long long n_tiles = (n_rows + PAIRED_UNPACK_TILE - 1) / PAIRED_UNPACK_TILE;
    uint64_t run = seed[col];
    long long t = 0;
    for (; t + 8 <= n_tiles; t += 8) {  // eight totals in flight: one wave per 64 columns walks every tile, so the loads' latency is its time
      uint64_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = carry[(t + u) * n_cols + col];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        carry[(t + u) * n_cols + col] = run;
        run ^= v[u];
      }
    }
    for (; t < n_tiles; ++t) {
      const uint64_t v = carry[t * n_cols + col];
      carry[t * n_cols + col] = run;
      run ^= v;
    }
    seed[col] = run;
    return;
  }
  const long long r0 = (long long)blockIdx.x * PAIRED_UNPACK_TILE;
  const long long r1 = r0 + PAIRED_UNPACK_TILE < n_rows ? r0 + PAIRED_UNPACK_TILE : n_rows;
  uint64_t run = 0;
  for (long long r = r0; r < r1; ++r) run ^= in[r * n_cols + col];
  carry[blockIdx.x * n_cols + col] = run;
}

__global__ __launch_bounds__(64) void paired_unpack_kernel(const ulonglong2* __restrict__ words, const ulonglong2* __restrict__ carry,
                                                           const int* __restrict__ own, int n_own, const int* __restrict__ partner,
                                                           int n_modes, long long n_rows, double r, double2* __restrict__ out,
                                                           long long ld_out) {
#pragma clang fp contract(off)
  const int k = blockIdx.y * 64 + threadIdx.x;
  if (k >= n_own) return;
  const int j = own[k], p = partner[j];  // j: column (l, m >= 0), p: column (l, -m)
  const long long r0 = (long long)blockIdx.x * PAIRED_UNPACK_TILE;
  const long long r1 = r0 + PAIRED_UNPACK_TILE < n_rows ? r0 + PAIRED_UNPACK_TILE : n_rows;
  ulonglong2 rs = carry[(long long)blockIdx.x * n_modes + j], rd = carry[(long long)blockIdx.x * n_modes + p];
  for (long long row = r0; row < r1; ++row) {
    const ulonglong2 ws = words[row * n_modes + j];
    rs.x ^= ws.x, rs.y ^= ws.y;
    const double2 s = make_double2(__longlong_as_double((long long)rs.x), __longlong_as_double((long long)rs.y));
    if (p == j) {
      out[row * ld_out + j] = s;
      continue;
    }
    const ulonglong2 wd = words[row * n_modes + p];
    rd.x ^= wd.x, rd.y ^= wd.y;
    const double2 d = make_double2(__longlong_as_double((long long)rd.x), __longlong_as_double((long long)rd.y));
    out[row * ld_out + j] = make_double2((s.x + d.x) * r, (s.y + d.y) * r);
    out[row * ld_out + p] = make_double2((s.x - d.x) * r, -((s.y - d.y) * r));
  }
}

long long paired_unpack_carry_words(long long n_rows, int n_modes) {
  return ((n_rows + PAIRED_UNPACK_TILE - 1) / PAIRED_UNPACK_TILE) * 2LL * n_modes;
}

hipError_t launch_paired_unpack(hipStream_t stream, const void* words, long long n_rows, const int* own, int n_own, const int* partner,
                                int n_modes, void* carry, void* seed, void* out, long long ld_out) {
  if (n_rows <= 0 || n_modes <= 0) return hipSuccess;
  const long long n_tiles = (n_rows + PAIRED_UNPACK_TILE - 1) / PAIRED_UNPACK_TILE, n_cols = 2LL * n_modes;
  if (n_tiles > 0x7fffffffLL || (n_cols + 255) / 256 > 65535) return hipErrorInvalidValue;
  const unsigned col_blocks = (unsigned)((n_cols + 255) / 256);
  hipLaunchKernelGGL(paired_unpack_scan_kernel, dim3((unsigned)n_tiles, col_blocks), dim3(256), 0, stream, (const uint64_t*)words,
                     (uint64_t*)carry, (uint64_t*)seed, n_rows, n_cols, 1);
  hipLaunchKernelGGL(paired_unpack_scan_kernel, dim3(1, col_blocks), dim3(256), 0, stream, (const uint64_t*)words, (uint64_t*)carry,
                     (uint64_t*)seed, n_rows, n_cols, 2);
  hipLaunchKernelGGL(paired_unpack_kernel, dim3((unsigned)n_tiles, (unsigned)((n_own + 63) / 64)), dim3(64), 0, stream,
                     (const ulonglong2*)words, (const ulonglong2*)carry, own, n_own, partner, n_modes, n_rows, 1.0 / sqrt(2.0),
                     (double2*)out, ld_out);
  return hipGetLastError();
}

}  // namespace bms
