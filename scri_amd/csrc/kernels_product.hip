// The product of two spin-weighted functions given by their modes, truncated at ell_out, on Gauss-Legendre rows: no phi grid, and
// n = floor((l_a + l_b + l_out) / 2) + 1 theta rows where the grid route takes (2 (l_a + l_b) + 1)^2 pixels.
//
// With f(theta, phi) = sum_m F_m(theta) e^{i m phi}, F_m(theta_j) = sum_l f_lm lambda^s_lm(theta_j), lambda^s_lm(theta) = sYlm(theta, 0) (real):
//     1. theta sums   A_m(theta_j), B_m(theta_j) of both operands                                  l ascending from max(|m|, |s|)
//     2. convolution  G_M(theta_j) = sum_m1 A_m1(theta_j) B_{M - m1}(theta_j)   (exact: no aliasing)  m1 ascending
//     3. quadrature   (a b)_{l M} = sum_j [2 pi w_j lambda^S_lM(theta_j)] G_M(theta_j),  S = s_a + s_b    j ascending
// The integrand of 3. is a polynomial of degree <= l_a + l_b + l_out in cos(theta), so the n nodes give the truncated product exactly.  The
// tables lambda^s (engine_product.hip: long double, rounded once; 2 pi w_j folded into the output spin's) are [n][(l + 1)^2] doubles read
// through L2.  bar(x)_lm = (-1)^(s + m) conj(x_{l, -m}) is applied as a row is loaded.
//
// Geometry: ONE workgroup of four waves per time step, persistent over the steps blockIdx.x, blockIdx.x + gridDim.x, ...  Everything between
// the input rows and the output row lives in LDS: the two rows, the panels A [n][2 l_a + 1], B [n][2 l_b + 1], G [n][2 l_out + 1] and the
// output row.  Each sum is owned by one thread and taken in the order stated above, every multiply-add spelled out with contraction off, so
// an output depends on nothing but its own rows: not on the steps around it, the number of workgroups, the row strides, or which outputs were
// asked for.
//
// SUPER: the operands are sigma (spin 2) and bar(sigma_dot) (spin -2), and the epilogue adds psi2 and the diagonal terms as the row is stored:
//     Psi_BS = psi2 + sigma sigma-bar-dot,  Psi_M = Psi_BS + eth^2 sigma-bar,  Psi_G = Psi_BS + (eth^2 sigma-bar - ethbar^2 sigma) / 2,
//     Psi_GW = Psi_BS - ethbar^2 sigma,  M = -(Psi_BS + bar Psi_BS) / 2
// with eth^2 sigma-bar = f_l bar(sigma), ethbar^2 sigma = f_l sigma, f_l = sqrt((l + 2)(l + 1) l (l - 1)) / 2 (GHP); INTEGRATED stores
// -bar(Psi) / (2 sqrt(pi)) for the four Psi.
#include "wigner.h"
#include "kernels.h"

namespace bms {

namespace {

constexpr int PRODUCT_THREADS = 256;

__device__ __forceinline__ int ell_of_column(int i) {
  int l = (int)sqrtf((float)i);
  while ((l + 1) * (l + 1) <= i) ++l;
  while (l * l > i) --l;
  return l;
}

// the row x c16[(l_max + 1)^2] of one step into LDS; conj: bar of a row of stored spin `spin`
__device__ __forceinline__ void load_row(double2* dst, const double* __restrict__ x, int n_cols, int spin, int conj) {
  for (int i = threadIdx.x; i < n_cols; i += PRODUCT_THREADS) {
    if (!conj) {
      dst[i] = *reinterpret_cast<const double2*>(x + 2 * (long long)i);
    } else {
      const int l = ell_of_column(i), m = i - l * (l + 1);
      const double2 v = *reinterpret_cast<const double2*>(x + 2 * (long long)(l * (l + 1) - m));
      dst[i] = ((spin + m) & 1) ? double2{-v.x, v.y} : double2{v.x, -v.y};
    }
  }
}

// panel[j][m + l_max] = sum_l row[(l, m)] tab[j][(l, m)], l = max(|m|, |spin|) .. l_max ascending
__device__ __forceinline__ void theta_sums(double2* panel, const double2* row, const double* __restrict__ tab, int l_max, int spin, int n_nodes) {
  const int width = 2 * l_max + 1, n_cols = (l_max + 1) * (l_max + 1), s_abs = spin < 0 ? -spin : spin;
  for (int idx = threadIdx.x; idx < n_nodes * width; idx += PRODUCT_THREADS) {
    const int j = idx / width, m = idx - j * width - l_max, m_abs = m < 0 ? -m : m;
    const double* t = tab + (long long)j * n_cols;
    double re = 0.0, im = 0.0;
    for (int l = m_abs > s_abs ? m_abs : s_abs; l <= l_max; ++l) {
      const int c = l * (l + 1) + m;
      const double2 f = row[c];
      const double lam = t[c];
      re = fma(f.x, lam, re);
      im = fma(f.y, lam, im);
    }
    panel[idx] = double2{re, im};
  }
}

// pan_g[j][M + l_out] = sum_m1 A[j][m1] B[j][M - m1], m1 = max(-l_a, M - l_b) .. min(l_a, M + l_b) ascending
__device__ __forceinline__ void convolution(double2* pan_g, const double2* pan_a, int l_a, const double2* pan_b, int l_b, int l_out, int n_nodes) {
  const int wa = 2 * l_a + 1, wb = 2 * l_b + 1, wo = 2 * l_out + 1;
  for (int idx = threadIdx.x; idx < n_nodes * wo; idx += PRODUCT_THREADS) {
    const int j = idx / wo, M = idx - j * wo - l_out;
    const double2* A = pan_a + j * wa + l_a;
    const double2* B = pan_b + j * wb + l_b;
    const int lo = -l_a > M - l_b ? -l_a : M - l_b, hi = l_a < M + l_b ? l_a : M + l_b;
    double re = 0.0, im = 0.0;
    for (int m1 = lo; m1 <= hi; ++m1) {
      const double2 x = A[m1], y = B[M - m1];
      re = fma(x.x, y.x, re);
      re = fma(-x.y, y.y, re);
      im = fma(x.x, y.y, im);
      im = fma(x.y, y.x, im);
    }
    pan_g[idx] = double2{re, im};
  }
}

// column c = (l, M) of the product: sum_j tab_out[j][c] pan_g[j][M + l_out], j ascending; an exact zero below l = |S|
__device__ __forceinline__ double2 quadrature(const double2* pan_g, const double* __restrict__ tab_out, int c, int l, int l_out, int S_abs, int n_nodes) {
  const int M = c - l * (l + 1), no = (l_out + 1) * (l_out + 1), wo = 2 * l_out + 1;
  double re = 0.0, im = 0.0;
  if (l >= S_abs)
    for (int j = 0; j < n_nodes; ++j) {
      const double w = tab_out[(long long)j * no + c];
      const double2 g = pan_g[j * wo + M + l_out];
      re = fma(w, g.x, re);
      im = fma(w, g.y, im);
    }
  return double2{re, im};
}

struct ProductOperands {
  const double *a, *b;    // rows c16[n_times][ld]
  long long ld_a, ld_b;
  int spin_a, spin_b;     // of the stored rows
  int conj_a, conj_b;
  int l_a, l_b, l_out, n_nodes;
  const double *tab_a, *tab_b, *tab_out;  // of the effective spins; tab_out with 2 pi w folded
};

struct SuperOutputs {
  const double* psi2;
  long long ld_psi2, ld_out;
  double *bs, *m, *g, *gw, *mass;
};

template <bool SUPER, bool INTEGRATED>
__global__ __launch_bounds__(PRODUCT_THREADS) void product_kernel(ProductOperands P, long long n_times, double* __restrict__ out, long long ld_out,
                                                                   SuperOutputs Q) {
#pragma clang fp contract(off)
  extern __shared__ double2 product_lds[];
  // (SUPER: the operands are sigma and bar(sigma_dot), both of ell_max = l_a: their fields of P are not read)
  const int l_a = P.l_a, l_b = SUPER ? P.l_a : P.l_b, l_out = P.l_out, n = P.n_nodes;
  const int spin_a = SUPER ? 2 : P.spin_a, spin_b = SUPER ? 2 : P.spin_b, conj_a = SUPER ? 0 : P.conj_a, conj_b = SUPER ? 1 : P.conj_b;
  const int na = (l_a + 1) * (l_a + 1), nb = (l_b + 1) * (l_b + 1), no = (l_out + 1) * (l_out + 1);
  const int wa = 2 * l_a + 1, wb = 2 * l_b + 1;
  double2* row_a = product_lds;
  double2* row_b = row_a + na;
  double2* row_o = row_b + nb;
  double2* pan_a = row_o + no;
  double2* pan_b = pan_a + n * wa;
  double2* pan_g = pan_b + n * wb;
  const int s_a = conj_a ? -spin_a : spin_a, s_b = conj_b ? -spin_b : spin_b, S = s_a + s_b, S_abs = S < 0 ? -S : S;
  for (long long step = blockIdx.x; step < n_times; step += gridDim.x) {  // (uniform in the workgroup: every wave takes every barrier)
    load_row(row_a, P.a + 2 * step * P.ld_a, na, spin_a, conj_a);
    load_row(row_b, P.b + 2 * step * P.ld_b, nb, spin_b, conj_b);
    __syncthreads();
    theta_sums(pan_a, row_a, P.tab_a, l_a, s_a, n);
    theta_sums(pan_b, row_b, P.tab_b, l_b, s_b, n);
    __syncthreads();
    convolution(pan_g, pan_a, l_a, pan_b, l_b, l_out, n);
    __syncthreads();
    for (int c = threadIdx.x; c < no; c += PRODUCT_THREADS) {
      const double2 p = quadrature(pan_g, P.tab_out, c, ell_of_column(c), l_out, S_abs, n);
      if (SUPER)
        row_o[c] = p;
      else
        *reinterpret_cast<double2*>(out + 2 * (step * ld_out + c)) = p;
    }
    if (SUPER) {
      __syncthreads();
      const double* p2 = Q.psi2 + 2 * step * Q.ld_psi2;
      const double root_pi = 0x1.c5bf891b4ef6ap+0;  // sqrt of the double pi, as numpy forms it (the reference divides by np.sqrt(np.pi))
      // every Psi at a column is one chain of operations on that column's entries, whichever thread and whichever call forms it
      auto bondi_sachs = [&](int col) -> double2 {
        const double2 q = *reinterpret_cast<const double2*>(p2 + 2 * col), p = row_o[col];
        return double2{q.x + p.x, q.y + p.y};
      };
      for (int c = threadIdx.x; c < no; c += PRODUCT_THREADS) {
        const int l = ell_of_column(c), M = c - l * (l + 1), cm = l * (l + 1) - M;
        const bool odd = M & 1;  // (-1)^M of bar at (l, M) and at (l, -M)
        const double2 bs_c = bondi_sachs(c), bs_m = bondi_sachs(cm);
        // the supermomenta at src = (l, M), or at (l, -M) where the stored value is -bar(Psi) / (2 sqrt(pi))
        const int src = INTEGRATED ? cm : c, mirror = INTEGRATED ? c : cm;
        const double2 bs = INTEGRATED ? bs_m : bs_c;
        double2 e2 = double2{0.0, 0.0}, eb2 = double2{0.0, 0.0};
        if (l >= 2) {
          const double f = sqrt((double)((long long)(l + 2) * (l + 1) * l * (l - 1))) * 0.5;
          const double2 sm = row_a[mirror], sg = row_a[src];
          const double2 sbar = odd ? double2{-sm.x, sm.y} : double2{sm.x, -sm.y};  // bar(sigma) at src = (-1)^M conj(sigma at its mirror)
          e2 = double2{f * sbar.x, f * sbar.y}, eb2 = double2{f * sg.x, f * sg.y};
        }
        const long long at = 2 * (step * Q.ld_out + c);
        auto store = [&](double* dst, double2 v) {
          if (INTEGRATED) {
            const double2 vb = odd ? double2{-v.x, v.y} : double2{v.x, -v.y};
            v = double2{-0.5 * vb.x / root_pi, -0.5 * vb.y / root_pi};
          }
          *reinterpret_cast<double2*>(dst + at) = v;
        };
        if (Q.bs) store(Q.bs, bs);
        if (Q.m) store(Q.m, l >= 2 ? double2{bs.x + e2.x, bs.y + e2.y} : bs);
        if (Q.g) store(Q.g, l >= 2 ? double2{bs.x + 0.5 * (e2.x - eb2.x), bs.y + 0.5 * (e2.y - eb2.y)} : bs);
        if (Q.gw) store(Q.gw, l >= 2 ? double2{bs.x - eb2.x, bs.y - eb2.y} : bs);
        if (Q.mass) {
          const double2 wb = odd ? double2{-bs_m.x, bs_m.y} : double2{bs_m.x, -bs_m.y};
          *reinterpret_cast<double2*>(Q.mass + at) = double2{-0.5 * (bs_c.x + wb.x), -0.5 * (bs_c.y + wb.y)};
        }
      }
    }
    __syncthreads();  // (the rows and panels of this step are read until here)
  }
}

// the factor of the GHP eth on a row of spin s: sqrt((l - s)(l + s + 1)) / sqrt(2), zero where l is below |s| or |s + 1|
__device__ __forceinline__ double eth_ghp_factor(int l, int s) {
  const int s_abs = s < 0 ? -s : s, up_abs = s + 1 < 0 ? -(s + 1) : s + 1;
  if (l < s_abs || l < up_abs) return 0.0;
  return sqrt((double)((l - s) * (l + s + 1))) / 0x1.6a09e667f3bcdp+0;  // (the double sqrt(2), as the host's factor tables divide by it)
}

__device__ __forceinline__ double2 bar_of(double2 x, int spin_plus_m) { return (spin_plus_m & 1) ? double2{-x.x, x.y} : double2{x.x, -x.y}; }

// The six Bondi-gauge violations of one time step and their norms (scri/asymptotic_bondi_data/constraints.py):
//     v0 = psi0' - eth psi1 - 3 sigma psi2     v1 = psi1' - eth psi2 - 2 sigma psi3     v2 = psi2' - eth psi3 - sigma psi4
//     v3 = psi3 + eth bar(sigma')              v4 = psi4 + bar(sigma'')                 v5 = Im[psi2 + eth^2 bar(sigma) + sigma bar(sigma')]
// with the GHP eth, the primes given as rows, Im(x) = -i (x - bar x) / 2.  The four products share sigma: its row and its theta sums are
// taken once, then each second operand (psi2, psi3, psi4, bar(sigma'): spins 0, -1, -2, -2) goes through the stages of product_kernel on the
// same two panels.  v0, v1, v2 finish column by column out of the quadrature; sigma bar(sigma') stays in LDS for its mirror column.  The
// diagonal terms are read from memory as stored.  LDS: the rows and panels of product_kernel at (l, l, l), nothing more.
// Norms: thread t adds |v_k[c]|^2 = re re + im im over its columns c = t, t + 256, ... ascending; the 256 partials of each k are added in
// LDS (rows and panels are free by then) in the tree stride = 128, 64, ... 1, red[t] += red[t + stride]; thread 0 takes the root.
// A product is formed only if an output asked for needs it, and no output depends on which others are asked for.
__global__ __launch_bounds__(PRODUCT_THREADS) void constraint_kernel(ConstraintArgs Q, long long n_times) {
#pragma clang fp contract(off)
  extern __shared__ double2 product_lds[];
  const int l_max = Q.l_max, n = Q.n_nodes, nc = (l_max + 1) * (l_max + 1), width = 2 * l_max + 1;
  double2* row_s = product_lds;  // sigma
  double2* row_b = row_s + nc;   // the second operand of the product at hand
  double2* row_o = row_b + nc;   // sigma bar(sigma')
  double2* pan_s = row_o + nc;
  double2* pan_b = pan_s + n * width;
  double2* pan_g = pan_b + n * width;
  double* red = reinterpret_cast<double*>(product_lds);  // [6][PRODUCT_THREADS], once the step's rows and panels are done with
  const bool norms = Q.norms != nullptr;
  // bit p: the product of sigma with psi2, psi3, psi4, bar(sigma') is needed (by v0, v1, v2, v5)
  const int need = norms ? 15 : (Q.v[0] ? 1 : 0) | (Q.v[1] ? 2 : 0) | (Q.v[2] ? 4 : 0) | (Q.v[5] ? 8 : 0);
  for (long long step = blockIdx.x; step < n_times; step += gridDim.x) {  // (uniform in the workgroup: every wave takes every barrier)
    auto at = [&](int which, int col) { return *reinterpret_cast<const double2*>(Q.in[which] + 2 * (step * Q.ld[which] + col)); };
    auto put = [&](double* dst, int col, double2 v) {
      if (dst) *reinterpret_cast<double2*>(dst + 2 * (step * Q.ld_out + col)) = v;
      const double sq = v.x * v.x;
      return sq + v.y * v.y;
    };
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0, n4 = 0.0, n5 = 0.0;
    if (need) {
      load_row(row_s, Q.in[CONSTRAINT_SIGMA] + 2 * step * Q.ld[CONSTRAINT_SIGMA], nc, 2, 0);
      __syncthreads();
      theta_sums(pan_s, row_s, Q.tab_sigma, l_max, 2, n);
    }
#pragma unroll 1
    for (int p = 0; p < 4; ++p) {  // sigma times psi2, psi3, psi4, bar(sigma')
      if (!((need >> p) & 1)) continue;
      const int t = p < 3 ? p : 2, operand = p < 3 ? p + 2 : CONSTRAINT_SIGMA_DOT;  // the operand has spin -t, the product spin 2 - t
      load_row(row_b, Q.in[operand] + 2 * step * Q.ld[operand], nc, p < 3 ? -p : 2, p == 3);
      __syncthreads();
      theta_sums(pan_b, row_b, Q.tab_in[t], l_max, -t, n);
      __syncthreads();
      convolution(pan_g, pan_s, l_max, pan_b, l_max, l_max, n);
      __syncthreads();
      double acc = 0.0;
      for (int c = threadIdx.x; c < nc; c += PRODUCT_THREADS) {
        const double2 prod = quadrature(pan_g, Q.tab_out[t], c, ell_of_column(c), l_max, 2 - t, n);
        if (p == 3) {
          row_o[c] = prod;
          continue;
        }
        // v_p = psi_p' - (eth psi_{p+1} + (3 - p) sigma psi_{p+2})
        const double f = eth_ghp_factor(ell_of_column(c), 1 - p), times = (double)(3 - p);
        const double2 d = at(CONSTRAINT_PSI_DOT + p, c), q = at(p + 1, c);
        const double2 rhs = double2{f * q.x + times * prod.x, f * q.y + times * prod.y};
        acc = acc + put(Q.v[p], c, double2{d.x - rhs.x, d.y - rhs.y});
      }
      if (p == 0) n0 = acc;
      if (p == 1) n1 = acc;
      if (p == 2) n2 = acc;
    }
#pragma unroll 1
    for (int k = 3; k < 5; ++k) {  // v3 = psi3 + eth bar(sigma'), v4 = psi4 + bar(sigma'')
      if (!norms && !Q.v[k]) continue;
      double acc = 0.0;
      for (int c = threadIdx.x; c < nc; c += PRODUCT_THREADS) {
        const int l = ell_of_column(c), m = c - l * (l + 1);
        const double2 b = bar_of(at(CONSTRAINT_SIGMA_DOT + k - 3, l * (l + 1) - m), 2 + m), q = at(k, c);
        if (k == 3) {
          const double f = eth_ghp_factor(l, -2);
          acc = acc + put(Q.v[k], c, double2{q.x + f * b.x, q.y + f * b.y});
        } else {
          acc = acc + put(Q.v[k], c, double2{q.x + b.x, q.y + b.y});
        }
      }
      if (k == 3) n3 = acc;
      if (k == 4) n4 = acc;
    }
    if (need & 8) {
      __syncthreads();
      // x = psi2 + eth eth bar(sigma) + sigma bar(sigma') at (l, m): one chain of operations, whichever thread forms it
      auto x_at = [&](int l, int m) -> double2 {
        const int col = l * (l + 1) + m;
        const double f1 = eth_ghp_factor(l, -2), f2 = eth_ghp_factor(l, -1);
        const double2 b = bar_of(row_s[l * (l + 1) - m], 2 + m), q = at(2, col), prod = row_o[col];
        return double2{(q.x + f2 * (f1 * b.x)) + prod.x, (q.y + f2 * (f1 * b.y)) + prod.y};
      };
      for (int c = threadIdx.x; c < nc; c += PRODUCT_THREADS) {
        const int l = ell_of_column(c), m = c - l * (l + 1);
        const double2 x = x_at(l, m), xb = bar_of(x_at(l, -m), m);
        n5 = n5 + put(Q.v[5], c, double2{0.5 * (x.y - xb.y), -0.5 * (x.x - xb.x)});  // -i (x - bar x) / 2
      }
    }
    if (norms) {
      __syncthreads();  // (rows and panels are read until here)
      const int t = threadIdx.x;
      red[t] = n0, red[PRODUCT_THREADS + t] = n1, red[2 * PRODUCT_THREADS + t] = n2;
      red[3 * PRODUCT_THREADS + t] = n3, red[4 * PRODUCT_THREADS + t] = n4, red[5 * PRODUCT_THREADS + t] = n5;
#pragma unroll 1
      for (int stride = PRODUCT_THREADS / 2; stride > 0; stride >>= 1) {
        __syncthreads();
        if (t < stride)
          for (int k = 0; k < 6; ++k) red[k * PRODUCT_THREADS + t] = red[k * PRODUCT_THREADS + t] + red[k * PRODUCT_THREADS + t + stride];
      }
      if (t == 0)
        for (int k = 0; k < 6; ++k) Q.norms[6 * step + k] = sqrt(red[k * PRODUCT_THREADS]);
    }
    __syncthreads();  // (the rows, panels and partial sums of this step are read until here)
  }
}

// One stage of the Bianchi identities run forwards (scri/asymptotic_bondi_data/from_initial_values.py:128-154): the inner step of
// constraint_kernel, stored where that kernel subtracts it from a given derivative.
//     rhs_k = eth a + (3 - k) sigma b       k = 1: a = psi2 (spin 0), b = psi3 (spin -1)      k = 0: a = psi1 (spin 1), b = psi2 (spin 0)
// k = 2, the head, takes sigma_dot and sigma_ddot as stored (spin 2) for a and b and forms, mode by mode,
//     psi4 = -bar(sigma_ddot)      psi3 = -eth bar(sigma_dot)      rhs_2 = eth psi3 + sigma psi4
// psi4 is negated in LDS by the thread that loaded the column and goes through the product from there, so the product is the one
// product_kernel forms of sigma and the stored psi4; psi3 at a column is formed by the thread that stores rhs_2 there.  sigma and
// sigma_ddot are read once, sigma_dot once in mirrored column order.  The diagonal term reads `a` from memory as stored.
// LDS: two rows and the three panels of product_kernel at (l, l, l).
__global__ __launch_bounds__(PRODUCT_THREADS) void bianchi_kernel(BianchiArgs Q, long long n_times) {
#pragma clang fp contract(off)
  extern __shared__ double2 product_lds[];
  const int k = Q.k, l_max = Q.l_max, n = Q.n_nodes, nc = (l_max + 1) * (l_max + 1), width = 2 * l_max + 1;
  double2* row_s = product_lds;  // sigma
  double2* row_b = row_s + nc;   // psi2, psi3 or psi4
  double2* pan_s = row_b + nc;
  double2* pan_b = pan_s + n * width;
  double2* pan_g = pan_b + n * width;
  const bool head = k == 2;
  const double times = (double)(3 - k);
  for (long long step = blockIdx.x; step < n_times; step += gridDim.x) {  // (uniform in the workgroup: every wave takes every barrier)
    load_row(row_s, Q.sigma + 2 * step * Q.ld_sigma, nc, 2, 0);
    load_row(row_b, Q.b + 2 * step * Q.ld_b, nc, head ? 2 : -k, head);
    if (head)  // (the columns this thread has just loaded)
      for (int c = threadIdx.x; c < nc; c += PRODUCT_THREADS) {
        const double2 v = row_b[c], p4 = double2{-v.x, -v.y};
        row_b[c] = p4;
        *reinterpret_cast<double2*>(Q.psi4 + 2 * (step * Q.ld_psi + c)) = p4;
      }
    __syncthreads();
    theta_sums(pan_s, row_s, Q.tab_sigma, l_max, 2, n);
    theta_sums(pan_b, row_b, Q.tab_b, l_max, -k, n);
    __syncthreads();
    convolution(pan_g, pan_s, l_max, pan_b, l_max, l_max, n);
    __syncthreads();
    for (int c = threadIdx.x; c < nc; c += PRODUCT_THREADS) {
      const int l = ell_of_column(c), m = c - l * (l + 1);
      const double2 prod = quadrature(pan_g, Q.tab_out, c, l, l_max, 2 - k, n);
      double2 q;
      if (head) {
        const double2 b = bar_of(*reinterpret_cast<const double2*>(Q.a + 2 * (step * Q.ld_a + l * (l + 1) - m)), 2 + m);
        const double f2 = eth_ghp_factor(l, -2);
        q = double2{-(f2 * b.x), -(f2 * b.y)};
        *reinterpret_cast<double2*>(Q.psi3 + 2 * (step * Q.ld_psi + c)) = q;
      } else {
        q = *reinterpret_cast<const double2*>(Q.a + 2 * (step * Q.ld_a + c));
      }
      const double f = eth_ghp_factor(l, 1 - k);
      *reinterpret_cast<double2*>(Q.rhs + 2 * (step * Q.ld_rhs + c)) = double2{f * q.x + times * prod.x, f * q.y + times * prod.y};
    }
    __syncthreads();  // (the rows and panels of this step are read until here)
  }
}

int product_compute_units() {
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  (void)hipGetLastError();
  return cus;
}

}  // namespace

int product_nodes(int l_a, int l_b, int l_out) { return (l_a + l_b + l_out) / 2 + 1; }

// one time step per pass of a workgroup: its three rows and three panels in LDS; as many workgroups as the device holds at once, by LDS
// and by its 32 waves per compute unit.  false: a step does not fit
bool product_launch_shape(int l_a, int l_b, int l_out, ProductShape* S) {
  if (l_a < 0 || l_b < 0 || l_out < 0) return false;
  const size_t n = (size_t)product_nodes(l_a, l_b, l_out);
  const size_t cells = (size_t)(l_a + 1) * (l_a + 1) + (size_t)(l_b + 1) * (l_b + 1) + (size_t)(l_out + 1) * (l_out + 1) +
                       n * ((size_t)2 * l_a + 1 + (size_t)2 * l_b + 1 + (size_t)2 * l_out + 1);
  int dev = 0;
  (void)hipGetDevice(&dev);
  const size_t room = (size_t)lds_per_workgroup(dev);
  if (16 * cells > room) return false;
  S->lds_bytes = 16 * cells;
  S->steps = 1;
  const long long per_cu = std::max<long long>(1, std::min<long long>((long long)(room / S->lds_bytes), 32 / (PRODUCT_THREADS / 64)));
  S->groups = (int)std::min<long long>(per_cu * product_compute_units(), 1 << 20);
  S->tables_in_lds = false;
  return true;
}

static hipError_t launch_product(hipStream_t stream, const ProductOperands& P, long long n_times, double* out, long long ld_out, const SuperOutputs* Q,
                                 bool integrated) {
  if (n_times <= 0) return hipSuccess;
  ProductShape S;
  if (!P.a || !P.b || !P.tab_a || !P.tab_b || !P.tab_out || P.n_nodes != product_nodes(P.l_a, P.l_b, P.l_out) || P.l_out > P.l_a + P.l_b ||
      !product_launch_shape(P.l_a, P.l_b, P.l_out, &S))
    return hipErrorInvalidValue;
  const long long groups = std::min<long long>(S.groups, n_times);
  auto go = [&](auto kernel, const SuperOutputs& q) -> hipError_t {
    if (S.lds_bytes > 64 * 1024) {
      hipError_t e = allow_dynamic_lds((const void*)kernel);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(PRODUCT_THREADS), S.lds_bytes, stream, P, n_times, out, ld_out, q);
    return hipGetLastError();
  };
  if (Q) return integrated ? go(product_kernel<true, true>, *Q) : go(product_kernel<true, false>, *Q);
  return go(product_kernel<false, false>, SuperOutputs{});
}

hipError_t launch_mode_product(hipStream_t stream, const double* a, long long ld_a, int spin_a, int l_a, int conj_a, const double* b, long long ld_b,
                               int spin_b, int l_b, int conj_b, long long n_times, int l_out, const double* tab_a, const double* tab_b,
                               const double* tab_out, double* out, long long ld_out) {
  if (!out) return hipErrorInvalidValue;
  const ProductOperands P{a, b, ld_a, ld_b, spin_a, spin_b, conj_a ? 1 : 0, conj_b ? 1 : 0, l_a, l_b, l_out, product_nodes(l_a, l_b, l_out), tab_a, tab_b, tab_out};
  return launch_product(stream, P, n_times, out, ld_out, nullptr, false);
}

hipError_t launch_supermomenta(hipStream_t stream, const double* psi2, long long ld_psi2, const double* sigma, long long ld_sigma,
                               const double* sigma_dot, long long ld_sigma_dot, long long n_times, int ell_max, int l_out, int integrated,
                               const double* tab_plus, const double* tab_minus, const double* tab_out, double* bondi_sachs, double* moreschi,
                               double* geroch, double* geroch_winicour, double* mass_aspect, long long ld_out) {
  if (!psi2 || ell_max < 2 || l_out > ell_max || (!bondi_sachs && !moreschi && !geroch && !geroch_winicour && !mass_aspect)) return hipErrorInvalidValue;
  const ProductOperands P{sigma, sigma_dot, ld_sigma, ld_sigma_dot, 2, 2, 0, 1, ell_max, ell_max, l_out, product_nodes(ell_max, ell_max, l_out),
                          tab_plus, tab_minus, tab_out};
  const SuperOutputs Q{psi2, ld_psi2, ld_out, bondi_sachs, moreschi, geroch, geroch_winicour, mass_aspect};
  return launch_product(stream, P, n_times, nullptr, 0, &Q, integrated != 0);
}

hipError_t launch_bondi_constraints(hipStream_t stream, const ConstraintArgs& Q, long long n_times) {
  if (n_times <= 0) return hipSuccess;
  ProductShape S;
  if (Q.l_max < 2 || Q.n_nodes != product_nodes(Q.l_max, Q.l_max, Q.l_max) || !product_launch_shape(Q.l_max, Q.l_max, Q.l_max, &S))
    return hipErrorInvalidValue;
  if (!Q.norms && !Q.v[0] && !Q.v[1] && !Q.v[2] && !Q.v[3] && !Q.v[4] && !Q.v[5]) return hipErrorInvalidValue;
  // (the partial sums of the norms lie over the rows and panels: six doubles per thread, which only ell_max <= 7 falls short of)
  const size_t lds = std::max(S.lds_bytes, sizeof(double) * 6 * PRODUCT_THREADS);
  if (lds > 64 * 1024) {
    hipError_t e = allow_dynamic_lds((const void*)constraint_kernel);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(constraint_kernel, dim3((unsigned)std::min<long long>(S.groups, n_times)), dim3(PRODUCT_THREADS), lds, stream, Q, n_times);
  return hipGetLastError();
}

hipError_t launch_bianchi_rhs(hipStream_t stream, const BianchiArgs& Q, long long n_times) {
  if (n_times <= 0) return hipSuccess;
  ProductShape S;
  if (Q.k < 0 || Q.k > 2 || Q.l_max < 2 || Q.n_nodes != product_nodes(Q.l_max, Q.l_max, Q.l_max) || !product_launch_shape(Q.l_max, Q.l_max, Q.l_max, &S))
    return hipErrorInvalidValue;
  const long long n_modes = (long long)(Q.l_max + 1) * (Q.l_max + 1);
  if (!Q.sigma || !Q.a || !Q.b || !Q.rhs || !Q.tab_sigma || !Q.tab_b || !Q.tab_out || (Q.k == 2) != (Q.psi3 != nullptr) || (Q.k == 2) != (Q.psi4 != nullptr))
    return hipErrorInvalidValue;
  if (Q.ld_sigma < n_modes || Q.ld_a < n_modes || Q.ld_b < n_modes || Q.ld_rhs < n_modes || (Q.k == 2 && Q.ld_psi < n_modes)) return hipErrorInvalidValue;
  if (S.lds_bytes > 64 * 1024) {
    hipError_t e = allow_dynamic_lds((const void*)bianchi_kernel);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(bianchi_kernel, dim3((unsigned)std::min<long long>(S.groups, n_times)), dim3(PRODUCT_THREADS), S.lds_bytes, stream, Q, n_times);
  return hipGetLastError();
}

}  // namespace bms
