// Fluxes of energy, momentum, angular momentum and boost (scri/flux.py:182-798) of modes resident in HBM, in one pass over the modes.
//
// Every operator of scri/flux.py is banded: a column (l, m) couples only to the rows (l + dl, m + mu), dl, mu in {-1, 0, 1}, and with the
// ladder factors of eth / ethbar folded into the coefficients only h and hdot = N are read.  Per (column, neighbour) three REAL
// coefficients remain (engine_flux.hip builds them in long double):
//     P   chi at s = -2                                    momentum flux <N|chi|N>, and the boost term -(u/2) <N|chi|N>: formed once
//     B1  (1/8)[ethbar' chi_-3 ethbar - eth' chi_-1 eth + 6 chi_-2] - (1/4) eth' (eth chi)       the pair (N, h)
//     B2  (1/8)[...the same bracket...]                            + (1/4) (ethbar chi) eth      the pair (h, N)
// and the angular-momentum operators need lambda_+- = sqrt((l -+ m)(l +- m + 1)) and m.  The image of one l range: 27 n + 2 n + n doubles,
//     image[(3 k + set) n + c]   k = 3 (dl + 1) + (mu + 1), set = 0 (P), 1 (B1), 2 (B2), column c      (lanes read consecutive doubles)
//     image[27 n + c], image[28 n + c]   lambda_+, lambda_-;      image[29 n + c]   l of the column
// A persistent workgroup copies the image into LDS ONCE (while it fits beside the rows: FluxShape::tables_in_lds, else it is read through
// L2) and then walks time steps, one wave per step: the two rows of the step go to LDS by 16-byte loads of consecutive lanes (coalesced
// for any n_modes and ld), lane j sums the columns j, j + 64, ... in that order, and the sixteen partial sums are added across the wave by
// a butterfly.  Nothing in that order depends on the launch geometry, so a step's result does not depend on the steps around it, on the
// number of waves or workgroups, or on which outputs were asked for.  No contraction: every multiply-add is spelled out.
// The brackets of two waveforms (pair_kernel below: <f|g>, <f|L_a|g>, <f|L_a L_b|g>) and the Bondi charges (charge_kernel) share that
// frame, the wave sum and the LDS-room rule.
#include "wigner.h"
#include "kernels.h"

namespace bms {

namespace {

constexpr int FLUX_IMAGE_PER_MODE = 30;  // doubles of the image per column
constexpr int FLUX_MAX_WAVES = 8;
constexpr int CHARGE_IMAGE_PER_MODE = 20;  // doubles of the charges' image per column

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <bool WITH_H, bool TAB_LDS>
__global__ __launch_bounds__(64 * FLUX_MAX_WAVES) void flux_kernel(const double* __restrict__ t, const double* __restrict__ H, long long ld_h,
                                                                   const double* __restrict__ N, long long ld_n, long long n_times, int ell_min,
                                                                   int ell_max, int n, const double* __restrict__ image, double* __restrict__ e_out,
                                                                   double* __restrict__ p_out, double* __restrict__ j_out, double* __restrict__ b_out) {
#pragma clang fp contract(off)
  extern __shared__ double2 flux_lds[];  // [waves][rows][n] rows of modes, then the image
  constexpr int ROWS = WITH_H ? 2 : 1;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double2* nrow = flux_lds + (size_t)wave * ROWS * n;
  double2* hrow = nrow + (WITH_H ? n : 0);
  double* ltab = reinterpret_cast<double*>(flux_lds + (size_t)waves * ROWS * n);
  if (TAB_LDS)
    for (int i = threadIdx.x; i < FLUX_IMAGE_PER_MODE * n; i += blockDim.x) ltab[i] = image[i];
  auto tab = [&](int i) { return TAB_LDS ? ltab[i] : image[i]; };
  const long long pass_steps = (long long)gridDim.x * waves, passes = (n_times + pass_steps - 1) / pass_steps;
  const int base = ell_min * ell_min;
  __syncthreads();
  for (long long pass = 0; pass < passes; ++pass) {  // (every wave takes every barrier: the trip count is the workgroup's)
    const long long step = pass * pass_steps + (long long)blockIdx.x * waves + wave;
    const bool live = step < n_times;
    if (live)
      for (int i = lane; i < n; i += 64) {
        nrow[i] = *reinterpret_cast<const double2*>(N + (step * ld_n + i) * 2);
        if (WITH_H) hrow[i] = *reinterpret_cast<const double2*>(H + (step * ld_h + i) * 2);
      }
    __syncthreads();
    if (live) {
      // + and - components as (re, im), z as re: P = <N|chi|N>, B = <N|B1|h> + <h|B2|N>, J = <N|J|h>
      double e = 0, P[5] = {0, 0, 0, 0, 0}, B[5] = {0, 0, 0, 0, 0}, J[5] = {0, 0, 0, 0, 0};
      for (int i = lane; i < n; i += 64) {
        const int l = (int)tab(29 * n + i), m = i + base - l * (l + 1);
        const double2 nc = nrow[i];
        const double2 hc = WITH_H ? hrow[i] : double2{0.0, 0.0};
        e = fma(nc.x, nc.x, e);
        e = fma(nc.y, nc.y, e);
#pragma unroll
        for (int dl = -1; dl <= 1; ++dl) {
          const int lp = l + dl;
          if (lp < ell_min || lp > ell_max) continue;
          const int shift = dl == 0 ? 0 : (dl > 0 ? 2 * l + 2 : -2 * l);
#pragma unroll
          for (int mu = -1; mu <= 1; ++mu) {
            if (m + mu < -lp || m + mu > lp) continue;
            const int r = i + shift + mu, k = 3 * (dl + 1) + (mu + 1);
            const int o = mu == 1 ? 0 : (mu == -1 ? 2 : 4);  // where the component's (re, im) live
            const double2 nr = nrow[r];
            const double cp = tab((3 * k + 0) * n + i);
            // conj(nr) nc
            const double qr = fma(nr.x, nc.x, nr.y * nc.y), qi = fma(nr.x, nc.y, -(nr.y * nc.x));
            P[o] = fma(cp, qr, P[o]);
            if (mu != 0) P[o + 1] = fma(cp, qi, P[o + 1]);
            if (WITH_H) {
              const double2 hr = hrow[r];
              const double c1 = tab((3 * k + 1) * n + i), c2 = tab((3 * k + 2) * n + i);
              const double ar = fma(nr.x, hc.x, nr.y * hc.y), ai = fma(nr.x, hc.y, -(nr.y * hc.x));  // conj(nr) hc
              const double br = fma(hr.x, nc.x, hr.y * nc.y), bi = fma(hr.x, nc.y, -(hr.y * nc.x));  // conj(hr) nc
              B[o] = fma(c1, ar, B[o]);
              B[o] = fma(c2, br, B[o]);
              if (mu != 0) {
                B[o + 1] = fma(c1, ai, B[o + 1]);
                B[o + 1] = fma(c2, bi, B[o + 1]);
              }
              if (dl == 0) {  // <l, m + mu| J |l, m> = i lambda: i (ar + i ai) = -ai + i ar
                const double lam = mu == 0 ? (double)m : tab((mu == 1 ? 27 : 28) * n + i);
                J[o] = fma(-lam, ai, J[o]);
                if (mu != 0) J[o + 1] = fma(lam, ar, J[o + 1]);
              }
            }
          }
        }
      }
      e = wave_sum(e);
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        P[q] = wave_sum(P[q]);
        if (WITH_H) B[q] = wave_sum(B[q]), J[q] = wave_sum(J[q]);
      }
      if (lane == 0) {
        const double e_scale = 16.0 * M_PI;
        if (e_out) e_out[step] = e / e_scale;
        if (p_out) {
          p_out[3 * step] = 0.5 * (P[0] + P[2]) / e_scale;
          p_out[3 * step + 1] = 0.5 * (P[1] - P[3]) / e_scale;
          p_out[3 * step + 2] = P[4] / e_scale;
        }
        if (WITH_H && j_out) {
          j_out[3 * step] = 0.5 * (J[0] + J[2]) / -e_scale;
          j_out[3 * step + 1] = 0.5 * (J[1] - J[3]) / -e_scale;
          j_out[3 * step + 2] = J[4] / -e_scale;
        }
        if (WITH_H && b_out) {
          const double half_u = 0.5 * t[step], b_scale = -32.0 * M_PI;
          double T[5];
#pragma unroll
          for (int q = 0; q < 5; ++q) T[q] = fma(-half_u, P[q], B[q]);
          b_out[3 * step] = 0.5 * (T[0] + T[2]) / b_scale;
          b_out[3 * step + 1] = 0.5 * (T[1] - T[3]) / b_scale;
          b_out[3 * step + 2] = T[4] / b_scale;
        }
      }
    }
    __syncthreads();
  }
}

// out[t] = sum_e op(a[t][rows_e]) values_e b[t][cols_e]: one wave per step, its row pair in LDS, element e on lane e mod 64, lane sums in
// element order, then the butterfly
__global__ __launch_bounds__(256) void expectation_kernel(const double* __restrict__ A, long long ld_a, int conj_a, const double* __restrict__ Bm,
                                                          long long ld_b, long long n_times, int n_cols, const int* __restrict__ rows,
                                                          const int* __restrict__ cols, const double2* __restrict__ values, long long n_el,
                                                          double* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ double2 exp_lds[];  // [waves][2][n_cols]
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double2* a = exp_lds + (size_t)wave * 2 * n_cols;
  double2* b = a + n_cols;
  const long long pass_steps = (long long)gridDim.x * waves, passes = (n_times + pass_steps - 1) / pass_steps;
  for (long long pass = 0; pass < passes; ++pass) {
    const long long step = pass * pass_steps + (long long)blockIdx.x * waves + wave;
    const bool live = step < n_times;
    if (live)
      for (int i = lane; i < n_cols; i += 64) {
        a[i] = *reinterpret_cast<const double2*>(A + (step * ld_a + i) * 2);
        b[i] = *reinterpret_cast<const double2*>(Bm + (step * ld_b + i) * 2);
      }
    __syncthreads();
    if (live) {
      double sr = 0, si = 0;
      for (long long el = lane; el < n_el; el += 64) {
        const double2 x = a[rows[el]], y = b[cols[el]], v = values[el];
        const double xi = conj_a ? -x.y : x.y;
        const double pr = fma(x.x, y.x, -(xi * y.y)), pi = fma(x.x, y.y, xi * y.x);  // x y
        sr = fma(pr, v.x, sr);
        sr = fma(-pi, v.y, sr);
        si = fma(pr, v.y, si);
        si = fma(pi, v.x, si);
      }
      sr = wave_sum(sr);
      si = wave_sum(si);
      if (lane == 0) out[2 * step] = sr, out[2 * step + 1] = si;
    }
    __syncthreads();
  }
}

// Brackets of two waveforms f, g (scri/mode_calculations.py:60-89, 106-180) per time step, in the (+, -, z) basis:
//     I = sum conj(f_i) g_i;   <L_a> = sum conj(f_{i'}) <l, m'| L_a |l, m> g_i;   <L_a L_b> likewise
// With q_k = conj(f[i + k]) g[i], k = -2 .. 2 (inside the l block of column i = (l, m)) and lp = sqrt((l - m)(l + m + 1)),
// lm = sqrt((l + m)(l - m + 1)), the thirteen brackets are real multiples of the five products:
//     q_0:  I 1, z m, zz m^2, pm lm^2 = (l + m)(l - m + 1) (m - 1 >= -l), mp lp^2 = (l - m)(l + m + 1) (m + 1 <= l)
//     q_+1: p lp, pz lp m, zp (m + 1) lp (m + 1 <= l);        q_-1: m lm, mz lm m, zm (m - 1) lm (m - 1 >= -l)
//     q_+2: pp sqrt((l - m - 1)(l + m + 2)) lp (m + 2 <= l);   q_-2: mm sqrt((l + m - 1)(l - m + 2)) lm (m - 2 >= -l)
// Geometry and order as the flux kernel's: one wave per step, the row of f in LDS (its neighbours are read), g at its own column straight
// from memory, lane j sums the columns j, j + 64, ... in that order, a butterfly closes.  GROUPS: bit 0 I, bit 1 <L>, bit 2 <LL>; an
// accumulator's chain of operations is the same in every instantiation.
template <int GROUPS>
__global__ __launch_bounds__(64 * FLUX_MAX_WAVES) void pair_kernel(const double* __restrict__ F, long long ld_f, const double* __restrict__ G,
                                                                   long long ld_g, long long n_times, int ell_min, int n,
                                                                   double* __restrict__ inner, double* __restrict__ l_out,
                                                                   double* __restrict__ ll_out) {
#pragma clang fp contract(off)
  extern __shared__ double2 pair_lds[];  // [waves][n] rows of f
  constexpr bool W_I = GROUPS & 1, W_L = GROUPS & 2, W_LL = GROUPS & 4;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double2* frow = pair_lds + (size_t)wave * n;
  const long long pass_steps = (long long)gridDim.x * waves, passes = (n_times + pass_steps - 1) / pass_steps;
  const int base = ell_min * ell_min;
  for (long long pass = 0; pass < passes; ++pass) {  // (every wave takes every barrier: the trip count is the workgroup's)
    const long long step = pass * pass_steps + (long long)blockIdx.x * waves + wave;
    const bool live = step < n_times;
    if (live)
      for (int i = lane; i < n; i += 64) frow[i] = *reinterpret_cast<const double2*>(F + (step * ld_f + i) * 2);
    __syncthreads();
    if (live) {
      double I[2] = {0, 0}, L[6] = {0, 0, 0, 0, 0, 0}, LL[18] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      auto add = [](double* acc, double c, double qr, double qi) { acc[0] = fma(c, qr, acc[0]), acc[1] = fma(c, qi, acc[1]); };
      int l = ell_min;
      for (int i = lane; i < n; i += 64) {
        while (i + base >= (l + 1) * (l + 1)) ++l;
        const int m = i + base - l * (l + 1);
        const double2 g = *reinterpret_cast<const double2*>(G + (step * ld_g + i) * 2);
        auto q = [&](int k, double& qr, double& qi) {  // conj(f[i + k]) g[i]
          const double2 f = frow[i + k];
          qr = fma(f.x, g.x, f.y * g.y), qi = fma(f.x, g.y, -(f.y * g.x));
        };
        const double md = (double)m;
        double qr, qi;
        q(0, qr, qi);
        if (W_I) add(I, 1.0, qr, qi);
        if (W_L) add(L + 4, md, qr, qi);
        if (W_LL) {
          add(LL + 16, md * md, qr, qi);
          if (m - 1 >= -l) add(LL + 2, (double)((l + m) * (l - m + 1)), qr, qi);
          if (m + 1 <= l) add(LL + 4, (double)((l - m) * (l + m + 1)), qr, qi);
        }
        if ((W_L || W_LL) && m + 1 <= l) {
          const double lp = sqrt((double)((l - m) * (l + m + 1)));
          q(1, qr, qi);
          if (W_L) add(L + 0, lp, qr, qi);
          if (W_LL) {
            add(LL + 8, lp * md, qr, qi);
            add(LL + 10, (md + 1.0) * lp, qr, qi);
            if (m + 2 <= l) {
              q(2, qr, qi);
              add(LL + 0, sqrt((double)((l - m - 1) * (l + m + 2))) * lp, qr, qi);
            }
          }
        }
        if ((W_L || W_LL) && m - 1 >= -l) {
          const double lm = sqrt((double)((l + m) * (l - m + 1)));
          q(-1, qr, qi);
          if (W_L) add(L + 2, lm, qr, qi);
          if (W_LL) {
            add(LL + 12, lm * md, qr, qi);
            add(LL + 14, (md - 1.0) * lm, qr, qi);
            if (m - 2 >= -l) {
              q(-2, qr, qi);
              add(LL + 6, sqrt((double)((l + m - 1) * (l - m + 2))) * lm, qr, qi);
            }
          }
        }
      }
      if (W_I) {
        I[0] = wave_sum(I[0]), I[1] = wave_sum(I[1]);
        if (lane == 0 && inner) inner[2 * step] = I[0], inner[2 * step + 1] = I[1];
      }
      if (W_L) {
#pragma unroll
        for (int k = 0; k < 6; ++k) L[k] = wave_sum(L[k]);
        if (lane == 0 && l_out)
#pragma unroll
          for (int k = 0; k < 6; ++k) l_out[6 * step + k] = L[k];
      }
      if (W_LL) {
#pragma unroll
        for (int k = 0; k < 18; ++k) LL[k] = wave_sum(LL[k]);
        if (lane == 0 && ll_out)
#pragma unroll
          for (int k = 0; k < 18; ++k) ll_out[18 * step + k] = LL[k];
      }
    }
    __syncthreads();
  }
}

// Bondi charges (scri/asymptotic_bondi_data/bms_charges.py:14-200) of AsymptoticBondiData rows (l from 0) per time step.  The l <= 1 modes
// of a product sigma b, b built from sigma-bar or its time derivative, are  sum C sigma[i] conj(x[r])  over the columns i = (l, m) of sigma
// and the neighbours r = (l + dl, m + mu) of x = sigma or sigma_dot, mode M = -mu, with real C (engine_flux.hip builds them in long double):
//     A0  spins (2, -2) -> L = 0, diagonal             with x = sigma_dot: the energy
//     A1  spins (2, -2) -> L = 1                       with x = sigma_dot: the momentum;  with x = sigma: (1/2) eth(sigma sigma-bar)
//     B   spins (2, -1) -> L = 1, eth's factor folded  with x = sigma: sigma eth sigma-bar
// The image of l = 0 .. ell_max: 18 n + n + n doubles,
//     image[(2 k + set) n + c]   k = 3 (dl + 1) + (mu + 1), set = 0 (A1), 1 (B), column c;    image[18 n + c]  A0;    image[19 n + c]  l
// From the sums E0 (A0), E (A1, sigma_dot), S (A1, sigma), Bc (B) and the l <= 1 entries of psi1 and psi2 (read by one lane, added after
// the wave sum), with vec(a) = (Re(a_-1 - a_1) / sqrt 6, Im(a_-1 + a_1) / sqrt 6, Re a_0 / sqrt 3) / sqrt(4 pi):
//     P = -(Re(psi2_00 + E0) / sqrt(4 pi), vec(psi2 + E)),  J = vec(i (psi1 + Bc)),  G = vec(g), g = -(psi1 + Bc + S / 2),  N = vec(g + t (psi2 + E))
// (the real part of a function changes nothing in vec; eth_GHP of a spin-0 l = 1 mode is a factor of 1).  Geometry and order as the flux
// kernel's.  WITH_DOT: sigma_dot and psi2 are read (P or N wanted); an accumulator's chain of operations is the same in both instantiations.
template <bool WITH_DOT, bool TAB_LDS>
__global__ __launch_bounds__(64 * FLUX_MAX_WAVES) void charge_kernel(const double* __restrict__ t, const double* __restrict__ psi1, long long ld_1,
                                                                     const double* __restrict__ psi2, long long ld_2, const double* __restrict__ Sg,
                                                                     long long ld_s, const double* __restrict__ Sd, long long ld_d, long long n_times,
                                                                     int ell_max, int n, const double* __restrict__ image, double* __restrict__ p_out,
                                                                     double* __restrict__ j_out, double* __restrict__ n_out, double* __restrict__ g_out) {
#pragma clang fp contract(off)
  extern __shared__ double2 charge_lds[];  // [waves][rows][n] rows of modes, then the image
  constexpr int ROWS = WITH_DOT ? 2 : 1;
  const int waves = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double2* srow = charge_lds + (size_t)wave * ROWS * n;
  double2* drow = srow + (WITH_DOT ? n : 0);
  double* ltab = reinterpret_cast<double*>(charge_lds + (size_t)waves * ROWS * n);
  if (TAB_LDS)
    for (int i = threadIdx.x; i < CHARGE_IMAGE_PER_MODE * n; i += blockDim.x) ltab[i] = image[i];
  auto tab = [&](int i) { return TAB_LDS ? ltab[i] : image[i]; };
  const long long pass_steps = (long long)gridDim.x * waves, passes = (n_times + pass_steps - 1) / pass_steps;
  __syncthreads();
  for (long long pass = 0; pass < passes; ++pass) {  // (every wave takes every barrier: the trip count is the workgroup's)
    const long long step = pass * pass_steps + (long long)blockIdx.x * waves + wave;
    const bool live = step < n_times;
    if (live)
      for (int i = lane; i < n; i += 64) {
        srow[i] = *reinterpret_cast<const double2*>(Sg + (step * ld_s + i) * 2);
        if (WITH_DOT) drow[i] = *reinterpret_cast<const double2*>(Sd + (step * ld_d + i) * 2);
      }
    __syncthreads();
    if (live) {
      // modes M = -1, +1 as (re, im) at 0, 2 and M = 0 at 4 (mu = +1, -1, 0): E, S need no imaginary part of M = 0
      double e0 = 0, E[5] = {0, 0, 0, 0, 0}, S[5] = {0, 0, 0, 0, 0}, Bc[6] = {0, 0, 0, 0, 0, 0};
      for (int i = lane; i < n; i += 64) {
        const int l = (int)tab(19 * n + i), m = i - l * (l + 1);
        if (l < 2) continue;
        const double2 sc = srow[i];
        if (WITH_DOT) {
          const double2 dc = drow[i];
          e0 = fma(tab(18 * n + i), fma(sc.x, dc.x, sc.y * dc.y), e0);  // Re(sigma conj(sigma_dot))
        }
#pragma unroll
        for (int dl = -1; dl <= 1; ++dl) {
          const int lp = l + dl;
          if (lp < 2 || lp > ell_max) continue;
          const int shift = dl == 0 ? 0 : (dl > 0 ? 2 * l + 2 : -2 * l);
#pragma unroll
          for (int mu = -1; mu <= 1; ++mu) {
            if (m + mu < -lp || m + mu > lp) continue;
            const int r = i + shift + mu, k = 3 * (dl + 1) + (mu + 1);
            const int o = mu == 1 ? 0 : (mu == -1 ? 2 : 4);  // where the mode's (re, im) live
            const double ca = tab((2 * k + 0) * n + i), cb = tab((2 * k + 1) * n + i);
            const double2 xs = srow[r];
            // sc conj(xs)
            const double qr = fma(sc.x, xs.x, sc.y * xs.y), qi = fma(sc.y, xs.x, -(sc.x * xs.y));
            Bc[o] = fma(cb, qr, Bc[o]);
            Bc[o + 1] = fma(cb, qi, Bc[o + 1]);
            S[o] = fma(ca, qr, S[o]);
            if (mu != 0) S[o + 1] = fma(ca, qi, S[o + 1]);
            if (WITH_DOT) {
              const double2 xd = drow[r];
              const double dr = fma(sc.x, xd.x, sc.y * xd.y), di = fma(sc.y, xd.x, -(sc.x * xd.y));  // sc conj(xd)
              E[o] = fma(ca, dr, E[o]);
              if (mu != 0) E[o + 1] = fma(ca, di, E[o + 1]);
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) Bc[q] = wave_sum(Bc[q]);
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        S[q] = wave_sum(S[q]);
        if (WITH_DOT) E[q] = wave_sum(E[q]);
      }
      if (WITH_DOT) e0 = wave_sum(e0);
      if (lane == 0) {
        const double r4 = 3.5449077018110320546, r12 = 6.1399602476789309309, r24 = 8.6832150546992119124;  // sqrt(4 pi), sqrt(12 pi), sqrt(24 pi)
        double a[5] = {0, 0, 0, 0, 0};  // psi2 + E, the modes (1, -1), (1, 1), (1, 0) as above
        if (WITH_DOT) {
          const double* p2 = psi2 + step * ld_2 * 2;
          a[0] = p2[2] + E[0], a[1] = p2[3] + E[1], a[2] = p2[6] + E[2], a[3] = p2[7] + E[3], a[4] = p2[4] + E[4];
          if (p_out) {
            p_out[4 * step] = -(p2[0] + e0) / r4;
            p_out[4 * step + 1] = -(a[0] - a[2]) / r24;
            p_out[4 * step + 2] = -(a[1] + a[3]) / r24;
            p_out[4 * step + 3] = -a[4] / r12;
          }
        }
        if (j_out || n_out || g_out) {
          const double* p1 = psi1 + step * ld_1 * 2;
          const double c[6] = {p1[2] + Bc[0], p1[3] + Bc[1], p1[6] + Bc[2], p1[7] + Bc[3], p1[4] + Bc[4], p1[5] + Bc[5]};  // psi1 + sigma eth sigma-bar
          if (j_out) {  // i c
            j_out[3 * step] = (c[3] - c[1]) / r24;
            j_out[3 * step + 1] = (c[0] + c[2]) / r24;
            j_out[3 * step + 2] = -c[5] / r12;
          }
          double g[5];
#pragma unroll
          for (int q = 0; q < 5; ++q) g[q] = -fma(0.5, S[q], c[q]);
          if (g_out) {
            g_out[3 * step] = (g[0] - g[2]) / r24;
            g_out[3 * step + 1] = (g[1] + g[3]) / r24;
            g_out[3 * step + 2] = g[4] / r12;
          }
          if (WITH_DOT && n_out) {
            const double u = t[step];
            double b[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) b[q] = fma(u, a[q], g[q]);
            n_out[3 * step] = (b[0] - b[2]) / r24;
            n_out[3 * step + 1] = (b[1] + b[3]) / r24;
            n_out[3 * step + 2] = b[4] / r12;
          }
        }
      }
    }
    __syncthreads();
  }
}

int compute_units() {
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  (void)hipGetLastError();
  return cus;
}

}  // namespace

int flux_image_doubles(int n_modes) { return FLUX_IMAGE_PER_MODE * n_modes; }
int charge_image_doubles(int n_modes) { return CHARGE_IMAGE_PER_MODE * n_modes; }

// THE LDS-room rule of the one-wave-per-step kernels: the most waves (8, 4, 2 or 1) whose rows of `row_bytes` each fit in LDS beside
// `table_bytes`, and as many workgroups as the device holds at once: by LDS, and by its 32 waves per compute unit.  false: not one fits
static bool fit_waves(size_t row_bytes, size_t table_bytes, FluxShape* S) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const size_t room = (size_t)lds_per_workgroup(dev);
  FluxShape s{};
  for (int w = FLUX_MAX_WAVES; w >= 1 && !s.waves; w >>= 1)
    if (w * row_bytes + table_bytes <= room) s.waves = w, s.tables_in_lds = table_bytes > 0, s.lds_bytes = w * row_bytes + table_bytes;
  if (!s.waves) return false;
  const long long per_cu = std::max<long long>(1, std::min<long long>((long long)(room / s.lds_bytes), 32 / s.waves));
  s.groups = (int)std::min<long long>(per_cu * compute_units(), 1 << 20);
  *S = s;
  return true;
}

// the image in LDS while it fits beside the rows; beyond that it stays in global memory and the waves' rows have the LDS
bool flux_launch_shape(int n_modes, FluxShape* S) {
  if (n_modes < 1) return false;
  const size_t row_pair = (size_t)32 * n_modes, image = (size_t)8 * flux_image_doubles(n_modes);
  return fit_waves(row_pair, image, S) || fit_waves(row_pair, 0, S);
}

// one row of f per wave; no tables
bool pair_launch_shape(int n_modes, FluxShape* S) { return n_modes >= 1 && fit_waves((size_t)16 * n_modes, 0, S); }

// rows of sigma and sigma_dot per wave.  The image goes into LDS only where that costs no wave: a workgroup of fewer waves hides less of
// the latency of its row loads than the table reads through L2 cost (from (ell_max + 1)^2 = 394 columns on with 160 KB)
bool charge_launch_shape(int n_modes, FluxShape* S) {
  if (n_modes < 1) return false;
  const size_t row_pair = (size_t)32 * n_modes, image = (size_t)8 * charge_image_doubles(n_modes);
  FluxShape rows_only;
  if (!fit_waves(row_pair, 0, &rows_only)) return false;
  if (!fit_waves(row_pair, image, S) || S->waves < rows_only.waves) *S = rows_only;
  return true;
}

hipError_t launch_poincare_fluxes(hipStream_t stream, const double* t, const double* h, long long ld_h, const double* hdot, long long ld_hdot,
                                  long long n_times, int ell_min, int ell_max, const double* image, double* energy, double* momentum,
                                  double* angular, double* boost) {
  if (n_times <= 0) return hipSuccess;
  const int n = (ell_max + 1) * (ell_max + 1) - ell_min * ell_min;
  const bool with_h = angular || boost;
  FluxShape S;
  if (!hdot || !image || (with_h && !h) || (boost && !t) || !flux_launch_shape(n, &S)) return hipErrorInvalidValue;
  const long long groups = std::min<long long>(S.groups, (n_times + S.waves - 1) / S.waves);
  // (the shape is that of two rows per wave; a launch without h leaves the second row's LDS unused)
  auto go = [&](auto kernel) -> hipError_t {
    if (S.lds_bytes > 64 * 1024) {
      hipError_t e = allow_dynamic_lds((const void*)kernel);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(64 * S.waves), S.lds_bytes, stream, t, h, ld_h, hdot, ld_hdot, n_times, ell_min, ell_max,
                       n, image, energy, momentum, angular, boost);
    return hipGetLastError();
  };
  if (with_h) return S.tables_in_lds ? go(flux_kernel<true, true>) : go(flux_kernel<true, false>);
  return S.tables_in_lds ? go(flux_kernel<false, true>) : go(flux_kernel<false, false>);
}

// inner c16[n], l_out c16[n][3] (+, -, z), ll_out c16[n][9] (pp, pm, mp, mm, pz, zp, mz, zm, zz), any may be null, of the rows f, g
// c16[n][ld] that START at column (ell_min, -ell_min) and hold n_modes columns of the common range
hipError_t launch_pair_brackets(hipStream_t stream, const double* f, long long ld_f, const double* g, long long ld_g, long long n_times,
                                int ell_min, int ell_max, double* inner, double* l_out, double* ll_out) {
  if (n_times <= 0) return hipSuccess;
  const int n = (ell_max + 1) * (ell_max + 1) - ell_min * ell_min;
  FluxShape S;
  if (!f || !g || (!inner && !l_out && !ll_out) || !pair_launch_shape(n, &S)) return hipErrorInvalidValue;
  const long long groups = std::min<long long>(S.groups, (n_times + S.waves - 1) / S.waves);
  auto go = [&](auto kernel) -> hipError_t {
    if (S.lds_bytes > 64 * 1024) {
      hipError_t e = allow_dynamic_lds((const void*)kernel);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(64 * S.waves), S.lds_bytes, stream, f, ld_f, g, ld_g, n_times, ell_min, n, inner, l_out,
                       ll_out);
    return hipGetLastError();
  };
  switch ((inner ? 1 : 0) | (l_out ? 2 : 0) | (ll_out ? 4 : 0)) {
    case 1: return go(pair_kernel<1>);
    case 2: return go(pair_kernel<2>);
    case 3: return go(pair_kernel<3>);
    case 4: return go(pair_kernel<4>);
    case 5: return go(pair_kernel<5>);
    case 6: return go(pair_kernel<6>);
    default: return go(pair_kernel<7>);
  }
}

hipError_t launch_bondi_charges(hipStream_t stream, const double* t, const double* psi1, long long ld_psi1, const double* psi2, long long ld_psi2,
                                const double* sigma, long long ld_sigma, const double* sigma_dot, long long ld_sigma_dot, long long n_times,
                                int ell_max, const double* image, double* four_momentum, double* angular, double* boost, double* com) {
  if (n_times <= 0) return hipSuccess;
  const int n = (ell_max + 1) * (ell_max + 1);
  const bool with_dot = four_momentum || boost, with_psi1 = angular || boost || com;
  FluxShape S;
  if (ell_max < 2 || !sigma || !image || (!with_dot && !with_psi1) || (with_dot && (!sigma_dot || !psi2)) || (with_psi1 && !psi1) || (boost && !t) ||
      !charge_launch_shape(n, &S))
    return hipErrorInvalidValue;
  const long long groups = std::min<long long>(S.groups, (n_times + S.waves - 1) / S.waves);
  // (the shape is that of two rows per wave; a launch without sigma_dot leaves the second row's LDS unused)
  auto go = [&](auto kernel) -> hipError_t {
    if (S.lds_bytes > 64 * 1024) {
      hipError_t e = allow_dynamic_lds((const void*)kernel);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(64 * S.waves), S.lds_bytes, stream, t, psi1, ld_psi1, psi2, ld_psi2, sigma, ld_sigma, sigma_dot,
                       ld_sigma_dot, n_times, ell_max, n, image, four_momentum, angular, boost, com);
    return hipGetLastError();
  };
  if (with_dot) return S.tables_in_lds ? go(charge_kernel<true, true>) : go(charge_kernel<true, false>);
  return S.tables_in_lds ? go(charge_kernel<false, true>) : go(charge_kernel<false, false>);
}

int expectation_max_cols() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return (int)((size_t)lds_per_workgroup(dev) / 32);
}

hipError_t launch_expectation_values(hipStream_t stream, const double* a, long long ld_a, int conj_a, const double* b, long long ld_b,
                                     long long n_times, int n_cols, const int* rows, const int* cols, const double* values, long long n_el,
                                     double* out) {
  if (n_times <= 0) return hipSuccess;
  if (n_cols < 1 || n_cols > expectation_max_cols()) return hipErrorInvalidValue;
  int dev = 0;
  (void)hipGetDevice(&dev);
  const size_t room = (size_t)lds_per_workgroup(dev);
  int waves = 4;
  while (waves > 1 && (size_t)waves * 32 * n_cols > room) waves >>= 1;
  const size_t lds = (size_t)waves * 32 * n_cols;
  if (lds > 64 * 1024) {
    hipError_t e = allow_dynamic_lds((const void*)expectation_kernel);
    if (e != hipSuccess) return e;
  }
  const long long groups = std::min<long long>((n_times + waves - 1) / waves, 8LL * compute_units());
  hipLaunchKernelGGL(expectation_kernel, dim3((unsigned)groups), dim3(64 * waves), lds, stream, a, ld_a, conj_a, b, ld_b, n_times, n_cols, rows, cols,
                     reinterpret_cast<const double2*>(values), n_el, out);
  return hipGetLastError();
}

}  // namespace bms
