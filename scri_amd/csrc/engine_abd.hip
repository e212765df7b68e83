// AsymptoticBondiData transformation: bms_transform_abd (+ _shard, _pipelined, _pipelined_part)
// (engine.h: the split of the engine by entry family; include/scri_amd.h: the C ABI)
#include "engine.h"

// ====================================================================================================== ABD flavour
static int transform_abd_impl(bms_ctx* c, const double* u, const void* raw, int mem, int64_t n_times, int ell_max,
                              const bms_transformation* tr, const bms_shard* sh, double* u_out, void* raw_out, int64_t* n_times_out,
                              int64_t* first_index_out);

extern "C" int bms_transform_abd_shard(bms_ctx* c, const double* u, const void* raw, int mem, int64_t n_times, int ell_max,
                                       const bms_transformation* tr, const bms_shard* sh, double* u_out, void* raw_out,
                                       int64_t* n_times_out, int64_t* first_index_out) try {
  if (!c) return BMS_ERR_INVALID;
  return with_smaller_chunks(c, [&] { return transform_abd_impl(c, u, raw, mem, n_times, ell_max, tr, sh, u_out, raw_out, n_times_out, first_index_out); });
} BMS_CATCH(c)

static int transform_abd_impl(bms_ctx* c, const double* u, const void* raw, int mem, int64_t n_times, int ell_max,
                              const bms_transformation* tr, const bms_shard* sh, double* u_out, void* raw_out, int64_t* n_times_out,
                              int64_t* first_index_out) {
  if (!u || !raw || !tr || !u_out || !raw_out || !n_times_out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  if (!valid_mem(mem)) return fail(c, BMS_ERR_INVALID, "mem is BMS_HOST or BMS_DEVICE, got %d", mem);
  HIP_TRY(c, hipSetDevice(c->device));
  const int64_t n = n_times;
  int64_t t_lo, t_hi;
  time_window(n, sh, t_lo, t_hi);
  bool regular_mesh = true;
  int rc;
  // The knot tables go first, as in the WaveformModes route: an axis the context has kept tables for (TimeAxisCache, engine.h) needs
  // neither them nor the walk again.  Speculative on a new axis: tables of samples the walk then rejects are never used nor kept.
  begin_setup_reuse(c);
  KnotTables kt;
  if ((rc = knot_tables_ahead(c, u, n, sh, t_lo, t_hi, kt))) return rc;
  // (scipy's CubicSpline, the interpolant of this flavour, takes 2 and 3 samples too: line and parabola)
  if (kt.axis_known) {
    rc = validate_transformation(c, n, u, tr, 2);
    regular_mesh = c->tcache.regular;
  } else
    rc = validate_common(c, n, u, tr, t_lo, t_hi, &regular_mesh, 2);
  if (rc) return rc;
  const bool short_series = n < 4;
  if (short_series && sh && !(sh->data_row0 == 0 && sh->data_rows == n && sh->col_parts <= 1))
    return fail(c, BMS_ERR_UNSUPPORTED, "a series of %lld samples cannot be sharded", (long long)n);
  if ((rc = refuse_sharded_graded_axis(c, regular_mesh, sh, n))) return rc;
  if (ell_max < 0 || tr->ell_max_out < 0) return fail(c, BMS_ERR_INVALID, "bad ell_max");
  if (ell_max > MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "ell_max = %d is beyond %d", ell_max, MAX_ELL);
  static const int spins[6] = {2, 1, 0, -1, -2, 2};  // psi0..psi4, sigma
  const int nm = (ell_max + 1) * (ell_max + 1);
  const int n_out = (tr->ell_max_out + 1) * (tr->ell_max_out + 1);
  const int lst = tr->ell_max_supertranslation;
  const cplx* st = (const cplx*)tr->supertranslation;

  // ---- per-pixel tables on the GPU (transformations.py:306-321), output window on the host (:391-396)
  hipStream_t S = c->stream;
  std::vector<cplx> c1((size_t)(lst + 1) * (lst + 1)), c2((size_t)(lst + 1) * (lst + 1));
  for (int l = 0; l <= lst; ++l)
    for (int m = -l; m <= l; ++m) {
      const cplx a = st[LM_index(l, m, 0)];
      const double f1 = std::sqrt((double)l * (l + 1.0)) / std::sqrt(2.0);                                          // eth alpha / sqrt2
      const double f2 = 0.5 * (std::sqrt((double)l * (l + 1.0)) * (l >= 1 ? std::sqrt((l - 1.0) * (l + 2.0)) : 0.0));  // eth eth alpha / 2
      c1[LM_index(l, m, 0)] = {f1 * a.re, f1 * a.im};
      c2[LM_index(l, m, 0)] = {f2 * a.re, f2 * a.im};
    }
  const double* v = tr->boost_velocity;
  const cplx cv[4] = {{0, 0},
                      {v[0] * std::sqrt(2 * M_PI / 3), v[1] * std::sqrt(2 * M_PI / 3)},
                      {v[2] * std::sqrt(4 * M_PI / 3), 0},
                      {-v[0] * std::sqrt(2 * M_PI / 3), v[1] * std::sqrt(2 * M_PI / 3)}};
  // Without a boost (every supertranslation and rotation step of map_to_superrest_frame, map_to_superrest_frame.py:443,610,641)
  // the six dense products give way to the separable synthesis on the rotated modes (kernels_synthesis_large.hip).
  // A boost along the polar axis of the rotated grid keeps the rings (separable_rotor_grid): the same synthesis at the aberrated
  // colatitudes; the mixing is time dependent then and stays on the grid.
  SynthesisPlan syn5[5];
  const bool no_boost = v[0] == 0 && v[1] == 0 && v[2] == 0;
  std::vector<double> ring_theta;
  bool sep = !(sh && sh->col_parts > 1) && tr->n_theta >= 3 && !c->opt.on(OPT_NO_SEPARABLE_SYNTHESIS) &&
             (no_boost || (axis_boost_pays(c, (ell_max + 1) * (ell_max + 1), tr->n_theta, tr->n_phi) &&
                           large_synthesis_route(c, tr->n_theta, tr->n_phi, 0, ell_max) && separable_rotor_grid(c, tr, ring_theta)));
  for (int si = 0; si < 5 && sep; ++si) {
    if ((rc = build_synthesis(c, tr->n_theta, tr->n_phi, si - 2, 0, ell_max, syn5[si], no_boost ? nullptr : &ring_theta))) return rc;
    sep = syn5[si].large;
  }
  PixelTables T;
  DevPixel DP;
  // (pieces of a pipelined call share the per-direction tables and the knot tables of the whole series)
  PieceTables* shared = c->async_pieces ? static_cast<PieceTables*>(c->piece_tables) : nullptr;
  if (shared && c->piece_tables_valid) {
    T = shared->T;
    DP = shared->DP;
  } else {
    if ((rc = device_pixel_tables(c, tr, T, 2, 0, 0, &c1, &c2, cv, DP, sep ? 0 : column_plan(c, tr, n_out), nullptr, nullptr, nullptr, reuse_tag(sh)))) return rc;
    if (shared) {
      shared->T = T;
      shared->DP = DP;
      c->piece_tables_valid = true;
    }
  }
  const int n_cols = T.n_pix;
  const bool col_split = sh && sh->col_parts > 1;
  int cA, cB;
  if ((rc = column_range(c, sh, n_cols, cA, cB))) return rc;
  const int n_pix = cB - cA;  // columns this call synthesises and splines
  // window: timeprime = (u - tt) / gamma  (division, unlike the WaveformModes flavour)
  int64_t i_lo, i_hi;
  if (!cached_window(c, true, i_lo, i_hi)) {
    output_window_abd(T, u, n, i_lo, i_hi);
    keep_window(c, true, i_lo, i_hi);
  }
  // the shard's share of the window, and the rows of the global series it was given
  int64_t row0 = 0, rows_avail = n, fs_out = n;
  if (sh) {
    row0 = sh->data_row0;
    rows_avail = sh->data_rows;
    if (row0 < 0 || rows_avail < 0 || row0 + rows_avail > n || sh->out_i1 < sh->out_i0) return fail(c, BMS_ERR_INVALID, "bad shard description");
    i_lo = std::max(i_lo, sh->out_i0);
    i_hi = std::max(i_lo, std::min(i_hi, sh->out_i1));
    fs_out = sh->out_i1 - sh->out_i0;
  }
  const int64_t n_new = i_hi - i_lo;
  *n_times_out = n_new;
  if (first_index_out) *first_index_out = i_lo;
  for (int64_t i = 0; i < n_new; ++i) u_out[i] = (u[i_lo + i] - T.tt) / T.gamma;
  if (n_new == 0) return BMS_OK;
  double *d_rot = DP.rotors, *d_skewa = DP.skew_a + cA, *d_skewb = DP.skew_b + cA, *d_alpha = DP.alpha + cA, *d_ethk = DP.ethk + 2 * cA,
         *d_etha = DP.etha + 2 * cA, *d_ethetha = DP.ethetha + 2 * cA, *d_ik = DP.ik + cA, *d_ik3 = DP.ik3 + cA;
  // the Horner mixing has time-dependent coefficients, so the elimination stays on the grid; the B-spline form still saves
  // the back substitution its second input stream (kernels_bspline.hip)
  const bool bsg = n >= 8 && regular_mesh && !c->opt.on(OPT_NO_BSPLINE);
  if (short_series) {
    void* vp;
    if ((rc = upload(c, "times", u, 8 * (size_t)n, &vp))) return rc;
    kt.d_x = (double*)vp;
  } else if ((rc = knot_tables_of_call(c, u, n, t_lo, t_hi, row0, rows_avail, bsg, shared, kt)))
    return rc;

  const long long P2 = 2LL * n_pix, ldg = round_up(P2, 16), ldb = round_up(2LL * n_cols, 128);
  const int K = 2 * nm;
  const long long brows = round_up(K, 16);
  // five distinct spins: matrices / analysis plans indexed by spin + 2
  double *d_B[5], *d_At[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  long long ld_at = 0;
  AnalysisPlan ana[5];
  // sigma' = (sigma - eth eth alpha) / k mixes with nothing and its offset and scale do not depend on time: it takes the evaluating
  // product of the WaveformModes route (its spline solved on the modes, evaluated in the product's epilogue, kernels_gemm_eval.hip) and
  // stays out of the mixing + elimination pass and of the back substitution -- two of the four passes over its grid
  const bool sigma_eval = !sep && bsg && !short_series && rows_avail >= 8 && !c->opt.on(OPT_NO_ABD_SIGMA_EVAL);
  // the five synthesis matrices are built from the per-direction tables alone: kept with them, in blocks of their own names (PixelCache)
  PixelCache& pc = c->pcache;
  const bool keep_B = !sep && pc.in_use && sizeof(double) * (size_t)brows * ldb <= SETUP_CACHE_MAX_BYTES;
  const bool have_B = keep_B && pc.B5_valid && pc.B5_ell_max == ell_max && pc.B5_cols == n_cols && pc.B5_sigma == sigma_eval;
  if (keep_B && !have_B) pc.B5_valid = false;
  for (int si = 0; si < 5; ++si) {
    char nm1[32], tag[16];
    snprintf(nm1, sizeof nm1, keep_B ? "pc_abd_B%d" : "abd_B%d", si);
    snprintf(tag, sizeof tag, "abd%d", si);
    if (!sep && have_B) {
      d_B[si] = pc.d_B5[si];
    } else if (!sep) {
      if ((rc = dev_buf_t(c, nm1, (size_t)brows * ldb, &d_B[si]))) return rc;
      HIP_TRY(c, hipMemsetAsync(d_B[si], 0, sizeof(double) * brows * ldb, S));
      TIMED(c, BMS_TAG_SETUP, launch_swsh_matrix_complex(S, d_rot, n_cols, si - 2, 0, ell_max, d_B[si], ldb));
    }
    if ((rc = build_analysis(c, tag, T.n_theta, T.n_phi, si - 2, 0, tr->ell_max_out, ana[si]))) return rc;
    if (col_split && n_pix > 0) {
      snprintf(nm1, sizeof nm1, "abd_At%d", si);
      if ((rc = part_analysis_matrix(c, ana[si], nm1, n_cols, DP.col_of_pixel, &d_At[si], &ld_at))) return rc;
    }
  }

  const long long ldG = (!col_split && analysis_reads_contiguous_rows(ana[2])) ? P2 : ldg;  // row stride of the evaluated grids
  const double* d_raw;
  if ((rc = stage_in(c, "in_data", raw, mem, (size_t)6 * rows_avail * nm * 16, &d_raw))) return rc;
  double* d_out = (double*)raw_out;
  if (mem == BMS_HOST)
    if ((rc = dev_buf_t(c, "out_data", (size_t)6 * fs_out * n_out * 2, &d_out))) return rc;
  // Without a boost the Horner mixing has time-independent coefficients (k = 1, eth k = 0: X = -eth alpha), so it commutes with the
  // spline's forward elimination: that runs on the MODES (6 x (l_max+1)^2 columns + the constant series, instead of six grids), the
  // fields are synthesised as eliminated coefficients and mixed on their way out of the phi stage (phi_synthesis_mix6_kernel)
  const bool fused_mix = sep && no_boost && bsg && !short_series && !c->opt.on(OPT_NO_FUSED_ABD_MIX) && large_synthesis_route(c, tr->n_theta, tr->n_phi, 0, ell_max) &&
                         abd_mix6_supported(tr->n_theta, tr->n_phi, ell_max);
  const long long ld_af = round_up(2LL * (nm + 1), 16);
  double* d_Af = nullptr;
  if (fused_mix) {
    if ((rc = dev_buf_t(c, "abd_Af", (size_t)6 * rows_avail * ld_af, &d_Af))) return rc;
    for (int f = 0; f < 6; ++f)
      TIMED(c, BMS_TAG_SPLINE_FORWARD, launch_bspline_forward_modes(S, d_raw + (size_t)f * rows_avail * nm * 2, 2LL * nm, nm, d_Af + (size_t)f * rows_avail * ld_af,
                                                                    ld_af, row0, rows_avail, n, kt.d_bsfwd, SPLINE_TILE, SPLINE_HALO, 1));
    if ((rc = rotate_into_grid_frame(c, tr, d_Af, 6 * rows_avail, ld_af / 2, 0, ell_max))) return rc;  // (the constant column stays)
  } else if (sep) {
    // the six fields as seen from the rotated frame, sYlm(F G) = sum_m' D_{m m'}(F) sYlm'(G): [6][rows][nm] is one series of
    // 6 x rows steps for the rotation kernel -- in place in the staging copy of a host caller, in a copy of device data
    if ((rc = rotated_input_in_grid_frame(c, tr, "abd_rot_in", mem, &d_raw, 6 * rows_avail, nm, 0, ell_max))) return rc;
  }

  if (n_pix == 0) {  // more parts than column tiles: this part contributes nothing
    for (int f = 0; f < 6; ++f) {
      if (mem == BMS_HOST)
        std::memset((char*)raw_out + (size_t)f * fs_out * n_out * 16, 0, (size_t)n_new * n_out * 16);
      else
        HIP_TRY(c, hipMemsetAsync(d_out + (size_t)f * fs_out * n_out * 2, 0, (size_t)n_new * n_out * 16, S));
    }
    HIP_TRY(c, hipStreamSynchronize(S));
    return BMS_OK;
  }

  double* d_As = nullptr;
  if (sigma_eval) {
    if ((rc = dev_buf_t(c, "abd_As", (size_t)rows_avail * ld_af, &d_As))) return rc;
    TIMED(c, BMS_TAG_SPLINE_FORWARD, launch_bspline_solve_modes(S, d_raw + (size_t)5 * rows_avail * nm * 2, 2LL * nm, nm, d_As, ld_af, row0, rows_avail,
                                                                kt.d_bsfwd, kt.d_bstab, 1));
    // row nm of the spin-2 harmonics (psi0 shares them and stops at row nm - 1) multiplies the solved constant series: -eth eth alpha.
    // Two invariants keep psi0's product, which shares the matrix, correct: the matrix has that row and the 8 rows a K chunk may read
    // past it (checked here), and launch_zgemm3m multiplies rows k >= K of B by ZERO-guarded A (kernels.h says so), because psi0's last
    // K chunk reads this now non-zero row.
    if (brows < (long long)nm + 1 + 8) return fail(c, BMS_ERR_HIP, "internal: the spin-2 matrix has %lld rows, sigma's offset row needs %d", brows, nm + 9);
    if (!have_B) TIMED(c, BMS_TAG_SETUP, launch_negated_row(S, DP.ethetha, d_B[4] + (size_t)nm * ldb, 2 * n_cols));
  }
  if (keep_B && !have_B) {
    pc.B5_valid = true, pc.B5_sigma = sigma_eval, pc.B5_ell_max = ell_max, pc.B5_cols = n_cols;
    for (int si = 0; si < 5; ++si) pc.d_B5[si] = d_B[si];
  }

  // ---- chunk loop: 6 fields x (Y, R, G)
  BsplineSpread spread = skew_spread(T, cA, cB, u);
  spread.launches = c->bwd_launches;
  const double bytes_per_row = 19.0 * ldg * 8.0;  // 6 x (Y, R, G) + F
  ChunkPlan plan;
  if ((rc = plan_chunks(c, c->ws_limit, bytes_per_row, n_new, regular_mesh, n, "six ", n_cols, plan))) return rc;
  for (int64_t c0 = i_lo; c0 < i_hi; c0 += plan.chunk) {
    const int64_t c1_ = std::min<int64_t>(c0 + plan.chunk, i_hi);
    int64_t g0, g1;
    if ((rc = chunk_rows(c, T, u, n, regular_mesh, c0, c1_, row0, rows_avail, g0, g1))) return rc;
    const int64_t rows_in = g1 - g0, rows_out = c1_ - c0;
    double *d_Y = nullptr, *d_R, *d_G;
    if (!fused_mix)
      if ((rc = dev_buf_t(c, "Y", (size_t)6 * rows_in * ldg, &d_Y))) return rc;
    if ((rc = dev_buf_t(c, "R", (size_t)6 * rows_in * ldg, &d_R))) return rc;
    if ((rc = dev_buf_t(c, "G", (size_t)6 * rows_out * ldG, &d_G))) return rc;
    AbdGrids grids;
    if (fused_mix) {
      const size_t f_stride = (size_t)rows_in * (2 * ell_max + 1) * large_analysis_jp(T.n_theta) * 2;
      double* d_F6;
      if ((rc = dev_buf_t(c, "Fsyn6", 6 * f_stride, &d_F6))) return rc;
      const double* F6[6];
      double* out6[6];
      for (int f = 0; f < 6; ++f) {
        F6[f] = d_F6 + f * f_stride;
        out6[f] = d_R + (size_t)f * rows_in * ldg;
        TIMED(c, BMS_TAG_GEMM_SYNTHESIS, launch_theta_synthesis(S, d_Af + ((size_t)f * rows_avail + (g0 - row0)) * ld_af, ld_af, rows_in, T.n_theta, 0, ell_max,
                                                                syn5[spins[f] + 2].d_T, d_F6 + f * f_stride));
      }
      TIMED(c, BMS_TAG_GEMM_SYNTHESIS, launch_phi_synthesis_mix6(S, F6, rows_in, T.n_theta, T.n_phi, ell_max, d_etha, d_ethetha,
                                                                 d_Af + (size_t)(g0 - row0) * ld_af + 2LL * nm, ld_af, out6, ldg));
    }
    for (int f = 0; f < 6 && !fused_mix; ++f) {
      grids.y[f] = d_Y + (size_t)f * rows_in * ldg;
      if (f == 5 && sigma_eval) continue;  // (straight to its samples, below)
      if (sep) {
        if ((rc = run_synthesis(c, syn5[spins[f] + 2], d_raw + ((size_t)f * rows_avail + (g0 - row0)) * nm * 2, 2LL * nm, rows_in, nullptr, grids.y[f], ldg)))
          return rc;
      } else
      {
        // (a field of spin weight s has no modes below l = |s|: the s^2 leading columns of its rows and the matching -- zero -- rows of
        // the harmonics stay out of the product; at l_max = 24 that is 78 instead of 79 k-chunks for five of the six fields)
        const int skip = spins[f] * spins[f] < nm ? spins[f] * spins[f] : 0;
        TIMED(c, BMS_TAG_GEMM_SYNTHESIS,
              launch_zgemm3m(S, d_raw + ((size_t)f * rows_avail + (g0 - row0)) * nm * 2 + 2 * skip, 2LL * nm, d_B[spins[f] + 2] + 2 * cA + (size_t)skip * ldb, ldb,
                             grids.y[f], ldg, rows_in, n_pix, K / 2 - skip, nullptr, nullptr));
      }
    }
    if (fused_mix) {
      // (synthesised, mixed and eliminated above)
    } else if (bsg) {  // mixing and elimination of the six fields in one pass over the grids
      AbdGrids elim;
      for (int f = 0; f < 6; ++f) elim.y[f] = d_R + (size_t)f * rows_in * ldg;
      TIMED(c, BMS_TAG_SPLINE_FORWARD, launch_abd_mix_forward(S, grids, elim, ldg, n_pix, g0, rows_in, kt.d_bsfwd, SPLINE_TILE, SPLINE_HALO, d_alpha, d_ethk,
                                                              d_etha, d_ethetha, d_ik, d_ik3, sigma_eval ? 5 : 6));
    } else {
      TIMED(c, BMS_TAG_POINTWISE,
            launch_abd_mix(S, grids, ldg, n_pix, rows_in, kt.d_x + g0, d_alpha, d_ethk, d_etha, d_ethetha, d_ik, d_ik3));
    }
    for (int f = 0; f < 6; ++f) {
      double* Rf = d_R + (size_t)f * rows_in * ldg;
      double* Gf = d_G + (size_t)f * rows_out * ldG;
      if (short_series) {
        TIMED(c, BMS_TAG_SPLINE_BACKWARD, launch_short_series_eval(S, grids.y[f], ldg, n_pix, (int)n, kt.d_x, kt.d_x, d_skewa, d_skewb, T.tt, c0, c1_, Gf, ldG));
      } else if (f == 5 && sigma_eval) {
        SplineEval ev;
        ev.skew_a = d_skewa, ev.skew_b = d_skewb;
        if ((rc = spline_eval_args(c, kt, T, cA, cB, u, n, g0, g1, c0, c1_, Gf, ldG, ldg, ev))) return rc;
        const int skip = 4 < nm ? 4 : 0;  // (spin 2: no modes below l = 2)
        TIMED(c, BMS_TAG_GEMM_SYNTHESIS, launch_zgemm3m_eval(S, d_As + (g0 - row0) * ld_af + 2 * skip, ld_af, d_B[4] + 2 * cA + (size_t)skip * ldb, ldb, rows_in,
                                                             n_pix, nm - skip + 1, DP.col_scale + 2 * cA, ev));
      } else if (bsg) {
        TIMED(c, BMS_TAG_SPLINE_BACKWARD, launch_bspline_backward_eval(S, Rf, ldg, n_pix, g0, rows_in, n, kt.d_x, kt.d_bstab, SPLINE_TILE, SPLINE_HALO,
                                                                       kt.d_x, d_skewa, d_skewb, T.tt, c0, c1_, Gf, ldG, c->n_cu, &spread));
      } else {
        TIMED(c, BMS_TAG_SPLINE_FORWARD,
              launch_spline_forward(S, grids.y[f], Rf, ldg, n_pix, g0, rows_in, n, kt.d_x, kt.d_tab, plan.spline_tile, SPLINE_HALO));
        TIMED(c, BMS_TAG_SPLINE_BACKWARD,
              launch_spline_backward_eval(S, grids.y[f], Rf, ldg, n_pix, g0, rows_in, n, kt.d_x, kt.d_tab, plan.spline_tile, SPLINE_HALO,
                                          kt.d_x, d_skewa, d_skewb, T.tt, c0, c1_, Gf, ldG));
      }
      double* out_f = d_out + ((size_t)f * fs_out + (c0 - i_lo)) * n_out * 2;
      if (col_split) {
        TIMED(c, BMS_TAG_GEMM_ANALYSIS, launch_zgemm3m(S, Gf, ldG, d_At[spins[f] + 2] + (size_t)cA * ld_at, ld_at, out_f, 2LL * n_out, rows_out, n_out, n_pix,
                                                       nullptr, nullptr));
      } else if ((rc = run_analysis(c, ana[spins[f] + 2], Gf, rows_out, out_f, 2LL * n_out, DP.col_of_pixel, ldG)))
        return rc;
    }
  }
  if (mem == BMS_HOST) {
    for (int f = 0; f < 6; ++f)
      HIP_TRY(c, hipMemcpyAsync((char*)raw_out + (size_t)f * fs_out * n_out * 16, d_out + (size_t)f * fs_out * n_out * 2,
                                (size_t)n_new * n_out * 16, hipMemcpyDeviceToHost, S));
  }
  time_axis_commit(c, kt.times_ahead, regular_mesh);  // (the walk covered the kept entry's range exactly when it was asked for ahead)
  if (!c->async_pieces) HIP_TRY(c, hipStreamSynchronize(S));  // (a piece of a pipelined call returns without waiting)
  return BMS_OK;
}

// AsymptoticBondiData.transform with host arrays in and out, as the three-stage pipeline of bms_transform_modes_pipelined: the
// rows (+ halo) of the six fields of shard k + 1 travel up, the kernels of shard k run and the results of shard k - 1 travel
// down at the same time.  raw: host c16[6][n][(ell_max+1)^2]; raw_out: host c16[6][i_hi - i_lo][n_out] (best page-locked).
extern "C" int bms_transform_abd_pipelined(bms_ctx* c, const double* u, const void* raw, int64_t n, int ell_max,
                                           const bms_transformation* tr, int pieces, double* u_out, void* raw_out, int64_t* n_times_out) try {
  return bms_transform_abd_pipelined_part(c, u, raw, n, ell_max, tr, pieces, 0, pieces < 1 ? 1 : pieces, u_out, raw_out, n_times_out);
} BMS_CATCH(c)

// Pieces [piece0, piece1) of the same plan (see bms_transform_modes_pipelined_part): u_out / raw_out are the arrays of the whole window.
extern "C" int bms_transform_abd_pipelined_part(bms_ctx* c, const double* u, const void* raw, int64_t n, int ell_max, const bms_transformation* tr,
                                                int pieces, int piece0, int piece1, double* u_out, void* raw_out, int64_t* n_times_out) try {
  if (!c) return BMS_ERR_INVALID;
  if (!u || !raw || !tr || !u_out || !raw_out || !n_times_out) return fail(c, BMS_ERR_INVALID, "NULL argument");
  HIP_TRY(c, hipSetDevice(c->device));
  bool regular = true;
  int rc = validate_common(c, n, u, tr, 0, n, &regular);
  if (rc) return rc;
  if (!regular) return fail(c, BMS_ERR_UNSUPPORTED, "the time steps vary by more than 1e3 within 48 samples: not sharded");
  if (ell_max < 0 || tr->ell_max_out < 0) return fail(c, BMS_ERR_INVALID, "bad ell_max");
  if (ell_max > MAX_ELL) return fail(c, BMS_ERR_UNSUPPORTED, "ell_max = %d is beyond %d", ell_max, MAX_ELL);
  PixelTables T;
  int64_t i_lo, i_hi;
  if ((rc = tables_and_window(c, tr, u, n, true, T, i_lo, i_hi))) return rc;
  *n_times_out = i_hi - i_lo;
  PiecePlan P;
  plan_pieces(T, u, n, i_lo, i_hi, pieces, piece0, piece1, P);
  if (P.p1 <= P.p0) return BMS_OK;
  const int64_t n_new = i_hi - i_lo;
  const int64_t nm = (int64_t)(ell_max + 1) * (ell_max + 1), n_out = (int64_t)(tr->ell_max_out + 1) * (tr->ell_max_out + 1);
  double *d_in[2], *d_out[2];
  if ((rc = dev_buf_t(c, "pipe_in0", (size_t)6 * P.max_rows * nm * 2, &d_in[0]))) return rc;
  if ((rc = dev_buf_t(c, "pipe_in1", (size_t)6 * P.max_rows * nm * 2, &d_in[1]))) return rc;
  if ((rc = dev_buf_t(c, "pipe_out0", (size_t)6 * P.max_out * n_out * 2, &d_out[0]))) return rc;
  if ((rc = dev_buf_t(c, "pipe_out1", (size_t)6 * P.max_out * n_out * 2, &d_out[1]))) return rc;
  SharedPieceTables shared(c);
  return run_host_pipeline(
      c, P.p0, P.p1, false, true, "pipelined upload", "pipelined transfer",
      [&](int k, int slot) {  // the six fields' rows [r0, r1) -> c16[6][rows][nm]
        const int64_t rows = P.r1[k] - P.r0[k];
        hipError_t e = hipSuccess;
        for (int f = 0; f < 6 && e == hipSuccess; ++f)
          e = hipMemcpyAsync(d_in[slot] + (size_t)f * rows * nm * 2, (const char*)raw + ((size_t)f * n + P.r0[k]) * nm * 16, (size_t)rows * nm * 16,
                             hipMemcpyHostToDevice, c->pipe_up);
        return e;
      },
      [&](int k, int slot) {
        const bms_shard sh = P.shard(k);
        int64_t got = 0, first = 0;
        const int rc2 = transform_abd_impl(c, u, d_in[slot], BMS_DEVICE, n, ell_max, tr, &sh, u_out + (P.cut[k] - i_lo), d_out[slot], &got, &first);
        return rc2 ? rc2 : piece_produced(c, P, k, got, first);
      },
      [&](int k, int slot) {
        const int64_t got = P.rows_out(k);
        hipError_t e = hipSuccess;
        for (int f = 0; f < 6 && e == hipSuccess; ++f)
          e = hipMemcpyAsync((char*)raw_out + ((size_t)f * n_new + (P.cut[k] - i_lo)) * n_out * 16, d_out[slot] + (size_t)f * got * n_out * 2,
                             (size_t)got * n_out * 16, hipMemcpyDeviceToHost, c->pipe_down);
        return e;
      });
} BMS_CATCH(c)

// the six fields over several contexts of one process (see bms_transform_modes_multi)
extern "C" int bms_transform_abd_multi(bms_ctx* const* ctxs, int n_ctx, const double* u, const void* raw, int64_t n, int ell_max,
                                       const bms_transformation* tr, int pieces, double* u_out, void* raw_out, int64_t* n_times_out) try {
  return run_dealt_over_contexts(ctxs, n_ctx, pieces, n_times_out, [&](bms_ctx* c, int p0, int p1, int64_t* got) {
    return bms_transform_abd_pipelined_part(c, u, raw, n, ell_max, tr, pieces < 1 ? 1 : pieces, p0, p1, u_out, raw_out, got);
  });
} BMS_CATCH(ctxs && n_ctx > 0 ? ctxs[0] : nullptr)

extern "C" int bms_transform_abd(bms_ctx* c, const double* u, const void* raw, int mem, int64_t n_times, int ell_max,
                                 const bms_transformation* tr, double* u_out, void* raw_out, int64_t* n_times_out) try {
  return bms_transform_abd_shard(c, u, raw, mem, n_times, ell_max, tr, nullptr, u_out, raw_out, n_times_out, nullptr);
} BMS_CATCH(c)
