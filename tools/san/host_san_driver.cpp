// Host-side sanitizer run (no GPU sanitizer exists on this pool: ASan / UBSan cover what runs on the host).
// `make -C scri_amd/csrc SAN=1` compiles this file -- which INCLUDES the host side of the engine (engine_*.hip, split by entry family
// behind engine.h), so that every planning helper is instrumented -- host-only with -fsanitize=address,undefined and runs it: shard plans, output windows, knot ranges, column
// parts, the chunk planner of the two transforms (plan_chunks, chunk_rows: caps that give 1, 2, 7 and several hundred chunks, the caps and shards it refuses), the pieces of the
// pipelined calls, rotor / harmonic / conformal tables, the frame integrator, the argument checks of the device frame chain, of the rotor interpolation and of the alignment entries, the planner and the per-step
// math of the precessing sample waveform, the argument checks, column tables and pieces of the paired-XOR storage entries, the argument checks of the centre-of-mass entries, the refusals of bms_dense_product and of the two dense-product launchers, the coefficient tables of the fused fluxes and the walk over a list of triplets, the inputs the Bondi-gauge violations asked for read and what their entry refuses, the prologues of the entries that stage host or device arguments (entry_mem, CallIO), over the five BASELINE shapes, 1..8 shards, 1..8 column parts, series of 2..9 samples and odd grids.  Nothing here touches a device.
#include "../../scri_amd/csrc/engine_context.hip"
#include "../../scri_amd/csrc/engine_tables.hip"
#include "../../scri_amd/csrc/engine_rotate.hip"
#include "../../scri_amd/csrc/engine_modes.hip"
#include "../../scri_amd/csrc/engine_abd.hip"
#include "../../scri_amd/csrc/engine_blocks.hip"
#include "../../scri_amd/csrc/engine_frames.hip"
#include "../../scri_amd/csrc/engine_align.hip"
#include "../../scri_amd/csrc/engine_sample.hip"
#include "../../scri_amd/csrc/engine_com.hip"
#include "../../scri_amd/csrc/engine_flux.hip"
#include "../../scri_amd/csrc/engine_product.hip"

#include <cstdio>
#include <random>

namespace {

struct Shape {
  const char* name;
  int ell_max, n_theta, n_phi, lst;
  long long n;
  double dt, boost_scale;
  bool abd;
};

int g_checks = 0;
#define REQUIRE(cond)                                                          \
  do {                                                                         \
    ++g_checks;                                                                \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      std::exit(2);                                                            \
    }                                                                          \
  } while (0)

void fill_transformation(bms_transformation& tr, std::vector<cplx>& st, const Shape& s) {
  st.assign((size_t)(s.lst + 1) * (s.lst + 1), cplx{0, 0});
  // a real supertranslation: alpha_{l,-m} = (-1)^m conj(alpha_{l,m})
  std::mt19937_64 rng(7);
  std::normal_distribution<double> g(0.0, 1e-3);
  for (int l = 0; l <= s.lst; ++l) {
    st[LM_index(l, 0, 0)] = {g(rng), 0.0};
    for (int m = 1; m <= l; ++m) {
      const cplx a = {g(rng), g(rng)};
      const double sg = (m & 1) ? -1.0 : 1.0;
      st[LM_index(l, m, 0)] = a;
      st[LM_index(l, -m, 0)] = {sg * a.re, -sg * a.im};
    }
  }
  tr = bms_transformation{};
  tr.supertranslation = st.data();
  tr.ell_max_supertranslation = s.lst;
  const double q[4] = {1, 2, 3, 4};
  const double nq = std::sqrt(30.0);
  for (int i = 0; i < 4; ++i) tr.frame_rotation[i] = q[i] / nq;
  tr.boost_velocity[0] = 1e-4 * s.boost_scale, tr.boost_velocity[1] = 2e-4 * s.boost_scale, tr.boost_velocity[2] = 3e-4 * s.boost_scale;
  tr.n_theta = s.n_theta, tr.n_phi = s.n_phi;
  tr.ell_max_out = s.ell_max;
}

// The chunk loops of the two transforms (plan_chunks, chunk_rows of engine_tables.hip) under work-space caps that give 1, 2, 7 and several
// hundred chunks: the chunks tile the output window once and in order, and each reads rows inside the series that hold its outputs'
// knots.  (No chunk is shorter than 4 * ROW_MARGIN outputs, so "several hundred" -- at least 200 chunks -- is asserted for the series of
// 1e5 steps and more; cfg1's 2000 steps make 15 chunks of that least length, and the tiling checks hold for them all the same.)
// Then what the planner refuses: a cap below 4 * ROW_MARGIN rows, a graded axis in more than one chunk, a shard one row short.
void chunk_walk(const Shape& s, const bms_transformation& tr, const PixelTables& T, const double* t, int64_t i_lo, int64_t i_hi) {
  bms_ctx dummy;
  const int64_t n = s.n, n_new = i_hi - i_lo;
  REQUIRE(n_new > 8 * ROW_MARGIN);
  const double bytes_per_row = (s.abd ? 19.0 : 4.0) * (double)round_up(2LL * T.n_pix, 16) * 8.0;  // as the two implementations count them
  const char* how_many = s.abd ? "six " : "";
  auto cap_for = [&](int64_t rows) { return (uint64_t)(((double)rows + 4.0 * ROW_MARGIN + 0.5) * bytes_per_row); };
  ChunkPlan P;
  for (int want : {1, 2, 7, 300}) {
    const int64_t rows = std::max<int64_t>((n_new + want - 1) / want, 4 * ROW_MARGIN);  // (no chunk is shorter than 4 * ROW_MARGIN)
    REQUIRE(plan_chunks(&dummy, cap_for(rows), bytes_per_row, n_new, true, n, how_many, T.n_pix, P) == BMS_OK);
    REQUIRE(P.chunk == rows && P.spline_tile == SPLINE_TILE);
    int64_t covered = i_lo, count = 0;
    for (int64_t c0 = i_lo; c0 < i_hi; c0 += P.chunk, ++count) {
      const int64_t c1 = std::min<int64_t>(c0 + P.chunk, i_hi);
      REQUIRE(c0 == covered && c1 > c0);
      int64_t g0 = -1, g1 = -1, ja, jb;
      REQUIRE(chunk_rows(&dummy, T, t, n, true, c0, c1, 0, n, g0, g1) == BMS_OK);
      needed_knots(T, t, n, c0, c1, ja, jb);
      REQUIRE(0 <= g0 && g0 <= ja && jb < g1 && g1 <= n);
      covered = c1;
    }
    REQUIRE(covered == i_hi && count == (n_new + rows - 1) / rows);
    REQUIRE(count == want || (want == 300 && (n < 100000 || count >= 200)));
  }
  char text[96];
  std::snprintf(text, sizeof text, "fewer than %d rows of the %s%d-column grids", 8 * ROW_MARGIN, how_many, T.n_pix);
  REQUIRE(plan_chunks(&dummy, cap_for(4 * ROW_MARGIN - 1), bytes_per_row, n_new, true, n, how_many, T.n_pix, P) == BMS_ERR_NOMEM);
  REQUIRE(std::strstr(bms_last_error(&dummy), text) != nullptr);
  REQUIRE(plan_chunks(&dummy, 0, bytes_per_row, n_new, true, n, how_many, T.n_pix, P) == BMS_ERR_NOMEM);
  REQUIRE(plan_chunks(&dummy, cap_for(4 * ROW_MARGIN - 1), bytes_per_row, 100, true, n, how_many, T.n_pix, P) == BMS_OK && P.chunk == 100);  // (a window that fits)
  // a graded axis is one chunk over the whole series, or refused
  REQUIRE(plan_chunks(&dummy, cap_for(n_new - 1), bytes_per_row, n_new, false, n, how_many, T.n_pix, P) == BMS_ERR_UNSUPPORTED);
  REQUIRE(plan_chunks(&dummy, cap_for(n_new), bytes_per_row, n_new, false, n, how_many, T.n_pix, P) == BMS_OK);
  REQUIRE(P.chunk == n_new && P.spline_tile == n + 1);
  int64_t g0 = -1, g1 = -1;
  REQUIRE(chunk_rows(&dummy, T, t, n, false, i_lo, i_hi, 0, n, g0, g1) == BMS_OK && g0 == 0 && g1 == n);
  bms_shard whole = {0, n, i_lo, i_hi, 0, 0}, part = {1, n - 1, i_lo, i_hi, 0, 0};
  REQUIRE(refuse_sharded_graded_axis(&dummy, false, nullptr, n) == BMS_OK && refuse_sharded_graded_axis(&dummy, false, &whole, n) == BMS_OK);
  REQUIRE(refuse_sharded_graded_axis(&dummy, true, &part, n) == BMS_OK && refuse_sharded_graded_axis(&dummy, false, &part, n) == BMS_ERR_UNSUPPORTED);
  // a mid-series shard: the rows bms_shard_plan names are enough, one row less at either end is not
  const int64_t o0 = i_lo + n_new / 3, o1 = i_lo + 2 * n_new / 3;
  int64_t need[2], win[2];
  REQUIRE(bms_shard_plan(nullptr, t, n, &tr, o0, o1, need, win) == BMS_OK && 0 < need[0] && need[1] < n);
  REQUIRE(chunk_rows(&dummy, T, t, n, true, o0, o1, need[0], need[1] - need[0], g0, g1) == BMS_OK && g0 == need[0] && g1 == need[1]);
  REQUIRE(chunk_rows(&dummy, T, t, n, true, o0, o1, need[0] + 1, need[1] - need[0] - 1, g0, g1) == BMS_ERR_INVALID);
  REQUIRE(std::strstr(bms_last_error(&dummy), "halo too small (use bms_shard_plan)") != nullptr);
  REQUIRE(chunk_rows(&dummy, T, t, n, true, o0, o1, need[0], need[1] - need[0] - 1, g0, g1) == BMS_ERR_INVALID);
}

void run_shape(const Shape& s) {
  std::vector<cplx> st;
  bms_transformation tr;
  fill_transformation(tr, st, s);
  std::vector<double> t((size_t)s.n);
  for (long long i = 0; i < s.n; ++i) t[(size_t)i] = s.dt * (double)i;
  bms_ctx dummy;  // (never given a device: the helpers use it for error texts only)
  bool regular = false;
  REQUIRE(validate_common(&dummy, s.n, t.data(), &tr, 0, -1, &regular, s.abd ? 2 : 4) == BMS_OK);
  REQUIRE(regular);
  REQUIRE(spline_tile_for(t.data(), s.n) == SPLINE_TILE);
  PixelTables T;
  build_pixel_tables(&tr, T);
  REQUIRE(T.n_pix == s.n_theta * s.n_phi);
  int64_t i_lo, i_hi;
  if (s.abd)
    output_window_abd(T, t.data(), s.n, i_lo, i_hi);
  else
    output_window(T, t.data(), s.n, i_lo, i_hi);
  REQUIRE(0 <= i_lo && i_lo <= i_hi && i_hi <= s.n);
  for (int shards = 1; shards <= 8; ++shards) {
    int64_t covered = i_lo;
    for (int r = 0; r < shards; ++r) {
      const int64_t o0 = i_lo + (i_hi - i_lo) * r / shards, o1 = i_lo + (i_hi - i_lo) * (r + 1) / shards;
      int64_t need[2], win[2];
      REQUIRE(bms_shard_plan(nullptr, t.data(), s.n, &tr, o0, o1, need, win) == BMS_OK);
      REQUIRE(win[0] == i_lo || s.abd);  // (the planner computes the WaveformModes window; the ABD one differs by rounding of 1/gamma only)
      if (o1 > o0) {
        REQUIRE(0 <= need[0] && need[0] <= o0 && o1 <= need[1] && need[1] <= s.n);
        int64_t ja, jb;
        needed_knots(T, t.data(), s.n, o0, o1, ja, jb);
        REQUIRE(need[0] <= ja && jb < need[1]);
        // the window of time samples a shard uploads, the skew ranges of its column blocks and the search bound of the evaluation
        bms_shard sh = {need[0], need[1] - need[0], o0, o1, 0, 0};
        int64_t lo, hi;
        time_window(s.n, &sh, lo, hi);
        REQUIRE(lo <= need[0] && need[1] <= hi);
        const int n_cols = T.n_pix;
        for (int parts = 1; parts <= 8; ++parts)
          for (int part = 0; part < parts; ++part) {
            sh.col_part = part, sh.col_parts = parts;
            int cA, cB;
            REQUIRE(column_range(&dummy, &sh, n_cols, cA, cB) == BMS_OK);
            REQUIRE(0 <= cA && cA <= cB && cB <= n_cols);
            if (cB > cA) {
              const BsplineSpread sp = skew_spread(T, cA, cB, t.data());
              REQUIRE(sp.skew_rate_range >= 0 && sp.skew_offset_range >= 0);
              REQUIRE(eval_search_halfwidth(T, cA, cB, t.data(), need[0], need[1]) >= 0);
            }
          }
      }
      covered = o1;
    }
    REQUIRE(covered == i_hi);
  }
  // the pieces of the pipelined calls (plan_pieces) read the rows bms_shard_plan names for their output ranges
  for (int pieces : {1, 3, 10, 20}) {
    PiecePlan P;
    plan_pieces(T, t.data(), s.n, i_lo, i_hi, pieces, 0, pieces, P);
    if (i_hi == i_lo) {
      REQUIRE(P.p0 == P.p1);
      continue;
    }
    REQUIRE(1 <= P.pieces && P.pieces <= pieces && P.p0 == 0 && P.p1 == P.pieces);
    REQUIRE(P.cut[0] == i_lo && P.cut[P.pieces] == i_hi);
    int64_t max_rows = 0, max_out = 0;
    for (int k = 0; k < P.pieces; ++k) {
      REQUIRE(P.rows_out(k) >= 8 || P.pieces == 1);
      int64_t need[2], win[2];
      REQUIRE(bms_shard_plan(nullptr, t.data(), s.n, &tr, P.cut[k], P.cut[k + 1], need, win) == BMS_OK);
      REQUIRE((win[0] <= P.cut[k] && P.cut[k + 1] <= win[1]) || s.abd);  // (the ABD window differs by the rounding of 1/gamma only)
      if (win[0] <= P.cut[k] && P.cut[k + 1] <= win[1]) REQUIRE(need[0] == P.r0[k] && need[1] == P.r1[k]);
      max_rows = std::max(max_rows, P.r1[k] - P.r0[k]);
      max_out = std::max(max_out, P.rows_out(k));
    }
    REQUIRE(P.max_rows == max_rows && P.max_out == max_out);
  }
  chunk_walk(s, tr, T, t.data(), i_lo, i_hi);
  // rotor grid, harmonics, conformal factors of the (boosted, rotated) grid through the ctx = NULL building blocks
  std::vector<double> rot((size_t)4 * T.n_pix);
  REQUIRE(bms_rotor_grid(nullptr, tr.frame_rotation, tr.boost_velocity, s.n_theta, s.n_phi, rot.data()) == BMS_OK);
  const int lm = std::min(s.ell_max, 12), nm = LM_total_size(0, lm);
  std::vector<cplx> Y((size_t)T.n_pix * nm);
  for (int spin = -2; spin <= 2; spin += 2) REQUIRE(bms_swsh_grid(nullptr, rot.data(), T.n_pix, spin, 0, lm, Y.data()) == BMS_OK);
  std::vector<double> k(T.n_pix), ik(T.n_pix), ik3(T.n_pix);
  std::vector<cplx> ek(T.n_pix);
  REQUIRE(bms_conformal_factors(nullptr, tr.boost_velocity, rot.data(), T.n_pix, k.data(), ek.data(), ik.data(), ik3.data()) == BMS_OK);
  std::vector<double> th((size_t)s.n_theta);
  (void)bms_ring_colatitudes(tr.frame_rotation, tr.boost_velocity, s.n_theta, s.n_phi, th.data());
  const double vz[3] = {0, 0, 0.1}, id[4] = {1, 0, 0, 0};
  REQUIRE(bms_ring_colatitudes(id, vz, s.n_theta, s.n_phi, th.data()) == 1);  // a boost along the grid's axis keeps the rings
  std::vector<double> q;
  theta_quadrature_weights(s.n_theta, q);
  REQUIRE((int)q.size() == s.n_theta);
  std::printf("%-22s n=%lld grid %dx%d window [%lld, %lld)\n", s.name, s.n, s.n_theta, s.n_phi, (long long)i_lo, (long long)i_hi);
}

void short_series_and_odd_grids() {
  for (int n = 2; n <= 9; ++n)
    for (int grid : {3, 4, 5, 8, 9, 11}) {
      Shape s = {"short", 2, grid, grid + (grid & 1 ? 0 : 1), 1, n, 0.37, 10.0, n < 4};
      std::vector<cplx> st;
      bms_transformation tr;
      fill_transformation(tr, st, s);
      tr.ell_max_out = 1;
      std::vector<double> t((size_t)n);
      for (int i = 0; i < n; ++i) t[(size_t)i] = 0.37 * i + 0.01 * i * i;
      bms_ctx dummy;
      REQUIRE(validate_common(&dummy, n, t.data(), &tr, 0, -1, nullptr, 2) == BMS_OK);
      PixelTables T;
      build_pixel_tables(&tr, T);
      int64_t a, b;
      output_window(T, t.data(), n, a, b);
      output_window_abd(T, t.data(), n, a, b);
      REQUIRE(0 <= a && a <= b && b <= n);
      if (b > a) {
        int64_t ja, jb;
        needed_knots(T, t.data(), n, a, b, ja, jb);
        REQUIRE(0 <= ja && ja <= jb && jb <= n - 1);
      }
      if (n >= 4) {
        int64_t need[2], win[2];
        REQUIRE(bms_shard_plan(nullptr, t.data(), n, &tr, 0, n, need, win) == BMS_OK);
      }
    }
  // rejected inputs go through the error path (formatted messages)
  bms_ctx dummy;
  std::vector<cplx> st;
  bms_transformation tr;
  Shape s = {"bad", 2, 5, 5, 1, 4, 0.1, 1.0, false};
  fill_transformation(tr, st, s);
  double t_bad[4] = {0.0, 0.1, 0.1, 0.3};
  REQUIRE(validate_common(&dummy, 4, t_bad, &tr) != BMS_OK);
  REQUIRE(std::strlen(bms_last_error(&dummy)) > 0);
  tr.boost_velocity[0] = 2.0;
  double t_ok[4] = {0.0, 0.1, 0.2, 0.3};
  REQUIRE(validate_common(&dummy, 4, t_ok, &tr) != BMS_OK);
}

void frame_integration() {
  const int n = 400;
  std::vector<double> t(n), om(3 * n), R(4 * n);
  for (int i = 0; i < n; ++i) {
    t[i] = 0.05 * i + 1e-4 * i * i;
    om[3 * i] = 0.3 * std::sin(0.1 * t[i]), om[3 * i + 1] = 0.2, om[3 * i + 2] = 1.0 + 0.01 * t[i];
  }
  const double R0[4] = {1, 0, 0, 0};
  REQUIRE(bms_integrate_angular_velocity(nullptr, t.data(), n, om.data(), R0, 1e-12, R.data()) == BMS_OK);
  for (int i = 0; i < n; ++i) {
    const double nn = R[4 * i] * R[4 * i] + R[4 * i + 1] * R[4 * i + 1] + R[4 * i + 2] * R[4 * i + 2] + R[4 * i + 3] * R[4 * i + 3];
    REQUIRE(std::fabs(nn - 1) < 1e-12);
  }
  for (int ell : {0, 1, 2, 7, 16, 24}) {
    std::vector<double> D;
    delta_matrix<long double>(ell, D);
    REQUIRE((int)D.size() == (2 * ell + 1) * (2 * ell + 1));
  }
}

// The device frame chain (engine_frames.hip) refuses what it cannot run before it touches a device: no context, no arrays.
void frame_chain_arguments() {
  double t[4] = {0.0, 0.1, 0.2, 0.3}, v[16] = {0}, out[16];
  const double R0[4] = {1, 0, 0, 0}, z[3] = {0, 0, 1};
  REQUIRE(bms_frame_from_angular_velocity(nullptr, t, 4, v, BMS_HOST, R0, 1e-12, out) == BMS_ERR_INVALID);
  REQUIRE(bms_dominant_axis(nullptr, v, 1, BMS_HOST, z, 0, out) == BMS_ERR_INVALID);
  REQUIRE(bms_minimal_rotation(nullptr, t, 4, v, BMS_HOST, 3, out) == BMS_ERR_INVALID);
  REQUIRE(bms_rotor_angular_velocity(nullptr, t, 4, v, BMS_HOST, out) == BMS_ERR_INVALID);
  REQUIRE(bms_frame_adjust(nullptr, v, 4, BMS_HOST, nullptr, 0.0, nullptr, nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_corotating_frame(nullptr, t, 4, v, 1, 0, 0, BMS_HOST, R0, 1e-12, out, nullptr, nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_coprecessing_frame(nullptr, t, 4, v, 1, 0, 0, BMS_HOST, z, 0, 3, nullptr, nullptr, out) == BMS_ERR_INVALID);
  bms_ctx dummy;
  REQUIRE(check_time_axis(&dummy, t, 3) == BMS_ERR_UNSUPPORTED);
  t[2] = t[1];
  REQUIRE(check_time_axis(&dummy, t, 4) == BMS_ERR_INVALID);
  int nm = 0;
  REQUIRE(modes_checks(&dummy, 2, 8, 77, &nm) == BMS_OK && nm == 77);
  REQUIRE(modes_checks(&dummy, 2, 8, 76, &nm) == BMS_ERR_INVALID);
  REQUIRE(modes_checks(&dummy, 2, MAX_ELL + 1, 1 << 30, &nm) == BMS_ERR_UNSUPPORTED);
  // rotor interpolation: no context, then what squad_checks reads in the two host arrays (any order of the arguments is fine)
  double ts[4] = {0.0, 0.1, 0.25, 0.3}, u[3] = {0.27, -0.5, 0.1};
  REQUIRE(bms_squad(nullptr, ts, 4, v, BMS_HOST, u, 3, out) == BMS_ERR_INVALID);
  REQUIRE(squad_checks(&dummy, ts, 4, u, 3) == BMS_OK);
  REQUIRE(squad_checks(&dummy, ts, 2, u, 0) == BMS_OK);
  REQUIRE(squad_checks(&dummy, ts, 1, u, 3) == BMS_ERR_INVALID);
  REQUIRE(squad_checks(&dummy, ts, 0, u, 3) == BMS_ERR_INVALID);
  REQUIRE(squad_checks(&dummy, ts, 4, u, -1) == BMS_ERR_INVALID);
  u[1] = std::numeric_limits<double>::infinity();
  REQUIRE(squad_checks(&dummy, ts, 4, u, 3) == BMS_ERR_INVALID);
  REQUIRE(squad_checks(&dummy, ts, 4, u, 1) == BMS_OK);
  u[1] = -0.5, ts[3] = std::nan("");
  REQUIRE(squad_checks(&dummy, ts, 4, u, 3) == BMS_ERR_INVALID);
  ts[3] = ts[2];
  REQUIRE(squad_checks(&dummy, ts, 4, u, 3) == BMS_ERR_INVALID);
  REQUIRE(squad_checks(&dummy, ts, 3, u, 3) == BMS_OK);
}

// The alignment entries (engine_align.hip) do the same, and their checks of the host arrays run before anything is staged.
void alignment_arguments() {
  double ta[4] = {0.0, 0.1, 0.2, 0.3}, tw[2] = {0.1, 0.2}, w[2] = {0.05, 0.05}, v[16] = {0}, dts[2] = {0.0, 0.05}, out[16];
  const int32_t col[1] = {0}, slot[1] = {0};
  REQUIRE(bms_align_moments(nullptr, ta, 4, v, v, 1, col, tw, w, 2, v, 1, col, 1, slot, 1, BMS_HOST, dts, 2, 0, out) == BMS_ERR_INVALID);
  REQUIRE(bms_align_residual(nullptr, ta, 4, v, v, 1, col, tw, w, 2, v, 1, col, 1, slot, BMS_HOST, 0.0, 0.0, out) == BMS_ERR_INVALID);
  bms_ctx dummy;
  AlignHost h = {ta, 4, v, v, 1, col, tw, w, 2, v, 1, col, 1, BMS_HOST};
  REQUIRE(align_checks(&dummy, h) == BMS_OK);
  h.na = 3;
  REQUIRE(align_checks(&dummy, h) == BMS_ERR_INVALID);
  h.na = 4, h.nw = 1;
  REQUIRE(align_checks(&dummy, h) == BMS_ERR_INVALID);
  h.nw = 2, h.n_cols = 0;
  REQUIRE(align_checks(&dummy, h) == BMS_ERR_INVALID);
  h.n_cols = 1, h.ld_a = 0;
  REQUIRE(align_checks(&dummy, h) == BMS_ERR_INVALID);
  h.ld_a = 1, h.ya = nullptr;
  REQUIRE(align_checks(&dummy, h) == BMS_ERR_INVALID);
  h.ya = v, ta[2] = ta[1];
  REQUIRE(align_checks(&dummy, h) == BMS_ERR_INVALID);
}

// The precessing sample waveform (engine_sample.hip): the planner finds the steps the reference's argmin searches find (the expected
// values are numpy's argmin results for these parameters), refuses what cannot be run, and the per-step math of sample_math.h gives
// unit rotors and transitions inside their bounds.
void sample_waveform_plan() {
  struct Case {
    double t_0, t_1, dt, mass_ratio;
    long long n, i0, i1, im, ir;
  };
  const Case cases[] = {{-20.0, 400.0, 0.5, 2.0, 841, 625, 635, 640, 680},
                        {-20.0, 236.0, 1.0, 1.0, 257, 148, 153, 156, 176},
                        {-20.0, 300.0, 0.25, 0.5, 1281, 850, 870, 880, 960},
                        {-20.0, 20000.0, 0.1, 2.0, 200201, 199124, 199174, 199200, 199400}};
  bms_ctx dummy;
  const int ell_max = 3;
  std::vector<cplx> coef((size_t)LM_total_size(2, ell_max), cplx{0.25, -0.5});
  std::vector<double> power(coef.size(), 1.5);
  for (const Case& cs : cases) {
    std::vector<double> t((size_t)cs.n);
    for (long long i = 0; i < cs.n; ++i) t[(size_t)i] = cs.t_0 + (double)i * cs.dt;  // numpy.arange fills start + i * step
    bms_precessing_params p = {cs.mass_ratio, cs.t_1 - 100.0, 0.5, 0.0, 0.1, 0.0, 1, 1, coef.data(), power.data()};
    SamplePlan P;
    REQUIRE(plan_precessing(&dummy, t.data(), cs.n, ell_max, &p, P) == BMS_OK);
    REQUIRE(P.n == cs.n && P.i0 == cs.i0 && P.i1 == cs.i1 && P.im == cs.im && P.ir == cs.ir);
    REQUIRE(P.ia() == cs.im + 1 && P.ib() == cs.ir && P.tb0 == t[(size_t)cs.i0] && P.tr1 == t[(size_t)cs.ir]);
    REQUIRE(P.opening_dot == 2.0 * 0.5 / (t[(size_t)cs.ir] - t[0]) && P.nutation == 0.05);
    std::vector<SampleMode> modes;
    REQUIRE(sample_mode_table(&dummy, ell_max, &p, modes) == BMS_OK);
    REQUIRE((int)modes.size() == 12 && modes[0].twice_power == 3 && modes[0].sign_m == -1 && modes[2].sign_m == 0 && modes[4].sign_m == 1);
    double last = 0.0;
    for (long long i = 0; i < cs.n; i += std::max<long long>(1, cs.n / 997)) {
      const double ti = t[(size_t)i];
      const double rising = sample_transition(ti, P.tr0, P.tr1, 0.0, 1.0), falling = sample_transition(ti, P.tr0, P.tr1, 1.0, 0.0);
      REQUIRE(rising >= last && rising <= 1.0 && std::fabs(rising + falling - 1.0) < 1e-15);
      REQUIRE(sample_transition_slope(ti, P.tr0, P.tr1, 1.0, 0.0) <= 0.0);
      last = rising;
      double phi, om;
      sample_pn_phase(P, ti, phi, om);
      om = sample_omega(P, i, ti, om);
      REQUIRE(om > 0.0 && om <= SAMPLE_OMEGA_MERGER);
      REQUIRE(sample_ringdown(P, i, ti, rising) > 0.0);
      if (i >= P.i0) phi = -3.0;  // (the integrated phase is the device's)
      const Quat q = sample_frame(phi, 0.4 * falling, phi / 0.1 * falling, P.nutation * rising);
      const Quat r = qmul(sample_conj_sqrt(q), sample_conj_sqrt(q));
      REQUIRE(std::fabs(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z - 1.0) < 1e-14);
      REQUIRE(std::fabs(r.w - q.w) < 1e-14 && std::fabs(r.x + q.x) < 1e-14 && std::fabs(r.y + q.y) < 1e-14 && std::fabs(r.z + q.z) < 1e-14);
    }
  }
  // refused before anything is staged
  std::vector<double> t(400);
  for (int i = 0; i < 400; ++i) t[(size_t)i] = (double)i;
  bms_precessing_params good = {2.0, 299.0, 0.5, 0.0, 0.1, 0.0, 1, 1, coef.data(), power.data()};
  SamplePlan P;
  REQUIRE(plan_precessing(&dummy, t.data(), 400, ell_max, &good, P) == BMS_OK);
  REQUIRE(plan_precessing(&dummy, nullptr, 400, ell_max, &good, P) == BMS_ERR_INVALID);
  REQUIRE(plan_precessing(&dummy, t.data(), 400, ell_max, nullptr, P) == BMS_ERR_INVALID);
  REQUIRE(plan_precessing(&dummy, t.data(), 0, ell_max, &good, P) == BMS_ERR_INVALID);
  REQUIRE(plan_precessing(&dummy, t.data(), 23, ell_max, &good, P) == BMS_ERR_INVALID);
  REQUIRE(plan_precessing(&dummy, t.data(), 400, 1, &good, P) == BMS_ERR_INVALID);
  REQUIRE(plan_precessing(&dummy, t.data(), 400, MAX_ELL + 1, &good, P) == BMS_ERR_UNSUPPORTED);
  double bms_precessing_params::*const fields[] = {&bms_precessing_params::mass_ratio,        &bms_precessing_params::t_merger,
                                                   &bms_precessing_params::opening_angle,     &bms_precessing_params::opening_angle_dot,
                                                   &bms_precessing_params::relative_rate,     &bms_precessing_params::nutation_angle};
  for (auto field : fields) {
    bms_precessing_params bad = good;
    bad.derive_opening_angle_dot = bad.derive_nutation_angle = 0;
    bad.*field = std::nan("");
    REQUIRE(plan_precessing(&dummy, t.data(), 400, ell_max, &bad, P) == BMS_ERR_INVALID);
  }
  bms_precessing_params bad = good;
  bad.t_merger = 10.0;  // the merger is step 10
  REQUIRE(plan_precessing(&dummy, t.data(), 400, ell_max, &bad, P) == BMS_ERR_INVALID);
  bad.t_merger = -5.0;  // ... or before the first step
  REQUIRE(plan_precessing(&dummy, t.data(), 400, ell_max, &bad, P) == BMS_ERR_INVALID);
  bad.t_merger = 398.0;  // the ringdown transition has no room
  REQUIRE(plan_precessing(&dummy, t.data(), 400, ell_max, &bad, P) == BMS_ERR_UNSUPPORTED);
  bad = good, bad.coef = nullptr;
  REQUIRE(plan_precessing(&dummy, t.data(), 400, ell_max, &bad, P) == BMS_ERR_INVALID);
  t[200] = t[199];
  REQUIRE(plan_precessing(&dummy, t.data(), 400, ell_max, &good, P) == BMS_ERR_INVALID);
  power[3] = 1.25;
  std::vector<SampleMode> modes;
  REQUIRE(sample_mode_table(&dummy, ell_max, &good, modes) == BMS_ERR_INVALID);
  REQUIRE(bms_precessing_waveform(nullptr, t.data(), 400, ell_max, &good, 0, t.data(), 12, BMS_HOST, nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_radius_terms(nullptr, t.data(), 400, t.data(), 1, 1, 3, 1.0, 100.0, t.data(), 1, BMS_HOST) == BMS_ERR_INVALID);
}

// The slab the named work-space buffers are carved from (bms_ctx_reserve): random grow / release sequences against a brute-force
// picture of the address range -- regions never overlap, freed neighbours coalesce, what is free plus what is held is the slab.
void slab_allocator() {
  std::mt19937_64 rng(11);
  for (int round = 0; round < 40; ++round) {
    Slab sl;
    sl.cap = 1 << 20;
    sl.free[0] = sl.cap;
    struct Held {
      size_t off, len;
    };
    std::vector<Held> held;
    for (int step = 0; step < 400; ++step) {
      const bool take = held.empty() || (rng() % 3) != 0;
      if (take) {
        const size_t want = ((size_t)(rng() % 60000) + 1 + 255) & ~(size_t)255;
        size_t off = 0;
        if (sl.take(want, &off)) {
          REQUIRE(off + want <= sl.cap && off % 256 == 0);
          for (const Held& h : held) REQUIRE(off + want <= h.off || h.off + h.len <= off);
          held.push_back({off, want});
        } else {
          for (const auto& f : sl.free) REQUIRE(f.second < want);  // refused only if no hole is large enough
        }
      } else {
        const size_t i = rng() % held.size();
        sl.give(held[i].off, held[i].len);
        held.erase(held.begin() + i);
      }
      size_t free_total = 0, prev_end = (size_t)-1;
      for (const auto& f : sl.free) {
        REQUIRE(f.second > 0);
        REQUIRE(prev_end == (size_t)-1 || prev_end < f.first);  // sorted, and coalesced: no two holes touch
        prev_end = f.first + f.second;
        free_total += f.second;
      }
      size_t held_total = 0;
      for (const Held& h : held) held_total += h.len;
      REQUIRE(free_total + held_total == sl.cap);
    }
    for (const Held& h : held) sl.give(h.off, h.len);
    REQUIRE(sl.free.size() == 1 && sl.free.begin()->first == 0 && sl.free.begin()->second == sl.cap);
  }
}

// The corotating paired-XOR entries (engine_blocks.hip): what they refuse before a device is touched, the column tables and the pieces a
// host array goes through under work-space caps that give 1, 2 and several hundred pieces -- the pieces tile the series once, in order.
void paired_xor_arguments() {
  bms_ctx dummy;
  std::vector<cplx> modes(40 * 12);
  std::vector<uint64_t> words(40 * 24);
  int64_t bad = 5;
  REQUIRE(bms_pack_paired_xor(nullptr, modes.data(), 12, 40, 2, 3, BMS_HOST, 1e-10, words.data(), &bad) == BMS_ERR_INVALID);
  for (double tol : {0.0, -1e-10, std::nan(""), HUGE_VAL}) {
    REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 12, 40, 2, 3, BMS_HOST, tol, words.data(), &bad) == BMS_ERR_INVALID && bad == -1);
    REQUIRE(std::strstr(bms_last_error(&dummy), "tolerance") != nullptr);
  }
  REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 11, 40, 2, 3, BMS_HOST, 1e-10, words.data(), &bad) == BMS_ERR_INVALID);
  REQUIRE(std::strstr(bms_last_error(&dummy), "row stride 11") != nullptr);
  REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 12, 40, 3, 2, BMS_HOST, 1e-10, words.data(), nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 12, 40, 2, 3, 9, 1e-10, words.data(), nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 12, -1, 2, 3, BMS_HOST, 1e-10, words.data(), nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_pack_paired_xor(&dummy, nullptr, 12, 40, 2, 3, BMS_HOST, 1e-10, words.data(), nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 12, 40, 2, 3, BMS_HOST, 1e-10, &modes[39 * 12 + 11], nullptr) == BMS_ERR_INVALID);  // the last input value
  REQUIRE(std::strstr(bms_last_error(&dummy), "overlap") != nullptr);
  REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 12, 40, 2, 3, BMS_DEVICE, 1e-10, (char*)words.data() + 8, nullptr) == BMS_ERR_INVALID);  // alignment
  REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 12, 40, 2, MAX_ELL + 1, BMS_HOST, 1e-10, words.data(), nullptr) == BMS_ERR_UNSUPPORTED);
  REQUIRE(bms_pack_paired_xor(&dummy, modes.data(), 1 << 20, 40, 0, 100, BMS_HOST, 1e-10, words.data(), nullptr) == BMS_ERR_UNSUPPORTED);  // beyond the LDS
  REQUIRE(bms_pack_paired_xor(&dummy, nullptr, 12, 0, 2, 3, BMS_HOST, 1e-10, nullptr, &bad) == BMS_OK && bad == -1);  // an empty series
  REQUIRE(bms_unpack_paired_xor(nullptr, words.data(), 40, 2, 3, BMS_HOST, modes.data(), 12) == BMS_ERR_INVALID);
  REQUIRE(bms_unpack_paired_xor(&dummy, words.data(), 40, 2, 3, BMS_HOST, modes.data(), 11) == BMS_ERR_INVALID);
  REQUIRE(bms_unpack_paired_xor(&dummy, words.data(), 40, 2, 3, BMS_HOST, words.data() + 24, 12) == BMS_ERR_INVALID);
  REQUIRE(bms_unpack_paired_xor(&dummy, words.data(), 0, 2, 3, BMS_HOST, modes.data(), 12) == BMS_OK);
  REQUIRE(bms_paired_xor_tile_rows() == PAIRED_PACK_TILE);
  const int ranges[][2] = {{2, 2}, {2, 8}, {0, 16}, {0, 24}, {3, 40}};
  for (const auto& lr : ranges) {
    const int ell_min = lr[0], ell_max = lr[1];
    const int n_modes = (ell_max + 1) * (ell_max + 1) - ell_min * ell_min;
    const int64_t n = 100000;
    for (int want : {1, 2, 300}) {
      const int64_t rows = (n + want - 1) / want;
      dummy.ws_limit = (uint64_t)rows * 32ull * (uint64_t)n_modes + 7;
      PairedPlan P;
      // (nothing is read through the pointers: any two ranges apart do)
      REQUIRE(plan_paired_xor(&dummy, "test", (const void*)0x1000, n_modes + 2, (const void*)((uintptr_t)1 << 40), n, ell_min, ell_max, BMS_HOST, P) == BMS_OK);
      REQUIRE(P.n_modes == n_modes && (int)P.partner.size() == n_modes && P.piece_rows == rows);
      int64_t covered = 0, count = 0;
      for (int64_t p0 = 0; p0 < n; p0 += P.piece_rows, ++count) {
        REQUIRE(p0 == covered);
        covered = std::min<int64_t>(p0 + P.piece_rows, n);
      }
      REQUIRE(covered == n && count == (n + rows - 1) / rows && (count == want || want == 300));
      REQUIRE(plan_paired_xor(&dummy, "test", (const void*)0x1000, n_modes, (const void*)((uintptr_t)1 << 40), n, ell_min, ell_max, BMS_DEVICE, P) == BMS_OK && P.piece_rows == n);
      // the tables: the partner of the partner is the column itself, own columns are those not below their partner, each pair once
      int pairs = 0;
      for (int j = 0; j < n_modes; ++j) REQUIRE(P.partner[(size_t)j] >= 0 && P.partner[(size_t)j] < n_modes && P.partner[(size_t)P.partner[(size_t)j]] == j);
      for (int k = 0; k < P.n_own; ++k) {
        const int j = P.own[(size_t)k];
        REQUIRE(j >= P.partner[(size_t)j] && (k == 0 || P.own[(size_t)k - 1] < j));
        pairs += j == P.partner[(size_t)j] ? 1 : 2;
      }
      REQUIRE(pairs == n_modes && P.n_own == (n_modes + (ell_max - ell_min + 1)) / 2);
    }
    dummy.ws_limit = 1;  // a cap below one row: one row per piece, never none
    PairedPlan P;
    REQUIRE(plan_paired_xor(&dummy, "test", (const void*)0x1000, n_modes, (const void*)((uintptr_t)1 << 40), 10, ell_min, ell_max, BMS_HOST, P) == BMS_OK && P.piece_rows == 1);
  }
}

// The centre-of-mass entries (engine_com.hip): what they refuse before a device is touched.
void com_motion_arguments() {
  bms_ctx dummy;
  std::vector<double> t(9, 1.0), x(27, 2.0), m(9, 0.5), out(27);
  bms_com_fit_result res;
  REQUIRE(bms_com_fit(nullptr, t.data(), x.data(), 9, BMS_HOST, 0.01, 0.1, 0, &res) == BMS_ERR_INVALID);
  REQUIRE(bms_com_fit(&dummy, nullptr, x.data(), 9, BMS_HOST, 0.01, 0.1, 0, &res) == BMS_ERR_INVALID);
  REQUIRE(bms_com_fit(&dummy, t.data(), nullptr, 9, BMS_HOST, 0.01, 0.1, 0, &res) == BMS_ERR_INVALID);
  REQUIRE(bms_com_fit(&dummy, t.data(), x.data(), 9, BMS_HOST, 0.01, 0.1, 0, nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_com_fit(&dummy, t.data(), x.data(), 9, 5, 0.01, 0.1, 0, &res) == BMS_ERR_INVALID);
  for (int64_t n : {(int64_t)1, (int64_t)0, (int64_t)-3}) REQUIRE(bms_com_fit(&dummy, t.data(), x.data(), n, BMS_HOST, 0.01, 0.1, 1, &res) == BMS_ERR_INVALID);
  for (double f : {(double)std::nan(""), (double)HUGE_VAL}) {
    REQUIRE(bms_com_fit(&dummy, t.data(), x.data(), 9, BMS_HOST, f, 0.1, 0, &res) == BMS_ERR_INVALID);
    REQUIRE(bms_com_fit(&dummy, t.data(), x.data(), 9, BMS_HOST, 0.01, f, 0, &res) == BMS_ERR_INVALID);
  }
  REQUIRE(bms_com_motion(nullptr, t.data(), x.data(), x.data(), m.data(), 9, m.data(), 1, 9, 0, BMS_HOST, nullptr, out.data()) == BMS_ERR_INVALID);
  REQUIRE(bms_com_motion(&dummy, nullptr, nullptr, x.data(), m.data(), 9, m.data(), 1, 9, 0, BMS_HOST, nullptr, out.data()) == BMS_ERR_INVALID);
  REQUIRE(bms_com_motion(&dummy, nullptr, x.data(), x.data(), m.data(), 9, m.data(), 1, 9, 0, BMS_HOST, nullptr, nullptr) == BMS_ERR_INVALID);
  REQUIRE(bms_com_motion(&dummy, nullptr, x.data(), x.data(), m.data(), 9, m.data(), 1, 9, 1, BMS_HOST, nullptr, out.data()) == BMS_ERR_INVALID);  // matter needs t
  REQUIRE(bms_com_motion(&dummy, t.data(), x.data(), x.data(), m.data(), 9, m.data(), 1, 9, 1, BMS_HOST, nullptr, out.data()) == BMS_ERR_INVALID);  // ... and t_out
  REQUIRE(bms_com_motion(&dummy, t.data(), x.data(), x.data(), m.data(), 4, m.data(), 1, 9, 0, BMS_HOST, nullptr, out.data()) == BMS_ERR_INVALID);
  REQUIRE(bms_com_motion(&dummy, t.data(), x.data(), x.data(), m.data(), 9, m.data(), 0, 9, 0, BMS_HOST, nullptr, out.data()) == BMS_ERR_INVALID);
  REQUIRE(bms_com_motion(&dummy, t.data(), x.data(), x.data(), m.data(), 1, m.data(), 1, 0, 0, BMS_HOST, nullptr, out.data()) == BMS_ERR_INVALID);
  REQUIRE(bms_com_motion(&dummy, t.data(), x.data(), x.data(), m.data(), 9, m.data(), 9, 9, 0, 3, nullptr, out.data()) == BMS_ERR_INVALID);
  REQUIRE(bms_com_fit_tile_panels() == COM_FIT_TILE);
  REQUIRE(com_fit_work_doubles(2) == com_fit_work_doubles(3) && com_fit_work_doubles(2 * COM_FIT_TILE + 2) == com_fit_work_doubles(3));
  REQUIRE(com_fit_work_doubles(2 * COM_FIT_TILE + 3) == com_fit_work_doubles(3) + 18);  // one more tile of double-double partials
}

// The argument helper of the building blocks (engine.h: entry_mem, CallIO).  Per family that stands on it, the refusal of a bad `mem`
// in that family's words, ahead of the size checks that follow it, and where the device is selected only after those checks (mode map,
// centre of mass, alignment, paired XOR) one bad size behind a good `mem`; then the helper on device memory, where it hands the
// caller's pointers through and keeps at most MAX_BACK copies.  No call here gets as far as selecting a device.
void staged_argument_prologues() {
  bms_ctx dummy;
  alignas(16) static double v[64], out[64];
  double t[4] = {0.0, 0.1, 0.2, 0.3};
  const int32_t idx[1] = {0};
  auto says = [&](const char* text) { return std::strstr(bms_last_error(&dummy), text) != nullptr; };
  // engine_blocks.hip
  REQUIRE(bms_row_norm(&dummy, v, 1, -1, 1, 7, 0, out) == BMS_ERR_INVALID && says("mem is BMS_HOST or BMS_DEVICE, got 7") && !says("bms_"));
  REQUIRE(bms_cubic_spline(&dummy, t, 3, v, 1, 1, 7, t, 1, out) == BMS_ERR_INVALID && says("got 7"));
  REQUIRE(bms_spline_derivative(&dummy, t, 3, v, 1, 1, 7, t, 1, 9, out) == BMS_ERR_INVALID && says("got 7"));
  REQUIRE(bms_angular_velocity(&dummy, t, 3, v, 0, 0, 0, 7, out, out, out) == BMS_ERR_INVALID && says("got 7"));
  REQUIRE(bms_xor_timeseries(&dummy, v, 7, -1, 1, 0) == BMS_ERR_INVALID && says("got 7"));
  REQUIRE(bms_mode_map(&dummy, out, 1, 1, 1, v, 1, idx, v, 0, v, 1, nullptr, nullptr, 0, nullptr, 7) == BMS_ERR_INVALID && says("got 7"));
  dummy.err.clear();
  REQUIRE(bms_mode_map(&dummy, out, 1, 1, 1, v, 1, idx, v, 0, v, 1, nullptr, nullptr, 0, nullptr, BMS_HOST) == BMS_ERR_INVALID && dummy.err.empty());
  // engine_frames.hip
  REQUIRE(bms_squad(&dummy, t, 1, v, 7, t, -1, out) == BMS_ERR_INVALID && says("mem is BMS_HOST or BMS_DEVICE, got 7"));
  REQUIRE(bms_frame_adjust(&dummy, v, -1, 7, nullptr, 0.0, nullptr, nullptr) == BMS_ERR_INVALID && says("got 7"));
  REQUIRE(bms_minimal_rotation(&dummy, t, 3, v, 7, 0, out) == BMS_ERR_INVALID && says("got 7"));
  REQUIRE(bms_coprecessing_frame(&dummy, t, 0, v, 1, 0, 0, 7, t, 0, 0, nullptr, nullptr, out) == BMS_ERR_INVALID && says("got 7"));
  // engine_com.hip: the entry's name in front, and the size checks behind a good `mem`
  bms_com_fit_result res;
  REQUIRE(bms_com_fit(&dummy, t, v, 1, 5, 0.01, 0.1, 0, &res) == BMS_ERR_INVALID && says("bms_com_fit: mem is BMS_HOST or BMS_DEVICE, got 5"));
  REQUIRE(bms_com_fit(&dummy, t, v, 1, BMS_DEVICE, 0.01, 0.1, 0, &res) == BMS_ERR_INVALID && says("at least 2 samples"));
  REQUIRE(bms_com_motion(&dummy, t, v, v, v, 3, v, 1, 0, 0, 3, nullptr, out) == BMS_ERR_INVALID && says("bms_com_motion: mem is BMS_HOST or BMS_DEVICE, got 3"));
  REQUIRE(bms_com_motion(&dummy, t, v, v, v, 3, v, 1, 4, 0, BMS_DEVICE, nullptr, out) == BMS_ERR_INVALID && says("one per sample"));
  // engine_align.hip
  AlignHost h = {t, 4, v, v, 1, idx, t, t, 2, v, 1, idx, 0, 9};
  REQUIRE(align_checks(&dummy, h) == BMS_ERR_INVALID && says("mem is BMS_HOST or BMS_DEVICE, got 9"));
  h.mem = BMS_DEVICE;
  REQUIRE(align_checks(&dummy, h) == BMS_ERR_INVALID && says("at least one common column"));
  // the paired-XOR plan
  PairedPlan P;
  REQUIRE(plan_paired_xor(&dummy, "bms_pack_paired_xor", v, 1, out, -1, 0, 0, 7, P) == BMS_ERR_INVALID && says("bms_pack_paired_xor: mem is BMS_HOST or BMS_DEVICE, got 7"));
  REQUIRE(plan_paired_xor(&dummy, "bms_unpack_paired_xor", v, 1, out, -1, 0, 0, BMS_HOST, P) == BMS_ERR_INVALID && says("bms_unpack_paired_xor: negative n_times"));
  // the helper on device memory
  CallIO io(&dummy, BMS_DEVICE);
  const double* d_in = nullptr;
  double *d_out = nullptr, *d_io = nullptr;
  REQUIRE(io.in("in_data", v, 64, &d_in) == BMS_OK && d_in == v);
  REQUIRE(io.out("out_data", out, 8, &d_out) == BMS_OK && d_out == out);
  REQUIRE(io.out_rows("out_data", out, 2, 2, 4, &d_out) == BMS_OK && d_out == out);
  REQUIRE(io.inout("fr_in", out, out, 8, &d_io) == BMS_OK && d_io == out && io.n_back == 0);  // (one array: no copy, nothing to bring home)
  REQUIRE(io.copy_back(nullptr, v, 8) == BMS_OK && io.n_back == 0);                            // (an output nobody asked for)
  for (int k = 0; k < CallIO::MAX_BACK; ++k) REQUIRE(io.copy_back(out + k, v, 8) == BMS_OK);
  REQUIRE(io.copy_back(out, v, 8) == BMS_ERR_INVALID && io.n_back == CallIO::MAX_BACK);
  REQUIRE(!dummy.host_copy_queued);  // (nothing was queued on a stream: the destructor has nothing to wait for)
}

// bms_dense_product (engine_blocks.hip) and the two launchers behind it (kernels_gemm.hip): every refusal of include/scri_amd.h comes
// back before a device is touched or anything is launched, and an empty product is BMS_OK.  The arrays are never read.
void dense_product_arguments() {
  bms_ctx dummy;
  alignas(16) static double a[64], b[64], c[64], off[8];
  const int64_t M = 5, N = 70, K = 18;  // pitches of the complex forms: lda >= 36, ldb >= 256, ldc >= 140; real form: 18, 128, 70
  auto call = [&](int form, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t m, int64_t n, int64_t k,
                  const void* o = nullptr, const void* s = nullptr) { return bms_dense_product(&dummy, form, A, lda, B, ldb, C, ldc, m, n, k, o, s); };
  REQUIRE(bms_dense_product(nullptr, BMS_PRODUCT_COMPLEX, a, 36, b, 256, c, 140, M, N, K, nullptr, nullptr) == BMS_ERR_INVALID);
  for (int form : {BMS_PRODUCT_COMPLEX, BMS_PRODUCT_REAL, BMS_PRODUCT_COMPLEX_4M}) {
    const bool real = form == BMS_PRODUCT_REAL;
    const int64_t lda = real ? 18 : 36, ldb = real ? 128 : 256, ldc = real ? 70 : 140;
    REQUIRE(call(form, nullptr, lda, b, ldb, c, ldc, M, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, nullptr, ldb, c, ldc, M, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, b, ldb, nullptr, ldc, M, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, -1, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, M, -1, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, M, N, 0) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda - 2, b, ldb, c, ldc, M, N, K) == BMS_ERR_INVALID && std::strstr(bms_last_error(&dummy), "pitch") != nullptr);
    REQUIRE(call(form, a, lda, b, ldb - 2, c, ldc, M, N, K) == BMS_ERR_INVALID);  // below the PADDED width
    REQUIRE(call(form, a, lda, b, ldc, c, ldc, M, N, K) == BMS_ERR_INVALID);      // the unpadded width
    REQUIRE(call(form, a, lda, b, ldb, c, ldc - 2, M, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a + 1, lda, b, ldb, c, ldc, M, N, K) == BMS_ERR_INVALID && std::strstr(bms_last_error(&dummy), "aligned") != nullptr);
    REQUIRE(call(form, a, lda, b + 1, ldb, c, ldc, M, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda + 1, b, ldb, c, ldc, M, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, b, ldb + 1, c, ldc, M, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, b, ldb, (char*)c + 4, ldc, M, N, K) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, M, N, K, (char*)off + 4, nullptr) == BMS_ERR_INVALID);
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, M, N, K, nullptr, (char*)off + 4) == BMS_ERR_INVALID);
    if (real) {
      REQUIRE(call(form, a, lda, b, ldb, c, ldc, M, N, K - 1) == BMS_ERR_INVALID && std::strstr(bms_last_error(&dummy), "even K") != nullptr);
    } else {
      REQUIRE(call(form, a, lda, b, ldb, c + 1, ldc, M, N, K) == BMS_ERR_INVALID);
      REQUIRE(call(form, a, lda, b, ldb, c, ldc + 1, M, N, K) == BMS_ERR_INVALID);
    }
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, M, (int64_t)1 << 31, K) == BMS_ERR_UNSUPPORTED);
    REQUIRE(call(form, a, (int64_t)1 << 33, b, ldb, c, ldc, M, N, (int64_t)1 << 31) == BMS_ERR_UNSUPPORTED);
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, (int64_t)1 << 40, N, K) == BMS_ERR_UNSUPPORTED);  // more tiles than a grid holds
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, 0, N, K) == BMS_OK);
    REQUIRE(call(form, a, lda, b, ldb, c, ldc, M, 0, K) == BMS_OK);
  }
  for (int form : {-1, 3}) REQUIRE(call(form, a, 36, b, 256, c, 140, M, N, K) == BMS_ERR_INVALID && std::strstr(bms_last_error(&dummy), "form") != nullptr);
  // the launchers' own preconditions (kernels.h): what every internal caller is held to
  REQUIRE(launch_dgemm(nullptr, a, 18, b, 128, c, 70, M, 70, 17, nullptr, nullptr) == hipErrorInvalidValue);  // odd K
  REQUIRE(launch_dgemm(nullptr, a, 18, b, 128, c, 70, M, 70, 0, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_dgemm(nullptr, a + 1, 18, b, 128, c, 70, M, 70, 18, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_dgemm(nullptr, a, 19, b, 128, c, 70, M, 70, 18, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_dgemm(nullptr, a, 18, b, 129, c, 70, M, 70, 18, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_dgemm(nullptr, a, 18, b, 128, c, 70, 0, 70, 17, nullptr, nullptr) == hipSuccess);  // nothing to do
  REQUIRE(launch_zgemm3m(nullptr, a, 36, b, 256, c, 140, M, 70, 0, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_zgemm3m(nullptr, a + 1, 36, b, 256, c, 140, M, 70, 18, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_zgemm3m(nullptr, a, 36, b + 1, 256, c, 140, M, 70, 18, nullptr, nullptr, true) == hipErrorInvalidValue);
  REQUIRE(launch_zgemm3m(nullptr, a, 36, b, 256, c + 1, 140, M, 70, 18, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_zgemm3m(nullptr, a, 37, b, 256, c, 140, M, 70, 18, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_zgemm3m(nullptr, a, 36, b, 256, c, 141, M, 70, 18, nullptr, nullptr) == hipErrorInvalidValue);
  REQUIRE(launch_zgemm3m(nullptr, a, 36, b, 256, c, 140, M, 0, 18, nullptr, nullptr) == hipSuccess);
}

// The fused fluxes (engine_flux.hip): the coefficient image of four l ranges -- every neighbour outside the range is zero, the image of
// sin(theta) e^{+i phi} is the transpose of that of sin(theta) e^{-i phi} and cos(theta)'s is symmetric (real matrices of adjoint
// operators) -- the walk over a triplet list with an index out of range, and what the two entries refuse before they select a device.
void flux_tables_and_triplets() {
  const int ranges[][2] = {{2, 2}, {2, 3}, {3, 5}, {2, 16}};
  for (const auto& lr : ranges) {
    const int ell_min = lr[0], ell_max = lr[1], n = LM_total_size(ell_min, ell_max);
    std::vector<double> image;
    build_flux_image(ell_min, ell_max, image);
    REQUIRE((int)image.size() == flux_image_doubles(n) && (int)image.size() == 30 * n);
    for (int l = ell_min; l <= ell_max; ++l)
      for (int m = -l; m <= l; ++m) {
        const int c = LM_index(l, m, ell_min);
        REQUIRE(image[(size_t)29 * n + c] == l);
        REQUIRE(image[(size_t)27 * n + c] == std::sqrt((double)((l - m) * (l + m + 1))) && image[(size_t)28 * n + c] == std::sqrt((double)((l + m) * (l - m + 1))));
        for (int dl = -1; dl <= 1; ++dl)
          for (int mu = -1; mu <= 1; ++mu) {
            const int lp = l + dl, k = 3 * (dl + 1) + (mu + 1);
            const bool inside = lp >= ell_min && lp <= ell_max && std::abs(m + mu) <= lp;
            for (int set = 0; set < 3; ++set) REQUIRE(std::isfinite(image[(size_t)(3 * k + set) * n + c]) && (inside || image[(size_t)(3 * k + set) * n + c] == 0.0));
            if (!inside) continue;
            const int r = LM_index(lp, m + mu, ell_min), back = 3 * (-dl + 1) + (-mu + 1);
            REQUIRE(r >= 0 && r < n);
            REQUIRE(std::fabs(image[(size_t)(3 * k) * n + c] - image[(size_t)(3 * back) * n + r]) <= 4e-16);
          }
      }
  }
  const int32_t rows[5] = {0, 3, 4, 2, 1}, cols[5] = {4, 0, 1, 5, 2}, low[3] = {0, -1, 2};
  REQUIRE(first_bad_triplet(rows, cols, 5, 6) == -1 && first_bad_triplet(rows, cols, 5, 5) == 3 && first_bad_triplet(rows, cols, 3, 5) == -1);
  REQUIRE(first_bad_triplet(low, cols, 3, 6) == 1 && first_bad_triplet(rows, low, 3, 6) == 1 && first_bad_triplet(rows, cols, 0, 1) == -1);
  bms_ctx dummy;
  alignas(16) static double v[64], out[64];
  double t[4] = {0.0, 0.1, 0.2, 0.3};
  auto says = [&](const char* text) { return std::strstr(bms_last_error(&dummy), text) != nullptr; };
  REQUIRE(expectation_checks(&dummy, v, 6, v, 6, 2, 6, rows, cols, v, 5, BMS_HOST, out) == BMS_OK);
  REQUIRE(expectation_checks(&dummy, v, 6, v, 6, 2, 5, rows, cols, v, 5, BMS_HOST, out) == BMS_ERR_INVALID && says("element 3 couples row 2 and column 5, outside [0, 5)"));
  REQUIRE(expectation_checks(&dummy, v, 5, v, 6, 2, 6, rows, cols, v, 5, BMS_HOST, out) == BMS_ERR_INVALID && says("row stride"));
  REQUIRE(expectation_checks(&dummy, nullptr, 6, v, 6, 2, 6, rows, cols, v, 5, BMS_HOST, out) == BMS_ERR_INVALID && says("NULL"));
  REQUIRE(expectation_checks(&dummy, v, 6, v, 6, 2, 6, rows, cols, v, 5, BMS_DEVICE, (char*)out + 8) == BMS_ERR_INVALID && says("aligned"));
  REQUIRE(bms_expectation_values(&dummy, v, 6, 1, v, 6, 2, 6, rows, cols, v, 5, 7, out) == BMS_ERR_INVALID && says("bms_expectation_values: mem is BMS_HOST or BMS_DEVICE, got 7"));
  REQUIRE(bms_expectation_values(&dummy, v, 6, 1, v, 6, 2, 5, rows, cols, v, 5, BMS_HOST, out) == BMS_ERR_INVALID && says("outside [0, 5)"));
  REQUIRE(bms_expectation_values(&dummy, v, 6, 1, v, 6, 0, 6, rows, cols, v, 5, BMS_HOST, out) == BMS_OK);
  REQUIRE(bms_expectation_values(nullptr, v, 6, 1, v, 6, 2, 6, rows, cols, v, 5, BMS_HOST, out) == BMS_ERR_INVALID);
  int nm = 0;
  REQUIRE(flux_checks(&dummy, t, v, 5, v, 5, 4, 2, 2, BMS_HOST, out, out, out, out, &nm) == BMS_OK && nm == 5);
  REQUIRE(flux_checks(&dummy, t, v, 5, nullptr, 5, 4, 2, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID && says("NULL hdot"));
  REQUIRE(flux_checks(&dummy, t, nullptr, 5, v, 5, 4, 2, 2, BMS_HOST, out, out, nullptr, nullptr, &nm) == BMS_OK);
  REQUIRE(flux_checks(&dummy, t, nullptr, 5, v, 5, 4, 2, 2, BMS_HOST, out, out, out, nullptr, &nm) == BMS_ERR_INVALID && says("need h"));
  REQUIRE(flux_checks(&dummy, nullptr, v, 5, v, 5, 4, 2, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID && says("needs the times"));
  REQUIRE(flux_checks(&dummy, t, v, 5, v, 5, 4, 2, 2, BMS_HOST, nullptr, nullptr, nullptr, nullptr, &nm) == BMS_ERR_INVALID);
  REQUIRE(flux_checks(&dummy, t, v, 4, v, 5, 4, 2, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID && says("row stride"));
  REQUIRE(flux_checks(&dummy, t, v, 5, v, 5, 4, 1, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_UNSUPPORTED && says("ell_min = 1"));
  REQUIRE(flux_checks(&dummy, t, v, 5, v, 5, 4, 3, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID);
  REQUIRE(flux_checks(&dummy, t, v, 1 << 30, v, 1 << 30, 4, 2, MAX_ELL + 1, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_UNSUPPORTED);
  REQUIRE(flux_checks(&dummy, t, v, 5, v, 5, -1, 2, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID);
  REQUIRE(flux_checks(&dummy, t, v + 1, 5, v, 5, 4, 2, 2, BMS_DEVICE, out, out, out, out, &nm) == BMS_ERR_INVALID && says("aligned"));
  REQUIRE(bms_poincare_fluxes(&dummy, t, v, 5, v, 5, 4, 2, 2, 7, out, out, out, out) == BMS_ERR_INVALID && says("bms_poincare_fluxes: mem is BMS_HOST or BMS_DEVICE, got 7"));
  REQUIRE(bms_poincare_fluxes(&dummy, t, v, 5, v, 5, 0, 2, 2, BMS_HOST, out, out, out, out) == BMS_OK);
  REQUIRE(bms_poincare_fluxes(nullptr, t, v, 5, v, 5, 4, 2, 2, BMS_HOST, out, out, out, out) == BMS_ERR_INVALID);
  std::vector<double> image((size_t)30 * 5);
  REQUIRE(bms_flux_coefficients(2, 2, image.data()) == BMS_OK && image[(size_t)29 * 5] == 2.0);
  REQUIRE(bms_flux_coefficients(1, 2, image.data()) == BMS_ERR_INVALID && bms_flux_coefficients(2, 2, nullptr) == BMS_ERR_INVALID);
  // the brackets of a pair: the common range l = 2..3 (12 columns) inside rows that start at l = 2 and at l = 0
  int64_t off_a = -1, off_b = -1;
  REQUIRE(pair_checks(&dummy, v, 12, 2, v, 16, 0, 2, 2, 3, BMS_HOST, out, out, out, &nm, &off_a, &off_b) == BMS_OK && nm == 12 && off_a == 0 && off_b == 4);
  REQUIRE(pair_checks(&dummy, v, 12, 2, v, 15, 0, 2, 2, 3, BMS_HOST, out, out, out, &nm, &off_a, &off_b) == BMS_ERR_INVALID && says("row stride"));
  REQUIRE(pair_checks(&dummy, v, 11, 2, v, 16, 0, 2, 2, 3, BMS_HOST, out, nullptr, nullptr, &nm, &off_a, &off_b) == BMS_ERR_INVALID && says("row stride"));
  REQUIRE(pair_checks(&dummy, nullptr, 12, 2, v, 16, 0, 2, 2, 3, BMS_HOST, out, out, out, &nm, &off_a, &off_b) == BMS_ERR_INVALID && says("NULL waveform"));
  REQUIRE(pair_checks(&dummy, v, 12, 2, v, 16, 0, 2, 2, 3, BMS_HOST, nullptr, nullptr, nullptr, &nm, &off_a, &off_b) == BMS_ERR_INVALID && says("every output"));
  REQUIRE(pair_checks(&dummy, v, 12, 3, v, 16, 0, 2, 2, 3, BMS_HOST, out, out, out, &nm, &off_a, &off_b) == BMS_ERR_INVALID && says("below a row's first ell"));
  REQUIRE(pair_checks(&dummy, v, 12, 2, v, 16, -1, 2, 2, 3, BMS_HOST, out, out, out, &nm, &off_a, &off_b) == BMS_ERR_INVALID);
  REQUIRE(pair_checks(&dummy, v, 12, 2, v, 16, 0, 2, 3, 2, BMS_HOST, out, out, out, &nm, &off_a, &off_b) == BMS_ERR_INVALID && says("bad ell range [3, 2]"));
  REQUIRE(pair_checks(&dummy, v, 12, 2, v, 16, 0, -1, 2, 3, BMS_HOST, out, out, out, &nm, &off_a, &off_b) == BMS_ERR_INVALID && says("negative n_times"));
  REQUIRE(pair_checks(&dummy, v, 1 << 30, 2, v, 1 << 30, 0, 2, 2, MAX_ELL + 1, BMS_HOST, out, out, out, &nm, &off_a, &off_b) == BMS_ERR_UNSUPPORTED);
  REQUIRE(pair_checks(&dummy, v, 12, 2, v, 16, 0, 2, 2, 3, BMS_DEVICE, out, out + 1, out, &nm, &off_a, &off_b) == BMS_ERR_INVALID && says("aligned"));
  REQUIRE(bms_pair_brackets(&dummy, v, 12, 2, v, 16, 0, 2, 2, 3, 7, out, out, out) == BMS_ERR_INVALID && says("bms_pair_brackets: mem is BMS_HOST or BMS_DEVICE, got 7"));
  REQUIRE(bms_pair_brackets(&dummy, v, 12, 2, v, 16, 0, 0, 2, 3, BMS_HOST, out, out, out) == BMS_OK);
  REQUIRE(bms_pair_brackets(nullptr, v, 12, 2, v, 16, 0, 2, 2, 3, BMS_HOST, out, out, out) == BMS_ERR_INVALID);
  // the Bondi charges: rows from l = 0 to 2 (9 columns), four columns of psi1 and psi2
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v, 9, v, 9, 4, 2, BMS_HOST, out, out, out, out, &nm) == BMS_OK && nm == 9);
  REQUIRE(charge_checks(&dummy, nullptr, v, 4, nullptr, 0, v, 9, nullptr, 0, 4, 2, BMS_HOST, nullptr, out, nullptr, out, &nm) == BMS_OK);
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v, 9, v, 9, 4, 2, BMS_HOST, nullptr, nullptr, nullptr, nullptr, &nm) == BMS_ERR_INVALID && says("every output"));
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, nullptr, 9, v, 9, 4, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID && says("NULL sigma"));
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v, 9, nullptr, 9, 4, 2, BMS_HOST, out, nullptr, nullptr, nullptr, &nm) == BMS_ERR_INVALID && says("need sigma_dot"));
  REQUIRE(charge_checks(&dummy, t, v, 9, nullptr, 9, v, 9, v, 9, 4, 2, BMS_HOST, nullptr, nullptr, out, nullptr, &nm) == BMS_ERR_INVALID && says("need psi2"));
  REQUIRE(charge_checks(&dummy, t, nullptr, 9, v, 9, v, 9, v, 9, 4, 2, BMS_HOST, nullptr, out, nullptr, nullptr, &nm) == BMS_ERR_INVALID && says("need psi1"));
  REQUIRE(charge_checks(&dummy, nullptr, v, 9, v, 9, v, 9, v, 9, 4, 2, BMS_HOST, nullptr, nullptr, out, nullptr, &nm) == BMS_ERR_INVALID && says("needs the times"));
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v, 8, v, 9, 4, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID && says("row stride"));
  REQUIRE(charge_checks(&dummy, t, v, 3, v, 9, v, 9, v, 9, 4, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID && says("four columns"));
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v, 9, v, 9, -1, 2, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID && says("negative n_times"));
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v, 9, v, 9, 4, 1, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_UNSUPPORTED && says("ell_max = 1"));
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v, 9, v, 9, 4, -1, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_INVALID);
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v, 1 << 30, v, 1 << 30, 4, MAX_ELL + 1, BMS_HOST, out, out, out, out, &nm) == BMS_ERR_UNSUPPORTED);
  REQUIRE(charge_checks(&dummy, t, v, 9, v, 9, v + 1, 9, v, 9, 4, 2, BMS_DEVICE, out, out, out, out, &nm) == BMS_ERR_INVALID && says("aligned"));
  REQUIRE(bms_bondi_charges(&dummy, t, v, 9, v, 9, v, 9, v, 9, 4, 2, 7, out, out, out, out) == BMS_ERR_INVALID && says("bms_bondi_charges: mem is BMS_HOST or BMS_DEVICE, got 7"));
  REQUIRE(bms_bondi_charges(&dummy, t, v, 9, v, 9, v, 9, v, 9, 0, 2, BMS_HOST, out, out, out, out) == BMS_OK);
  REQUIRE(bms_bondi_charges(nullptr, t, v, 9, v, 9, v, 9, v, 9, 4, 2, BMS_HOST, out, out, out, out) == BMS_ERR_INVALID);
  std::vector<double> charge_image((size_t)20 * 16);
  REQUIRE(bms_charge_coefficients(3, charge_image.data()) == BMS_OK && charge_image[(size_t)19 * 16 + 15] == 3.0 && charge_image[(size_t)18 * 16 + 3] == 0.0);
  REQUIRE(bms_charge_coefficients(1, charge_image.data()) == BMS_ERR_INVALID && bms_charge_coefficients(3, nullptr) == BMS_ERR_INVALID);
  // the products on Gauss-Legendre rows: the nodes and tables (a pure host routine) and what the two entries refuse
  for (int n_nodes : {1, 2, 5, 13}) {
    std::vector<double> x((size_t)n_nodes), w((size_t)n_nodes), table((size_t)n_nodes * 25);
    REQUIRE(bms_product_tables(-2, 4, n_nodes, x.data(), w.data(), table.data()) == BMS_OK);
    double sum = 0;
    for (int j = 0; j < n_nodes; ++j) {
      sum += w[(size_t)j];
      REQUIRE(x[(size_t)j] == -x[(size_t)(n_nodes - 1 - j)] && table[(size_t)j * 25 + 3] == 0.0 && std::isfinite(table[(size_t)j * 25 + 24]));
    }
    REQUIRE(std::fabs(sum - 2.0) < 1e-15);
  }
  REQUIRE(bms_product_tables(5, 4, 3, out, out, out) == BMS_ERR_INVALID && bms_product_tables(0, 4, 0, out, out, out) == BMS_ERR_INVALID &&
          bms_product_tables(0, 4, 3, nullptr, out, out) == BMS_ERR_INVALID);
  int nn = 0;
  REQUIRE(product_checks(&dummy, v, 9, 2, 2, 0, v, 16, -2, 3, 1, 4, 5, BMS_HOST, out, 36, &nn) == BMS_OK && nn == 6);
  REQUIRE(product_checks(&dummy, nullptr, 9, 2, 2, 0, v, 16, -2, 3, 1, 4, 5, BMS_HOST, out, 36, &nn) == BMS_ERR_INVALID && says("NULL a, b or out"));
  REQUIRE(product_checks(&dummy, v, 8, 2, 2, 0, v, 16, -2, 3, 1, 4, 5, BMS_HOST, out, 36, &nn) == BMS_ERR_INVALID && says("row stride of a or b"));
  REQUIRE(product_checks(&dummy, v, 9, 2, 2, 0, v, 16, -2, 3, 1, 4, 5, BMS_HOST, out, 35, &nn) == BMS_ERR_INVALID && says("row stride of out"));
  REQUIRE(product_checks(&dummy, v, 9, 2, 2, 0, v, 16, -2, 3, 1, 4, 6, BMS_HOST, out, 49, &nn) == BMS_ERR_INVALID && says("where the product ends"));
  REQUIRE(product_checks(&dummy, v, 9, 2, 2, 0, v, 16, -2, 3, 1, -1, 5, BMS_HOST, out, 36, &nn) == BMS_ERR_INVALID && says("negative n_times"));
  REQUIRE(product_checks(&dummy, v, 9, 2, -1, 0, v, 16, -2, 3, 1, 4, 5, BMS_HOST, out, 36, &nn) == BMS_ERR_INVALID && says("negative ell_max"));
  REQUIRE(product_checks(&dummy, v, 9, 3, 2, 0, v, 16, -2, 3, 1, 4, 5, BMS_HOST, out, 36, &nn) == BMS_ERR_UNSUPPORTED && says("up to |s| = 4"));
  REQUIRE(product_checks(&dummy, v, 1 << 30, 2, MAX_ELL + 1, 0, v, 16, -2, 3, 1, 4, 5, BMS_HOST, out, 36, &nn) == BMS_ERR_UNSUPPORTED);
  REQUIRE(product_checks(&dummy, v + 1, 9, 2, 2, 0, v, 16, -2, 3, 1, 4, 5, BMS_DEVICE, out, 36, &nn) == BMS_ERR_INVALID && says("aligned"));
  REQUIRE(supermomenta_checks(&dummy, v, 9, v, 16, v, 16, 4, 3, 2, BMS_HOST, out, nullptr, nullptr, nullptr, out, 9, &nn) == BMS_OK && nn == 5);
  REQUIRE(supermomenta_checks(&dummy, v, 9, v, 16, v, 16, 4, 3, 2, BMS_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, 9, &nn) == BMS_ERR_INVALID && says("every output"));
  REQUIRE(supermomenta_checks(&dummy, v, 9, nullptr, 16, v, 16, 4, 3, 2, BMS_HOST, out, out, out, out, out, 9, &nn) == BMS_ERR_INVALID && says("NULL psi2, sigma or sigma_dot"));
  REQUIRE(supermomenta_checks(&dummy, v, 9, v, 15, v, 16, 4, 3, 2, BMS_HOST, out, out, out, out, out, 9, &nn) == BMS_ERR_INVALID && says("row stride of sigma"));
  REQUIRE(supermomenta_checks(&dummy, v, 8, v, 16, v, 16, 4, 3, 2, BMS_HOST, out, out, out, out, out, 9, &nn) == BMS_ERR_INVALID && says("row stride of psi2"));
  REQUIRE(supermomenta_checks(&dummy, v, 25, v, 16, v, 16, 4, 3, 4, BMS_HOST, out, out, out, out, out, 25, &nn) == BMS_ERR_INVALID && says("beyond ell_max = 3"));
  REQUIRE(supermomenta_checks(&dummy, v, 9, v, 16, v, 16, 4, 1, 1, BMS_HOST, out, out, out, out, out, 9, &nn) == BMS_ERR_UNSUPPORTED && says("ell_max = 1"));
  REQUIRE(bms_mode_product(&dummy, v, 9, 2, 2, 0, v, 16, -2, 3, 1, 4, 5, 7, out, 36) == BMS_ERR_INVALID && says("bms_mode_product: mem is BMS_HOST or BMS_DEVICE, got 7"));
  REQUIRE(bms_mode_product(&dummy, v, 9, 2, 2, 0, v, 16, -2, 3, 1, 0, 5, BMS_HOST, out, 36) == BMS_OK);
  REQUIRE(bms_supermomenta(&dummy, v, 9, v, 16, v, 16, 0, 3, 2, BMS_HOST, 1, out, out, out, out, out, 9) == BMS_OK);
  REQUIRE(bms_supermomenta(nullptr, v, 9, v, 16, v, 16, 4, 3, 2, BMS_HOST, 1, out, out, out, out, out, 9) == BMS_ERR_INVALID);
  // the Bondi-gauge violations: which inputs the outputs asked for read, and what the entry refuses
  {
    const void* in[CONSTRAINT_INPUTS];
    int64_t ld[CONSTRAINT_INPUTS];
    for (int i = 0; i < CONSTRAINT_INPUTS; ++i) in[i] = v, ld[i] = 16;
    const void* const all[6] = {out, out, out, out, out, out};
    const void* const none[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const void* const third[6] = {nullptr, nullptr, nullptr, out, nullptr, nullptr};
    unsigned reads = 0;
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, all, 16, out, &reads, &nn) == BMS_OK && nn == 5 && reads == 0x7feu);
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_OK && reads == (1u << 3 | 1u << 9));
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, none, 16, out, &reads, &nn) == BMS_OK && reads == 0x7feu);
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, none, 16, nullptr, &reads, &nn) == BMS_ERR_INVALID && says("every output is NULL"));
    in[0] = nullptr;  // psi0 is never read
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, all, 16, out, &reads, &nn) == BMS_OK);
    in[9] = nullptr;
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_ERR_INVALID && says("NULL sigma_dot"));
    in[9] = v, ld[3] = 15;
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_ERR_INVALID && says("row stride of psi3"));
    ld[3] = 16, ld[10] = 15;  // (sigma_ddot is not read by v3)
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_OK);
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, third, 15, nullptr, &reads, &nn) == BMS_ERR_INVALID && says("row stride of the violations"));
    REQUIRE(constraint_checks(&dummy, in, ld, -1, 3, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_ERR_INVALID && says("negative n_times"));
    REQUIRE(constraint_checks(&dummy, in, ld, 4, -1, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_ERR_INVALID && says("negative ell_max"));
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 1, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_ERR_UNSUPPORTED && says("ell_max = 1"));
    REQUIRE(constraint_checks(&dummy, in, ld, 4, MAX_ELL + 1, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_ERR_UNSUPPORTED);
    in[3] = v + 1;
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_DEVICE, third, 16, nullptr, &reads, &nn) == BMS_ERR_INVALID && says("aligned"));
    REQUIRE(constraint_checks(&dummy, in, ld, 4, 3, BMS_HOST, third, 16, nullptr, &reads, &nn) == BMS_OK);
    const int64_t ld6[6] = {16, 16, 16, 16, 16, 16};
    void* const homes[6] = {out, out, out, out, out, out};
    REQUIRE(bms_bondi_constraints(&dummy, in, ld6, in, ld6, v, 16, v, 16, 4, 3, 7, homes, 16, out) == BMS_ERR_INVALID && says("bms_bondi_constraints: mem is BMS_HOST or BMS_DEVICE, got 7"));
    REQUIRE(bms_bondi_constraints(&dummy, nullptr, ld6, in, ld6, v, 16, v, 16, 4, 3, BMS_HOST, homes, 16, out) == BMS_ERR_INVALID && says("NULL list"));
    REQUIRE(bms_bondi_constraints(&dummy, in + 1, ld6, in + 1, ld6, v, 16, v, 16, 0, 3, BMS_HOST, homes, 16, out) == BMS_OK);
    REQUIRE(bms_bondi_constraints(&dummy, in + 1, ld6, in + 1, ld6, v, 16, v, 16, 4, 3, BMS_HOST, nullptr, 16, nullptr) == BMS_ERR_INVALID && says("every output"));
    REQUIRE(bms_bondi_constraints(nullptr, in + 1, ld6, in + 1, ld6, v, 16, v, 16, 4, 3, BMS_HOST, homes, 16, out) == BMS_ERR_INVALID);
  }
  // a stage of the Bianchi identities run forwards: which stage writes psi3 and psi4, and what the entry refuses
  REQUIRE(bianchi_checks(&dummy, 2, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, out, 16, out, out, 16, &nn) == BMS_OK && nn == 5);
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v, 17, v, 18, 4, 3, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_OK && nn == 5);
  REQUIRE(bianchi_checks(&dummy, 0, v, 16, v, 16, v, 16, 0, 3, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_OK);
  REQUIRE(bianchi_checks(&dummy, 3, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("names no stage"));
  REQUIRE(bianchi_checks(&dummy, -1, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("names no stage"));
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, nullptr, 16, v, 16, 4, 3, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("NULL sigma, a, b or rhs"));
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, nullptr, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("NULL sigma, a, b or rhs"));
  REQUIRE(bianchi_checks(&dummy, 2, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, out, 16, out, nullptr, 16, &nn) == BMS_ERR_INVALID && says("NULL psi3 or psi4"));
  REQUIRE(bianchi_checks(&dummy, 0, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, out, 16, nullptr, out, 16, &nn) == BMS_ERR_INVALID && says("must be NULL at k = 0"));
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v, 16, v, 15, 4, 3, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("columns read"));
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, out, 15, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("columns written"));
  REQUIRE(bianchi_checks(&dummy, 2, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, out, 16, out, out, 15, &nn) == BMS_ERR_INVALID && says("columns written"));
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v, 16, v, 16, -1, 3, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("negative n_times"));
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v, 16, v, 16, 4, -1, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("negative ell_max"));
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v, 16, v, 16, 4, 1, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_UNSUPPORTED && says("ell_max = 1"));
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v, 16, v, 16, 4, MAX_ELL + 1, BMS_HOST, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_UNSUPPORTED);
  REQUIRE(bianchi_checks(&dummy, 1, v, 16, v + 1, 16, v, 16, 4, 3, BMS_DEVICE, out, 16, nullptr, nullptr, 0, &nn) == BMS_ERR_INVALID && says("aligned"));
  REQUIRE(bms_bianchi_rhs(&dummy, 1, v, 16, v, 16, v, 16, 4, 3, 7, out, 16, nullptr, nullptr, 0) == BMS_ERR_INVALID && says("bms_bianchi_rhs: mem is BMS_HOST or BMS_DEVICE, got 7"));
  REQUIRE(bms_bianchi_rhs(&dummy, 2, v, 16, v, 16, v, 16, 0, 3, BMS_HOST, out, 16, out, out, 16) == BMS_OK);
  REQUIRE(bms_bianchi_rhs(nullptr, 1, v, 16, v, 16, v, 16, 4, 3, BMS_HOST, out, 16, nullptr, nullptr, 0) == BMS_ERR_INVALID);
}

}  // namespace

int main() {
  // BASELINE.json configs 1..5 (cfg4's 1e6 steps and cfg5's 2e5 as they are: the planners are O(n log n) at worst)
  const Shape shapes[] = {
      {"cfg1 (l<=4, 2000)", 4, 11, 11, 1, 2000, 0.055, 1.0, false},
      {"cfg2 (l<=8, 1e5)", 8, 21, 21, 2, 100000, 0.1, 0.0, false},
      {"cfg3 (l<=16, 1e5)", 16, 37, 37, 2, 100000, 0.1, 1.0, false},
      {"cfg3 beta=1e-2", 16, 37, 37, 2, 100000, 0.1, 26.7, false},
      {"cfg3 beta=0.1", 16, 37, 37, 2, 100000, 0.1, 267.0, false},
      {"cfg4 (l<=16, 1e6)", 16, 37, 37, 2, 1000000, 0.1, 1.0, false},
      {"cfg5 (ABD l<=24, 2e5)", 24, 99, 99, 2, 200000, 0.1, 1.0, true},
  };
  for (const Shape& s : shapes) run_shape(s);
  short_series_and_odd_grids();
  frame_integration();
  frame_chain_arguments();
  alignment_arguments();
  sample_waveform_plan();
  paired_xor_arguments();
  com_motion_arguments();
  dense_product_arguments();
  staged_argument_prologues();
  flux_tables_and_triplets();
  slab_allocator();
  std::printf("host sanitizer run: %d checks, clean\n", g_checks);
  return 0;
}
