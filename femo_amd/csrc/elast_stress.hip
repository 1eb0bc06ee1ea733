// The aggregated von Mises stress of the SIMP elasticity, for one load case or several in one pass (C-ABI in
// include/femo_hip.h: "femo_elast_pnorm_stress", "femo_elast_von_mises" and their "_multi" forms).
//
//   J_l = 1/alpha sum_e |T_e| (m_l rho_e^q sigma_vm,e(u_l))^p,     J = sum_l w_l J_l
//
// Layout as in elast_solve.hip: L columns (1 <= L <= FEMO_ELAST_MAX_COLS), column l of the state and of dJ/du at l * n_dof.
// What the columns share -- the cell's vertices, the gradients of its barycentric coordinates, its volume and rho^q -- is
// computed once per cell (cell kernel) and once per cell visit (dJ/du kernel), not once per column.  One column is the
// L = 1 case: the single-column entry points run one-column instantiations of the same two kernels.  m, w and the field
// scales travel as by-value structs of FEMO_ELAST_MAX_COLS doubles.  No float atomics: one writer per cell and per vertex,
// the per-column partials folded in a fixed order, so every call gives the same bits.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

// columns per thread of the dJ/du kernel: D accumulators and one deviator per column in registers
template <int D>
struct StressChunk { static constexpr int value = 4; };

// One thread per cell; the geometry once, then the columns one after the other.  Every output optional by null pointer:
//   part[l * ps + block] = sum over the block of J_{l,c} = |T_c| / alpha (m_l rho_c^q sigma_vm(u_l))^p
//   drho[c] (+)= sum_l w_l p q / rho_c J_{l,c}, summed in ascending l
//   field[c] = max_l s_l rho_c^q sigma_vm(u_l) (column < 0: the envelope), or s_column rho_c^q sigma_vm(u_column)
// rho == null reads as q = 0.  A (cell, column) with sigma_vm = 0 gives 0 everywhere (pow(0, p) = 0 for p >= 1; no division
// by it); the guard is a test for == 0, so a non-finite stress is no zero: it shows in the value, in drho and in the field
// (the envelope's maximum keeps a NaN).  A column with w_l = 0 takes no part in drho.  ONE: the one-column instantiation
// (n_cols = 1, column 0, known at compile time), which keeps no geometry alive across a column loop and writes the field as
// it is.
template <int D, bool ONE>
__global__ __launch_bounds__(EB) void k_elast_stress_cell_multi(
    int64_t n_cell, const int32_t* __restrict__ conn, const double* __restrict__ xv, const double* __restrict__ rho,
    const double* __restrict__ u, int64_t vs, int n_cols, double mu, ColScalars m, ColScalars w, ColScalars sc, double p,
    double q, double inv_alpha, int column, double* __restrict__ field, double* __restrict__ part, int64_t ps,
    double* __restrict__ drho, int accumulate) {
  __shared__ double lds[EB / 64];
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  const bool live = c < n_cell;
  ElastCell<D> K = {};           // a thread past the last cell stays for the block sums, on a cell of zeros
  double r = 1.0, rq = 1.0;
  if (live) {
    K = elast_cell<D>(conn, xv, c);
    r = rho ? rho[c] : 1.0;
    rq = rho && q != 0.0 ? pow(r, q) : 1.0;
  }
  const bool sums = part || drho;
  const int l0 = !ONE && field && !sums && column >= 0 ? column : 0;          // a single field: that column only
  const int l1 = ONE ? 1 : (field && !sums && column >= 0 ? column + 1 : n_cols);
  double dsum = 0.0, fmax_ = 0.0;
  for (int l = l0; l < l1; ++l) {
    double Jc = 0.0;
    if (live) {
      double s[D][D];
      const double vm = cell_von_mises<D>(K.g, K.v, u + l * vs, mu, s);
      const double relaxed = rq * vm;
      if (ONE) fmax_ = sc.v[0] * relaxed;
      else if (field && (column < 0 || column == l)) {
        const double f = sc.v[l] * relaxed;
        fmax_ = f > fmax_ || f != f ? f : fmax_;          // a sticky maximum: fmax would drop a NaN
      }
      if (sums) {
        Jc = vm == 0.0 ? 0.0 : K.vol * inv_alpha * pow(m.v[l] * relaxed, p);
        if (drho && q != 0.0 && Jc != 0.0 && w.v[l] != 0.0) dsum += w.v[l] * (p * q / r * Jc);
      }
    }
    if (part) {
      const double t = femo_block_sum<EB>(Jc, lds);
      if (threadIdx.x == 0) part[l * ps + blockIdx.x] = t;
    }
  }
  if (live) {
    if (field) field[c] = fmax_;
    if (drho) drho[c] = accumulate ? drho[c] + dsum : dsum;
  }
}

// dJ/du: one thread per vertex row on the shared visit walk (elast_visits), for the columns c0 = MC * blockIdx.y ...
// min(c0 + MC, n_cols) - 1.  Column l of y (+)= w_l dJ_l/du_l:
//   y_(v, r) (+)= sum over the cells c around v of (tau_c grad phi_v)_r, tau = 2 mu S + lam tr(S) I,
//   S = dJ_c/dsigma = |T| / alpha p (m rho^q)^p sigma_vm^(p-2) 3/2 s.
// S is a deviator, so the lam term is zero and tau = 2 mu S; only its d x d block meets grad phi.  Written as wt (s / sigma_vm)
// with wt = w 3 mu p |T| / alpha (m rho^q)^p sigma_vm^(p-1): no negative power of sigma_vm for p >= 1, and the cell is skipped
// when sigma_vm = 0.  One writer per vertex, cells in ascending order.  The geometry and rho^q once per visited cell, D accumulators
// per column.  A column with w_l = 0 takes no part in the walk: it is written as zeros (left alone with accumulate).
template <int D, int MC>
__global__ __launch_bounds__(EB) void k_elast_stress_du_multi(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, const double* __restrict__ rho, const double* __restrict__ u, int64_t vs, int n_cols,
    double mu, ColScalars m, ColScalars w, double p, double q, double inv_alpha, double* __restrict__ y, int accumulate) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int c0 = (int)blockIdx.y * MC;
  bool on[MC], act[MC];      // uniform over the block
  double mm[MC], ww[MC];
  bool any = false;
#pragma unroll
  for (int cc = 0; cc < MC; ++cc) {
    on[cc] = c0 + cc < n_cols;
    mm[cc] = on[cc] ? m.v[c0 + cc] : 1.0;
    ww[cc] = on[cc] ? w.v[c0 + cc] : 0.0;
    act[cc] = on[cc] && ww[cc] != 0.0;
    any = any || act[cc];
  }
  double acc[MC][D];
#pragma unroll
  for (int cc = 0; cc < MC; ++cc)
#pragma unroll
    for (int i = 0; i < D; ++i) acc[cc][i] = 0.0;
  if (any) {
    const ElastVisits V = elast_visits(row, vptr);
    for (int k = 0; k < V.n; ++k) {
      const ElastVisit t = elast_visit(V, visit_cell, k);
      if (!t.live) continue;
      const int64_t c = t.c;
      const int a = t.a;
      int32_t v[D + 1];          // g[a]: an array of its own, as in k_elast_assemble
      double pt[D + 1][D], g[D + 1][D], vol;
      load_cell<D>(conn, xv, c, v, pt);
      simplex_grads<D>(pt, g, vol);
      // One column takes rho^q after the zero-stress test and reads grad lambda_a where it is used: with either of them
      // up here the 3-D one-column kernel needs more than 128 registers and loses a wave.
      double rq = 1.0, ga[D];
      if (MC > 1) rq = q != 0.0 ? pow(rho[c], q) : 1.0;
#pragma unroll
      for (int j = 0; j < D; ++j) ga[j] = g[a][j];
      const double base = 3.0 * mu * p * vol * inv_alpha;
#pragma unroll
      for (int cc = 0; cc < MC; ++cc) {
        if (!act[cc]) continue;
        double s[D][D];
        const double vm = cell_von_mises<D>(g, v, u + (c0 + cc) * vs, mu, s);
        if (vm == 0.0) continue;                          // exactly zero only: a NaN stress goes on and shows in y
        if (MC == 1) rq = q != 0.0 ? pow(rho[c], q) : 1.0;
        const double mr = mm[cc] * rq;
        const double wt = ww[cc] * (base * mr * pow(mr * vm, p - 1.0));
        if (wt == 0.0) continue;
#pragma unroll
        for (int i = 0; i < D; ++i) {
          double t = 0.0;
#pragma unroll
          for (int j = 0; j < D; ++j) t += (s[i][j] / vm) * (MC == 1 ? g[a][j] : ga[j]);
          acc[cc][i] += wt * t;
        }
      }
    }
  }
#pragma unroll
  for (int cc = 0; cc < MC; ++cc) {
    if (!on[cc] || (accumulate && !act[cc])) continue;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int64_t o = (c0 + cc) * vs + row * D + i;
      y[o] = accumulate ? y[o] + acc[cc][i] : acc[cc][i];
    }
  }
}

// one column: the ONE instantiation (as femo_elast_spmv in elast_solve.hip picks MC = 1)
int cell_launch(femo_elast* e, int nc, const double* rho, const double* u, const ColScalars& m, const ColScalars& w,
                const ColScalars& sc, double p, double q, double inv_alpha, int column, double* field, double* part, int64_t ps,
                double* drho, int accumulate) {
  femo_mesh* mh = e->mesh;
  FEMO_REQUIRE((int64_t)grid_of(mh->n_cell) * EB >= mh->n_cell, "too many cells for one launch");
  return elast_dispatch_d(e->d, [&](auto dim) {
    constexpr int D = decltype(dim)::value;
    auto* kernel = nc == 1 ? k_elast_stress_cell_multi<D, true> : k_elast_stress_cell_multi<D, false>;
    return elast_launch_cells(e, kernel, mh->d_conn, mh->d_x, rho, u, mh->n_vert * D, nc, e->mu0, m, w, sc, p, q, inv_alpha, column,
                              field, part, ps, drho, accumulate);
  });
}

// one column: the MC = 1 instantiation; the columns of a chunk in the grid's second dimension
int du_launch(femo_elast* e, int nc, const double* rho, const double* u, const ColScalars& m, const ColScalars& w, double p,
              double q, double inv_alpha, double* y, int accumulate) {
  femo_mesh* mh = e->mesh;
  return elast_dispatch_d(e->d, [&](auto dim) {
    constexpr int D = decltype(dim)::value;
    const int mc = nc == 1 ? 1 : StressChunk<D>::value;
    auto* kernel = nc == 1 ? k_elast_stress_du_multi<D, 1> : k_elast_stress_du_multi<D, StressChunk<D>::value>;
    return elast_launch(e, mh->n_rows, (unsigned)((nc + mc - 1) / mc), kernel, mh->d_vptr, mh->d_visit_cell, mh->d_conn, mh->d_x, rho,
                        u, mh->n_vert * D, nc, e->mu0, m, w, p, q, inv_alpha, y, accumulate);
  });
}

// m and w of n_cols load cases as kernel arguments (w == null: ones), checked; the absent columns read m = 1, w = 0
int col_scalars(int n_cols, const double* m, const double* w, ColScalars& ms, ColScalars& ws) {
  for (int l = 0; l < EMC; ++l) {
    ms.v[l] = l < n_cols ? m[l] : 1.0;
    ws.v[l] = l < n_cols ? (w ? w[l] : 1.0) : 0.0;
    FEMO_REQUIRE(ms.v[l] > 0.0 && std::isfinite(ms.v[l]), "bad parameters of the stress aggregate: need m > 0 (load case %d)", l);
    FEMO_REQUIRE(ws.v[l] >= 0.0 && std::isfinite(ws.v[l]), "bad parameters of the stress aggregate: need a weight >= 0 (load case %d)", l);
  }
  return 0;
}

ColScalars ones() {
  ColScalars o;
  for (double& v : o.v) v = 1.0;
  return o;
}

// The aggregate of femo_elast_pnorm_stress (one column, w = 1) and femo_elast_pnorm_stress_multi, which have checked their
// arguments.  The partials are allocated for FEMO_ELAST_MAX_COLS columns by whichever call comes first.
int pnorm_stress(femo_elast* e, int n_cols, const femo_vec* rho, const femo_vec* u, const ColScalars& ms, const ColScalars& ws,
                 double p, double q, double alpha, double* values, femo_vec* grad_u, femo_vec* grad_rho, int accumulate) {
  femo_mesh* mh = e->mesh;
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(u));
  hipStream_t st = mh->ctx->stream;
  const int nb = (int)grid_of(mh->n_cell);
  // one fold for all columns while a slab fits the fold's slot, one fold per column beyond that
  const int64_t ps = std::max<int64_t>(nb, FEMO_MAX_PARTIALS);
  if (values && !e->w_smpart) FEMO_TRY(dalloc(&e->w_smpart, ps * EMC + EMC));
  const double inv_alpha = 1.0 / alpha;
  if (grad_rho) femo_vec_touch(grad_rho);
  if (values || grad_rho)
    FEMO_TRY(cell_launch(e, n_cols, rho->d, u->d, ms, ws, ones(), p, q, inv_alpha, -1, nullptr, values ? e->w_smpart : nullptr, ps,
                         grad_rho ? grad_rho->d : nullptr, accumulate));
  if (grad_u) {
    femo_vec_touch(grad_u);
    FEMO_TRY(du_launch(e, n_cols, rho->d, u->d, ms, ws, p, q, inv_alpha, grad_u->d, accumulate));
  }
  if (values) {
    double* out = e->w_smpart + ps * EMC;
    if (ps == FEMO_MAX_PARTIALS) FEMO_TRY(femo_launch_fold(1024, nb, n_cols, e->w_smpart, out, st));
    else
      for (int l = 0; l < n_cols; ++l) FEMO_TRY(femo_launch_fold(1024, nb, 1, e->w_smpart + l * ps, out + l, st));
    FEMO_HIP_CHECK(hipMemcpyAsync(e->h_s, out, (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    for (int l = 0; l < n_cols; ++l) values[l] = e->h_s[l];
  }
  return 0;
}

// The cell field of femo_elast_von_mises (one column, scale 1) and femo_elast_von_mises_multi, arguments checked.
int von_mises(femo_elast* e, int n_cols, const femo_vec* rho, const femo_vec* u, const ColScalars& sc, double q, int column,
              femo_vec* out_cells) {
  FEMO_TRY(femo_vec_await(u));
  if (rho) FEMO_TRY(femo_vec_await(rho));
  femo_vec_touch(out_cells);
  return cell_launch(e, n_cols, rho ? rho->d : nullptr, u->d, ones(), ones(), sc, 1.0, q, 1.0, column, out_cells->d, nullptr, 0,
                     nullptr, 0);
}

}  // namespace

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_pnorm_stress(femo_elast* e, const femo_vec* rho, const femo_vec* u, double m, double p, double q, double alpha,
                            double* value, femo_vec* grad_u, femo_vec* grad_rho, int accumulate) {
  FEMO_REQUIRE(e && rho && u, "null argument");
  femo_mesh* mh = e->mesh;
  const int64_t n = mh->n_vert * e->d;
  FEMO_REQUIRE(rho->n >= mh->n_cell && u->n >= n && (!grad_u || grad_u->n >= n) && (!grad_rho || grad_rho->n >= mh->n_cell),
               "vector size mismatch in femo_elast_pnorm_stress");
  FEMO_REQUIRE(m > 0.0 && p >= 1.0 && q >= 0.0 && alpha > 0.0 && std::isfinite(m) && std::isfinite(p) && std::isfinite(q) &&
               std::isfinite(alpha), "bad parameters of the stress aggregate: need m > 0, p >= 1, q >= 0, alpha > 0");
  FEMO_REQUIRE(grad_u != u && grad_u != rho && grad_rho != rho && grad_rho != u && (!grad_u || grad_u != grad_rho),
               "femo_elast_pnorm_stress: output aliases an input");
  ColScalars ms, ws;
  FEMO_TRY(col_scalars(1, &m, nullptr, ms, ws));
  return pnorm_stress(e, 1, rho, u, ms, ws, p, q, alpha, value, grad_u, grad_rho, accumulate);
}

int femo_elast_pnorm_stress_multi(femo_elast* e, int n_cols, const femo_vec* rho, const femo_vec* u, const double* m,
                                  const double* w, double p, double q, double alpha, double* values, femo_vec* grad_u,
                                  femo_vec* grad_rho, int accumulate) {
  FEMO_REQUIRE(e && rho && u && m, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_pnorm_stress_multi: %d columns (1 to %d)", n_cols, EMC);
  femo_mesh* mh = e->mesh;
  const int64_t n = mh->n_vert * e->d, nl = n * n_cols;
  FEMO_REQUIRE(rho->n >= mh->n_cell && u->n >= nl && (!grad_u || grad_u->n >= nl) && (!grad_rho || grad_rho->n >= mh->n_cell),
               "vector size mismatch in femo_elast_pnorm_stress_multi: %d columns need %lld entries", n_cols, (long long)nl);
  FEMO_REQUIRE(p >= 1.0 && q >= 0.0 && alpha > 0.0 && std::isfinite(p) && std::isfinite(q) && std::isfinite(alpha),
               "bad parameters of the stress aggregate: need m > 0, p >= 1, q >= 0, alpha > 0");
  ColScalars ms, ws;
  FEMO_TRY(col_scalars(n_cols, m, w, ms, ws));
  FEMO_REQUIRE(grad_u != u && grad_u != rho && grad_rho != rho && grad_rho != u && (!grad_u || grad_u != grad_rho),
               "femo_elast_pnorm_stress_multi: output aliases an input");
  return pnorm_stress(e, n_cols, rho, u, ms, ws, p, q, alpha, values, grad_u, grad_rho, accumulate);
}

int femo_elast_von_mises(femo_elast* e, const femo_vec* rho, const femo_vec* u, double q, femo_vec* out_cells) {
  FEMO_REQUIRE(e && u && out_cells, "null argument");
  FEMO_REQUIRE(q >= 0.0 && std::isfinite(q), "femo_elast_von_mises: need q >= 0");
  FEMO_REQUIRE(rho || q == 0.0, "femo_elast_von_mises: q > 0 needs the density");
  femo_mesh* mh = e->mesh;
  FEMO_REQUIRE(u->n >= mh->n_vert * e->d && out_cells->n >= mh->n_cell && (!rho || rho->n >= mh->n_cell),
               "vector size mismatch in femo_elast_von_mises");
  FEMO_REQUIRE(out_cells != u && out_cells != rho, "femo_elast_von_mises: output aliases an input");
  return von_mises(e, 1, rho, u, ones(), q, 0, out_cells);
}

int femo_elast_von_mises_multi(femo_elast* e, int n_cols, const femo_vec* rho, const femo_vec* u, const double* scale, double q,
                               int column, femo_vec* out_cells) {
  FEMO_REQUIRE(e && u && out_cells, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_von_mises_multi: %d columns (1 to %d)", n_cols, EMC);
  FEMO_REQUIRE(column >= -1 && column < n_cols, "femo_elast_von_mises_multi: column %d of %d (-1: the envelope)", column, n_cols);
  FEMO_REQUIRE(q >= 0.0 && std::isfinite(q), "femo_elast_von_mises_multi: need q >= 0");
  FEMO_REQUIRE(rho || q == 0.0, "femo_elast_von_mises_multi: q > 0 needs the density");
  femo_mesh* mh = e->mesh;
  const int64_t nl = mh->n_vert * e->d * n_cols;
  FEMO_REQUIRE(u->n >= nl && out_cells->n >= mh->n_cell && (!rho || rho->n >= mh->n_cell),
               "vector size mismatch in femo_elast_von_mises_multi: %d columns need %lld entries", n_cols, (long long)nl);
  FEMO_REQUIRE(out_cells != u && out_cells != rho, "femo_elast_von_mises_multi: output aliases an input");
  ColScalars sc = ones();
  for (int l = 0; l < n_cols && scale; ++l) sc.v[l] = scale[l];
  for (int l = 0; l < n_cols; ++l)
    FEMO_REQUIRE(sc.v[l] > 0.0 && std::isfinite(sc.v[l]), "femo_elast_von_mises_multi: need a scale > 0 (load case %d)", l);
  return von_mises(e, n_cols, rho, u, sc, q, column, out_cells);
}

}  // extern "C"
