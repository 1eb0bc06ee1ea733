// SIMP topology optimisation: body loads of the linear elasticity -- self-weight and inertial load cases (C-ABI in
// include/femo_hip.h, femo_elast_body_apply).
//
// A body force b_l in R^d (mass density times acceleration) is constant per load case l, and the mass is linear in the DG0
// density, so the load is the linear operator G_B : R^{n_cell} -> R^{L n_dof} of B = (b_0 ... b_{L-1}),
//   (G_B w)[l n_dof + d v + i] = b_l[i] sum_{c around v} w_c |T_c| / (d + 1),
//   (G_B^T x)[c]               = |T_c| / (d + 1) sum_l b_l . sum_{a in c} x_l[a].
// Layout as in elast_solve.hip: column l at l * n_dof.  What the columns share is computed once: the vertex sum
// s_v = sum_c w_c |T_c| / (d + 1) per vertex (N), the cell volume per cell (T).  One launch serves all columns.  The b_l
// travel as a by-value struct of FEMO_ELAST_MAX_COLS x 3 doubles.  No float atomics: one writer per vertex and per cell,
// the cells around a vertex in ascending order and the columns in ascending order, so every call gives the same bits and
// column l does not depend on how many columns go with it.
#include "elast_internal.h"

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

struct BodyForces { double v[EMC][3]; };

// N: one thread per vertex row on the shared visit walk (elast_visits).  s_v once, then every column and component:
//   y = [accumulate ? y : (base ? base : 0)] + a s_v b_l[i],   or 0 on a fixed dof (fixed != null: the same set per column)
template <int D>
__global__ __launch_bounds__(EB) void k_elast_body_N(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, const double* __restrict__ w, int n_cols, BodyForces bf, double a,
    const double* __restrict__ base, const uint8_t* __restrict__ fixed, double* __restrict__ y, int accumulate) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  double sv = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    sv += w[t.c] * (elast_cell_volume<D>(conn, xv, t.c).vol * (1.0 / (D + 1)));
  }
  const double asv = a * sv;
  const int64_t n_dof = n_rows * D;
  for (int l = 0; l < n_cols; ++l)
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int64_t k = (int64_t)l * n_dof + row * D + i;
      double r;
      if (fixed && fixed[row * D + i]) r = 0.0;
      else r = (accumulate ? y[k] : (base ? base[k] : 0.0)) + asv * bf.v[l][i];
      y[k] = r;
    }
}

// T: one thread per cell, the columns in ascending order:  y_c = (accumulate ? y_c : 0) + a |T_c| / (d + 1) sum_l b_l . sum_a x_l[v_a]
template <int D>
__global__ __launch_bounds__(EB) void k_elast_body_T(int64_t n_cell, int64_t n_dof, const int32_t* __restrict__ conn,
                                                     const double* __restrict__ xv, const double* __restrict__ x, int n_cols,
                                                     BodyForces bf, double a, double* __restrict__ y, int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= n_cell) return;
  const ElastCellVolume<D> K = elast_cell_volume<D>(conn, xv, c);
  const double vol = K.vol * (1.0 / (D + 1));
  double acc = 0.0;
  for (int l = 0; l < n_cols; ++l) {
    const double* __restrict__ xl = x + (int64_t)l * n_dof;
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double sx = 0.0;
#pragma unroll
      for (int b = 0; b <= D; ++b) sx += xl[(int64_t)K.v[b] * D + i];
      t += bf.v[l][i] * sx;
    }
    acc += t;
  }
  const double val = a * (vol * acc);
  y[c] = accumulate ? y[c] + val : val;
}

int body_launch(femo_elast* e, int n_cols, const BodyForces& bf, int transpose, double a, const double* x, const double* base,
                const uint8_t* fixed, double* y, int accumulate) {
  femo_mesh* m = e->mesh;
  return elast_dispatch_d(e->d, [&](auto dim) {
    constexpr int D = decltype(dim)::value;
    if (transpose) return elast_launch_cells(e, k_elast_body_T<D>, m->n_vert * D, m->d_conn, m->d_x, x, n_cols, bf, a, y, accumulate);
    return elast_launch_rows(e, k_elast_body_N<D>, m->d_vptr, m->d_visit_cell, m->d_conn, m->d_x, x, n_cols, bf, a, base, fixed, y,
                             accumulate);
  });
}

}  // namespace

extern "C" int femo_elast_body_apply(femo_elast* e, int n_cols, const double* b, int transpose, double a, const femo_vec* x,
                                     const femo_vec* base, int zero_fixed, femo_vec* y, int accumulate) {
  FEMO_REQUIRE(e && b && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= FEMO_ELAST_MAX_COLS, "femo_elast_body_apply: %d columns (1 to %d)", n_cols,
               FEMO_ELAST_MAX_COLS);
  femo_mesh* m = e->mesh;
  const int64_t nl = m->n_vert * e->d * n_cols;
  FEMO_REQUIRE(transpose ? (x->n >= nl && y->n >= m->n_cell) : (x->n >= m->n_cell && y->n >= nl),
               "vector size mismatch in femo_elast_body_apply");
  FEMO_REQUIRE(y != x && y != base, "femo_elast_body_apply: output aliases an input");
  FEMO_REQUIRE(!transpose || (!base && !zero_fixed), "femo_elast_body_apply: base and zero_fixed belong to the forward product");
  FEMO_REQUIRE(!base || base->n >= nl, "vector size mismatch in femo_elast_body_apply");
  FEMO_REQUIRE(!zero_fixed || e->has_fixed, "femo_elast_body_apply: zero_fixed without a fixed set (femo_elast_set_fixed)");
  BodyForces bf;
  for (int l = 0; l < EMC; ++l)
    for (int i = 0; i < 3; ++i) bf.v[l][i] = (l < n_cols && i < e->d) ? b[l * 3 + i] : 0.0;
  FEMO_TRY(femo_vec_await(x));
  if (base) FEMO_TRY(femo_vec_await(base));
  femo_vec_touch(y);
  const uint8_t* fx = zero_fixed ? e->d_fixed : nullptr;
  const double* bs = base ? base->d : nullptr;
  return body_launch(e, n_cols, bf, transpose, a, x->d, bs, fx, y->d, accumulate);
}
