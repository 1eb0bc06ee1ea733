// SIMP topology optimisation: the thermal expansion load of the linear elasticity (C-ABI in include/femo_hip.h,
// femo_elast_thermal_apply).
//
// With sigma = C(rho) (sigma_0(u) - beta_0 theta I), beta_0 = (3 lambda_0 + 2 mu_0) alpha and theta = T - T_ref a P1 field,
// the load of the thermal strain is F_th = s_l H(C(rho); theta) with the operator
//   H(w; theta)[d v + i] = sum_{c around v} w_c beta_0 thetabar_c |T_c| d_i phi_v^c,
// thetabar_c the mean of the d + 1 nodal values of theta (exact: div v is constant per cell).  H is linear in w and in theta,
// so one operator gives the load (w = C(rho)), dR/drho forward (w = C'(rho) drho) and dR/dT forward (theta := dT); its two
// transposes, with div(x)_c = sum_a grad phi_a . x[a], are
//   T_rho:  y_c = a C'(rho_c) beta_0 thetabar_c |T_c| sum_l s_l div(x_l)_c
//   T_T:    y_v = a sum_{c around v} C(rho_c) beta_0 |T_c| / (d + 1) sum_l s_l div(x_l)_c
// Layout as in elast_body.hip: column l at l * n_dof, the scales s_l by value.  What the columns share is computed once: the
// vector h_v of N per vertex, the cell factor of T_rho and T_T.  No float atomics: one writer per vertex and per cell, the
// cells around a vertex in ascending order and the columns in ascending order, so every call gives the same bits and column
// l does not depend on how many columns go with it.
#include <cmath>

#include "elast_internal.h"

namespace {

// thetabar_c: the mean of T over the vertices of the cell in `conn` order minus t_ref, or the uniform value (temp == null)
template <int D>
__device__ __forceinline__ double cell_theta(const int32_t (&v)[D + 1], const double* __restrict__ temp, double t_uniform,
                                             double t_ref) {
  if (!temp) return t_uniform - t_ref;
  double s = temp[v[0]];
#pragma unroll
  for (int b = 1; b <= D; ++b) s += temp[v[b]];
  return s * (1.0 / (D + 1)) - t_ref;
}

// sum_l s_l div(x_l)_c in ascending l; div(x)_c = sum_b g_b . x[v_b], b and the components ascending
template <int D>
__device__ __forceinline__ double scaled_div(const ElastCell<D> K, const double* __restrict__ x, int64_t n_dof, int n_cols,
                                             ColScalars sc) {
  double acc = 0.0;
  for (int l = 0; l < n_cols; ++l) {
    const double* __restrict__ xl = x + (int64_t)l * n_dof;
    double dv = 0.0;
#pragma unroll
    for (int b = 0; b <= D; ++b)
#pragma unroll
      for (int i = 0; i < D; ++i) dv += K.g[b][i] * xl[(int64_t)K.v[b] * D + i];
    acc += sc.v[l] * dv;
  }
  return acc;
}

// N: one thread per vertex row on the shared visit walk.  h_v once, then every column and component:
//   y = [accumulate ? y : (base ? base : 0)] + (a s_l) h_v[i],   or 0 on a fixed dof (fixed != null: the same set per column)
// w_c = C(rho_c), or C'(rho_c) drho_c with drho != null.
template <int D>
__global__ __launch_bounds__(EB) void k_elast_thermal_N(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, int method, double beta0, const double* __restrict__ rho, const double* __restrict__ drho,
    const double* __restrict__ temp, double t_uniform, double t_ref, int n_cols, ColScalars sc, double a,
    const double* __restrict__ base, const uint8_t* __restrict__ fixed, double* __restrict__ y, int accumulate) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  double h[D];
#pragma unroll
  for (int i = 0; i < D; ++i) h[i] = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    int32_t v[D + 1];
    double p[D + 1][D], g[D + 1][D], vol;
    load_cell<D>(conn, xv, t.c, v, p);
    simplex_grads<D>(p, g, vol);
    // g_a by selection: a run-time index would send g through scratch memory (k_pde_assemble)
    double ga[D];
#pragma unroll
    for (int k = 0; k < D; ++k) ga[k] = g[0][k];
#pragma unroll
    for (int b = 1; b <= D; ++b)
      if (t.a == b) {
#pragma unroll
        for (int k = 0; k < D; ++k) ga[k] = g[b][k];
      }
    const double r = rho[t.c];
    const double w = drho ? penal_d(method, r) * drho[t.c] : penal(method, r);
    const double q = w * (beta0 * cell_theta<D>(v, temp, t_uniform, t_ref)) * vol;
#pragma unroll
    for (int i = 0; i < D; ++i) h[i] += q * ga[i];
  }
  const int64_t n_dof = n_rows * D;
  for (int l = 0; l < n_cols; ++l) {
    const double as = a * sc.v[l];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int64_t k = (int64_t)l * n_dof + row * D + i;
      double r;
      if (fixed && fixed[row * D + i]) r = 0.0;
      else r = (accumulate ? y[k] : (base ? base[k] : 0.0)) + as * h[i];
      y[k] = r;
    }
  }
}

// T_rho: one thread per cell:  y_c = (accumulate ? y_c : 0) + a C'(rho_c) beta_0 thetabar_c |T_c| sum_l s_l div(x_l)_c
template <int D>
__global__ __launch_bounds__(EB) void k_elast_thermal_Trho(int64_t n_cell, int64_t n_dof, const int32_t* __restrict__ conn,
                                                           const double* __restrict__ xv, int method, double beta0,
                                                           const double* __restrict__ rho, const double* __restrict__ temp,
                                                           double t_uniform, double t_ref, const double* __restrict__ x,
                                                           int n_cols, ColScalars sc, double a, double* __restrict__ y,
                                                           int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= n_cell) return;
  const ElastCell<D> K = elast_cell<D>(conn, xv, c);
  const double q = penal_d(method, rho[c]) * (beta0 * cell_theta<D>(K.v, temp, t_uniform, t_ref)) * K.vol;
  const double val = a * (q * scaled_div<D>(K, x, n_dof, n_cols, sc));
  y[c] = accumulate ? y[c] + val : val;
}

// T_T: one thread per vertex on the visit walk:  y_v = (accumulate ? y_v : 0) + a sum_c C(rho_c) beta_0 |T_c| / (d+1) sum_l s_l div(x_l)_c
template <int D>
__global__ __launch_bounds__(EB) void k_elast_thermal_Ttemp(int64_t n_rows, const int64_t* __restrict__ vptr,
                                                            const int32_t* __restrict__ visit_cell,
                                                            const int32_t* __restrict__ conn, const double* __restrict__ xv,
                                                            int method, double beta0, const double* __restrict__ rho,
                                                            const double* __restrict__ x, int n_cols, ColScalars sc, double a,
                                                            double* __restrict__ y, int accumulate) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t n_dof = n_rows * D;
  double acc = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    const ElastCell<D> K = elast_cell<D>(conn, xv, t.c);
    const double q = penal(method, rho[t.c]) * beta0 * (K.vol * (1.0 / (D + 1)));
    acc += q * scaled_div<D>(K, x, n_dof, n_cols, sc);
  }
  const double val = a * acc;
  y[row] = accumulate ? y[row] + val : val;
}

}  // namespace

extern "C" int femo_elast_thermal_apply(femo_elast* e, int method, int product, int n_cols, const double* s, double alpha,
                                        const femo_vec* rho, const femo_vec* temp, double t_uniform, double t_ref, double a,
                                        const femo_vec* x, const femo_vec* base, int zero_fixed, femo_vec* y, int accumulate) {
  FEMO_REQUIRE(e && s && rho && y, "null argument");
  FEMO_REQUIRE(method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP, "femo_elast_thermal_apply: unknown method %d", method);
  FEMO_REQUIRE(product == FEMO_ELAST_THERMAL_N || product == FEMO_ELAST_THERMAL_T_RHO || product == FEMO_ELAST_THERMAL_T_TEMP,
               "femo_elast_thermal_apply: unknown product %d", product);
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= FEMO_ELAST_MAX_COLS, "femo_elast_thermal_apply: %d columns (1 to %d)", n_cols,
               FEMO_ELAST_MAX_COLS);
  femo_mesh* m = e->mesh;
  FEMO_REQUIRE((e->d == 2 || e->d == 3) && m->tdim == e->d, "femo_elast_thermal_apply: triangles or tetrahedra are needed");
  FEMO_REQUIRE(m->ctx->nranks == 1 && m->n_nbr == 0 && m->n_rows == m->n_vert,
               "femo_elast_thermal_apply: one rank only (partitioned meshes are out of scope)");
  const bool fwd = product == FEMO_ELAST_THERMAL_N;
  const int64_t nl = m->n_vert * e->d * n_cols;
  const int64_t ny = fwd ? nl : (product == FEMO_ELAST_THERMAL_T_RHO ? m->n_cell : m->n_vert);
  FEMO_REQUIRE(fwd || x, "femo_elast_thermal_apply: a transposed product needs x");
  FEMO_REQUIRE(rho->n >= m->n_cell && y->n >= ny && (!temp || temp->n >= m->n_vert) && (!x || x->n >= (fwd ? m->n_cell : nl)) &&
                   (!base || base->n >= nl),
               "vector size mismatch in femo_elast_thermal_apply");
  FEMO_REQUIRE(y != x && y != base && y != rho && y != temp, "femo_elast_thermal_apply: output aliases an input");
  FEMO_REQUIRE(fwd || (!base && !zero_fixed), "femo_elast_thermal_apply: base and zero_fixed belong to the forward product");
  FEMO_REQUIRE(!zero_fixed || e->has_fixed, "femo_elast_thermal_apply: zero_fixed without a fixed set (femo_elast_set_fixed)");
  ColScalars sc;
  for (int l = 0; l < FEMO_ELAST_MAX_COLS; ++l) sc.v[l] = l < n_cols ? s[l] : 0.0;
  const double beta0 = (3.0 * e->lam0 + 2.0 * e->mu0) * alpha;
  FEMO_TRY(femo_vec_await(rho));
  if (temp) FEMO_TRY(femo_vec_await(temp));
  if (x) FEMO_TRY(femo_vec_await(x));
  if (base) FEMO_TRY(femo_vec_await(base));
  femo_vec_touch(y);
  const double* tp = temp ? temp->d : nullptr;
  const double* xp = x ? x->d : nullptr;
  return elast_dispatch_d(e->d, [&](auto dim) {
    constexpr int D = decltype(dim)::value;
    if (product == FEMO_ELAST_THERMAL_T_RHO)
      return elast_launch_cells(e, k_elast_thermal_Trho<D>, m->n_vert * D, m->d_conn, m->d_x, method, beta0, rho->d, tp, t_uniform,
                                t_ref, xp, n_cols, sc, a, y->d, accumulate);
    if (product == FEMO_ELAST_THERMAL_T_TEMP)
      return elast_launch_rows(e, k_elast_thermal_Ttemp<D>, m->d_vptr, m->d_visit_cell, m->d_conn, m->d_x, method, beta0, rho->d,
                               xp, n_cols, sc, a, y->d, accumulate);
    return elast_launch_rows(e, k_elast_thermal_N<D>, m->d_vptr, m->d_visit_cell, m->d_conn, m->d_x, method, beta0, rho->d, xp, tp,
                             t_uniform, t_ref, n_cols, sc, a, base ? base->d : nullptr,
                             zero_fixed ? (const uint8_t*)e->d_fixed : nullptr, y->d, accumulate);
  });
}
