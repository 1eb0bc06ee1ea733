// SIMP topology optimisation: linearised buckling load factors of the linear elasticity, (K + lambda K_G(u, rho)) phi = 0 on
// the free dofs (C-ABI in include/femo_hip.h: femo_elast_geom_stress, femo_elast_geom_stress_get,
// femo_elast_geom_apply_multi, femo_elast_buckle_du, femo_elast_buckle_drho, femo_elast_buckle).
//
//   sigma_e = C(rho_e) sigma_0(u_e),   sigma_0 = lam0 tr(eps) I + 2 mu0 eps (the d x d in-plane block)
//   K_G,e[(a,i),(b,j)] = delta_ij |T_e| g_a . sigma_e g_b,   g_a the barycentric gradients
//
// Layout as in elast_solve.hip: column l at l * n_dof.  K_G is never stored: the product walks the cells around a vertex row
// like k_elast_mass (the shared visit walk), and reads the cell stress from a buffer of the handle that
// femo_elast_geom_stress fills once per solve, so the product touches neither u nor rho.  No float atomics: one writer per
// dof and per cell; the cells around a
// vertex, the columns and the modes are summed in a fixed order, so every call gives the same bits, and a column of the
// product does not depend on how many columns travel with it.
//
// femo_elast_buckle is the block iteration of elast_block.hip on the pencil (-K_G) phi = mu K phi, mu = 1 / lambda, K
// positive definite and -K_G indefinite, for the largest positive mu: the operator product is (-K_G)_ff (k_elast_geom, one
// launch for the block), the modes come back K-orthonormal with mu descending, and the inner PCG K Y = (-K_G) X starts from
// zero (its stopping level is relative to |B|).  It stops when |(-K_G) x_k - mu_k K x_k| <= rtol mu_k |K x_k| and mu_k > 0
// for every k < n_modes.  The block converges to the modes of largest |mu| of either sign (negative mu: buckling under the
// reversed load): when one of the n_modes largest Ritz values is still not positive at the last outer step, the block is
// too small for this load and the call fails.
#include "elast_internal.h"

#include <cmath>

using namespace elast_block;

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

struct ModeWeights { double w1[EMC], w2[EMC]; };

// component of the symmetric d x d tensor at (i, k): the diagonal first, then 01[, 02, 12]
template <int D>
__device__ __forceinline__ constexpr int sym_at(int i, int k) {
  return i == k ? i : (D == 2 ? 2 : (i + k + 2));
}

// sigma_0 = lam tr(eps) I + 2 mu eps of the gradient Gu
template <int D>
__device__ __forceinline__ void solid_stress(const double (&Gu)[D][D], double lam, double mu, double (&s)[D][D]) {
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) tr += Gu[i][i];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int k = 0; k < D; ++k) s[i][k] = mu * (Gu[i][k] + Gu[k][i]) + (i == k ? lam * tr : 0.0);
}

// H (+)= w (grad phi)^T (grad phi): H[k][l] += w sum_i d_k phi_i d_l phi_i
template <int D>
__device__ __forceinline__ void add_gram(const double (&G)[D][D], double w, double (&H)[D][D]) {
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int l = 0; l < D; ++l) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) s += G[i][k] * G[i][l];
      H[k][l] += w * s;
    }
}

// ------------------------------------------------------------------------------------------- cell stress ----
// One thread per cell: the d (d+1) / 2 components of C(rho_c) sigma_0(u_c), component-major.
template <int D>
__global__ __launch_bounds__(EB) void k_elast_cell_stress(int64_t n_cell, const int32_t* __restrict__ conn,
                                                          const double* __restrict__ xv, const double* __restrict__ rho,
                                                          int method, double lam, double mu, const double* __restrict__ u,
                                                          double* __restrict__ sig) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= n_cell) return;
  const ElastCell<D> K = elast_cell<D>(conn, xv, c);
  double Gu[D][D], s[D][D];
  cell_gradient<D>(K.g, K.v, u, Gu);
  solid_stress<D>(Gu, lam, mu, s);
  const double C = penal(method, rho[c]);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int k = i; k < D; ++k) sig[(int64_t)sym_at<D>(i, k) * n_cell + c] = C * s[i][k];
}

// ------------------------------------------------------------------------------------- geometric stiffness ----
// One thread per vertex row on the shared visit walk (elast_visits).  A visit of cell c as its vertex a adds, per column and
// component i, |T_c| sum_k (sigma_c g_a)_k d_k x_i = sum_b w_b x_i[v_b] with w_b = |T_c| (sigma_c g_a) . g_b; y = a * that.
// MASKED: fixed entries of x read as 0 and fixed entries of y are 0.  The geometry, the stress, the weights and the fixed
// bytes of a visit (one bit per dof of the cell) serve all columns.
template <int D, bool MASKED>
__global__ __launch_bounds__(EB) void k_elast_geom(
    int64_t n_rows, int64_t n_cell, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell,
    const int32_t* __restrict__ conn, const double* __restrict__ xv, const double* __restrict__ sig,
    const uint8_t* __restrict__ fixed, int n_cols, double a, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t n_dof = n_rows * D;
  double acc[EMC][D];
#pragma unroll
  for (int l = 0; l < EMC; ++l)
#pragma unroll
    for (int i = 0; i < D; ++i) acc[l][i] = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit vis = elast_visit(V, visit_cell, s);
    if (!vis.live) continue;
    const int64_t c = vis.c;
    const int va = vis.a;
    const ElastCell<D> K = elast_cell<D>(conn, xv, c);
    double w[D + 1];
    {
      double t[D], ga[D];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        ga[k] = 0.0;
#pragma unroll
        for (int b = 0; b <= D; ++b) ga[k] = b == va ? K.g[b][k] : ga[k];
      }
#pragma unroll
      for (int k = 0; k < D; ++k) {
        double tk = 0.0;
#pragma unroll
        for (int m = 0; m < D; ++m) tk += sig[(int64_t)sym_at<D>(k < m ? k : m, k < m ? m : k) * n_cell + c] * ga[m];
        t[k] = K.vol * tk;
      }
#pragma unroll
      for (int b = 0; b <= D; ++b) {
        double wb = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) wb += t[k] * K.g[b][k];
        w[b] = wb;
      }
    }
    unsigned fx = 0u;                                                 // bit b * D + i: dof (v_b, i) is fixed
    if (MASKED) {
#pragma unroll
      for (int b = 0; b <= D; ++b)
#pragma unroll
        for (int i = 0; i < D; ++i) fx |= fixed[(int64_t)K.v[b] * D + i] ? 1u << (b * D + i) : 0u;
    }
#pragma unroll
    for (int l = 0; l < EMC; ++l) {
      if (l >= n_cols) break;
      const double* __restrict__ xl = x + (int64_t)l * n_dof;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double sx = 0.0;
#pragma unroll
        for (int b = 0; b <= D; ++b) {
          const double t = xl[(int64_t)K.v[b] * D + i];               // loaded whatever the mask says: a select, no branch
          sx += w[b] * ((fx >> (b * D + i)) & 1u ? 0.0 : t);
        }
        acc[l][i] += sx;
      }
    }
  }
#pragma unroll
  for (int l = 0; l < EMC; ++l) {
    if (l >= n_cols) break;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const bool f = MASKED && fixed[row * D + i];
      y[(int64_t)l * n_dof + row * D + i] = f ? 0.0 : a * acc[l][i];
    }
  }
}

// --------------------------------------------------------------------------------------- d lambda / d u ----
// One thread per vertex row, the same walk: out[(v,j)] = sum_{c around v} C(rho_c) |T_c| (Sigma_H g_a)_j with
// Sigma_H = lam0 tr(H) I + 2 mu0 H and H = sum_k w_k (grad phi_k)^T (grad phi_k), the modes in ascending order.
template <int D>
__global__ __launch_bounds__(EB) void k_elast_buckle_du(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, const double* __restrict__ rho, int method, double lam, double mu, int n_modes,
    ModeWeights mw, const double* __restrict__ phi, double* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t n_dof = n_rows * D;
  double acc[D];
#pragma unroll
  for (int j = 0; j < D; ++j) acc[j] = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit vis = elast_visit(V, visit_cell, s);
    if (!vis.live) continue;
    const int64_t c = vis.c;
    const int va = vis.a;
    const ElastCell<D> K = elast_cell<D>(conn, xv, c);
    double H[D][D];
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
      for (int l = 0; l < D; ++l) H[k][l] = 0.0;
#pragma unroll 1
    for (int k = 0; k < n_modes; ++k) {
      double G[D][D];
      cell_gradient<D>(K.g, K.v, phi + (int64_t)k * n_dof, G);
      add_gram<D>(G, mw.w1[k], H);
    }
    double tr = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) tr += H[k][k];
    const double cw = penal(method, rho[c]) * K.vol;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double t = 0.0;
#pragma unroll
      for (int m = 0; m < D; ++m) {
        double gam = 0.0;
#pragma unroll
        for (int b = 0; b <= D; ++b) gam = b == va ? K.g[b][m] : gam;
        t += (2.0 * mu * H[j][m] + (j == m ? lam * tr : 0.0)) * gam;
      }
      acc[j] += cw * t;
    }
  }
#pragma unroll
  for (int j = 0; j < D; ++j) out[row * D + j] = acc[j];
}

// ------------------------------------------------------------------------------------- d lambda / d rho ----
// One thread per cell, the modes in ascending order:
//   y_c (+)= C'(rho_c) |T_c| sum_k [ w1_k (lam0 (div phi_k)^2 + 2 mu0 eps(phi_k) : eps(phi_k)) + w2_k sigma_0(u_c) : H_c(phi_k) ]
// The first bracket is the arithmetic of elastic_form (elast_internal.h) in a text of its own: through the helper the 3-D
// kernel goes from 94 to 78 registers and from 5 to 6 waves, which is not the code object it was (DESIGN_LOG.md R26).
template <int D>
__global__ __launch_bounds__(EB) void k_elast_buckle_drho(int64_t n_cell, int64_t n_dof, const int32_t* __restrict__ conn,
                                                          const double* __restrict__ xv, const double* __restrict__ rho,
                                                          int method, double lam, double mu, int n_modes, ModeWeights mw,
                                                          const double* __restrict__ u, const double* __restrict__ phi,
                                                          double* __restrict__ y, int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= n_cell) return;
  const ElastCell<D> K = elast_cell<D>(conn, xv, c);
  double Gu[D][D], s0[D][D];
  cell_gradient<D>(K.g, K.v, u, Gu);
  solid_stress<D>(Gu, lam, mu, s0);
  const double dC = penal_d(method, rho[c]) * K.vol;
  double acc = 0.0;
#pragma unroll 1
  for (int k = 0; k < n_modes; ++k) {
    double G[D][D];
    cell_gradient<D>(K.g, K.v, phi + (int64_t)k * n_dof, G);
    double div = 0.0, ee = 0.0, sh = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) div += G[i][i];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) { const double t = G[i][j] + G[j][i]; ee += 0.25 * t * t; }
#pragma unroll
    for (int m = 0; m < D; ++m)
#pragma unroll
      for (int l = 0; l < D; ++l) {
        double h = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) h += G[i][m] * G[i][l];
        sh += s0[m][l] * h;
      }
    acc += mw.w1[k] * (dC * (lam * div * div + 2.0 * mu * ee)) + mw.w2[k] * (dC * sh);
  }
  y[c] = accumulate ? y[c] + acc : acc;
}

// ----------------------------------------------------------------------------------------------- launches ----
int stress_launch(femo_elast* e, int method, const double* rho, const double* u) {
  femo_mesh* m = e->mesh;
  if (!e->w_gstress) FEMO_TRY(dalloc(&e->w_gstress, (int64_t)(e->d * (e->d + 1) / 2) * m->n_cell));
  FEMO_TRY(elast_dispatch_d(e->d, [&](auto dim) {
    return elast_launch_cells(e, k_elast_cell_stress<decltype(dim)::value>, m->d_conn, m->d_x, rho, method, e->lam0, e->mu0, u,
                              e->w_gstress);
  }));
  e->has_gstress = true;
  return 0;
}

int geom_launch(femo_elast* e, bool masked, int n_cols, double a, const double* x, double* y) {
  femo_mesh* m = e->mesh;
  int rc = 0;
  elast_dispatch(e->d, masked, [&](auto dim, auto mask) {
    rc = elast_launch_rows(e, k_elast_geom<decltype(dim)::value, decltype(mask)::value>, m->n_cell, m->d_vptr, m->d_visit_cell,
                           m->d_conn, m->d_x, e->w_gstress, e->d_fixed, n_cols, a, x, y);
  });
  return rc;
}

}  // namespace

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_geom_stress(femo_elast* e, int method, const femo_vec* rho, const femo_vec* u) {
  FEMO_REQUIRE(e && rho && u, "null argument");
  FEMO_REQUIRE(method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP, "unknown penalisation method %d", method);
  femo_mesh* m = e->mesh;
  FEMO_REQUIRE(rho->n >= m->n_cell && u->n >= m->n_vert * e->d, "vector size mismatch in femo_elast_geom_stress: need %lld cells and %lld dofs",
               (long long)m->n_cell, (long long)(m->n_vert * e->d));
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(u));
  return stress_launch(e, method, rho->d, u->d);
}

int femo_elast_geom_stress_get(femo_elast* e, femo_vec* out) {
  FEMO_REQUIRE(e && out, "null argument");
  FEMO_REQUIRE(e->has_gstress, "femo_elast_geom_stress_get: no cell stress -- call femo_elast_geom_stress first");
  const int64_t n = (int64_t)(e->d * (e->d + 1) / 2) * e->mesh->n_cell;
  FEMO_REQUIRE(out->n >= n, "vector size mismatch in femo_elast_geom_stress_get: need %lld entries", (long long)n);
  femo_vec_touch(out);
  FEMO_HIP_CHECK(hipMemcpyAsync(out->d, e->w_gstress, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, e->mesh->ctx->stream));
  return 0;
}

int femo_elast_geom_apply_multi(femo_elast* e, int masked, int n_cols, double a, const femo_vec* x, femo_vec* y) {
  FEMO_REQUIRE(e && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_geom_apply_multi: %d columns (1 to %d)", n_cols, EMC);
  const int64_t nl = e->mesh->n_vert * e->d * n_cols;
  FEMO_REQUIRE(x->n >= nl && y->n >= nl, "vector size mismatch in femo_elast_geom_apply_multi: %d columns need %lld entries", n_cols,
               (long long)nl);
  FEMO_REQUIRE(e->has_gstress, "femo_elast_geom_apply_multi: no cell stress -- call femo_elast_geom_stress first");
  FEMO_REQUIRE(!masked || e->has_fixed, "femo_elast_geom_apply_multi: masked product without a fixed set");
  FEMO_REQUIRE(y != x, "femo_elast_geom_apply_multi: output aliases an input");
  FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(y);
  return geom_launch(e, masked != 0, n_cols, a, x->d, y->d);
}

int femo_elast_buckle_du(femo_elast* e, int method, int n_modes, const femo_vec* rho, const femo_vec* phi, const double* w,
                         femo_vec* out) {
  FEMO_REQUIRE(e && rho && phi && w && out, "null argument");
  FEMO_REQUIRE(n_modes >= 1 && n_modes <= EMC, "femo_elast_buckle_du: %d columns (1 to %d)", n_modes, EMC);
  FEMO_REQUIRE(method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP, "unknown penalisation method %d", method);
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d;
  FEMO_REQUIRE(rho->n >= m->n_cell && out->n >= n && phi->n >= n * n_modes,
               "vector size mismatch in femo_elast_buckle_du: %d columns need %lld entries", n_modes, (long long)(n * n_modes));
  FEMO_REQUIRE(out != rho && out != phi, "femo_elast_buckle_du: output aliases an input");
  ModeWeights mw;
  for (int k = 0; k < EMC; ++k) { mw.w1[k] = k < n_modes ? w[k] : 0.0; mw.w2[k] = 0.0; }
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(phi));
  femo_vec_touch(out);
  return elast_dispatch_d(e->d, [&](auto dim) {
    return elast_launch_rows(e, k_elast_buckle_du<decltype(dim)::value>, m->d_vptr, m->d_visit_cell, m->d_conn, m->d_x, rho->d,
                             method, e->lam0, e->mu0, n_modes, mw, phi->d, out->d);
  });
}

int femo_elast_buckle_drho(femo_elast* e, int method, int n_modes, const femo_vec* rho, const femo_vec* u, const femo_vec* phi,
                           const double* w1, const double* w2, femo_vec* y, int accumulate) {
  FEMO_REQUIRE(e && rho && u && phi && w1 && w2 && y, "null argument");
  FEMO_REQUIRE(n_modes >= 1 && n_modes <= EMC, "femo_elast_buckle_drho: %d columns (1 to %d)", n_modes, EMC);
  FEMO_REQUIRE(method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP, "unknown penalisation method %d", method);
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d;
  FEMO_REQUIRE(rho->n >= m->n_cell && y->n >= m->n_cell && u->n >= n && phi->n >= n * n_modes,
               "vector size mismatch in femo_elast_buckle_drho: %d columns need %lld entries", n_modes, (long long)(n * n_modes));
  FEMO_REQUIRE(y != rho && y != u && y != phi, "femo_elast_buckle_drho: output aliases an input");
  ModeWeights mw;
  for (int k = 0; k < EMC; ++k) { mw.w1[k] = k < n_modes ? w1[k] : 0.0; mw.w2[k] = k < n_modes ? w2[k] : 0.0; }
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(u)); FEMO_TRY(femo_vec_await(phi));
  femo_vec_touch(y);
  return elast_dispatch_d(e->d, [&](auto dim) {
    return elast_launch_cells(e, k_elast_buckle_drho<decltype(dim)::value>, n, m->d_conn, m->d_x, rho->d, method, e->lam0, e->mu0,
                              n_modes, mw, u->d, phi->d, y->d, accumulate);
  });
}

int femo_elast_buckle(femo_elast* e, int method, const femo_vec* rho, const femo_vec* u, int n_modes, int block, femo_vec* X,
                      const femo_eig_opts* opts, double* lambda, femo_eig_info* info) {
  FEMO_REQUIRE(e && rho && u && X && opts && lambda, "null argument");
  FEMO_REQUIRE(block >= 1 && block <= EMC, "femo_elast_buckle: %d columns (1 to %d)", block, EMC);
  FEMO_REQUIRE(n_modes >= 1 && n_modes <= block, "femo_elast_buckle: %d modes in a block of %d (1 <= n_modes <= block)", n_modes, block);
  FEMO_REQUIRE(method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP, "unknown penalisation method %d", method);
  FEMO_REQUIRE(e->assembled, "femo_elast_buckle: assemble K first");
  FEMO_REQUIRE(e->has_fixed, "femo_elast_buckle: no fixed set -- K is singular on a free-free structure");
  FEMO_REQUIRE(opts->rtol > 0.0 && opts->pcg_rtol > 0.0, "femo_elast_buckle: need rtol > 0 and pcg_rtol > 0");
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d, nl = n * block;
  FEMO_REQUIRE(rho->n >= m->n_cell && u->n >= n && X->n >= nl, "vector size mismatch in femo_elast_buckle: %d columns need %lld entries",
               block, (long long)nl);
  FEMO_REQUIRE(X != rho && X != u, "femo_elast_buckle: the block aliases the density or the state");
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(u)); FEMO_TRY(femo_vec_await(X));
  femo_vec_touch(X);
  FEMO_TRY(stress_launch(e, method, rho->d, u->d));
  // (-K_G) phi = mu K phi: K is the positive definite side; mu descending and positive, lambda = 1 / mu; the PCG from zero, so
  // that its stopping level is relative to |B|
  const Pencil pencil = {"femo_elast_buckle", "K", [=](int n_cols, const double* x, double* y) {
                           return geom_launch(e, true, n_cols, -1.0, x, y); },
                         /*p_is_op*/ false, /*descending*/ true, /*zero_guess*/ 1, /*max_outer*/ 400, /*positive_only*/ true,
                         /*reciprocal*/ true};
  return block_iteration(e, pencil, n_modes, block, X, opts, lambda, info);
}

}  // extern "C"
