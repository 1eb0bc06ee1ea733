// SIMP topology optimisation: the lowest eigenfrequencies of the linear elasticity, K(rho) phi = lambda M(rho) phi on the
// free dofs (C-ABI in include/femo_hip.h: femo_elast_mass_apply_multi, femo_elast_eig_drho, femo_elast_eigs).
//
//   M(rho) = rho0 sum_e m(rho_e) M0_e,   M0_e[(a,i),(b,j)] = delta_ij |T_e| (1 + delta_ab) / ((d+1)(d+2))   (consistent P1)
//   m = rho (linear) or Du & Olhoff's law: rho for rho >= 0.1, 6e5 rho^6 - 5e6 rho^7 below (C^1 at 0.1)
//
// Layout as in elast_solve.hip: column l at l * n_dof.  The mass matrix is never stored: the product walks the cells around
// a vertex row on the shared visit walk (elast_internal.h).  No float atomics: one writer per dof and per cell; the cells
// around a vertex and the columns are summed in a fixed order, so every call gives the same bits, and a column of the mass
// product does not depend on how many columns travel with it.
//
// femo_elast_eigs is the block iteration of elast_block.hip on the pencil K phi = lambda M phi: the operator product is
// M_ff (k_elast_mass, one launch for the block), which is also the positive definite side, so the modes come back
// M-orthonormal with lambda ascending; the inner PCG K Y = M X starts from X.  It stops when
// |K x_k - lambda_k M x_k| <= rtol lambda_k |M x_k| for every k < n_modes.
#include "elast_internal.h"

#include <cmath>

using namespace elast_block;

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

struct ModeScalars { double lam[EMC], c[EMC]; };

// ------------------------------------------------------------------------------------------- mass product ----
// One thread per vertex row on the shared visit walk (elast_visits).  A visit of cell c as its vertex a adds, per column and
// component, w_c (sum_b x[v_b] + x[v_a]) with w_c = rho0 m(rho_c) |T_c| / ((d+1)(d+2)) (mass_row_add, mass_weight);
// y = a * that.  MASKED: fixed entries of x read as 0 and fixed entries of y are 0.  The geometry and the fixed bytes of a
// visit serve all columns.
template <int D, bool MASKED>
__global__ __launch_bounds__(EB) void k_elast_mass(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, const double* __restrict__ rho, int law, double rho0, const uint8_t* __restrict__ fixed,
    int n_cols, double a, const double* __restrict__ x, double* __restrict__ y) {
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
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    const ElastCellVolume<D> K = elast_cell_volume<D>(conn, xv, t.c);
    mass_row_add<D, MASKED>(K.v, t.a, mass_weight<D>(rho0 * mass_law(law, rho[t.c]), K.vol), fixed, n_cols, n_dof, x, acc);
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

// ------------------------------------------------------------------------------------ eigenvalue sensitivity ----
// One thread per cell, the modes in ascending order:
//   y_c (+)= sum_k c_k [ C'(rho_c) phi_k^T K0_c phi_k - lambda_k rho0 m'(rho_c) phi_k^T M0_c phi_k ]
template <int D>
__global__ __launch_bounds__(EB) void k_elast_eig_drho(int64_t n_cell, int64_t n_dof, const int32_t* __restrict__ conn,
                                                       const double* __restrict__ xv, const double* __restrict__ rho, int method,
                                                       int law, double rho0, double lam, double mu, int n_modes, ModeScalars ms,
                                                       const double* __restrict__ phi, double* __restrict__ y, int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= n_cell) return;
  const ElastCell<D> K = elast_cell<D>(conn, xv, c);
  const double r = rho[c];
  const double dC = penal_d(method, r) * K.vol;
  const double dM = mass_weight<D>(rho0 * mass_law_d(law, r), K.vol);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < EMC; ++k) {
    if (k >= n_modes) break;
    const double* __restrict__ u = phi + (int64_t)k * n_dof;
    double Gu[D][D], su[D], qu = 0.0;
    cell_gradient<D>(K.g, K.v, u, Gu);
    // the mass part sums qu + sum_i su_i^2: not the order of k_elast_mass_drho_T
#pragma unroll
    for (int i = 0; i < D; ++i) su[i] = 0.0;
#pragma unroll
    for (int b = 0; b <= D; ++b)
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double ub = u[(int64_t)K.v[b] * D + i];
        su[i] += ub;
        qu += ub * ub;
      }
    double mm = qu;
#pragma unroll
    for (int i = 0; i < D; ++i) mm += su[i] * su[i];
    acc += ms.c[k] * (dC * elastic_form<D>(Gu, Gu, lam, mu) - ms.lam[k] * (dM * mm));
  }
  y[c] = accumulate ? y[c] + acc : acc;
}

// ----------------------------------------------------------------------------------------------- launches ----
int mass_launch(femo_elast* e, int law, double rho0, bool masked, int n_cols, double a, const double* rho, const double* x,
                double* y) {
  femo_mesh* m = e->mesh;
  int rc = 0;
  elast_dispatch(e->d, masked, [&](auto dim, auto mask) {
    rc = elast_launch_rows(e, k_elast_mass<decltype(dim)::value, decltype(mask)::value>, m->d_vptr, m->d_visit_cell, m->d_conn,
                           m->d_x, rho, law, rho0, e->d_fixed, n_cols, a, x, y);
  });
  return rc;
}

}  // namespace

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_mass_apply_multi(femo_elast* e, int mass_law, double density, int masked, int n_cols, double a,
                                const femo_vec* rho, const femo_vec* x, femo_vec* y) {
  FEMO_REQUIRE(e && rho && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_mass_apply_multi: %d columns (1 to %d)", n_cols, EMC);
  FEMO_REQUIRE(mass_law == FEMO_ELAST_MASS_LINEAR || mass_law == FEMO_ELAST_MASS_DU_OLHOFF, "unknown mass law %d", mass_law);
  femo_mesh* m = e->mesh;
  const int64_t nl = m->n_vert * e->d * n_cols;
  FEMO_REQUIRE(rho->n >= m->n_cell && x->n >= nl && y->n >= nl,
               "vector size mismatch in femo_elast_mass_apply_multi: %d columns need %lld entries", n_cols, (long long)nl);
  FEMO_REQUIRE(!masked || e->has_fixed, "femo_elast_mass_apply_multi: masked product without a fixed set");
  FEMO_REQUIRE(y != x && y != rho, "femo_elast_mass_apply_multi: output aliases an input");
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(y);
  return mass_launch(e, mass_law, density, masked != 0, n_cols, a, rho->d, x->d, y->d);
}

int femo_elast_eig_drho(femo_elast* e, int method, int mass_law, double density, int n_modes, const femo_vec* rho,
                        const femo_vec* phi, const double* lambda, const double* c, femo_vec* y, int accumulate) {
  FEMO_REQUIRE(e && rho && phi && lambda && c && y, "null argument");
  FEMO_REQUIRE(n_modes >= 1 && n_modes <= EMC, "femo_elast_eig_drho: %d columns (1 to %d)", n_modes, EMC);
  FEMO_REQUIRE(method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP, "unknown penalisation method %d", method);
  FEMO_REQUIRE(mass_law == FEMO_ELAST_MASS_LINEAR || mass_law == FEMO_ELAST_MASS_DU_OLHOFF, "unknown mass law %d", mass_law);
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d;
  FEMO_REQUIRE(rho->n >= m->n_cell && y->n >= m->n_cell && phi->n >= n * n_modes,
               "vector size mismatch in femo_elast_eig_drho: %d columns need %lld entries", n_modes, (long long)(n * n_modes));
  FEMO_REQUIRE(y != rho && y != phi, "femo_elast_eig_drho: output aliases an input");
  ModeScalars ms;
  for (int k = 0; k < EMC; ++k) { ms.lam[k] = k < n_modes ? lambda[k] : 0.0; ms.c[k] = k < n_modes ? c[k] : 0.0; }
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(phi));
  femo_vec_touch(y);
  return elast_dispatch_d(e->d, [&](auto dim) {
    return elast_launch_cells(e, k_elast_eig_drho<decltype(dim)::value>, n, m->d_conn, m->d_x, rho->d, method, mass_law, density,
                              e->lam0, e->mu0, n_modes, ms, phi->d, y->d, accumulate);
  });
}

int femo_elast_eigs(femo_elast* e, int mass_law, double density, const femo_vec* rho, int n_modes, int block, femo_vec* X,
                    const femo_eig_opts* opts, double* lambda, femo_eig_info* info) {
  FEMO_REQUIRE(e && rho && X && opts && lambda, "null argument");
  FEMO_REQUIRE(block >= 1 && block <= EMC, "femo_elast_eigs: %d columns (1 to %d)", block, EMC);
  FEMO_REQUIRE(n_modes >= 1 && n_modes <= block, "femo_elast_eigs: %d modes in a block of %d (1 <= n_modes <= block)", n_modes, block);
  FEMO_REQUIRE(mass_law == FEMO_ELAST_MASS_LINEAR || mass_law == FEMO_ELAST_MASS_DU_OLHOFF, "unknown mass law %d", mass_law);
  FEMO_REQUIRE(e->assembled, "femo_elast_eigs: assemble K first");
  FEMO_REQUIRE(e->has_fixed, "femo_elast_eigs: no fixed set -- K is singular on a free-free structure (a shift is out of scope)");
  FEMO_REQUIRE(density > 0.0 && std::isfinite(density) && opts->rtol > 0.0 && opts->pcg_rtol > 0.0,
               "femo_elast_eigs: need density > 0, rtol > 0 and pcg_rtol > 0");
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d, nl = n * block;
  FEMO_REQUIRE(rho->n >= m->n_cell && X->n >= nl, "vector size mismatch in femo_elast_eigs: %d columns need %lld entries", block,
               (long long)nl);
  FEMO_REQUIRE(X != rho, "femo_elast_eigs: the block aliases the density");
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(X));
  femo_vec_touch(X);
  // K phi = lambda M phi: the product M_ff is the positive definite side; lambda ascending, the PCG from the previous block
  const Pencil pencil = {"femo_elast_eigs", "M", [=](int n_cols, const double* x, double* y) {
                           return mass_launch(e, mass_law, density, true, n_cols, 1.0, rho->d, x, y); },
                         /*p_is_op*/ true, /*descending*/ false, /*zero_guess*/ 0, /*max_outer*/ 200, /*positive_only*/ false,
                         /*reciprocal*/ false};
  return block_iteration(e, pencil, n_modes, block, X, opts, lambda, info);
}

}  // extern "C"
