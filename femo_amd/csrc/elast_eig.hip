// SIMP topology optimisation: the lowest eigenfrequencies of the linear elasticity, K(rho) phi = lambda M(rho) phi on the
// free dofs (C-ABI in include/femo_hip.h: femo_elast_mass_apply_multi, femo_elast_eig_drho, femo_elast_eigs).
//
//   M(rho) = rho0 sum_e m(rho_e) M0_e,   M0_e[(a,i),(b,j)] = delta_ij |T_e| (1 + delta_ab) / ((d+1)(d+2))   (consistent P1)
//   m = rho (linear) or Du & Olhoff's law: rho for rho >= 0.1, 6e5 rho^6 - 5e6 rho^7 below (C^1 at 0.1)
//
// Layout as in elast_solve.hip: column l at l * n_dof.  The mass matrix is never stored: the product walks the cells around
// a vertex row like k_elast_body_N.  No float atomics: one writer per dof and per cell; the cells around a vertex and the
// columns are summed in a fixed order, so every call gives the same bits, and a column of the mass product does not depend
// on how many columns travel with it.
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
// One thread per vertex row, the visit walk of k_elast_body_N.  A visit of cell c as its vertex a adds, per column and
// component, w_c (sum_b x[v_b] + x[v_a]) with w_c = rho0 m(rho_c) |T_c| / ((d+1)(d+2)); y = a * that.  MASKED: fixed entries
// of x read as 0 and fixed entries of y are 0.  The geometry and the fixed bytes of a visit serve all columns.
template <int D, bool MASKED>
__global__ __launch_bounds__(EB) void k_elast_mass(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, const double* __restrict__ rho, int law, double rho0, const uint8_t* __restrict__ fixed,
    int n_cols, double a, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t slice = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t vb = vptr[slice];
  const int nvis = (int)((vptr[slice + 1] - vb) >> 6);
  const int64_t n_dof = n_rows * D;
  double acc[EMC][D];
#pragma unroll
  for (int l = 0; l < EMC; ++l)
#pragma unroll
    for (int i = 0; i < D; ++i) acc[l][i] = 0.0;
  for (int s = 0; s < nvis; ++s) {
    const int32_t ca = visit_cell[vb + (int64_t)s * 64 + lane];
    if (ca < 0) continue;
    const int64_t c = ca >> 2;
    const int va = ca & 3;
    int32_t v[D + 1];
    double p[D + 1][D];
    load_cell<D>(conn, xv, c, v, p);
    const double w = rho0 * mass_law(law, rho[c]) * (simplex_volume<D>(p) * (1.0 / ((D + 1) * (D + 2))));
    bool fx[D + 1][D];
#pragma unroll
    for (int b = 0; b <= D; ++b)
#pragma unroll
      for (int i = 0; i < D; ++i) fx[b][i] = MASKED && fixed[(int64_t)v[b] * D + i];
#pragma unroll
    for (int l = 0; l < EMC; ++l) {
      if (l >= n_cols) break;
      const double* __restrict__ xl = x + (int64_t)l * n_dof;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double sx = 0.0, own = 0.0;
#pragma unroll
        for (int b = 0; b <= D; ++b) {
          const double t = fx[b][i] ? 0.0 : xl[(int64_t)v[b] * D + i];
          sx += t;
          if (b == va) own = t;
        }
        acc[l][i] += w * (sx + own);
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
  int32_t v[D + 1];
  double p[D + 1][D], g[D + 1][D], vol;
  load_cell<D>(conn, xv, c, v, p);
  simplex_grads<D>(p, g, vol);
  const double r = rho[c];
  const double dC = penal_d(method, r) * vol;
  const double dM = rho0 * mass_law_d(law, r) * (vol * (1.0 / ((D + 1) * (D + 2))));
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < EMC; ++k) {
    if (k >= n_modes) break;
    const double* __restrict__ u = phi + (int64_t)k * n_dof;
    double Gu[D][D], su[D], qu = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      su[i] = 0.0;
#pragma unroll
      for (int j = 0; j < D; ++j) Gu[i][j] = 0.0;
    }
#pragma unroll
    for (int b = 0; b <= D; ++b)
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double ub = u[(int64_t)v[b] * D + i];
        su[i] += ub;
        qu += ub * ub;
#pragma unroll
        for (int j = 0; j < D; ++j) Gu[i][j] += ub * g[b][j];
      }
    double div = 0.0, ee = 0.0, mm = qu;
#pragma unroll
    for (int i = 0; i < D; ++i) { div += Gu[i][i]; mm += su[i] * su[i]; }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) { const double t = Gu[i][j] + Gu[j][i]; ee += 0.25 * t * t; }
    acc += ms.c[k] * (dC * (lam * div * div + 2.0 * mu * ee) - ms.lam[k] * (dM * mm));
  }
  y[c] = accumulate ? y[c] + acc : acc;
}

// ----------------------------------------------------------------------------------------------- launches ----
int mass_launch(femo_elast* e, int law, double rho0, bool masked, int n_cols, double a, const double* rho, const double* x,
                double* y) {
  femo_mesh* m = e->mesh;
  hipStream_t st = m->ctx->stream;
#define FEMO_MASS(D, MK) hipLaunchKernelGGL((k_elast_mass<D, MK>), dim3(grid_of(m->n_rows)), dim3(EB), 0, st, m->n_rows, m->d_vptr, \
                                            m->d_visit_cell, m->d_conn, m->d_x, rho, law, rho0, e->d_fixed, n_cols, a, x, y)
  if (e->d == 2) { if (masked) FEMO_MASS(2, true); else FEMO_MASS(2, false); }
  else { if (masked) FEMO_MASS(3, true); else FEMO_MASS(3, false); }
#undef FEMO_MASS
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
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
  hipStream_t st = m->ctx->stream;
  if (e->d == 2)
    hipLaunchKernelGGL(k_elast_eig_drho<2>, dim3(grid_of(m->n_cell)), dim3(EB), 0, st, m->n_cell, n, m->d_conn, m->d_x, rho->d, method,
                       mass_law, density, e->lam0, e->mu0, n_modes, ms, phi->d, y->d, accumulate);
  else
    hipLaunchKernelGGL(k_elast_eig_drho<3>, dim3(grid_of(m->n_cell)), dim3(EB), 0, st, m->n_cell, n, m->d_conn, m->d_x, rho->d, method,
                       mass_law, density, e->lam0, e->mu0, n_modes, ms, phi->d, y->d, accumulate);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
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
