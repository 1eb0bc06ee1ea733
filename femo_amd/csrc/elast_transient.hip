// SIMP topology optimisation: transient response of the linear elasticity by a device-resident Newmark(beta, gamma) march
// with Rayleigh damping C = c_m M + c_k K (C-ABI in include/femo_hip.h: femo_elast_newmark_march, femo_elast_newmark_apply,
// femo_elast_newmark_drho, femo_elast_newmark_dots, femo_elast_newmark_outer).
//
// The scheme is written as its two-step recurrence in the displacements only; with u_0 = u_-1 = 0 and g_-1 = 0, for
// n = 0 ... N - 1:
//
//   A1 u_{n+1} + A0 u_n + A- u_{n-1} = dt^2 (beta g_{n+1} + b0 g_n + b- g_{n-1}) F,      A_j = m_j M + k_j K
//   m1 =  1 + gamma dt c_m          k1 = gamma dt c_k        + beta dt^2
//   m0 = -2 + (1 - 2 gamma) dt c_m  k0 = (1 - 2 gamma) dt c_k + b0 dt^2      b0 = 1/2 + gamma - 2 beta
//   m- =  1 - (1 - gamma) dt c_m    k- = -(1 - gamma) dt c_k  + b- dt^2      b- = 1/2 - gamma + beta
//
// The history U = (u_1 ... u_N), column t = u_{t+1} at t * n_dof, solves the block lower-banded block-Toeplitz system
// L U = B with symmetric blocks, so L^T is the same recurrence run from the last column to the first: ONE loop with a
// `reverse` flag is the state solve, the forward-mode solve and the adjoint solve.  With a fixed set, A1 carries identity
// rows / columns on the fixed dofs and A0, A- zero ones: L is the identity there.
//
// One step issues
//   b = (rhs_t - A0 u_prev - A- u_prev2) / k1     k_newmark_band<NV = 2>: K's blocks, M's scalars and the column indices are
//                                                 read ONCE for both vectors; the coefficients travel by value
//   the first guess 2 u_prev - u_prev2            k_newmark_guess (zero on fixed dofs)
//   (K + sigma' M) u = b, sigma' = m1 / k1        the batched PCG of elast_solve.hip with the shifted product as its operator
//                                                 and the inverse diagonal blocks of K + sigma' M (k_newmark_dinv) in the
//                                                 Jacobi term; the lattice term of the multilevel form is that of K
// on the context's stream; the host waits only where the PCG polls its flag.  Nothing is allocated after the first step.
// No float atomics: the same inputs give the same bits.
//
// k_newmark_band<NV = 3> with the column (time step) dimension in its grid is the banded product Y = L X or L^T X,
// FEMO_ELAST_MAX_COLS columns per launch.  dR/drho of R_t = A1 u_{t+1} + A0 u_t + A- u_{t-1} - ... is
// C'(rho) K0 uK_t + density m'(rho) M0 uM_t with uK_t = sum_j k_j u_{t+j}, uM_t = sum_j m_j u_{t+j} (k_newmark_combine), fed
// to femo_elast_drho_multi / femo_elast_mass_drho_multi in windows of FEMO_ELAST_MAX_COLS columns in ascending order.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

// the scalars of the three blocks, index 0: A1, 1: A0, 2: A-
struct NmBlocks { double m[3], k[3], b0, bm; };

NmBlocks nm_blocks(const femo_newmark_params& p) {
  NmBlocks c;
  const double dt = p.dt, dt2 = p.dt * p.dt;
  c.b0 = 0.5 + p.gamma - 2.0 * p.beta;
  c.bm = 0.5 - p.gamma + p.beta;
  c.m[0] = 1.0 + p.gamma * dt * p.c_m;
  c.k[0] = p.gamma * dt * p.c_k + p.beta * dt2;
  c.m[1] = -2.0 + (1.0 - 2.0 * p.gamma) * dt * p.c_m;
  c.k[1] = (1.0 - 2.0 * p.gamma) * dt * p.c_k + c.b0 * dt2;
  c.m[2] = 1.0 - (1.0 - p.gamma) * dt * p.c_m;
  c.k[2] = -(1.0 - p.gamma) * dt * p.c_k + c.bm * dt2;
  return c;
}

bool params_ok(const femo_newmark_params* p) {
  return std::isfinite(p->dt) && p->dt > 0.0 && std::isfinite(p->beta) && p->beta > 0.0 && std::isfinite(p->gamma) &&
         p->gamma >= 0.5 && std::isfinite(p->c_m) && p->c_m >= 0.0 && std::isfinite(p->c_k) && p->c_k >= 0.0;
}

// what k_newmark_band adds up: input i is column (col + off[i]) of X, absent outside [0, n_steps), and enters as
// (m[i] M + k[i] K) x_i.  cr scales the right-hand side on the free rows, crf on the fixed ones; idc adds idc x_0 on the
// fixed rows (the identity of A1).
struct BandArgs {
  double m[3], k[3];
  int off[3];
  double cr, crf, idc;
};

// Column col0 + blockIdx.y of
//   y = cr rhs + sum_{i < NV} (m_i M + k_i K) x_i
// over the SELL rows (elast_row_walk): each d x d block of K, each scalar of M and each column index is read once for the NV
// vectors.  MASKED: the fixed entries of every x read as 0; a fixed row gives crf rhs + idc x_0.  rhs may be null.  rhs and
// y are those of the launch's first column, their columns rs and vs apart.
template <int D, bool MASKED, int NV>
__global__ __launch_bounds__(EB) void k_newmark_band(
    int64_t n_rows, const int64_t* __restrict__ mptr, const int32_t* __restrict__ cols, const int32_t* __restrict__ rowlen,
    const double* __restrict__ vals, const double* __restrict__ diag, const double* __restrict__ mvals,
    const double* __restrict__ mdiag, const uint8_t* __restrict__ fixed, BandArgs A, int n_steps, int col0, int64_t vs,
    const double* __restrict__ X, const double* __restrict__ rhs, int64_t rs, double* __restrict__ y) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int col = col0 + (int)blockIdx.y;
  ElastRowIn<NV> in;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int t = col + A.off[i];
    in.on[i] = t >= 0 && t < n_steps;
    in.x[i] = in.on[i] ? X + (int64_t)t * vs : nullptr;
  }
  if (rhs) rhs += (int64_t)blockIdx.y * rs;
  y += (int64_t)blockIdx.y * vs;
  const auto w = elast_row_walk<D, MASKED, NV, true>(row, mptr, cols, rowlen, vals, diag, fixed, mvals, mdiag, in);
#pragma unroll
  for (int r = 0; r < D; ++r) {
    const double f = rhs ? rhs[row * D + r] : 0.0;
    double o;
    if (MASKED && w.fo[r]) {
      o = A.crf * f + A.idc * w.xo[0][r];
    } else {
      o = A.cr * f;
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (in.on[i]) o += A.k[i] * w.acc[i][r] + A.m[i] * w.accm[i][r];
    }
    y[row * D + r] = o;
  }
}

// dinv = the inverse of the diagonal blocks of K + sigma M, rows / columns of fixed dofs replaced by the identity
template <int D>
__global__ __launch_bounds__(EB) void k_newmark_dinv(int64_t n_rows, const double* __restrict__ diag,
                                                     const double* __restrict__ mdiag, const uint8_t* __restrict__ fixed,
                                                     double sigma, double* __restrict__ dinv) {
  constexpr int DD = D * D;
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const double md = sigma * mdiag[row];
  double B[DD], Bi[DD];
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int cc = 0; cc < D; ++cc) B[r * D + cc] = diag[row * DD + r * D + cc] + (r == cc ? md : 0.0);
  block_inverse_fixed<D>(B, fixed ? fixed + row * D : nullptr, Bi);
#pragma unroll
  for (int q = 0; q < DD; ++q) dinv[row * DD + q] = Bi[q];
}

// x = 2 a - b (an absent vector is null and reads as 0), zero on fixed dofs
__global__ __launch_bounds__(EB) void k_newmark_guess(int64_t n, const uint8_t* __restrict__ fixed, const double* __restrict__ a,
                                                      const double* __restrict__ b, double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  double v = 0.0;
  if (a) v = 2.0 * a[i];
  if (b) v -= b[i];
  if (fixed && fixed[i]) v = 0.0;
  x[i] = v;
}

// column col0 + blockIdx.y: outK = k1 U_c + k0 U_{c-1} + k- U_{c-2}, outM likewise with m_j; a column before the first is 0
__global__ __launch_bounds__(EB) void k_newmark_combine(int64_t n, int col0, NmBlocks c, const double* __restrict__ U,
                                                        double* __restrict__ outK, double* __restrict__ outM) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  const int col = col0 + (int)blockIdx.y;
  const double u1 = U[(int64_t)col * n + i];
  const double u0 = col >= 1 ? U[(int64_t)(col - 1) * n + i] : 0.0;
  const double um = col >= 2 ? U[(int64_t)(col - 2) * n + i] : 0.0;
  outK[(int64_t)blockIdx.y * n + i] = c.k[0] * u1 + c.k[1] * u0 + c.k[2] * um;
  outM[(int64_t)blockIdx.y * n + i] = c.m[0] * u1 + c.m[1] * u0 + c.m[2] * um;
}

// column blockIdx.y: y = a_c f
__global__ __launch_bounds__(EB) void k_newmark_outer(int64_t n, ColScalars a, const double* __restrict__ f, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  y[(int64_t)blockIdx.y * n + i] = a.v[blockIdx.y] * f[i];
}

template <int NV>
int band(femo_elast* e, bool masked, const BandArgs& A, int n_steps, int col0, int n_cols, const double* X, const double* rhs,
         int64_t rs, double* y) {
  femo_mesh* m = e->mesh;
  elast_dispatch(e->d, masked, [&](auto dim, auto mask) {
    constexpr int D = decltype(dim)::value;
    constexpr bool MASKED = decltype(mask)::value;
    hipLaunchKernelGGL((k_newmark_band<D, MASKED, NV>), dim3(grid_of(m->n_rows), (unsigned)n_cols), dim3(EB), 0, m->ctx->stream,
                       m->n_rows, m->d_mptr, m->d_cols, m->d_rowlen, e->d_vals, e->d_diag, e->d_mvals, e->d_mdiag, e->d_fixed, A,
                       n_steps, col0, m->n_rows * D, X, rhs, rs, y);
  });
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// the step's right-hand side, the two windows of combined columns and the shifted inverse diagonal blocks, on first use
int nm_reserve(femo_elast* e, const char* who) {
  if (e->w_nm && e->d_nm_dinv) return 0;
  const int64_t n = e->mesh->n_vert * e->d;
  if ((!e->w_nm && dalloc(&e->w_nm, (1 + 2 * EMC) * n)) || (!e->d_nm_dinv && dalloc(&e->d_nm_dinv, e->mesh->n_vert * e->d * e->d))) {
    femo_set_error("%s: device allocation failed", who);
    return 1;
  }
  return 0;
}

}  // namespace

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_newmark_rhs(femo_elast* e, int masked, double cr, double crf, double m0, double k0, double mm, double km,
                           const femo_vec* rhs, const femo_vec* u, femo_vec* y) {
  FEMO_REQUIRE(e && u && y, "null argument");
  FEMO_REQUIRE(e->assembled, "femo_elast_newmark_rhs: assemble K first");
  FEMO_REQUIRE(e->mass_assembled, "femo_elast_newmark_rhs: assemble M first (femo_elast_mass_assemble)");
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(u->n >= 2 * n && y->n >= n && (!rhs || rhs->n >= n), "vector size mismatch in femo_elast_newmark_rhs");
  FEMO_REQUIRE(!masked || e->has_fixed, "femo_elast_newmark_rhs: masked product without a fixed set");
  FEMO_REQUIRE(y != u && y != rhs, "femo_elast_newmark_rhs: output aliases an input");
  FEMO_TRY(femo_vec_await(u));
  if (rhs) FEMO_TRY(femo_vec_await(rhs));
  femo_vec_touch(y);
  // u_n and u_{n-1} are columns 0 and 1 of a two-column history seen from column -1: offsets +1 and +2
  BandArgs A = {};
  A.m[0] = -m0; A.k[0] = -k0; A.off[0] = 1;
  A.m[1] = -mm; A.k[1] = -km; A.off[1] = 2;
  A.cr = cr; A.crf = crf; A.idc = 0.0;
  return band<2>(e, masked != 0, A, 2, -1, 1, u->d, rhs ? rhs->d : nullptr, 0, y->d);
}

int femo_elast_newmark_march(femo_elast* e, const femo_newmark_params* p, int n_steps, int reverse, const femo_vec* rhs,
                             const femo_vec* F, const double* g, femo_vec* U, const femo_solver_opts* opts, int extrapolate,
                             femo_solve_info* info, int32_t* stopped_at) {
  FEMO_REQUIRE(e && p && U && opts && stopped_at, "null argument");
  FEMO_REQUIRE(e->assembled, "femo_elast_newmark_march: assemble K first");
  FEMO_REQUIRE(e->mass_assembled, "femo_elast_newmark_march: assemble M first (femo_elast_mass_assemble)");
  FEMO_REQUIRE(params_ok(p), "femo_elast_newmark_march: need dt > 0, beta > 0, gamma >= 1/2 and c_m, c_k >= 0, all finite");
  FEMO_REQUIRE(n_steps >= 1, "femo_elast_newmark_march: %d steps (at least 1)", n_steps);
  FEMO_REQUIRE((rhs != nullptr) != (F != nullptr && g != nullptr),
               "femo_elast_newmark_march: give either the right-hand-side history or the load pattern with its signal");
  FEMO_REQUIRE(rhs || !reverse, "femo_elast_newmark_march: the reversed march takes a right-hand-side history");
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d;
  FEMO_REQUIRE(U->n >= n * n_steps && (!rhs || rhs->n >= n * n_steps) && (!F || F->n >= n) && U != rhs && U != F,
               "vector size mismatch in femo_elast_newmark_march: %d steps need %lld entries", n_steps, (long long)(n * n_steps));
  if (!rhs)
    for (int k = 0; k <= n_steps; ++k) FEMO_REQUIRE(std::isfinite(g[k]), "femo_elast_newmark_march: the signal must be finite");
  *stopped_at = -1;
  if (info) std::memset(info, 0, (size_t)n_steps * sizeof(*info));     // the records of steps that are never taken read as zeros
  const NmBlocks c = nm_blocks(*p);
  const double sigma = c.m[0] / c.k[0], ik1 = 1.0 / c.k[0];
  FEMO_TRY(nm_reserve(e, "femo_elast_newmark_march"));
  FEMO_TRY(femo_elast_work_reserve(e, 1, "femo_elast_newmark_march"));
  if (rhs) FEMO_TRY(femo_vec_await(rhs));
  if (F) FEMO_TRY(femo_vec_await(F));
  femo_vec_touch(U);
  hipStream_t st = m->ctx->stream;
  const uint8_t* fx = e->has_fixed ? e->d_fixed : nullptr;
  FEMO_TRY(elast_dispatch_d(e->d, [&](auto dim) {
    return elast_launch_rows(e, k_newmark_dinv<decltype(dim)::value>, e->d_diag, e->d_mdiag, fx, sigma, e->d_nm_dinv);
  }));
  const femo_elast_op op = {sigma, e->d_nm_dinv};
  femo_solver_opts so = *opts;
  so.zero_guess = extrapolate ? 0 : 1;
  const int dir = reverse ? 1 : -1;                 // where the two earlier columns of the march lie
  BandArgs A = {};
  A.m[0] = -c.m[1] * ik1; A.k[0] = -c.k[1] * ik1; A.off[0] = dir;
  A.m[1] = -c.m[2] * ik1; A.k[1] = -c.k[2] * ik1; A.off[1] = 2 * dir;
  A.idc = 0.0;
  double* b = e->w_nm;
  femo_vec bv = elast_block::wrap(m->ctx, b, n);
  femo_solve_info one;
  for (int k = 0; k < n_steps; ++k) {
    const int t = reverse ? n_steps - 1 - k : k;
    if (rhs) {
      A.cr = ik1; A.crf = 1.0;
    } else {
      const double gm = t >= 1 ? g[t - 1] : 0.0;
      A.cr = p->dt * p->dt * (p->beta * g[t + 1] + c.b0 * g[t] + c.bm * gm) * ik1;
      A.crf = 0.0;
    }
    FEMO_TRY(band<2>(e, fx != nullptr, A, n_steps, t, 1, U->d, rhs ? rhs->d + (int64_t)t * n : F->d, 0, b));
    double* x = U->d + (int64_t)t * n;
    if (extrapolate) {
      const int t1 = t + dir, t2 = t + 2 * dir;
      const double* a1 = t1 >= 0 && t1 < n_steps ? U->d + (int64_t)t1 * n : nullptr;
      const double* a2 = t2 >= 0 && t2 < n_steps ? U->d + (int64_t)t2 * n : nullptr;
      hipLaunchKernelGGL(k_newmark_guess, dim3(grid_of(n)), dim3(EB), 0, st, n, fx, a1, a2, x);
      FEMO_HIP_CHECK(hipGetLastError());
    }
    femo_vec xv = elast_block::wrap(m->ctx, x, n);
    femo_solve_info* si = info ? info + t : &one;
    FEMO_TRY(femo_elast_pcg(e, 1, &bv, &xv, &so, si, "femo_elast_newmark_march", &op));
    if (si->converged != 1) {
      *stopped_at = t;
      break;
    }
  }
  return 0;
}

int femo_elast_newmark_apply(femo_elast* e, const femo_newmark_params* p, int n_steps, int transpose, int masked,
                             const femo_vec* X, femo_vec* Y) {
  FEMO_REQUIRE(e && p && X && Y, "null argument");
  FEMO_REQUIRE(e->assembled, "femo_elast_newmark_apply: assemble K first");
  FEMO_REQUIRE(e->mass_assembled, "femo_elast_newmark_apply: assemble M first (femo_elast_mass_assemble)");
  FEMO_REQUIRE(params_ok(p), "femo_elast_newmark_apply: need dt > 0, beta > 0, gamma >= 1/2 and c_m, c_k >= 0, all finite");
  FEMO_REQUIRE(n_steps >= 1, "femo_elast_newmark_apply: %d steps (at least 1)", n_steps);
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(X->n >= n * n_steps && Y->n >= n * n_steps && X != Y,
               "vector size mismatch in femo_elast_newmark_apply: %d steps need %lld entries", n_steps, (long long)(n * n_steps));
  FEMO_REQUIRE(!masked || e->has_fixed, "femo_elast_newmark_apply: masked product without a fixed set");
  FEMO_TRY(femo_vec_await(X));
  femo_vec_touch(Y);
  const NmBlocks c = nm_blocks(*p);
  const int dir = transpose ? 1 : -1;
  BandArgs A = {};
  for (int i = 0; i < 3; ++i) { A.m[i] = c.m[i]; A.k[i] = c.k[i]; A.off[i] = i * dir; }
  A.cr = 0.0; A.crf = 0.0; A.idc = 1.0;
  for (int col0 = 0; col0 < n_steps; col0 += EMC)
    FEMO_TRY(band<3>(e, masked != 0, A, n_steps, col0, std::min(EMC, n_steps - col0), X->d, nullptr, 0, Y->d + (int64_t)col0 * n));
  return 0;
}

int femo_elast_newmark_drho(femo_elast* e, const femo_newmark_params* p, int method, int mass_law, double density, int transpose,
                            int n_steps, int first, int count, const femo_vec* rho, const femo_vec* U, const femo_vec* x,
                            femo_vec* y, int accumulate) {
  FEMO_REQUIRE(e && p && rho && U && x && y, "null argument");
  FEMO_REQUIRE(params_ok(p), "femo_elast_newmark_drho: need dt > 0, beta > 0, gamma >= 1/2 and c_m, c_k >= 0, all finite");
  FEMO_REQUIRE(n_steps >= 1 && first >= 0 && count >= 1 && first <= n_steps - count,
               "femo_elast_newmark_drho: columns %d ... %d of %d steps", first, first + count - 1, n_steps);
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d, nh = n * n_steps;
  FEMO_REQUIRE(rho->n >= m->n_cell && U->n >= nh, "vector size mismatch in femo_elast_newmark_drho");
  FEMO_REQUIRE(transpose ? (x->n >= nh && y->n >= m->n_cell) : (x->n >= m->n_cell && y->n >= nh),
               "vector size mismatch in femo_elast_newmark_drho");
  FEMO_REQUIRE(y != x && y != U && y != rho, "femo_elast_newmark_drho: output aliases an input");
  FEMO_TRY(nm_reserve(e, "femo_elast_newmark_drho"));
  FEMO_TRY(femo_vec_await(U));
  FEMO_TRY(femo_vec_await(x));            // the windows below are wrapped views of x: they carry no upload of their own to wait for
  const NmBlocks c = nm_blocks(*p);
  hipStream_t st = m->ctx->stream;
  double *uK = e->w_nm + n, *uM = e->w_nm + n + (int64_t)EMC * n;
  double ones[EMC];
  for (int l = 0; l < EMC; ++l) ones[l] = 1.0;
  if (!transpose) femo_vec_touch(y);
  for (int col0 = first; col0 < first + count; col0 += EMC) {           // ascending: the order of the sum over the windows
    const int w = std::min(EMC, first + count - col0);
    hipLaunchKernelGGL(k_newmark_combine, dim3(grid_of(n), (unsigned)w), dim3(EB), 0, st, n, col0, c, U->d, uK, uM);
    FEMO_HIP_CHECK(hipGetLastError());
    femo_vec vK = elast_block::wrap(m->ctx, uK, n * w), vM = elast_block::wrap(m->ctx, uM, n * w);
    if (transpose) {
      femo_vec xw = elast_block::wrap(m->ctx, x->d + (int64_t)col0 * n, n * w);
      FEMO_TRY(femo_elast_drho_multi(e, method, 1, w, rho, &vK, &xw, y, (accumulate || col0 > first) ? 1 : 0));
      FEMO_TRY(femo_elast_mass_drho_multi(e, mass_law, density, 1, w, ones, rho, &vM, &xw, y, 1));
    } else {
      femo_vec yw = elast_block::wrap(m->ctx, y->d + (int64_t)col0 * n, n * w);
      FEMO_TRY(femo_elast_drho_multi(e, method, 0, w, rho, &vK, x, &yw, accumulate));
      FEMO_TRY(femo_elast_mass_drho_multi(e, mass_law, density, 0, w, ones, rho, &vM, x, &yw, 1));
    }
  }
  return 0;
}

int femo_elast_newmark_dots(femo_elast* e, int n_steps, const femo_vec* f, const femo_vec* U, double* out) {
  FEMO_REQUIRE(e && f && U && out, "null argument");
  FEMO_REQUIRE(n_steps >= 1, "femo_elast_newmark_dots: %d steps (at least 1)", n_steps);
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(f->n >= n && U->n >= n * n_steps, "vector size mismatch in femo_elast_newmark_dots");
  FEMO_TRY(femo_vec_await(f)); FEMO_TRY(femo_vec_await(U));
  FEMO_TRY(elast_block::gram_reserve(e));
  for (int col0 = 0; col0 < n_steps; col0 += EMC) {
    const int w = std::min(EMC, n_steps - col0);
    FEMO_TRY(elast_block::gram_launch(e, 0, n, 1, f->d, w, U->d + (int64_t)col0 * n));
    FEMO_TRY(elast_block::gram_fetch(e, n, w, 0));
    for (int j = 0; j < w; ++j) out[col0 + j] = e->h_gram[j];
  }
  return 0;
}

int femo_elast_newmark_outer(femo_elast* e, int n_steps, const double* a, const femo_vec* f, femo_vec* Y) {
  FEMO_REQUIRE(e && a && f && Y, "null argument");
  FEMO_REQUIRE(n_steps >= 1, "femo_elast_newmark_outer: %d steps (at least 1)", n_steps);
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(f->n >= n && Y->n >= n * n_steps && f != Y, "vector size mismatch in femo_elast_newmark_outer");
  FEMO_TRY(femo_vec_await(f));
  femo_vec_touch(Y);
  for (int col0 = 0; col0 < n_steps; col0 += EMC) {
    const int w = std::min(EMC, n_steps - col0);
    ColScalars s = {};
    for (int j = 0; j < w; ++j) s.v[j] = a[col0 + j];
    hipLaunchKernelGGL(k_newmark_outer, dim3(grid_of(n), (unsigned)w), dim3(EB), 0, e->mesh->ctx->stream, n, s, f->d,
                       Y->d + (int64_t)col0 * n);
  }
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
