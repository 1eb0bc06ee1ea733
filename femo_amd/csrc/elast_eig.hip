// SIMP topology optimisation: the lowest eigenfrequencies of the linear elasticity, K(rho) phi = lambda M(rho) phi on the
// free dofs (C-ABI in include/femo_hip.h: femo_elast_mass_apply_multi, femo_elast_block_gram, femo_elast_block_rotate,
// femo_elast_eig_drho, femo_elast_eigs).
//
//   M(rho) = rho0 sum_e m(rho_e) M0_e,   M0_e[(a,i),(b,j)] = delta_ij |T_e| (1 + delta_ab) / ((d+1)(d+2))   (consistent P1)
//   m = rho (linear) or Du & Olhoff's law: rho for rho >= 0.1, 6e5 rho^6 - 5e6 rho^7 below (C^1 at 0.1)
//
// Layout as in elast_solve.hip: column l at l * n_dof.  The mass matrix is never stored: the product walks the cells around
// a vertex row like k_elast_body_N.  No float atomics: one writer per dof, per cell and per partial; the cells around a
// vertex, the columns and the partials are summed in a fixed order, so every call gives the same bits, and neither a column
// of the mass product nor an entry of a Gram matrix depends on how many columns travel with it.
//
// femo_elast_eigs is block inverse iteration with Rayleigh-Ritz.  An outer step issues
//
//   B = M_ff X                               k_elast_mass            one launch for the block
//   K Y = B, first guess X                   the batched PCG of elast_solve.hip (Y overwrites X)
//   MY = M_ff Y, KY = A Y                    k_elast_mass, k_elast_spmv_multi
//   G_M = Y^T MY, G_K = Y^T KY               k_block_gram twice, one fold, one copy to the pinned mirror
//   host: Cholesky of G_M, cyclic Jacobi on L^-1 G_K L^-T  ->  theta ascending, Q = L^-T V
//   X = Y Q, MX = MY Q, R = KY Q - MY Q Theta   k_block_rotate three times (X in place)
//   |R_k|^2, |MX_k|^2                        k_block_gram twice, one fold, one copy
//
// and stops when |R_k| <= rtol theta_k |MX_k| for every k < n_modes.  MY, KY, MX and R live in the PCG work vectors, which
// are free between two solves; B is the one vector of its own.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace elast_block;

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;
constexpr int GRAM_GRID = 512;       // blocks of the Gram kernel at the most (one partial per block and pair)

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

// --------------------------------------------------------------------------------------------- block Gram ----
// part[(i * n_b + j) * FEMO_MAX_PARTIALS + block] = the block's share of a_i . b_j.  A thread streams all columns of one dof
// (grid stride); the share of a pair is the same sum whatever n_a and n_b are.
__global__ __launch_bounds__(EB) void k_block_gram(int64_t n, int n_a, const double* __restrict__ A, int n_b,
                                                   const double* __restrict__ B, double* __restrict__ part) {
  __shared__ double lds[EB / 64];
  double acc[EMC][EMC];
#pragma unroll
  for (int i = 0; i < EMC; ++i)
#pragma unroll
    for (int j = 0; j < EMC; ++j) acc[i][j] = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * EB + threadIdx.x; k < n; k += (int64_t)gridDim.x * EB) {
    double av[EMC], bv[EMC];
#pragma unroll
    for (int i = 0; i < EMC; ++i) {
      av[i] = i < n_a ? A[(int64_t)i * n + k] : 0.0;
      bv[i] = i < n_b ? B[(int64_t)i * n + k] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < EMC; ++i)
#pragma unroll
      for (int j = 0; j < EMC; ++j) acc[i][j] += av[i] * bv[j];
  }
#pragma unroll
  for (int i = 0; i < EMC; ++i) {
    if (i >= n_a) break;
#pragma unroll
    for (int j = 0; j < EMC; ++j) {
      if (j >= n_b) break;
      const double s = femo_block_sum<EB>(acc[i][j], lds);
      if (threadIdx.x == 0) part[(int64_t)(i * n_b + j) * FEMO_MAX_PARTIALS + blockIdx.x] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------- block rotate ----
// y_j = sum_i x_i Q[i][j] (+ sum_i x2_i Q2[i][j] when TWO), i, j < n_cols, summed in ascending i.  A thread reads all
// inputs of its dof before it writes, so y may be x (or x2).
template <bool TWO>
__global__ __launch_bounds__(EB) void k_block_rotate(int64_t n, int n_cols, BlockMatrix Q, const double* x, BlockMatrix Q2,
                                                     const double* x2, double* y) {
  const int64_t k = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (k >= n) return;
  double xi[EMC], x2i[EMC];
#pragma unroll
  for (int i = 0; i < EMC; ++i) {
    xi[i] = i < n_cols ? x[(int64_t)i * n + k] : 0.0;
    x2i[i] = TWO && i < n_cols ? x2[(int64_t)i * n + k] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < EMC; ++j) {
    if (j >= n_cols) break;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < EMC; ++i)
      if (i < n_cols) s += xi[i] * Q.v[i][j];
    if (TWO) {
#pragma unroll
      for (int i = 0; i < EMC; ++i)
        if (i < n_cols) s += x2i[i] * Q2.v[i][j];
    }
    y[(int64_t)j * n + k] = s;
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

// ------------------------------------------------------------------------------------------ sign convention ----
// One workgroup per column: the entry of largest magnitude (the first of equals) becomes positive.
__global__ __launch_bounds__(1024) void k_eig_sign(int64_t n, double* __restrict__ x) {
  __shared__ double sv[1024];
  __shared__ int64_t si[1024];
  x += (int64_t)blockIdx.x * n;
  double best = -1.0;
  int64_t at = 0;
  for (int64_t k = threadIdx.x; k < n; k += 1024) {
    const double t = fabs(x[k]);
    if (t > best) { best = t; at = k; }
  }
  sv[threadIdx.x] = best; si[threadIdx.x] = at;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const double o = sv[threadIdx.x + off];
      const int64_t oi = si[threadIdx.x + off];
      if (o > sv[threadIdx.x] || (o == sv[threadIdx.x] && oi < si[threadIdx.x])) { sv[threadIdx.x] = o; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  const bool flip = sv[0] > 0.0 && x[si[0]] < 0.0;
  __syncthreads();
  if (!flip) return;
  for (int64_t k = threadIdx.x; k < n; k += 1024) x[k] = -x[k];
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

inline int gram_grid(int64_t n) { return (int)grid_of(n, GRAM_GRID); }

// The Gram partials: two slabs of EMC * EMC slots of FEMO_MAX_PARTIALS, and the 2 * EMC * EMC folded values behind them.
constexpr int64_t GRAM_SLAB = (int64_t)EMC * EMC * FEMO_MAX_PARTIALS;

}  // namespace

// ------------------------------------------------------------- shared with elast_buckle.hip (elast_internal.h) ----
namespace elast_block {

int gram_reserve(femo_elast* e) {
  if (e->w_gram) return 0;
  FEMO_TRY(dalloc(&e->w_gram, 2 * GRAM_SLAB + 2 * EMC * EMC));
  if (hipHostMalloc(reinterpret_cast<void**>(&e->h_gram), 2 * EMC * EMC * sizeof(double)) != hipSuccess) {
    e->h_gram = nullptr;
    femo_set_error("femo_elast: pinned allocation failed");
    return 1;
  }
  return 0;
}

// slab s (0 or 1) <- partials of A^T B; folded by gram_fetch
int gram_launch(femo_elast* e, int slab, int64_t n, int n_a, const double* A, int n_b, const double* B) {
  hipLaunchKernelGGL(k_block_gram, dim3(gram_grid(n)), dim3(EB), 0, e->mesh->ctx->stream, n, n_a, A, n_b, B,
                     e->w_gram + slab * GRAM_SLAB);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// folds the first `sums0` pairs of slab 0 and `sums1` of slab 1 and waits for them in h_gram[0 ...], h_gram[EMC * EMC ...]
int gram_fetch(femo_elast* e, int64_t n, int sums0, int sums1) {
  hipStream_t st = e->mesh->ctx->stream;
  double* out = e->w_gram + 2 * GRAM_SLAB;
  const int nb = gram_grid(n);
  FEMO_TRY(femo_launch_fold(1024, nb, sums0, e->w_gram, out, st));
  if (sums1 > 0) FEMO_TRY(femo_launch_fold(1024, nb, sums1, e->w_gram + GRAM_SLAB, out + EMC * EMC, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(e->h_gram, out, (size_t)(sums1 > 0 ? 2 : 1) * EMC * EMC * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

int rotate_launch(femo_elast* e, int64_t n, int n_cols, const BlockMatrix& Q, const double* x, const BlockMatrix* Q2,
                  const double* x2, double* y) {
  hipStream_t st = e->mesh->ctx->stream;
  if (Q2) hipLaunchKernelGGL(k_block_rotate<true>, dim3(grid_of(n)), dim3(EB), 0, st, n, n_cols, Q, x, *Q2, x2, y);
  else hipLaunchKernelGGL(k_block_rotate<false>, dim3(grid_of(n)), dim3(EB), 0, st, n, n_cols, Q, x, Q, x, y);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------- the small eigenproblem ----
// G_K q = theta G_M q for symmetric L x L matrices, G_M positive definite: Cholesky G_M = C C^T, cyclic Jacobi on
// C^-1 G_K C^-T = V Theta V^T, Q = C^-T V with the columns in ascending theta.  Then Q^T G_M Q = I, Q^T G_K Q = Theta.
// Returns false when G_M is not positive definite.
bool small_eigs(int L, const double (&GM)[EMC][EMC], const double (&GK)[EMC][EMC], double (&theta)[EMC], double (&Q)[EMC][EMC]) {
  double C[EMC][EMC] = {}, A[EMC][EMC] = {}, V[EMC][EMC] = {};
  for (int j = 0; j < L; ++j) {
    double s = GM[j][j];
    for (int k = 0; k < j; ++k) s -= C[j][k] * C[j][k];
    if (!(s > 0.0) || !std::isfinite(s)) return false;
    C[j][j] = std::sqrt(s);
    for (int i = j + 1; i < L; ++i) {
      double t = 0.5 * (GM[i][j] + GM[j][i]);
      for (int k = 0; k < j; ++k) t -= C[i][k] * C[j][k];
      C[i][j] = t / C[j][j];
    }
  }
  // T = C^-1 GK (forward substitution per column), A = T C^-T = (C^-1 T^T)^T
  double T[EMC][EMC] = {};
  for (int c = 0; c < L; ++c)
    for (int i = 0; i < L; ++i) {
      double t = 0.5 * (GK[i][c] + GK[c][i]);
      for (int k = 0; k < i; ++k) t -= C[i][k] * T[k][c];
      T[i][c] = t / C[i][i];
    }
  for (int r = 0; r < L; ++r)
    for (int i = 0; i < L; ++i) {
      double t = T[r][i];
      for (int k = 0; k < i; ++k) t -= C[i][k] * A[r][k];
      A[r][i] = t / C[i][i];
    }
  for (int i = 0; i < L; ++i)
    for (int j = i + 1; j < L; ++j) A[i][j] = A[j][i] = 0.5 * (A[i][j] + A[j][i]);
  for (int i = 0; i < L; ++i) V[i][i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < L; ++j) (i == j ? dg : off) += A[i][j] * A[i][j];
    if (off <= 1e-34 * dg) break;                 // off and dg are sums of squares
    for (int p = 0; p < L - 1; ++p)
      for (int q = p + 1; q < L; ++q) {
        if (A[p][q] == 0.0) continue;
        const double tau = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs;
        for (int k = 0; k < L; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = cs * akp - sn * akq;
          A[k][q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < L; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = cs * apk - sn * aqk;
          A[q][k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < L; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
  }
  int order[EMC];
  for (int i = 0; i < L; ++i) order[i] = i;
  std::stable_sort(order, order + L, [&](int a, int b) { return A[a][a] < A[b][b]; });
  for (int j = 0; j < L; ++j) {
    const int s = order[j];
    theta[j] = A[s][s];
    // column j of Q = C^-T V[:, s] (back substitution)
    for (int i = L - 1; i >= 0; --i) {
      double t = V[i][s];
      for (int k = i + 1; k < L; ++k) t -= C[k][i] * Q[k][j];
      Q[i][j] = t / C[i][i];
    }
  }
  return true;
}

femo_vec wrap(femo_ctx* ctx, double* d, int64_t n) {
  femo_vec v;
  v.ctx = ctx; v.d = d; v.n = n; v.owned = false;
  return v;
}

int sign_launch(femo_elast* e, int64_t n, int n_cols, double* x) {
  hipLaunchKernelGGL(k_eig_sign, dim3((unsigned)n_cols), dim3(1024), 0, e->mesh->ctx->stream, n, x);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace elast_block

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

int femo_elast_block_gram(femo_elast* e, int n_a, const femo_vec* a, int n_b, const femo_vec* b, double* G) {
  FEMO_REQUIRE(e && a && b && G, "null argument");
  FEMO_REQUIRE(n_a >= 1 && n_a <= EMC && n_b >= 1 && n_b <= EMC, "femo_elast_block_gram: %d x %d columns (1 to %d each)", n_a,
               n_b, EMC);
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(a->n >= n * n_a && b->n >= n * n_b, "vector size mismatch in femo_elast_block_gram: %d and %d columns of %lld",
               n_a, n_b, (long long)n);
  FEMO_TRY(femo_vec_await(a)); FEMO_TRY(femo_vec_await(b));
  FEMO_TRY(gram_reserve(e));
  FEMO_TRY(gram_launch(e, 0, n, n_a, a->d, n_b, b->d));
  FEMO_TRY(gram_fetch(e, n, n_a * n_b, 0));
  for (int k = 0; k < n_a * n_b; ++k) G[k] = e->h_gram[k];
  return 0;
}

int femo_elast_block_rotate(femo_elast* e, int n_cols, const double* Q, const femo_vec* x, femo_vec* y) {
  FEMO_REQUIRE(e && Q && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_block_rotate: %d columns (1 to %d)", n_cols, EMC);
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(x->n >= n * n_cols && y->n >= n * n_cols, "vector size mismatch in femo_elast_block_rotate: %d columns need %lld entries",
               n_cols, (long long)(n * n_cols));
  BlockMatrix Qm;
  std::memset(&Qm, 0, sizeof(Qm));
  for (int i = 0; i < n_cols; ++i)
    for (int j = 0; j < n_cols; ++j) Qm.v[i][j] = Q[i * n_cols + j];
  FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(y);
  return rotate_launch(e, n, n_cols, Qm, x->d, nullptr, nullptr, y->d);
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
  femo_ctx* ctx = m->ctx;
  const int64_t n = m->n_vert * e->d, nl = n * block;
  FEMO_REQUIRE(rho->n >= m->n_cell && X->n >= nl, "vector size mismatch in femo_elast_eigs: %d columns need %lld entries", block,
               (long long)nl);
  FEMO_REQUIRE(X != rho, "femo_elast_eigs: the block aliases the density");
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(X));
  femo_vec_touch(X);
  FEMO_TRY(femo_elast_work_reserve(e, block, "femo_elast_eigs"));
  FEMO_TRY(gram_reserve(e));
  if (e->w_eig_cols < block) {
    double* b = nullptr;
    FEMO_TRY(dalloc(&b, nl));
    FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    hipFree(e->w_eig);
    e->w_eig = b;
    e->w_eig_cols = block;
  }
  femo_solver_opts so;
  std::memset(&so, 0, sizeof(so));
  so.rtol = opts->pcg_rtol;
  so.max_it = opts->pcg_max_it;
  so.zero_guess = 0;
  so.pc = opts->pc;
  const int max_outer = opts->max_outer > 0 ? opts->max_outer : 200;
  femo_vec Bv = wrap(ctx, e->w_eig, nl);
  femo_solve_info si[EMC];
  femo_eig_info out;
  std::memset(&out, 0, sizeof(out));
  double theta[EMC] = {};
  const int L = block, LL = EMC * EMC;
  for (int outer = 1; outer <= max_outer; ++outer) {
    FEMO_TRY(mass_launch(e, mass_law, density, true, L, 1.0, rho->d, X->d, e->w_eig));             // B = M_ff X
    FEMO_TRY(femo_elast_pcg(e, L, &Bv, X, &so, si, "femo_elast_eigs"));                             // K Y = B, Y in X
    int its = 0;
    for (int l = 0; l < L; ++l) {
      FEMO_REQUIRE(si[l].converged == 1, "femo_elast_eigs: the inner PCG did not converge (outer step %d, column %d: %d iterations)",
                   outer, l, si[l].iterations);
      its = std::max(its, (int)si[l].iterations);
      out.solve_ms += l == 0 ? si[l].solve_ms : 0.0;
    }
    out.pcg_iterations += its;
    out.outer_iterations = outer;
    double *MY = e->w_z, *KY = e->w_q, *MX = e->w_p, *R = e->w_r;      // the PCG work vectors are free until the next solve
    FEMO_TRY(mass_launch(e, mass_law, density, true, L, 1.0, rho->d, X->d, MY));
    FEMO_TRY(femo_elast_spmv(e, true, L, 1.0, X->d, 0.0, nullptr, KY, nullptr, 0, nullptr));
    FEMO_TRY(gram_launch(e, 0, n, L, X->d, L, MY));
    FEMO_TRY(gram_launch(e, 1, n, L, X->d, L, KY));
    FEMO_TRY(gram_fetch(e, n, L * L, L * L));
    double GM[EMC][EMC] = {}, GK[EMC][EMC] = {}, Qh[EMC][EMC] = {};
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < L; ++j) { GM[i][j] = e->h_gram[i * L + j]; GK[i][j] = e->h_gram[LL + i * L + j]; }
    FEMO_REQUIRE(small_eigs(L, GM, GK, theta, Qh),
                 "femo_elast_eigs: the block lost rank (Y^T M Y is not positive definite at outer step %d): start from another block",
                 outer);
    BlockMatrix Q, QT;
    std::memset(&Q, 0, sizeof(Q)); std::memset(&QT, 0, sizeof(QT));
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < L; ++j) { Q.v[i][j] = Qh[i][j]; QT.v[i][j] = -Qh[i][j] * theta[j]; }
    FEMO_TRY(rotate_launch(e, n, L, Q, X->d, nullptr, nullptr, X->d));          // X = Y Q
    FEMO_TRY(rotate_launch(e, n, L, Q, KY, &QT, MY, R));                        // R = KY Q - MY Q Theta
    FEMO_TRY(rotate_launch(e, n, L, Q, MY, nullptr, nullptr, MX));              // MX = MY Q
    FEMO_TRY(gram_launch(e, 0, n, L, R, L, R));
    FEMO_TRY(gram_launch(e, 1, n, L, MX, L, MX));
    FEMO_TRY(gram_fetch(e, n, L * L, L * L));
    bool ok = true;
    for (int k = 0; k < L; ++k) {
      const double rn = std::sqrt(std::fabs(e->h_gram[k * L + k])), mn = std::sqrt(std::fabs(e->h_gram[LL + k * L + k]));
      out.residual[k] = rn / (std::fabs(theta[k]) * mn);
      if (k < n_modes && !(out.residual[k] <= opts->rtol)) ok = false;
    }
    if (ok) { out.converged = 1; break; }
  }
  FEMO_TRY(sign_launch(e, n, L, X->d));
  FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < L; ++k) lambda[k] = theta[k];
  if (info) *info = out;
  return 0;
}

}  // extern "C"
