// SIMP topology optimisation: the block linear algebra of the eigen solves of the linear elasticity and the one block
// iteration that femo_elast_eigs (elast_eig.hip) and femo_elast_buckle (elast_buckle.hip) run (C-ABI in include/femo_hip.h:
// femo_elast_block_gram, femo_elast_block_rotate; the rest is namespace elast_block of elast_internal.h).
//
// Layout as in elast_solve.hip: column l at l * n_dof.  No float atomics: one writer per dof and per partial; the columns and
// the partials are summed in a fixed order, so every call gives the same bits, and an entry of a Gram matrix does not depend
// on how many columns travel with it.
//
// block_iteration is block inverse iteration with Rayleigh-Ritz on a pencil N phi = theta P phi, P positive definite, of
// which K is one side and the pencil's matrix-free operator Op the other (eigenfrequencies: Op = M = P, N = K, theta
// ascending; buckling: Op = -K_G = N, P = K, theta descending).  An outer step issues
//
//   B = Op X                                 the pencil's product      one launch for the block
//   K Y = B                                  the batched PCG of elast_solve.hip (Y overwrites X), from X or from zero
//   BY = Op Y, KY = A Y                      the pencil's product, k_elast_spmv_multi; PY, NY name these two
//   G_P = Y^T PY, G_N = Y^T NY               k_block_gram twice, one fold, one copy to the pinned mirror
//   host: Cholesky of G_P, cyclic Jacobi on C^-1 G_N C^-T  ->  theta in the pencil's order, Q = C^-T V
//   X = Y Q, PX = PY Q, R = NY Q - PY Q Theta   k_block_rotate three times (X in place)
//   |R_k|^2, |PX_k|^2                        k_block_gram twice, one fold, one copy
//
// and stops when |R_k| <= rtol |theta_k| |PX_k| (and, for a pencil that asks for it, theta_k > 0) for every k < n_modes.  BY,
// KY, PX and R live in the PCG work vectors, which are free between two solves; B is the one vector of its own.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;
constexpr int GRAM_GRID = 512;       // blocks of the Gram kernel at the most (one partial per block and pair)

using elast_block::BlockMatrix;

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

inline int gram_grid(int64_t n) { return (int)grid_of(n, GRAM_GRID); }

// The Gram partials: two slabs of EMC * EMC slots of FEMO_MAX_PARTIALS, and the 2 * EMC * EMC folded values behind them.
constexpr int64_t GRAM_SLAB = (int64_t)EMC * EMC * FEMO_MAX_PARTIALS;

}  // namespace

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

int rhs_reserve(femo_elast* e, int n_cols) {
  if (e->w_eig_cols >= n_cols) return 0;
  double* b = nullptr;
  FEMO_TRY(dalloc(&b, e->mesh->n_vert * e->d * n_cols));
  FEMO_HIP_CHECK(hipStreamSynchronize(e->mesh->ctx->stream));
  std::swap(b, e->w_eig);
  e->w_eig_cols = n_cols;
  FEMO_HIP_CHECK(hipFree(b));
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

// ------------------------------------------------------------------------------------------ the block iteration ----
int block_iteration(femo_elast* e, const Pencil& pen, int n_modes, int block, femo_vec* X, const femo_eig_opts* opts,
                    double* lambda, femo_eig_info* info) {
  femo_ctx* ctx = e->mesh->ctx;
  const int L = block, LL = EMC * EMC;
  const int64_t n = e->mesh->n_vert * e->d, nl = n * L;
  FEMO_TRY(femo_elast_work_reserve(e, L, pen.who));
  FEMO_TRY(gram_reserve(e));
  FEMO_TRY(rhs_reserve(e, L));
  femo_solver_opts so;
  std::memset(&so, 0, sizeof(so));
  so.rtol = opts->pcg_rtol;
  so.max_it = opts->pcg_max_it;
  so.zero_guess = pen.zero_guess;
  so.pc = opts->pc;
  const int max_outer = opts->max_outer > 0 ? opts->max_outer : pen.max_outer;
  femo_vec Bv = wrap(ctx, e->w_eig, nl);
  femo_solve_info si[EMC];
  femo_eig_info out;
  std::memset(&out, 0, sizeof(out));
  double theta[EMC] = {};
  int positive = 0;                                                   // tested columns with theta > 0 at the last outer step
  for (int outer = 1; outer <= max_outer; ++outer) {
    FEMO_TRY(pen.apply(L, X->d, e->w_eig));                                                          // B = Op X
    FEMO_TRY(femo_elast_pcg(e, L, &Bv, X, &so, si, pen.who));                                        // K Y = B, Y in X
    int its = 0;
    for (int l = 0; l < L; ++l) {
      FEMO_REQUIRE(si[l].converged == 1, "%s: the inner PCG did not converge (outer step %d, column %d: %d iterations)", pen.who,
                   outer, l, si[l].iterations);
      its = std::max(its, (int)si[l].iterations);
      out.solve_ms += l == 0 ? si[l].solve_ms : 0.0;
    }
    out.pcg_iterations += its;
    out.outer_iterations = outer;
    double *BY = e->w_z, *KY = e->w_q, *PX = e->w_p, *R = e->w_r;      // the PCG work vectors are free until the next solve
    double *PY = pen.p_is_op ? BY : KY, *NY = pen.p_is_op ? KY : BY;
    FEMO_TRY(pen.apply(L, X->d, BY));
    FEMO_TRY(femo_elast_spmv(e, true, L, 1.0, X->d, 0.0, nullptr, KY, nullptr, 0, nullptr));
    FEMO_TRY(gram_launch(e, 0, n, L, X->d, L, PY));
    FEMO_TRY(gram_launch(e, 1, n, L, X->d, L, NY));
    FEMO_TRY(gram_fetch(e, n, L * L, L * L));
    double GP[EMC][EMC] = {}, GN[EMC][EMC] = {}, Qa[EMC][EMC] = {}, asc[EMC] = {};
    for (int i = 0; i < L; ++i)
      for (int j = 0; j < L; ++j) { GP[i][j] = e->h_gram[i * L + j]; GN[i][j] = e->h_gram[LL + i * L + j]; }
    FEMO_REQUIRE(small_eigs(L, GP, GN, asc, Qa),
                 "%s: the block lost rank (Y^T %s Y is not positive definite at outer step %d): start from another block", pen.who,
                 pen.p_name, outer);
    BlockMatrix Q, QT;                                                // the columns in the pencil's order
    std::memset(&Q, 0, sizeof(Q)); std::memset(&QT, 0, sizeof(QT));
    for (int j = 0; j < L; ++j) {
      const int s = pen.descending ? L - 1 - j : j;
      theta[j] = asc[s];
      for (int i = 0; i < L; ++i) { Q.v[i][j] = Qa[i][s]; QT.v[i][j] = -Q.v[i][j] * theta[j]; }
    }
    FEMO_TRY(rotate_launch(e, n, L, Q, X->d, nullptr, nullptr, X->d));          // X = Y Q
    FEMO_TRY(rotate_launch(e, n, L, Q, NY, &QT, PY, R));                        // R = NY Q - PY Q Theta
    FEMO_TRY(rotate_launch(e, n, L, Q, PY, nullptr, nullptr, PX));              // PX = PY Q
    FEMO_TRY(gram_launch(e, 0, n, L, R, L, R));
    FEMO_TRY(gram_launch(e, 1, n, L, PX, L, PX));
    FEMO_TRY(gram_fetch(e, n, L * L, L * L));
    bool ok = true;
    positive = 0;
    for (int k = 0; k < L; ++k) {
      const double rn = std::sqrt(std::fabs(e->h_gram[k * L + k])), pn = std::sqrt(std::fabs(e->h_gram[LL + k * L + k]));
      out.residual[k] = rn / (std::fabs(theta[k]) * pn);
      const bool accepted = !pen.positive_only || theta[k] > 0.0;
      if (k < n_modes && accepted) ++positive;
      if (k < n_modes && !(out.residual[k] <= opts->rtol && accepted)) ok = false;
    }
    if (ok) { out.converged = 1; break; }
  }
  FEMO_TRY(sign_launch(e, n, L, X->d));
  FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  FEMO_REQUIRE(out.converged == 1 || positive == n_modes,
               "%s: the block is too small for this load -- no positive load factor for %d of the %d modes after %d "
               "outer steps (the block of %d columns fills up with negative mu, buckling under the reversed load): raise block",
               pen.who, n_modes - positive, n_modes, out.outer_iterations, L);
  for (int k = 0; k < L; ++k) lambda[k] = pen.reciprocal ? 1.0 / theta[k] : theta[k];
  if (info) *info = out;
  return 0;
}

}  // namespace elast_block

using namespace elast_block;

// ===================================================================================================== C-ABI ====
extern "C" {

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

}  // extern "C"
