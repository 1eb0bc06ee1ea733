// Method of Moving Asymptotes: the device-resident design update of the SIMP track (include/femo_hip.h, "Method of Moving
// Asymptotes", states the formulation; tests/mma_ref.py restates it in NumPy).
//
// Layout.  Everything per variable runs in element-wise kernels with grid-stride loops, 256 threads (4 wave64); every sum
// and maximum goes wave shuffle -> LDS -> one partial per block into the handle's own buffer (a Newton pass of m = 8 needs
// m + m (m + 1) / 2 = 44 sums, more than the 12 slots of femo_ctx::d_partials) and is folded by k_mma_fold in the fixed order
// of femo_fold_partials.  The grid depends on n alone, so a step gives the same bits from run to run; no float atomics.
//
// Per variable the handle keeps x1, x2, L, U, alpha, beta, p_i, q_i (i = 0..m), xi, eta; U - x, x - L and the Newton
// direction (dx, dxi, deta) are recomputed in registers from lambda and delta lambda, which travel as kernel arguments.
// The unknowns of size m (y, lambda, mu, s) live on the host, where the m x m system is solved (small_solve.h).
// Svanberg's variable z and constants a_i are dropped: a_i = 0 makes z = 0 at the optimum.
//
// One Newton step: k_mma_assemble (sums of the dual system) -> host solve -> k_mma_stepmax (largest step that keeps x, xi,
// eta positive) -> k_mma_trial (residual at the trial point; once more per halving) -> k_mma_trial<WRITE> (commit).
// Bytes per Newton step: see DESIGN.md section 10, "Optimiser".
//
// Out of scope: GCMMA's inner conservative loop, equality constraints, m > 8, partitioned meshes.  xmax = xmin is refused:
// passive cells go through the projection (project.hip), which also carries the Heaviside step of the continuation.
#include <chrono>
#include <cmath>

#include "femo_internal.h"
#include "small_solve.h"

namespace {

constexpr int MMA_MAX_M = FEMO_MMA_MAX_M;
constexpr int MMA_BLOCK = 256;
constexpr int MMA_WAVES = MMA_BLOCK / FEMO_WAVE;
constexpr int MMA_MAX_SUMS = 64;                        // sums + maxima of one pass; the blocking copy is at most this long
constexpr double ASYINIT = 0.5, ASYINCR = 1.2, ASYDECR = 0.7, ASYMIN = 0.01, ASYMAX = 10.0, ALBEFA = 0.1, RAA0 = 1e-5;
constexpr int MMA_MAX_NEWTON = 200, MMA_MAX_HALVINGS = 50;

// the unknowns of size m as a pass needs them (kernel argument, by value)
struct MmaSmall {
  double lam[MMA_MAX_M];     // lambda the direction is taken at
  double dlam[MMA_MAX_M];    // delta lambda
  double lamt[MMA_MAX_M];    // lambda of the trial point (formed on the host, so that both sides use the same bits)
  double eps, steg;
};

struct MmaArrays {           // device arrays of the handle, by value
  double *x, *xsi, *eta;
  const double *L, *U, *alfa, *beta, *p, *q;   // p, q: m + 1 rows of n
  int64_t n;
};

__device__ __forceinline__ double mma_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;   // valid in lane 0
}

// NS sums and NX maxima of the block into part[j * nb + blockIdx.x] (sums first): one barrier, fixed order
template <int NS, int NX>
__device__ __forceinline__ void mma_block_reduce(const double* s, const double* x, double* lds /* MMA_WAVES * (NS + NX) */,
                                                 double* __restrict__ part, int nb) {
  constexpr int NV = NS + NX;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const double t = femo_wave_sum(s[j]);
    if (lane == 0) lds[w * NV + j] = t;
  }
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    const double t = mma_wave_max(x[j]);
    if (lane == 0) lds[w * NV + NS + j] = t;
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < NV) {
    double t = lds[j];
    if (j < NS) { for (int k = 1; k < MMA_WAVES; ++k) t += lds[k * NV + j]; }
    else { for (int k = 1; k < MMA_WAVES; ++k) t = fmax(t, lds[k * NV + j]); }
    part[(int64_t)j * nb + blockIdx.x] = t;
  }
}

// block j folds entry j: a sum (j < nsum) in the order of femo_fold_partials, or a maximum
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_fold(int nb, int nsum, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double lds[MMA_WAVES];
  const int j = blockIdx.x;
  const double* p = part + (int64_t)j * nb;
  if (j < nsum) {
    const double t = femo_fold_partials<MMA_BLOCK>(p, nb, lds);
    if (threadIdx.x == 0) out[j] = t;
  } else {
    double a = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += MMA_BLOCK) a = fmax(a, p[i]);
    a = mma_wave_max(a);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = lds[0];
      for (int k = 1; k < MMA_WAVES; ++k) t = fmax(t, lds[k]);
      out[j] = t;
    }
  }
}

// ---- checks ---------------------------------------------------------------------------------------------------------
// sums: [0] bounds that are not finite, [1] entries with xmax <= xmin
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_check_bounds(int64_t n, const double* __restrict__ xmin, const double* __restrict__ xmax,
                                                                double* __restrict__ part, int nb) {
  __shared__ double lds[MMA_WAVES * 2];
  double s[2] = {0.0, 0.0};
  for (int64_t j = (int64_t)blockIdx.x * MMA_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * MMA_BLOCK) {
    const double a = xmin[j], b = xmax[j];
    if (!isfinite(a) || !isfinite(b)) s[0] += 1.0;
    else if (!(b > a)) s[1] += 1.0;
  }
  mma_block_reduce<2, 0>(s, nullptr, lds, part, nb);
}

// sums: [0] entries of x, df0, df that are not finite, [1] entries of x outside [xmin, xmax]
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_check_input(int64_t n, int m, const double* __restrict__ x, const double* __restrict__ xmin,
                                                               const double* __restrict__ xmax, const double* __restrict__ df0,
                                                               const double* __restrict__ df, double* __restrict__ part, int nb) {
  __shared__ double lds[MMA_WAVES * 2];
  double s[2] = {0.0, 0.0};
  for (int64_t j = (int64_t)blockIdx.x * MMA_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * MMA_BLOCK) {
    const double xv = x[j];
    bool bad = !isfinite(xv) || !isfinite(df0[j]);
    for (int i = 0; i < m; ++i) bad = bad || !isfinite(df[(int64_t)i * n + j]);
    if (bad) s[0] += 1.0;
    if (xv < xmin[j] || xv > xmax[j]) s[1] += 1.0;
  }
  mma_block_reduce<2, 0>(s, nullptr, lds, part, nb);
}

// ---- per design step: asymptotes, move limits, p, q, the sums of b; history ---------------------------------------------
// Written operation by operation as tests/mma_ref.py has it, without contraction into fused multiply-adds, so that L, U,
// alpha, beta, p and q carry the restatement's roundings.
template <int M>
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_setup(int64_t n, int k, double move, const double* __restrict__ x,
                                                         const double* __restrict__ xmin, const double* __restrict__ xmax,
                                                         double* __restrict__ x1, double* __restrict__ x2, double* __restrict__ L,
                                                         double* __restrict__ U, double* __restrict__ alfa, double* __restrict__ beta,
                                                         double* __restrict__ p, double* __restrict__ q, const double* __restrict__ df0,
                                                         const double* __restrict__ df, double* __restrict__ part, int nb) {
#pragma clang fp contract(off)
  __shared__ double lds[MMA_WAVES * (M > 0 ? M : 1)];
  double bs[M > 0 ? M : 1];
#pragma unroll
  for (int i = 0; i < (M > 0 ? M : 1); ++i) bs[i] = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * MMA_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * MMA_BLOCK) {
    const double xv = x[j], lo = xmin[j], hi = xmax[j], range = hi - lo;
    const double xo1 = x1[j];
    double Lj, Uj;
    if (k <= 2) {
      Lj = xv - ASYINIT * range;
      Uj = xv + ASYINIT * range;
    } else {
      const double z = (xv - xo1) * (xo1 - x2[j]);
      const double gam = z > 0.0 ? ASYINCR : z < 0.0 ? ASYDECR : 1.0;
      Lj = xv - gam * (xo1 - L[j]);
      Uj = xv + gam * (U[j] - xo1);
      Lj = fmin(fmax(Lj, xv - ASYMAX * range), xv - ASYMIN * range);
      Uj = fmax(fmin(Uj, xv + ASYMAX * range), xv + ASYMIN * range);
    }
    const double ux = Uj - xv, xl = xv - Lj;
    alfa[j] = fmax(fmax(Lj + ALBEFA * xl, xv - move * range), lo);
    beta[j] = fmin(fmin(Uj - ALBEFA * ux, xv + move * range), hi);
    L[j] = Lj;
    U[j] = Uj;
    x2[j] = xo1;
    x1[j] = xv;
    const double rho = RAA0 / range, ux2 = ux * ux, xl2 = xl * xl;
#pragma unroll
    for (int i = 0; i <= M; ++i) {
      const double g = i == 0 ? df0[j] : df[(int64_t)(i - 1) * n + j];
      const double gp = fmax(g, 0.0), gm = fmax(-g, 0.0);
      const double pj = ux2 * (1.001 * gp + 0.001 * gm + rho), qj = xl2 * (0.001 * gp + 1.001 * gm + rho);
      p[(int64_t)i * n + j] = pj;
      q[(int64_t)i * n + j] = qj;
      if (i > 0) bs[i - 1] += pj / ux + qj / xl;
    }
  }
  if (M > 0) mma_block_reduce<(M > 0 ? M : 1), 0>(bs, nullptr, lds, part, nb);
}

// ---- the subproblem's starting point; for M = 0 its solution -------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_start(MmaArrays a) {
  for (int64_t j = (int64_t)blockIdx.x * MMA_BLOCK + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * MMA_BLOCK) {
    const double al = a.alfa[j], be = a.beta[j];
    if (M == 0) {
      const double sp = sqrt(a.p[j]), sq = sqrt(a.q[j]);
      a.x[j] = fmin(fmax((sp * a.L[j] + sq * a.U[j]) / (sp + sq), al), be);
    } else {
      const double xs = 0.5 * (al + be);
      a.x[j] = xs;
      a.xsi[j] = fmax(1.0 / (xs - al), 1.0);
      a.eta[j] = fmax(1.0 / (be - xs), 1.0);
    }
  }
}

// ---- one variable of the Newton system -------------------------------------------------------------------------------------
template <int M>
struct MmaPoint {
  double x, xsi, eta, xa, bx;       // xa = x - alpha, bx = beta - x
  double L, U, alfa, beta;
  double p[M + 1], q[M + 1];
  double delx, diagx, GG[M];

  __device__ __forceinline__ void load(const MmaArrays& a, int64_t j) {
    x = a.x[j]; xsi = a.xsi[j]; eta = a.eta[j];
    L = a.L[j]; U = a.U[j]; alfa = a.alfa[j]; beta = a.beta[j];
#pragma unroll
    for (int i = 0; i <= M; ++i) { p[i] = a.p[(int64_t)i * a.n + j]; q[i] = a.q[(int64_t)i * a.n + j]; }
    xa = x - alfa; bx = beta - x;
  }
  // delx, diagx, GG at (x, xsi, eta, lam) and barrier eps
  __device__ __forceinline__ void system(const double* lam, double eps) {
    const double ux = U - x, xl = x - L, iux2 = 1.0 / (ux * ux), ixl2 = 1.0 / (xl * xl);
    double plam = p[0], qlam = q[0];
#pragma unroll
    for (int i = 0; i < M; ++i) { plam += lam[i] * p[i + 1]; qlam += lam[i] * q[i + 1]; }
    delx = plam * iux2 - qlam * ixl2 - eps / xa + eps / bx;
    diagx = 2.0 * (plam * iux2 / ux + qlam * ixl2 / xl) + xsi / xa + eta / bx;
#pragma unroll
    for (int i = 0; i < M; ++i) GG[i] = p[i + 1] * iux2 - q[i + 1] * ixl2;
  }
  __device__ __forceinline__ void direction(const double* dlam, double eps, double& dx, double& dxsi, double& deta) const {
    double gd = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) gd += GG[i] * dlam[i];
    dx = -delx / diagx - gd / diagx;
    dxsi = -xsi + eps / xa - xsi * dx / xa;
    deta = -eta + eps / bx + eta * dx / bx;
  }
};

// sums: GG (delx / diagx) [M], then the upper triangle of GG diag(1 / diagx) GG^T row by row [M (M + 1) / 2]
template <int M>
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_assemble(MmaArrays a, MmaSmall S, double* __restrict__ part, int nb) {
  constexpr int NS = M + M * (M + 1) / 2;
  __shared__ double lds[MMA_WAVES * NS];
  double s[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) s[i] = 0.0;
  MmaPoint<M> P;
  for (int64_t j = (int64_t)blockIdx.x * MMA_BLOCK + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * MMA_BLOCK) {
    P.load(a, j);
    P.system(S.lam, S.eps);
    const double id = 1.0 / P.diagx, t = P.delx * id;
    int o = M;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      s[i] += P.GG[i] * t;
      const double gi = P.GG[i] * id;
#pragma unroll
      for (int k = i; k < M; ++k) s[o++] += gi * P.GG[k];
    }
  }
  mma_block_reduce<NS, 0>(s, nullptr, lds, part, nb);
}

// maximum: 1.01 times the largest of -dx / (x - alpha), dx / (beta - x), -dxi / xi, -deta / eta
template <int M>
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_stepmax(MmaArrays a, MmaSmall S, double* __restrict__ part, int nb) {
  __shared__ double lds[MMA_WAVES];
  double mx[1] = {-INFINITY};
  MmaPoint<M> P;
  for (int64_t j = (int64_t)blockIdx.x * MMA_BLOCK + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * MMA_BLOCK) {
    P.load(a, j);
    P.system(S.lam, S.eps);
    double dx, dxsi, deta;
    P.direction(S.dlam, S.eps, dx, dxsi, deta);
    const double t = fmax(fmax(-1.01 * dx / P.xa, 1.01 * dx / P.bx), fmax(-1.01 * dxsi / P.xsi, -1.01 * deta / P.eta));
    mx[0] = fmax(mx[0], t);
  }
  mma_block_reduce<0, 1>(nullptr, mx, lds, part, nb);
}

// The point (x, xi, eta) + steg (dx, dxi, deta), lambda = lamt.  WRITE: stored (the step is taken).  Otherwise its residual:
// sums: [0] the squares of the rows of size n (stationarity in x, xi (x - alpha) - eps, eta (beta - x) - eps), [1..M] g_i(x);
// maximum: the largest modulus among those rows.  steg = 0 gives the residual of the point as it stands.
template <int M, bool WRITE>
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_trial(MmaArrays a, MmaSmall S, double* __restrict__ part, int nb) {
  __shared__ double lds[MMA_WAVES * (M + 2)];
  double s[M + 1], mx[1] = {0.0};
#pragma unroll
  for (int i = 0; i <= M; ++i) s[i] = 0.0;
  MmaPoint<M> P;
  for (int64_t j = (int64_t)blockIdx.x * MMA_BLOCK + threadIdx.x; j < a.n; j += (int64_t)gridDim.x * MMA_BLOCK) {
    P.load(a, j);
    double xt = P.x, xsit = P.xsi, etat = P.eta;
    if (S.steg != 0.0) {
      P.system(S.lam, S.eps);
      double dx, dxsi, deta;
      P.direction(S.dlam, S.eps, dx, dxsi, deta);
      xt += S.steg * dx; xsit += S.steg * dxsi; etat += S.steg * deta;
    }
    if (WRITE) {
      a.x[j] = xt; a.xsi[j] = xsit; a.eta[j] = etat;
    } else {
      const double ux = P.U - xt, xl = xt - P.L, iux = 1.0 / ux, ixl = 1.0 / xl;
      double plam = P.p[0], qlam = P.q[0];
#pragma unroll
      for (int i = 0; i < M; ++i) {
        plam += S.lamt[i] * P.p[i + 1]; qlam += S.lamt[i] * P.q[i + 1];
        s[i + 1] += P.p[i + 1] * iux + P.q[i + 1] * ixl;
      }
      const double rex = plam * iux * iux - qlam * ixl * ixl - xsit + etat;
      const double rexsi = xsit * (xt - P.alfa) - S.eps, reeta = etat * (P.beta - xt) - S.eps;
      s[0] += rex * rex + rexsi * rexsi + reeta * reeta;
      mx[0] = fmax(mx[0], fmax(fabs(rex), fmax(fabs(rexsi), fabs(reeta))));
    }
  }
  if (!WRITE) mma_block_reduce<M + 1, 1>(s, mx, lds, part, nb);
}

// maxima: |x - x1|, |x - x1| / (xmax - xmin)
__global__ __launch_bounds__(MMA_BLOCK) void k_mma_change(int64_t n, const double* __restrict__ x, const double* __restrict__ x1,
                                                          const double* __restrict__ xmin, const double* __restrict__ xmax,
                                                          double* __restrict__ part, int nb) {
  __shared__ double lds[MMA_WAVES * 2];
  double mx[2] = {0.0, 0.0};
  for (int64_t j = (int64_t)blockIdx.x * MMA_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * MMA_BLOCK) {
    const double d = fabs(x[j] - x1[j]);
    mx[0] = fmax(mx[0], d);
    mx[1] = fmax(mx[1], d / (xmax[j] - xmin[j]));
  }
  mma_block_reduce<0, 2>(nullptr, mx, lds, part, nb);
}

}  // namespace

struct femo_mma {
  femo_ctx* ctx = nullptr;
  int64_t n = 0;
  int m = 0;
  femo_mma_params par{};
  int k = 0;                                  // design steps taken since creation / reset
  int nb = 1;                                 // grid of every pass: a function of n alone
  double* d_block = nullptr;                  // one allocation for all per-variable arrays
  double *xmin = nullptr, *xmax = nullptr, *x1 = nullptr, *x2 = nullptr, *L = nullptr, *U = nullptr, *alfa = nullptr, *beta = nullptr;
  double *xsi = nullptr, *eta = nullptr, *p = nullptr, *q = nullptr, *xsub = nullptr;   // xsub: x of femo_mma_solve_subproblem
  double* d_part = nullptr;                   // [MMA_MAX_SUMS][nb]
  double* d_out = nullptr;                    // [MMA_MAX_SUMS]
  double* h_out = nullptr;                    // pinned mirror
  double b[MMA_MAX_M] = {}, bsum[MMA_MAX_M] = {};
  int copies = 0;                             // blocking copies of the call in progress
};

namespace {

// fold nsum sums + nmax maxima of the pass just enqueued and wait for them in h->h_out
int mma_fetch(femo_mma* h, int nsum, int nmax) {
  hipStream_t st = h->ctx->stream;
  hipLaunchKernelGGL(k_mma_fold, dim3(nsum + nmax), dim3(MMA_BLOCK), 0, st, h->nb, nsum, h->d_part, h->d_out);
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_HIP_CHECK(hipMemcpyAsync(h->h_out, h->d_out, (size_t)(nsum + nmax) * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  ++h->copies;
  return 0;
}

MmaArrays mma_arrays(femo_mma* h, double* x) {
  return MmaArrays{x, h->xsi, h->eta, h->L, h->U, h->alfa, h->beta, h->p, h->q, h->n};
}

#define MMA_DISPATCH(m, CALL)                                                                     \
  switch (m) {                                                                                    \
    case 1: { constexpr int M = 1; CALL; } break;  case 2: { constexpr int M = 2; CALL; } break;  \
    case 3: { constexpr int M = 3; CALL; } break;  case 4: { constexpr int M = 4; CALL; } break;  \
    case 5: { constexpr int M = 5; CALL; } break;  case 6: { constexpr int M = 6; CALL; } break;  \
    case 7: { constexpr int M = 7; CALL; } break;  case 8: { constexpr int M = 8; CALL; } break;  \
    default: break;                                                                               \
  }

int mma_launch_assemble(femo_mma* h, const MmaArrays& a, const MmaSmall& S) {
  MMA_DISPATCH(h->m, hipLaunchKernelGGL(k_mma_assemble<M>, dim3(h->nb), dim3(MMA_BLOCK), 0, h->ctx->stream, a, S, h->d_part, h->nb));
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}
int mma_launch_stepmax(femo_mma* h, const MmaArrays& a, const MmaSmall& S) {
  MMA_DISPATCH(h->m, hipLaunchKernelGGL(k_mma_stepmax<M>, dim3(h->nb), dim3(MMA_BLOCK), 0, h->ctx->stream, a, S, h->d_part, h->nb));
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}
int mma_launch_trial(femo_mma* h, const MmaArrays& a, const MmaSmall& S, bool write) {
  if (write) {
    MMA_DISPATCH(h->m, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mma_trial<M, true>), dim3(h->nb), dim3(MMA_BLOCK), 0, h->ctx->stream, a, S, h->d_part, h->nb));
  } else {
    MMA_DISPATCH(h->m, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mma_trial<M, false>), dim3(h->nb), dim3(MMA_BLOCK), 0, h->ctx->stream, a, S, h->d_part, h->nb));
  }
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}
int mma_launch_start(femo_mma* h, const MmaArrays& a) {
  if (h->m == 0) hipLaunchKernelGGL(k_mma_start<0>, dim3(h->nb), dim3(MMA_BLOCK), 0, h->ctx->stream, a);
  else hipLaunchKernelGGL(k_mma_start<1>, dim3(h->nb), dim3(MMA_BLOCK), 0, h->ctx->stream, a);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// the unknowns of size m
struct MmaHost {
  double y[MMA_MAX_M], lam[MMA_MAX_M], mu[MMA_MAX_M], s[MMA_MAX_M];
};

// residual of the trial point: the device part from h->h_out (sum of squares, g, maximum), the rows of size m from T
void mma_residual(const femo_mma* h, const MmaHost& T, double eps, double* gvec, double* resi, double* resmax) {
  const int m = h->m;
  double ss = h->h_out[0], mx = h->h_out[m + 1];
  for (int i = 0; i < m; ++i) {
    gvec[i] = h->h_out[1 + i];
    const double r[4] = {h->par.c[i] + h->par.d[i] * T.y[i] - T.mu[i] - T.lam[i], gvec[i] - T.y[i] + T.s[i] - h->b[i],
                         T.mu[i] * T.y[i] - eps, T.lam[i] * T.s[i] - eps};
    for (double v : r) { ss += v * v; mx = std::fmax(mx, std::fabs(v)); }
    if (std::isnan(r[0] + r[1] + r[2] + r[3])) mx = NAN;     // fmax drops a NaN: keep it
  }
  *resi = std::sqrt(ss);
  *resmax = std::isnan(ss) ? NAN : mx;
}

// Svanberg's primal-dual Newton iteration on the subproblem in the handle's arrays; x: n entries, overwritten
int mma_subsolve(femo_mma* h, double* x, femo_mma_info* info, MmaHost* out) {
  const int m = h->m;
  const MmaArrays a = mma_arrays(h, x);
  FEMO_TRY(mma_launch_start(h, a));
  info->converged = 1;
  info->stages = info->newton_steps = info->halvings = 0;
  info->residual_max = 0.0;
  if (m == 0) return 0;                       // closed form, no iteration
  MmaHost V;
  for (int i = 0; i < m; ++i) { V.y[i] = V.lam[i] = V.s[i] = 1.0; V.mu[i] = std::fmax(1.0, 0.5 * h->par.c[i]); }
  const int stages = (int)std::ceil(-std::log10(h->par.sub_tol)) + 1;     // barrier 10^0 ... 10^-K: K + 1 values
  MmaSmall S{};
  double gvec[MMA_MAX_M], resi = 0.0, resmax = 0.0;
  int64_t pow10 = 1;
  for (int stage = 0; stage < stages && info->converged == 1; ++stage, pow10 *= 10) {
    const double eps = 1.0 / (double)pow10;
    ++info->stages;
    S.eps = eps; S.steg = 0.0;
    for (int i = 0; i < m; ++i) { S.lam[i] = S.lamt[i] = V.lam[i]; S.dlam[i] = 0.0; }
    FEMO_TRY(mma_launch_trial(h, a, S, false));
    FEMO_TRY(mma_fetch(h, m + 1, 1));
    mma_residual(h, V, eps, gvec, &resi, &resmax);
    int it = 0;
    while (resmax > 0.9 * eps && it < MMA_MAX_NEWTON) {
      ++it;
      ++info->newton_steps;
      FEMO_TRY(mma_launch_assemble(h, a, S));
      FEMO_TRY(mma_fetch(h, m + m * (m + 1) / 2, 0));
      double A[FEMO_SMALL_MAX * FEMO_SMALL_MAX] = {}, dlam[FEMO_SMALL_MAX] = {}, dely[MMA_MAX_M], diagy[MMA_MAX_M];
      int o = m;
      for (int i = 0; i < m; ++i) {
        dely[i] = h->par.c[i] + h->par.d[i] * V.y[i] - V.lam[i] - eps / V.y[i];
        diagy[i] = h->par.d[i] + V.mu[i] / V.y[i];
        const double dellam = gvec[i] - V.y[i] - h->b[i] + eps / V.lam[i];
        dlam[i] = dellam + dely[i] / diagy[i] - h->h_out[i];
        for (int k = i; k < m; ++k, ++o) A[i * FEMO_SMALL_MAX + k] = A[k * FEMO_SMALL_MAX + i] = h->h_out[o];
        A[i * FEMO_SMALL_MAX + i] += V.s[i] / V.lam[i] + 1.0 / diagy[i];
      }
      if (femo_small_solve(m, A, FEMO_SMALL_MAX, dlam) != 0) { info->converged = 0; break; }
      MmaHost D;      // the direction of the unknowns of size m
      double stmax = 1.0;
      for (int i = 0; i < m; ++i) {
        D.lam[i] = dlam[i];
        D.y[i] = -dely[i] / diagy[i] + dlam[i] / diagy[i];
        D.mu[i] = -V.mu[i] + eps / V.y[i] - V.mu[i] * D.y[i] / V.y[i];
        D.s[i] = -V.s[i] + eps / V.lam[i] - V.s[i] * dlam[i] / V.lam[i];
        stmax = std::fmax(stmax, std::fmax(std::fmax(-1.01 * D.y[i] / V.y[i], -1.01 * D.lam[i] / V.lam[i]),
                                           std::fmax(-1.01 * D.mu[i] / V.mu[i], -1.01 * D.s[i] / V.s[i])));
        S.dlam[i] = dlam[i];
      }
      FEMO_TRY(mma_launch_stepmax(h, a, S));
      FEMO_TRY(mma_fetch(h, 0, 1));
      stmax = std::fmax(stmax, h->h_out[0]);
      if (!std::isfinite(stmax)) { info->converged = 0; break; }
      double steg = 1.0 / stmax, resinew = 0.0, resmaxnew = 0.0, gnew[MMA_MAX_M];
      MmaHost T;
      int halv = 0;
      for (;;) {
        ++halv;
        for (int i = 0; i < m; ++i) {
          T.y[i] = V.y[i] + steg * D.y[i]; T.lam[i] = V.lam[i] + steg * D.lam[i];
          T.mu[i] = V.mu[i] + steg * D.mu[i]; T.s[i] = V.s[i] + steg * D.s[i];
          S.lamt[i] = T.lam[i];
        }
        S.steg = steg;
        FEMO_TRY(mma_launch_trial(h, a, S, false));
        FEMO_TRY(mma_fetch(h, m + 1, 1));
        mma_residual(h, T, eps, gnew, &resinew, &resmaxnew);
        if (!(resinew > resi) || halv >= MMA_MAX_HALVINGS) break;
        steg *= 0.5;
      }
      info->halvings += halv - 1;
      if (resinew > resi) info->converged = 0;           // 50 halvings did not bring the residual down: reported, the step is taken
      FEMO_TRY(mma_launch_trial(h, a, S, true));
      V = T;
      for (int i = 0; i < m; ++i) { gvec[i] = gnew[i]; S.lam[i] = V.lam[i]; S.dlam[i] = 0.0; }
      S.steg = 0.0;
      resi = resinew; resmax = resmaxnew;
      if (!std::isfinite(resmax)) { info->converged = 0; break; }
    }
    if (resmax > 0.9 * eps) info->converged = 0;         // 200 steps did not finish the stage
  }
  info->residual_max = resmax;
  for (int i = 0; i < m; ++i) { info->lam[i] = V.lam[i]; info->y[i] = V.y[i]; }
  if (out) *out = V;
  return 0;
}

int mma_grid(const femo_ctx* ctx, int64_t n) {
  int64_t g = (n + MMA_BLOCK - 1) / MMA_BLOCK;
  const int64_t cap = (int64_t)ctx->n_cu * 4;
  if (g > cap) g = cap;
  if (g > FEMO_MAX_PARTIALS) g = FEMO_MAX_PARTIALS;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int femo_mma_destroy(femo_mma* h) {
  if (!h) return 0;
  hipFree(h->d_block); hipFree(h->d_part); hipFree(h->d_out);
  if (h->h_out) hipHostFree(h->h_out);
  delete h;
  return 0;
}

extern "C" int femo_mma_create(femo_ctx* ctx, int64_t n, int m, const femo_vec* xmin, const femo_vec* xmax,
                               const femo_mma_params* params, femo_mma** out) {
  FEMO_REQUIRE(ctx && xmin && xmax && out, "null argument");
  *out = nullptr;
  FEMO_REQUIRE(ctx->nranks == 1, "mma: one rank only (partitioned meshes are out of scope)");
  FEMO_REQUIRE(n >= 1, "mma: n = %lld, need at least one variable", (long long)n);
  FEMO_REQUIRE(m >= 0 && m <= MMA_MAX_M, "mma: m = %d general constraints, supported: 0 to %d", m, MMA_MAX_M);
  FEMO_REQUIRE(xmin->n >= n && xmax->n >= n, "mma: bounds shorter than n");
  femo_mma_params par;
  if (params) par = *params;
  else {
    par.move = 0.5; par.sub_tol = 1e-7;
    for (int i = 0; i < MMA_MAX_M; ++i) { par.c[i] = 1000.0; par.d[i] = 1.0; }
  }
  FEMO_REQUIRE(par.move > 0.0 && std::isfinite(par.move), "mma: move = %g, must be positive", par.move);
  FEMO_REQUIRE(par.sub_tol > 0.0 && par.sub_tol <= 1.0, "mma: sub_tol = %g, must lie in (0, 1]", par.sub_tol);
  for (int i = 0; i < m; ++i)
    FEMO_REQUIRE(par.c[i] >= 0.0 && par.d[i] > 0.0 && std::isfinite(par.c[i]) && std::isfinite(par.d[i]),
                 "mma: c[%d] = %g, d[%d] = %g: need c >= 0 and d > 0", i, par.c[i], i, par.d[i]);
  FEMO_TRY(femo_vec_await(xmin));
  FEMO_TRY(femo_vec_await(xmax));
  femo_mma* h = new femo_mma;
  h->ctx = ctx; h->n = n; h->m = m; h->par = par;
  h->nb = mma_grid(ctx, n);
  const int64_t stride = (n + 31) & ~(int64_t)31;                  // 256-byte aligned arrays
  const int64_t n_arrays = 11 + 2 * (int64_t)(m + 1);
  auto fail = [&](int rc) { femo_mma_destroy(h); return rc; };
  if (hipMalloc(&h->d_block, (size_t)(n_arrays * stride) * sizeof(double)) != hipSuccess ||
      hipMalloc(&h->d_part, (size_t)MMA_MAX_SUMS * h->nb * sizeof(double)) != hipSuccess ||
      hipMalloc(&h->d_out, MMA_MAX_SUMS * sizeof(double)) != hipSuccess ||
      hipHostMalloc(&h->h_out, MMA_MAX_SUMS * sizeof(double), hipHostMallocDefault) != hipSuccess) {
    femo_set_error("mma: out of memory for %lld variables, %d constraints", (long long)n, m);
    return fail(1);
  }
  double* w = h->d_block;
  for (double** a : {&h->xmin, &h->xmax, &h->x1, &h->x2, &h->L, &h->U, &h->alfa, &h->beta, &h->xsi, &h->eta, &h->xsub}) { *a = w; w += stride; }
  // p and q: m + 1 rows exactly n apart (the kernels index row i at i * n)
  h->p = w; h->q = w + (int64_t)(m + 1) * stride;
  hipStream_t st = ctx->stream;
  if (hipMemsetAsync(h->d_block, 0, (size_t)(n_arrays * stride) * sizeof(double), st) != hipSuccess ||
      hipMemcpyAsync(h->xmin, xmin->d, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(h->xmax, xmax->d, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) {
    femo_set_error("mma: copying the bounds failed");
    return fail(1);
  }
  hipLaunchKernelGGL(k_mma_check_bounds, dim3(h->nb), dim3(MMA_BLOCK), 0, st, n, h->xmin, h->xmax, h->d_part, h->nb);
  int rc = mma_fetch(h, 2, 0);
  if (rc != 0) return fail(rc);
  if (h->h_out[0] != 0.0) { femo_set_error("mma: %.0f bounds are not finite (MMA needs a box)", h->h_out[0]); return fail(2); }
  if (h->h_out[1] != 0.0) {
    femo_set_error("mma: xmax <= xmin in %.0f entries (passive regions are out of scope)", h->h_out[1]);
    return fail(2);
  }
  *out = h;
  return 0;
}

extern "C" int femo_mma_reset(femo_mma* h) {
  FEMO_REQUIRE(h, "null argument");
  h->k = 0;
  return 0;
}

extern "C" int femo_mma_update(femo_mma* h, femo_vec* x, double f0, const femo_vec* df0, const double* f, const femo_vec* df,
                               femo_mma_info* info) {
  FEMO_REQUIRE(h && x && df0 && info, "null argument");
  const int m = h->m;
  const int64_t n = h->n;
  FEMO_REQUIRE(m == 0 || (f && df), "mma: %d constraints need their values and gradients", m);
  FEMO_REQUIRE(x->n >= n && df0->n >= n && (m == 0 || df->n >= (int64_t)m * n), "mma: a vector is shorter than n (x %lld, df0 %lld)",
               (long long)x->n, (long long)df0->n);
  FEMO_REQUIRE(std::isfinite(f0), "mma: the objective value is not finite");
  for (int i = 0; i < m; ++i) FEMO_REQUIRE(std::isfinite(f[i]), "mma: the value of constraint %d is not finite", i);
  const auto t0 = std::chrono::steady_clock::now();
  h->copies = 0;
  FEMO_TRY(femo_vec_await(x));
  FEMO_TRY(femo_vec_await(df0));
  if (m > 0) FEMO_TRY(femo_vec_await(df));
  hipStream_t st = h->ctx->stream;
  const double* dfd = m > 0 ? df->d : nullptr;
  hipLaunchKernelGGL(k_mma_check_input, dim3(h->nb), dim3(MMA_BLOCK), 0, st, n, m, x->d, h->xmin, h->xmax, df0->d, dfd, h->d_part, h->nb);
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_TRY(mma_fetch(h, 2, 0));
  FEMO_REQUIRE(h->h_out[0] == 0.0, "mma: %.0f entries of x or of a gradient are not finite", h->h_out[0]);
  FEMO_REQUIRE(h->h_out[1] == 0.0, "mma: x lies outside its bounds in %.0f entries", h->h_out[1]);
  femo_vec_touch(x);
  const int k = ++h->k;
  *info = femo_mma_info{};
  info->step = k;
#define MMA_SETUP(MM) hipLaunchKernelGGL(k_mma_setup<MM>, dim3(h->nb), dim3(MMA_BLOCK), 0, st, n, k, h->par.move, x->d, h->xmin, h->xmax, \
                                         h->x1, h->x2, h->L, h->U, h->alfa, h->beta, h->p, h->q, df0->d, dfd, h->d_part, h->nb)
  if (m == 0) MMA_SETUP(0);
  else MMA_DISPATCH(m, MMA_SETUP(M));
#undef MMA_SETUP
  FEMO_HIP_CHECK(hipGetLastError());
  if (m > 0) {
    FEMO_TRY(mma_fetch(h, m, 0));
    for (int i = 0; i < m; ++i) { h->bsum[i] = h->h_out[i]; h->b[i] = h->bsum[i] - f[i]; }
  }
  FEMO_TRY(mma_subsolve(h, x->d, info, nullptr));
  hipLaunchKernelGGL(k_mma_change, dim3(h->nb), dim3(MMA_BLOCK), 0, st, n, x->d, h->x1, h->xmin, h->xmax, h->d_part, h->nb);
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_TRY(mma_fetch(h, 0, 2));
  info->max_dx = h->h_out[0];
  info->max_dx_rel = h->h_out[1];
  info->blocking_copies = h->copies;
  info->update_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int femo_mma_get(femo_mma* h, int what, int i, double* out) {
  FEMO_REQUIRE(h && out, "null argument");
  FEMO_REQUIRE(what >= 0 && what <= 9, "mma: no such array (%d)", what);
  if (what == 6 || what == 7) {
    for (int k = 0; k < h->m; ++k) out[k] = what == 6 ? h->b[k] : h->bsum[k];
    return 0;
  }
  const double* src = nullptr;
  if (what == 4 || what == 5) {
    FEMO_REQUIRE(i >= 0 && i <= h->m, "mma: function %d of 0..%d", i, h->m);
    src = (what == 4 ? h->p : h->q) + (int64_t)i * h->n;
  } else {
    const double* a[] = {h->L, h->U, h->alfa, h->beta, nullptr, nullptr, nullptr, nullptr, h->xsi, h->eta};
    src = a[what];
  }
  FEMO_HIP_CHECK(hipMemcpyAsync(out, src, (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
  FEMO_HIP_CHECK(hipStreamSynchronize(h->ctx->stream));
  return 0;
}

extern "C" int femo_mma_solve_subproblem(femo_mma* h, const double* L, const double* U, const double* alpha, const double* beta,
                                         const double* p, const double* q, const double* b, double* x, double* xi, double* eta,
                                         double* small, femo_mma_info* info) {
  FEMO_REQUIRE(h && L && U && alpha && beta && p && q && x && info, "null argument");
  const int m = h->m;
  const int64_t n = h->n;
  FEMO_REQUIRE(m == 0 || (b && small), "mma: %d constraints need b and room for the unknowns of size m", m);
  hipStream_t st = h->ctx->stream;
  const size_t nb = (size_t)n * sizeof(double);
  FEMO_HIP_CHECK(hipMemcpyAsync(h->L, L, nb, hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(h->U, U, nb, hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(h->alfa, alpha, nb, hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(h->beta, beta, nb, hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(h->p, p, nb * (size_t)(m + 1), hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(h->q, q, nb * (size_t)(m + 1), hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < m; ++i) { h->b[i] = b[i]; h->bsum[i] = 0.0; }
  *info = femo_mma_info{};
  h->copies = 0;
  MmaHost V{};
  FEMO_TRY(mma_subsolve(h, h->xsub, info, &V));
  info->blocking_copies = h->copies;
  FEMO_HIP_CHECK(hipMemcpyAsync(x, h->xsub, nb, hipMemcpyDeviceToHost, st));
  if (m > 0 && xi) FEMO_HIP_CHECK(hipMemcpyAsync(xi, h->xsi, nb, hipMemcpyDeviceToHost, st));
  if (m > 0 && eta) FEMO_HIP_CHECK(hipMemcpyAsync(eta, h->eta, nb, hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < m; ++i) { small[i] = V.y[i]; small[m + i] = V.lam[i]; small[2 * m + i] = V.mu[i]; small[3 * m + i] = V.s[i]; }
  return 0;
}
