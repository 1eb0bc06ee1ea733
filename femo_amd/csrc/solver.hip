// Krylov solvers for gfx950 on the SELL-64 operator of spmv.hip: the vector reductions, Jacobi-CG, single-reduction CG,
// BPX-PCG and BiCGSTAB, and their host drivers.
//
// Replaces the reference's PETSc calls:
//   KSP preonly + LU(MUMPS)  utils_dolfinx.py:476-512            (fea_dolfinx.py:192-222)
// CG + Jacobi instead of LU is BASELINE.json's design: a sparse
// LU of the 10 M-DOF 3-D operator does not fit, and CSR/SELL SpMV streams at the
// HBM roofline.
//
// CG keeps every scalar of the recurrence on the device: kernels reduce into
// per-block partials, a one-block kernel folds them (plus an RCCL all-reduce
// when nranks > 1) and the consumers read the folded scalars.  The host only
// polls a "done" flag every `check_every` iterations, two batches deep.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "femo_internal.h"

namespace {

// ------------------------------------------------------------- CG kernels ---
// Jacobi-preconditioned CG is run as plain CG on the symmetrically scaled system
//     (S A S) xh = S b,   x = S xh,   S = diag(A)^-1/2
// which generates the same iterates in exact arithmetic, has a unit diagonal (no
// diagonal or D^-1 stream per iteration) and makes gamma = rh.rh = r^T D^-1 r the
// only norm needed.  Convergence: sqrt(gamma) <= max(rtol sqrt(bh.bh), atol), the
// "natural" norm of preconditioned CG (PETSc KSP_NORM_NATURAL [ext]).
//
// Per iteration (single GPU, 3 launches, 10 N-vectors of traffic besides the matrix):
//   k_spmv_sell<true,true>   qh = Ah ph, partial ph.qh                  (x gather N, y write N)
//   k_cg_update_r            alpha = gamma/delta; rh -= alpha qh; partial rh.rh     (3 N)
//   k_cg_update_xp           xh += alpha ph; ph = rh + beta ph; convergence flag    (5 N)
// Scalars never visit the host: every block folds the producers' per-block partials
// itself in a fixed order, so all blocks see bitwise identical values.  With nranks > 1
// the single-reduction recurrence further down is used instead (one fold + one RCCL
// all-reduce per iteration).  Not captured in a hipGraph on purpose: every launch runs
// >= 40 us at the sizes of interest against ~3.5 us of host cost per launch, and the
// device-side boundary costs the same eagerly or replayed (MI355X_MICROARCH.md price list).
// partial slots: 0 = delta, 1/2 = gamma of even/odd iterations, 3 = scratch.
// scal: [0],[1] = gamma even/odd, [2] = delta, [3] = tol^2.   flags: [0] done, [1] iterations, [2] breakdown.
constexpr int S_GAMMA = 0, S_DELTA = 2, S_TOL2 = 3;
constexpr int P_DELTA = 0, P_GAMMA = 1;

// rh = S (b - q) (q = A x0 or null); ph = rh; xh = 0; partials: slot 1 = rh.rh, slot 2 = (S b).(S b).
// Identity rows (idrow: the Dirichlet rows of the last assembly; their columns are eliminated too) are solved
// here, xh = rh exactly, and take no part in the iteration or in either norm: with u = 1 as initial state the
// lifted values on those rows are O(1) while the interior right-hand side is O(h^3), and a tolerance relative to
// the whole vector would be no tolerance for the interior unknowns.
__global__ __launch_bounds__(FEMO_BLOCK) void k_cg_init(int64_t n, const double* __restrict__ b, const double* __restrict__ q,
                                                        const double* __restrict__ s, double* __restrict__ r,
                                                        double* __restrict__ p, double* __restrict__ xh,
                                                        double* __restrict__ partials, const uint8_t* __restrict__ idrow) {
  __shared__ double lds[FEMO_BLOCK / 64];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FEMO_BLOCK) {
    const double si = s[i], bi = si * b[i];
    const double ri = q ? si * (b[i] - q[i]) : bi;
    if (idrow != nullptr && idrow[i]) {
      r[i] = 0.0; p[i] = 0.0; xh[i] = ri;
      continue;
    }
    r[i] = ri; p[i] = ri; xh[i] = 0.0;
    s0 += ri * ri; s1 += bi * bi;
  }
  double t = femo_block_sum<FEMO_BLOCK>(s0, lds);
  if (threadIdx.x == 0) partials[1 * FEMO_MAX_PARTIALS + blockIdx.x] = t;
  t = femo_block_sum<FEMO_BLOCK>(s1, lds);
  if (threadIdx.x == 0) partials[2 * FEMO_MAX_PARTIALS + blockIdx.x] = t;
}

// rh -= alpha qh ; partial rh.rh into the gamma slot of the next parity
__global__ __launch_bounds__(FEMO_BLOCK) void k_cg_update_r(int64_t n, int cur, int nb_d, int nb_g,
                                                            double* __restrict__ partials, const double* __restrict__ scal,
                                                            const double* __restrict__ q, double* __restrict__ r,
                                                            const int32_t* __restrict__ done) {
  if (*done) return;
  __shared__ double lds[FEMO_BLOCK / 64];
  const double gamma = femo_fold_partials<FEMO_BLOCK>(partials + (P_GAMMA + cur) * FEMO_MAX_PARTIALS, nb_g, lds);
  const double delta = femo_fold_partials<FEMO_BLOCK>(partials + P_DELTA * FEMO_MAX_PARTIALS, nb_d, lds);
  const double alpha = delta != 0.0 ? gamma / delta : 0.0;
  double s0 = 0.0;
  const int64_t n2 = n >> 1;
  const double2* q2 = reinterpret_cast<const double2*>(q);
  double2* r2 = reinterpret_cast<double2*>(r);
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * FEMO_BLOCK) {
    const double2 qi = q2[i];
    double2 ri = r2[i];
    ri.x -= alpha * qi.x; ri.y -= alpha * qi.y;
    r2[i] = ri;
    s0 += ri.x * ri.x + ri.y * ri.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const double ri = r[n - 1] - alpha * q[n - 1];
    r[n - 1] = ri;
    s0 += ri * ri;
  }
  const double t = femo_block_sum<FEMO_BLOCK>(s0, lds);
  if (threadIdx.x == 0) partials[(P_GAMMA + (cur ^ 1)) * FEMO_MAX_PARTIALS + blockIdx.x] = t;
}

// xh += alpha ph ; then (unless converged) ph = rh + beta ph
__global__ __launch_bounds__(FEMO_BLOCK) void k_cg_update_xp(int64_t n, int cur, int it, int nb_d, int nb_g,
                                                             const double* __restrict__ partials, const double* __restrict__ scal,
                                                             const double* __restrict__ r, double* __restrict__ p,
                                                             double* __restrict__ xh, int32_t* __restrict__ flags) {
  // flags[0] = (iteration index + 1) at which convergence was detected, 0 while running.
  // A block of THIS launch may already have set it; only an earlier iteration's stamp
  // means "done" here, otherwise late blocks would skip their part of the x update.
  const int32_t stamp = flags[0];
  if (stamp != 0 && stamp != it + 1) return;
  __shared__ double lds[FEMO_BLOCK / 64];
  const int nxt = cur ^ 1;
  const double gamma = femo_fold_partials<FEMO_BLOCK>(partials + (P_GAMMA + cur) * FEMO_MAX_PARTIALS, nb_g, lds);
  const double gamma1 = femo_fold_partials<FEMO_BLOCK>(partials + (P_GAMMA + nxt) * FEMO_MAX_PARTIALS, nb_g, lds);
  const double delta = femo_fold_partials<FEMO_BLOCK>(partials + P_DELTA * FEMO_MAX_PARTIALS, nb_d, lds);
  const double alpha = delta != 0.0 ? gamma / delta : 0.0;
  const bool bad = !(gamma1 == gamma1) || !(alpha == alpha);  // NaN: not SPD or diverged
  const bool converged = gamma1 <= scal[S_TOL2] || bad;
  const double beta = gamma != 0.0 ? gamma1 / gamma : 0.0;
  const int64_t n2 = n >> 1;
  const double2* r2 = reinterpret_cast<const double2*>(r);
  double2* p2 = reinterpret_cast<double2*>(p);
  double2* x2 = reinterpret_cast<double2*>(xh);
  if (converged) {
    if (!bad) {
      for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * FEMO_BLOCK) {
        const double2 pi = p2[i];
        double2 xi = x2[i];
        xi.x += alpha * pi.x; xi.y += alpha * pi.y;
        x2[i] = xi;
      }
      if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) xh[n - 1] += alpha * p[n - 1];
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * FEMO_BLOCK) {
      const double2 ri = r2[i];
      double2 pi = p2[i], xi = x2[i];
      xi.x += alpha * pi.x; xi.y += alpha * pi.y;
      pi.x = ri.x + beta * pi.x; pi.y = ri.y + beta * pi.y;
      x2[i] = xi; p2[i] = pi;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      const int64_t i = n - 1;
      const double pi = p[i];
      xh[i] += alpha * pi;
      p[i] = r[i] + beta * pi;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    flags[1] = it + 1;
    if (converged) {
      flags[2] = bad ? 1 : 0;
      __threadfence();
      flags[0] = it + 1;
    }
  }
}

// ---- BPX-preconditioned CG (bpx.hip) ------------------------------------------------
// scal: [0],[1] = gamma = rh.zh of even/odd iterations, [2] = delta = ph.Ah ph, [3] = tol^2,
// [4] = rho = rh.rh (the natural-norm residual the stopping test uses, same as Jacobi-CG).
constexpr int S_RHO = 4;
constexpr int S_ALPHA = 8;  // alpha of the current iteration (k_pcg_xr with carry_x: the x update runs inside the preconditioner)
constexpr int S_TOLG = 5;   // rtol^2 * gamma_0: the stopping threshold on gamma = rh.zh (set on the device by the first apply)

// xh += alpha ph ; rh -= alpha qh ; partial rh.rh.  nb_d > 0: delta is folded here from the
// SpMV's per-block partials (single GPU: no fold kernel, no all-reduce), else read from scal.
__global__ __launch_bounds__(FEMO_BLOCK) void k_pcg_xr(int64_t n, int cur, int nb_d, const double* __restrict__ partials_d,
                                                       double* __restrict__ scal,
                                                       const double* __restrict__ q, const double* __restrict__ p,
                                                       const double* r_in, double* r, double* __restrict__ xh,
                                                       double* __restrict__ partials, const int32_t* __restrict__ done, int carry_x = 0) {
  // r = r_in - alpha q: in place (r_in == r) or into the other residual buffer when the restriction of the
  // caller keeps the old residual
  if (*done) return;
  __shared__ double lds[FEMO_BLOCK / 64];
  const double gamma = scal[S_GAMMA + cur];
  const double delta = nb_d > 0 ? femo_fold_partials<FEMO_BLOCK>(partials_d, nb_d, lds) : scal[S_DELTA];
  if (nb_d > 0 && blockIdx.x == 0 && threadIdx.x == 0) scal[S_DELTA] = delta;   // for the breakdown test
  const double alpha = delta != 0.0 ? gamma / delta : 0.0;
  double s0 = 0.0;
  const int64_t n2 = n >> 1;
  const double2* q2 = reinterpret_cast<const double2*>(q);
  const double2* p2 = reinterpret_cast<const double2*>(p);
  double2* r2 = reinterpret_cast<double2*>(r);
  const double2* r2_in = reinterpret_cast<const double2*>(r_in);
  double2* x2 = reinterpret_cast<double2*>(xh);
  if (carry_x) {
    // the residual only (3 of the 6 vector streams); x += alpha p is carried by the preconditioner's coarse-lattice launch
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[S_ALPHA] = alpha;
    for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * FEMO_BLOCK) {
      const double2 qi = q2[i];
      double2 ri = r2_in[i];
      ri.x -= alpha * qi.x; ri.y -= alpha * qi.y;
      r2[i] = ri;
      s0 += ri.x * ri.x + ri.y * ri.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
      const double ri = r_in[n - 1] - alpha * q[n - 1];
      r[n - 1] = ri;
      s0 += ri * ri;
    }
    const double t = femo_block_sum<FEMO_BLOCK>(s0, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * FEMO_BLOCK) {
    const double2 qi = q2[i], pi = p2[i];
    double2 ri = r2_in[i], xi = x2[i];
    xi.x += alpha * pi.x; xi.y += alpha * pi.y;
    ri.x -= alpha * qi.x; ri.y -= alpha * qi.y;
    x2[i] = xi; r2[i] = ri;
    s0 += ri.x * ri.x + ri.y * ri.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    xh[i] += alpha * p[i];
    const double ri = r_in[i] - alpha * q[i];
    r[i] = ri;
    s0 += ri * ri;
  }
  const double t = femo_block_sum<FEMO_BLOCK>(s0, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// stopping test on the reduced rho; runs alone on the stream, so later kernels see a settled flag.
// nb > 0: folds the rho partials first (single GPU); else rho was folded and all-reduced before.
__global__ __launch_bounds__(1024) void k_pcg_check(int it, int nb, const double* __restrict__ partials,
                                                    double* __restrict__ scal, int32_t* __restrict__ flags) {
  if (flags[0]) return;
  __shared__ double lds[1024 / 64];
  double rho = nb > 0 ? femo_fold_partials<1024>(partials, nb, lds) : 0.0;
  if (threadIdx.x != 0) return;
  if (nb > 0) scal[S_RHO] = rho; else rho = scal[S_RHO];
  const double delta = scal[S_DELTA];
  const bool bad = !(rho == rho) || !(delta == delta);
  flags[1] = it + 1;
  if (rho <= scal[S_TOL2] || bad) {
    flags[2] = bad ? 1 : 0;
    flags[0] = it + 1;
  }
}

// ---- single-reduction CG (Chronopoulos & Gear) for nranks > 1 ---------------------
// One all-reduce of (gamma = r.r, delta = r.Ar) and one halo exchange per iteration:
//   beta = gamma/gamma_old; alpha = gamma / (delta - beta*gamma/alpha_old)
//   p = r + beta p; s = w + beta s; x += alpha p; r -= alpha s;   then w = A r with both dots
// fused into the SpMV.  scal: (delta, gamma) of parity c at [2c], [2c+1] (contiguous for one
// all-reduce); alpha of parity c at [4+c]; tol^2 at [6].
constexpr int M_A = 4, M_TOL2 = 6;

__global__ __launch_bounds__(FEMO_BLOCK) void k_cgm_update(int64_t n, int it, double* __restrict__ scal,
                                                           const double* __restrict__ w, double* __restrict__ r,
                                                           double* __restrict__ p, double* __restrict__ sv,
                                                           double* __restrict__ xh, int32_t* __restrict__ flags) {
  const int32_t stamp = flags[0];
  if (stamp != 0 && stamp != it + 1) return;
  const int cur = it & 1, prv = cur ^ 1;
  const double delta = scal[2 * cur], gamma = scal[2 * cur + 1];
  const bool bad = !(gamma == gamma) || !(delta == delta);
  if (gamma <= scal[M_TOL2] || bad) {              // converged before this update: `it` iterations done
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      flags[1] = it;
      flags[2] = bad ? 1 : 0;
      __threadfence();
      flags[0] = it + 1;
    }
    return;
  }
  double beta = 0.0, alpha;
  if (it == 0) {
    alpha = delta != 0.0 ? gamma / delta : 0.0;
  } else {
    const double g_old = scal[2 * prv + 1], a_old = scal[M_A + prv];
    beta = g_old != 0.0 ? gamma / g_old : 0.0;
    const double den = delta - beta * gamma / a_old;
    alpha = den != 0.0 ? gamma / den : 0.0;
  }
  const int64_t n2 = n >> 1;
  const double2* w2 = reinterpret_cast<const double2*>(w);
  double2* r2 = reinterpret_cast<double2*>(r);
  double2* p2 = reinterpret_cast<double2*>(p);
  double2* s2 = reinterpret_cast<double2*>(sv);
  double2* x2 = reinterpret_cast<double2*>(xh);
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n2; i += (int64_t)gridDim.x * FEMO_BLOCK) {
    const double2 wi = w2[i];
    double2 ri = r2[i], pi = p2[i], si = s2[i], xi = x2[i];
    pi.x = ri.x + beta * pi.x; pi.y = ri.y + beta * pi.y;
    si.x = wi.x + beta * si.x; si.y = wi.y + beta * si.y;
    xi.x += alpha * pi.x; xi.y += alpha * pi.y;
    ri.x -= alpha * si.x; ri.y -= alpha * si.y;
    p2[i] = pi; s2[i] = si; x2[i] = xi; r2[i] = ri;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    const double pi = r[i] + beta * p[i], si = w[i] + beta * sv[i];
    p[i] = pi; sv[i] = si; xh[i] += alpha * pi; r[i] -= alpha * si;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    scal[M_A + cur] = alpha;                         // read by the next iteration (other parity slot)
    flags[1] = it + 1;
  }
}

// ---- BiCGSTAB on the scaled system (non-symmetric operators) --------------------------
// van der Vorst's recurrence; S A S keeps a unit diagonal, i.e. Jacobi preconditioning.
// Scalars live in scal[]; producers write partials, a one-block fold (plus all-reduce when
// nranks > 1) sits between producer and consumer.  Not the headline path: kept simple.
constexpr int B_RHO = 0, B_RHO_OLD = 1, B_ALPHA = 2, B_OMEGA = 3, B_R0V = 4, B_TS = 5, B_TT = 6, B_RR = 7, B_TOL2 = 8;

__global__ __launch_bounds__(FEMO_BLOCK) void k_bi_init(int64_t n, const double* __restrict__ b, const double* __restrict__ q,
                                                        const double* __restrict__ s, double* __restrict__ r, double* __restrict__ r0,
                                                        double* __restrict__ p, double* __restrict__ v, double* __restrict__ xh,
                                                        double* __restrict__ partials) {
  __shared__ double lds[FEMO_BLOCK / 64];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FEMO_BLOCK) {
    const double si = s[i], bi = si * b[i];
    const double ri = q ? si * (b[i] - q[i]) : bi;
    r[i] = ri; r0[i] = ri; p[i] = 0.0; v[i] = 0.0; xh[i] = 0.0;
    s0 += ri * ri; s1 += bi * bi;
  }
  double t = femo_block_sum<FEMO_BLOCK>(s0, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  t = femo_block_sum<FEMO_BLOCK>(s1, lds);
  if (threadIdx.x == 0) partials[FEMO_MAX_PARTIALS + blockIdx.x] = t;
}

// convergence test on (rho, rr) after `it` finished iterations (one thread; every later launch sees the flag)
__global__ void k_bi_check(int it, const double* __restrict__ scal, int32_t* __restrict__ flags) {
  if (flags[0]) return;
  const double rho = scal[B_RHO], rr = scal[B_RR];
  const bool bad = !(rr == rr) || !(rho == rho);
  if (rr <= scal[B_TOL2] || bad) {
    flags[1] = it;
    flags[2] = bad ? 1 : 0;
    flags[0] = 1;
  }
}

// p = r + beta (p - omega v)
__global__ __launch_bounds__(FEMO_BLOCK) void k_bi_p(int64_t n, int it, const double* __restrict__ scal, const double* __restrict__ r,
                                                     const double* __restrict__ v, double* __restrict__ p, const int32_t* __restrict__ flags) {
  if (flags[0]) return;
  double beta = 0.0, omega = 0.0;
  if (it > 0) {
    omega = scal[B_OMEGA];
    beta = (scal[B_RHO] / scal[B_RHO_OLD]) * (scal[B_ALPHA] / omega);
  }
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FEMO_BLOCK)
    p[i] = r[i] + beta * (p[i] - omega * v[i]);
}

// alpha = rho / (r0, v); s = r - alpha v
__global__ __launch_bounds__(FEMO_BLOCK) void k_bi_s(int64_t n, double* __restrict__ scal, const double* __restrict__ r,
                                                     const double* __restrict__ v, double* __restrict__ sv, const int32_t* __restrict__ done) {
  if (*done) return;
  const double alpha = scal[B_RHO] / scal[B_R0V];
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FEMO_BLOCK)
    sv[i] = r[i] - alpha * v[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[B_ALPHA] = alpha;   // not read by this launch
}

// omega = (t,s)/(t,t); x += alpha p + omega s; r = s - omega t; partials (r0, r), (r, r)
__global__ __launch_bounds__(FEMO_BLOCK) void k_bi_xr(int64_t n, int it, double* __restrict__ scal, const double* __restrict__ p,
                                                      const double* __restrict__ sv, const double* __restrict__ t,
                                                      const double* __restrict__ r0, double* __restrict__ xh, double* __restrict__ r,
                                                      double* __restrict__ partials, int32_t* __restrict__ flags) {
  if (flags[0]) return;
  __shared__ double lds[FEMO_BLOCK / 64];
  const double tt = scal[B_TT];
  const double omega = tt != 0.0 ? scal[B_TS] / tt : 0.0;
  const double alpha = scal[B_ALPHA];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FEMO_BLOCK) {
    const double si = sv[i];
    xh[i] += alpha * p[i] + omega * si;
    const double ri = si - omega * t[i];
    r[i] = ri;
    s0 += r0[i] * ri; s1 += ri * ri;
  }
  double f = femo_block_sum<FEMO_BLOCK>(s0, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = f;
  f = femo_block_sum<FEMO_BLOCK>(s1, lds);
  if (threadIdx.x == 0) partials[FEMO_MAX_PARTIALS + blockIdx.x] = f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    scal[B_OMEGA] = omega;               // read by the next launches only
    scal[B_RHO_OLD] = scal[B_RHO];       // rho of this iteration; B_RHO is overwritten by the next fold
    flags[1] = it + 1;
  }
}

// (rho, rr) of one fold land in buf[0], buf[1]; move them to their scal slots
__global__ void k_bi_set_rho(const double* __restrict__ buf, double* __restrict__ scal, const int32_t* __restrict__ done) {
  if (*done) return;
  scal[B_RHO] = buf[0];
  scal[B_RR] = buf[1];
}

// x = (add ? x : 0) + s .* xh
__global__ void k_unscale(int64_t n, int add, const double* __restrict__ s, const double* __restrict__ xh, double* __restrict__ x) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    x[i] = (add ? x[i] : 0.0) + s[i] * xh[i];
}

// the same, but only once the loop has converged (flags[0] != 0): enqueued behind every batch of the merged loop so that
// the poll that finds the solve converged finds the solution too -- one host round trip less per solve (round 6)
__global__ void k_unscale_done(int64_t n, int add, const double* __restrict__ s, const double* __restrict__ xh, double* __restrict__ x,
                               const int32_t* __restrict__ flags) {
  if (flags[0] == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    x[i] = (add ? x[i] : 0.0) + s[i] * xh[i];
}

// Kept search directions of the one-rank merged BPX-PCG (ensure_ring): x^ += sum_j alpha_j p_j over j = base .. flags[1] - 1,
// one fma per direction in the order of the iterations -- what the carriers' per-iteration x^ = fma(alpha, p, x^) leaves.
// Direction j sits in slot j % slots of `ring` (slots `stride` doubles apart), alpha_j in alpha_hist[j % slots].  flags[1]
// counts the iterations DONE, not those enqueued (launches behind the converging one return at once), and the direction of
// the converging iteration belongs in x^: no early exit on flags[0] unless only_done asks for the opposite (the batch poll:
// nothing to do while the loop runs).  Nothing to add: x^ is not written.  s != nullptr: x = (add ? x : 0) + s .* x^ as
// k_unscale, from the sum in registers.
__global__ __launch_bounds__(256) void k_pcg_flush(int64_t n, double* __restrict__ xh, const double* __restrict__ ring, int64_t stride,
                                                   int slots, const double* __restrict__ alpha_hist, int base,
                                                   const int32_t* __restrict__ flags, int only_done, int add,
                                                   const double* __restrict__ s, double* __restrict__ x) {
  if (only_done && flags[0] == 0) return;
  const int count = min(flags[1], base + slots);          // (the host flushes before a slot is reused: never more than `slots`)
  if (count <= base && s == nullptr) return;
  const int k0 = base % slots;                            // slot of direction `base`; the walk below wraps without a division
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double acc = xh[i];
    int k = k0;
#pragma unroll 4
    for (int j = base; j < count; ++j) {
      acc = fma(alpha_hist[k], ring[(int64_t)k * stride + i], acc);
      k = k + 1 == slots ? 0 : k + 1;
    }
    if (count > base) xh[i] = acc;
    if (s != nullptr) x[i] = (add ? x[i] : 0.0) + s[i] * acc;
  }
}

__global__ __launch_bounds__(FEMO_BLOCK) void k_dot(int64_t n, const double* __restrict__ a, const double* __restrict__ b,
                                                    double* __restrict__ partials) {
  __shared__ double lds[FEMO_BLOCK / 64];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FEMO_BLOCK) s += a[i] * b[i];
  const double t = femo_block_sum<FEMO_BLOCK>(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// the one stand-alone fold (femo_launch_fold): what an all-reduce between a producer and its consumers works on
template <int NT>
__global__ __launch_bounds__(NT) void k_fold(int nb, int nsums, const double* __restrict__ partials, int nb2,
                                             const double* __restrict__ partials2, double* __restrict__ out,
                                             const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  __shared__ double lds[NT / 64];
  for (int j = 0; j < nsums; ++j) {
    const int64_t o = (int64_t)j * FEMO_MAX_PARTIALS;
    const double t = femo_fold_partials<NT>(partials + o, nb, lds, partials2 != nullptr ? partials2 + o : nullptr, nb2);
    if (threadIdx.x == 0) out[j] = t;
  }
}

inline int vec_grid(const femo_ctx* ctx, int64_t n) {
  int64_t g = (n / 2 + FEMO_BLOCK - 1) / FEMO_BLOCK;
  const int64_t cap = (int64_t)ctx->n_cu * 8;
  if (g > cap) g = cap;
  if (g > FEMO_MAX_PARTIALS) g = FEMO_MAX_PARTIALS;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

int femo_launch_fold(int nt, int nb, int nsums, const double* partials, double* out, hipStream_t st,
                     const int32_t* done, int nb2, const double* partials2) {
  FEMO_REQUIRE(nt == 1024 || nt == 256, "femo_launch_fold: 1024 or 256 threads");
  if (nt == 1024) hipLaunchKernelGGL(k_fold<1024>, dim3(1), dim3(1024), 0, st, nb, nsums, partials, nb2, partials2, out, done);
  else hipLaunchKernelGGL(k_fold<256>, dim3(1), dim3(256), 0, st, nb, nsums, partials, nb2, partials2, out, done);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int femo_vec_dot(const femo_vec* x, const femo_vec* y, int64_t n, double* out) {
  FEMO_REQUIRE(x && y && out, "null argument");
  FEMO_REQUIRE(n <= x->n && n <= y->n, "dot length exceeds vector size");
  FEMO_TRY(femo_vec_await(x));
  FEMO_TRY(femo_vec_await(y));
  femo_ctx* ctx = x->ctx;
  const int g = vec_grid(ctx, n);
  hipLaunchKernelGGL(k_dot, dim3(g), dim3(FEMO_BLOCK), 0, ctx->stream, n, x->d, y->d, ctx->d_partials);
  FEMO_HIP_CHECK(hipGetLastError());
  return femo_reduce_to_host(ctx, g, 1, out);
}

namespace {
// rb != nullptr: one more sum behind the k pairs (slot k) -- rho_0 of the Krylov loops for the right-hand side rb and the
// operator with diagonal `diag`, sum over the rows that are not identity rows of (rb_i / sqrt(diag_i))^2, formed exactly as
// k_invsqrt_diag + k_cg_init form it: Newton takes the solver's own "nothing to iterate on" decision from it (round 6)
struct DotPairs { const double* a[4]; const double* b[4]; int k; const double* rb; const double* diag; const uint8_t* idrow; };
__global__ __launch_bounds__(FEMO_BLOCK) void k_dots(int64_t n, DotPairs d, double* __restrict__ partials) {
  __shared__ double lds[FEMO_BLOCK / 64];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  double rho = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FEMO_BLOCK) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < d.k) s[j] += d.a[j][i] * d.b[j][i];
    if (d.rb != nullptr && !(d.idrow != nullptr && d.idrow[i])) {
      const double si = 1.0 / sqrt(d.diag[i]);
      const double ri = si * d.rb[i];
      rho += ri * ri;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < d.k) {
      const double t = femo_block_sum<FEMO_BLOCK>(s[j], lds);
      if (threadIdx.x == 0) partials[(int64_t)j * FEMO_MAX_PARTIALS + blockIdx.x] = t;
    }
  }
  if (d.rb != nullptr) {
    const double t = femo_block_sum<FEMO_BLOCK>(rho, lds);
    if (threadIdx.x == 0) partials[(int64_t)d.k * FEMO_MAX_PARTIALS + blockIdx.x] = t;
  }
}
}  // namespace

// x = what a Krylov solve of A x = b returns when it decides not to iterate from the zero guess: b_i / diag_i on the identity
// rows of the last assembly (the loops solve them up front, k_cg_init), 0 elsewhere
// flag != null (Newton's flagged passes): raised when an entry stored to x is anything but +0.0 in its bits (-0.0 and NaN
// count as non-zero: y += a x may change y's bits with them).  Cleared on the stream before this launch.
__global__ void k_identity_solve(int64_t n, int64_t n_all, const double* __restrict__ b, const double* __restrict__ diag,
                                 const uint8_t* __restrict__ idrow, double* __restrict__ x, int32_t* __restrict__ flag) {
  bool nz = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += (int64_t)gridDim.x * blockDim.x) {
    double v = 0.0;
    if (i < n && idrow != nullptr && idrow[i]) { const double si = 1.0 / sqrt(diag[i]); v = si * (si * b[i]); }
    x[i] = v;
    nz = nz || __double_as_longlong(v) != 0;
  }
  if (flag != nullptr && nz) atomicOr(flag, 1);
}
static int identity_solve(const femo_mat* A, const femo_vec* b, femo_vec* x, bool flagged) {
  FEMO_REQUIRE(A && b && x, "null argument");
  const femo_mesh* m = A->mesh;
  FEMO_REQUIRE(b->n >= m->n_rows && x->n >= m->n_rows, "vector size mismatch");
  FEMO_TRY(femo_vec_await(b));
  femo_vec_touch(x);
  auto& nk = m->ctx->newton;
  if (flagged) {
    // the flag speaks about the right-hand side in place only if this b IS that right-hand side; x becomes the dx it describes.
    // Otherwise nobody will be handed the flag: the plain launch
    nk.live = nk.rhs_valid && b->uid != 0 && b->uid == nk.b_uid && b->gen == nk.b_gen && x->uid != 0 && x->ctx == m->ctx && x->n > 0;
    nk.dx_uid = x->uid; nk.dx_gen = x->gen;
    flagged = nk.live;
    if (flagged) FEMO_HIP_CHECK(hipMemsetAsync(m->ctx->d_newton, 0, sizeof(int32_t), m->ctx->stream));
  }
  if (x->n == 0) return 0;
  hipLaunchKernelGGL(k_identity_solve, dim3(2048), dim3(256), 0, m->ctx->stream, m->n_rows, x->n, b->d, A->d_diag, A->has_idrows ? A->d_idrows : nullptr, x->d,
                     flagged ? m->ctx->d_newton : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}
extern "C" int femo_mat_identity_solve(const femo_mat* A, const femo_vec* b, femo_vec* x) { return identity_solve(A, b, x, false); }
extern "C" int femo_mat_identity_solve_flag(const femo_mat* A, const femo_vec* b, femo_vec* x) { return identity_solve(A, b, x, true); }

static int vec_dots(int k, const femo_vec* const* x, const femo_vec* const* y, int64_t n, double* out, const femo_mat* A, const femo_vec* rb);
extern "C" int femo_vec_dots(int k, const femo_vec* const* x, const femo_vec* const* y, int64_t n, double* out) {
  return vec_dots(k, x, y, n, out, nullptr, nullptr);
}
// ... and out[k] = rho_0 a Krylov solve of A with right-hand side rb would start from (see k_dots): the same launch, the same
// reduction, the same host synchronisation
extern "C" int femo_vec_dots_rhs(int k, const femo_vec* const* x, const femo_vec* const* y, int64_t n, double* out,
                                 const femo_mat* A, const femo_vec* rb) {
  FEMO_REQUIRE(A && rb && A->d_diag, "femo_vec_dots_rhs: null matrix / right-hand side");
  FEMO_REQUIRE(n <= rb->n && n <= A->mesh->n_rows, "femo_vec_dots_rhs: length exceeds the operator's rows");
  return vec_dots(k, x, y, n, out, A, rb);
}
static int vec_dots(int k, const femo_vec* const* x, const femo_vec* const* y, int64_t n, double* out, const femo_mat* A, const femo_vec* rb) {
  FEMO_REQUIRE(x && y && out && k >= 1 && k <= 4, "femo_vec_dots: 1..4 pairs");
  DotPairs d;
  d.k = k;
  d.rb = nullptr; d.diag = nullptr; d.idrow = nullptr;
  if (A != nullptr) {
    FEMO_TRY(femo_vec_await(rb));
    d.rb = rb->d; d.diag = A->d_diag; d.idrow = A->has_idrows ? A->d_idrows : nullptr;
  }
  for (int j = 0; j < 4; ++j) {
    const int jj = j < k ? j : 0;
    FEMO_REQUIRE(x[jj] && y[jj] && n <= x[jj]->n && n <= y[jj]->n, "dot length exceeds vector size");
    d.a[j] = x[jj]->d; d.b[j] = y[jj]->d;
    FEMO_TRY(femo_vec_await(x[jj]));
    FEMO_TRY(femo_vec_await(y[jj]));
  }
  femo_ctx* ctx = x[0]->ctx;
  const int g = vec_grid(ctx, n);
  hipLaunchKernelGGL(k_dots, dim3(g), dim3(FEMO_BLOCK), 0, ctx->stream, n, d, ctx->d_partials);
  FEMO_HIP_CHECK(hipGetLastError());
  return femo_reduce_to_host(ctx, g, k + (A != nullptr ? 1 : 0), out);
}

namespace {
struct CgWork {
  double *r, *p, *q, *xh, *sv, *t, *r0;
};

// need: 0 = standard CG, 1 = single-reduction CG (+sv), 2 = BiCGSTAB (+sv, t, r0)
int ensure_work(femo_ctx* ctx, int64_t n_rows, int64_t n_vert, CgWork& w, int need, bool zero = true) {
  const int64_t len = std::max(n_rows, n_vert) + 2;
  if (ctx->cg_n < len) {
    hipFree(ctx->cg_r); hipFree(ctx->cg_p); hipFree(ctx->cg_q); hipFree(ctx->cg_dinv); hipFree(ctx->cg_s);
    hipFree(ctx->cg_t); hipFree(ctx->cg_r0); hipFree(ctx->cg_ring);
    ctx->cg_r = ctx->cg_p = ctx->cg_q = ctx->cg_dinv = ctx->cg_s = ctx->cg_t = ctx->cg_r0 = ctx->cg_ring = nullptr;
    ctx->cg_n = 0; ctx->cg_ring_slots = ctx->cg_ring_want = 0;
    FEMO_HIP_CHECK(hipMalloc(&ctx->cg_r, len * sizeof(double)));
    FEMO_HIP_CHECK(hipMalloc(&ctx->cg_p, len * sizeof(double)));
    FEMO_HIP_CHECK(hipMalloc(&ctx->cg_q, len * sizeof(double)));
    FEMO_HIP_CHECK(hipMalloc(&ctx->cg_dinv, len * sizeof(double)));   // holds xh
    ctx->cg_n = len;
  }
  if (need >= 1 && !ctx->cg_s) FEMO_HIP_CHECK(hipMalloc(&ctx->cg_s, ctx->cg_n * sizeof(double)));
  if (need >= 2 && !ctx->cg_t) FEMO_HIP_CHECK(hipMalloc(&ctx->cg_t, ctx->cg_n * sizeof(double)));
  if (need >= 2 && !ctx->cg_r0) FEMO_HIP_CHECK(hipMalloc(&ctx->cg_r0, ctx->cg_n * sizeof(double)));
  // (zero == false: the caller's init kernel writes every entry it will read -- no ghost tail)
  if (zero) {
    FEMO_HIP_CHECK(hipMemsetAsync(ctx->cg_p, 0, ctx->cg_n * sizeof(double), ctx->stream));
    FEMO_HIP_CHECK(hipMemsetAsync(ctx->cg_r, 0, ctx->cg_n * sizeof(double), ctx->stream));
    if (need >= 1) FEMO_HIP_CHECK(hipMemsetAsync(ctx->cg_s, 0, ctx->cg_n * sizeof(double), ctx->stream));
  }
  w.r = ctx->cg_r; w.p = ctx->cg_p; w.q = ctx->cg_q; w.xh = ctx->cg_dinv; w.sv = ctx->cg_s;
  w.t = ctx->cg_t; w.r0 = ctx->cg_r0;
  return 0;
}

// Ring of kept search directions for the one-rank merged BPX-PCG (after ensure_work: slots of ctx->cg_n doubles).  Nothing
// in that loop reads x^, so instead of streaming it through the carriers of k_lattice_coarse_m every iteration (24 of their
// 48 B per row) the loop leaves p_k in slot k % R -- k_prolong_mesh reads the old direction and writes the new one anyway --
// and k_pcg_flush adds alpha_k p_k to x^ in the order of the iterations when the ring is full and at the end of the solve.
// The rule for R (returned; 0: the per-iteration update):
//   FEMO_PCG_RING unset -> 32 on meshes of at least FEMO_RING_MIN_ROWS rows, 0 below; "0" -> 0; any other value, on any
//   mesh, clamped to 2 .. 64; then halved while the ring exceeds one eighth of the device's memory or hipMalloc fails; a
//   result below 2 -> 0, counted in femo_ctx::pcg_ring_short like every solve that got fewer slots than it asked for.
//   The ring is allocated on the first solve that asks for this R at this vector length and kept until the CG vectors are
//   reallocated or the context goes: a warmed-up cycle allocates nothing.
// FEMO_RING_MIN_ROWS: the carriers run beside workgroup 0 of their launch (the LDS-resident lattice levels, W = 14-21 us); per
// million rows they take 7.6 us with the x^ stream and 4.1 without, a flush 1.5 per iteration, so the ring gains 6.1 us x M rows
// - W per iteration once the carriers outlast workgroup 0 and only costs below (DESIGN_LOG R14: measured at 1.03 M and 10.08 M rows).
constexpr int64_t FEMO_RING_MIN_ROWS = 3000000;
// doubles from one slot to the next: cg_n rounded up to 256 B, so that every slot starts on a cache line like a vector of its own
int64_t ring_stride(const femo_ctx* ctx) { return (ctx->cg_n + 31) & ~int64_t(31); }
int ensure_ring(femo_ctx* ctx, int64_t n_rows, int* slots) {
  *slots = 0;
  const char* env = getenv("FEMO_PCG_RING");              // read once per solve (the tests switch it), never per launch
  int want = n_rows >= FEMO_RING_MIN_ROWS ? 32 : 0;
  if (env != nullptr) {
    want = atoi(env);
    if (want != 0) want = std::min(64, std::max(2, want));
  }
  if (want == 0 || n_rows <= 0) return 0;
  if (!ctx->cg_alpha_hist) FEMO_HIP_CHECK(hipMalloc(&ctx->cg_alpha_hist, 64 * sizeof(double)));   // one per slot of the largest ring
  if (ctx->cg_ring_want != want) {
    hipFree(ctx->cg_ring);
    ctx->cg_ring = nullptr;
    ctx->cg_ring_slots = 0;
    size_t free_b = 0, total_b = 0;
    FEMO_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    (void)free_b;                                          // (the rule is on the device's size, not on what happens to be free)
    const size_t slot_b = (size_t)ring_stride(ctx) * sizeof(double);
    bool refused = false;
    for (int r = want; r >= 2 && ctx->cg_ring_slots == 0; r /= 2) {
      if ((size_t)r * slot_b > total_b / 8) continue;
      if (hipMalloc(&ctx->cg_ring, (size_t)r * slot_b) == hipSuccess) ctx->cg_ring_slots = r;
      else { (void)hipGetLastError(); ctx->cg_ring = nullptr; refused = true; }
    }
    // the outcome is remembered (no attempt per solve) unless hipMalloc refused every size: that may pass, the next solve asks again
    ctx->cg_ring_want = (ctx->cg_ring_slots > 0 || !refused) ? want : 0;
  }
  if (ctx->cg_ring_slots < want) ++ctx->pcg_ring_short;   // visible through femo_mesh_pcg_info
  *slots = ctx->cg_ring_slots;
  return 0;
}
}  // namespace

// ---- host side shared by the Krylov drivers --------------------------------------------------------------------------
// The N-rank code path (folds + all-reduces between producers and consumers): a partitioned run, or FEMO_FORCE_MULTI=1 on
// a 1-rank communicator (tests)
static bool multi_path(const femo_ctx* ctx) {
  return ctx->nranks > 1 || (ctx->comm != nullptr && femo_env_flag("FEMO_FORCE_MULTI"));
}

// r0 = b - q: a zero guess leaves *q0 null (and clears x when clear_x), any other takes q = A x0 with the unscaled operator
// `vals`, the ghosts of x refreshed first
static int initial_guess(femo_mat* A, const double* vals, femo_vec* x, bool zero_guess, bool clear_x, double* q,
                         const double** q0) {
  femo_mesh* m = A->mesh;
  *q0 = nullptr;
  if (zero_guess) {
    if (clear_x) FEMO_HIP_CHECK(hipMemsetAsync(x->d, 0, x->n * sizeof(double), m->ctx->stream));
    return 0;
  }
  if (m->n_nbr > 0) FEMO_TRY(femo_halo_raw(m, x->d, m->ctx->stream));
  FEMO_TRY(femo_launch_spmv(A, x->d, q, {.vals = vals}));
  *q0 = q;
  return 0;
}

// the two sums an init kernel left in consecutive partial slots, folded into d[0], d[1], all-reduced on the N-rank path
// and read back with one host synchronisation: r0.r0 and b.b of the scaled system
static int initial_norms(femo_ctx* ctx, bool multi, int nb, const double* partials, double* d, double* rr0, double* bb) {
  hipStream_t st = ctx->stream;
  FEMO_TRY(femo_launch_fold(1024, nb, 2, partials, d, st));
  if (multi) FEMO_TRY(femo_coll_allreduce(ctx, d, 2, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(ctx->h_scal, d, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  *rr0 = ctx->h_scal[0];
  *bb = ctx->h_scal[1];
  return 0;
}

// x = S xh (+ x0 unless the guess was zero), then ev1, waited for
static int unscale_x(femo_mat* A, const double* xh, femo_vec* x, bool zero_guess) {
  femo_ctx* ctx = A->mesh->ctx;
  const int64_t n = A->mesh->n_rows;
  if (n > 0) {
    hipLaunchKernelGGL(k_unscale, dim3(2048), dim3(256), 0, ctx->stream, n, zero_guess ? 0 : 1, A->d_s, xh, x->d);
    FEMO_HIP_CHECK(hipGetLastError());
  }
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev1, ctx->stream));
  FEMO_HIP_CHECK(hipEventSynchronize(ctx->ev1));
  return 0;
}

// what every driver reports; the solve's time runs from ev0 (recorded first thing) to `end`
static int fill_info(femo_ctx* ctx, hipEvent_t end, femo_solve_info* info, int iters, int conv, double rr) {
  float ms = 0.f;
  FEMO_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, end));
  info->iterations = iters;
  info->converged = conv;
  info->residual_norm = std::sqrt(rr);
  info->solve_ms = ms;
  return 0;
}

static int finish_solve(femo_mat* A, const double* xh, femo_vec* x, bool zero_guess, femo_solve_info* info, int iters,
                        int conv, double rr) {
  FEMO_TRY(unscale_x(A, xh, x, zero_guess));
  femo_mat_compact_settle(A);                    // (the host has just waited for the stream)
  return fill_info(A->mesh->ctx, A->mesh->ctx->ev1, info, iters, conv, rr);
}

// Events around the SpMV of iterations [from, from + N) (ev_pool[0 .. 2N)): info->spmv_ms / spmv_samples, the roofline
// record of bench.py
struct SpmvSamples {
  static constexpr int N = 4;
  femo_ctx* ctx;
  int from;
  int n = 0;
  bool on = false;
  SpmvSamples(femo_ctx* c, int first) : ctx(c), from(first) {}
  int begin(int it) {
    on = it >= from && it < from + N;
    if (on) FEMO_HIP_CHECK(hipEventRecord(ctx->ev_pool[2 * n], ctx->stream));
    return 0;
  }
  int end() {
    if (on) { FEMO_HIP_CHECK(hipEventRecord(ctx->ev_pool[2 * n + 1], ctx->stream)); ++n; }
    return 0;
  }
  int report(femo_solve_info* info) const {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
      float t = 0.f;
      FEMO_HIP_CHECK(hipEventElapsedTime(&t, ctx->ev_pool[2 * i], ctx->ev_pool[2 * i + 1]));
      acc += t;
    }
    info->spmv_ms = acc;
    info->spmv_samples = n;
    return 0;
  }
};
constexpr int POLL_EV = 2 * SpmvSamples::N;   // ev_pool[POLL_EV + slot]: the flag polls

// The host's view of the "done" stamp of a loop enqueued in batches: behind every batch a copy of the four flag words
// (h_flags: two slots of four) and an event.  Two deep: the host waits for the previous batch's copy while the one just
// enqueued runs; `sync` waits for the batch just enqueued instead.  A batch that reaches max_it (`last`) ends the loop.
struct FlagPoll {
  femo_ctx* ctx;
  int32_t* h_flags;
  int polled = 0;
  bool pending[2] = {false, false};
  static int32_t* host_words(femo_ctx* c) { return reinterpret_cast<int32_t*>(c->h_scal + FEMO_NSCAL); }   // two slots of four behind the scalars
  explicit FlagPoll(femo_ctx* c) : ctx(c), h_flags(host_words(c)) {}
  int after_batch(bool last, bool sync, bool* done) {
    hipStream_t st = ctx->stream;
    const int slot = polled & 1;
    FEMO_HIP_CHECK(hipMemcpyAsync(h_flags + 4 * slot, ctx->d_flags, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipEventRecord(ctx->ev_pool[POLL_EV + slot], st));
    pending[slot] = true;
    ++polled;
    const int prev = polled & 1;
    if (sync) {
      FEMO_HIP_CHECK(hipEventSynchronize(ctx->ev_pool[POLL_EV + slot]));
      if (h_flags[4 * slot] || last) *done = true;
      pending[slot] = false;
      return 0;
    }
    if (pending[prev]) {
      FEMO_HIP_CHECK(hipEventSynchronize(ctx->ev_pool[POLL_EV + prev]));
      if (h_flags[4 * prev]) *done = true;
      pending[prev] = false;
    }
    if (!*done && last) {
      FEMO_HIP_CHECK(hipEventSynchronize(ctx->ev_pool[POLL_EV + slot]));
      *done = true;
    }
    return 0;
  }
};

// The four flag words (first host slot) and the device scalars behind everything enqueued so far, waited for: on `ev`,
// recorded behind the two copies, or on the stream when ev is null
static int read_back(femo_ctx* ctx, hipEvent_t ev) {
  hipStream_t st = ctx->stream;
  FEMO_HIP_CHECK(hipMemcpyAsync(FlagPoll::host_words(ctx), ctx->d_flags, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal, FEMO_NSCAL * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ev == nullptr) {
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
  }
  FEMO_HIP_CHECK(hipEventRecord(ev, st));
  FEMO_HIP_CHECK(hipEventSynchronize(ev));
  return 0;
}

// ---- merged BPX-PCG (round 4) ---------------------------------------------------------------------------------------
// One all-reduce + one halo exchange per iteration on N ranks, five launches per iteration on one (SpMV, brick
// restriction of q = A p, coarse lattice + vector updates, fine lattice, mesh prolongation + direction update), one
// host synchronisation before the loop and one after it.  See femo_internal.h "merged BPX-PCG" and DESIGN.md section 4.
// Set-up on the device: rho0 = r0.r0 and bb = b.D^-1 b (folded here on one rank, reduced before on several), the
// thresholds, and the decision not to iterate at all when the initial residual is below the absolute tolerance.
__global__ __launch_bounds__(1024) void k_pcg_setup(int nb, const double* __restrict__ partials, double* __restrict__ S,
                                                    double rtol2, double atol2, int32_t* __restrict__ flags) {
  __shared__ double lds[1024 / 64];
  double rho0, bb;
  if (nb > 0) {
    rho0 = femo_fold_partials<1024>(partials, nb, lds);
    bb = femo_fold_partials<1024>(partials + FEMO_MAX_PARTIALS, nb, lds);
  } else {
    rho0 = S[MS_RED]; bb = S[MS_RED + 1];
  }
  if (threadIdx.x != 0) return;
  S[MS_GAMMA] = 0.0; S[MS_GAMMA + 1] = 0.0; S[MS_PQ] = 0.0; S[MS_ALPHA] = 0.0; S[MS_DOTC] = 0.0; S[MS_TOLG] = 0.0;
  S[MS_TOL2] = atol2;
  S[MS_RR] = rho0;
  S[MS_BB] = bb;
  S[MS_FACTOR] = rtol2 * (rho0 > 0.0 ? bb / rho0 : 1.0);
  flags[1] = 0; flags[2] = 0; flags[3] = 0;
  const bool bad = !(rho0 == rho0);
  if (!(rho0 > atol2) || rho0 == 0.0) {          // nothing to iterate on (or NaN): every later launch returns at once
    flags[2] = bad ? 1 : 0;
    __threadfence();
    flags[0] = 1;
  } else {
    flags[0] = 0;
  }
}

static int solve_pcg_bpx_merged(femo_mat* A, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info) {
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  const int64_t n = m->n_rows;
  hipStream_t st = ctx->stream;
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev0, st));
  FEMO_TRY(femo_mat_ensure_s(A));
  CgWork w;
  const bool multi = ctx->nranks > 1;
  // k_cg_init writes every owned entry of r, p and x^; only the ghost tails have to be defined (zero) -- they and the ghost
  // tail of the solution are cleared by the preconditioner's own clearing launch (round 6; round 5: three memsets)
  FEMO_TRY(ensure_work(ctx, n, m->n_vert, w, 0, /*zero=*/false));
  // one rank without ghost entries: the directions are kept in a ring and x^ is formed from them (ensure_ring); direction k in
  // slot(k), alpha_k beside it
  int R = 0;
  if (!multi && m->n_vert <= n) FEMO_TRY(ensure_ring(ctx, n, &R));
  const int64_t stride = ring_stride(ctx);
  auto slot = [&](int k) -> double* { return ctx->cg_ring + (int64_t)(k % R) * stride; };
  int flushed = 0;                                               // directions below this one are in x^
  ctx->pcg_last_ring = R; ctx->pcg_last_flushes = 0;
  auto flush = [&](bool only_done, bool unscale) {
    ++ctx->pcg_last_flushes;
    hipLaunchKernelGGL(k_pcg_flush, dim3(2048), dim3(256), 0, ctx->stream, n, w.xh, (const double*)ctx->cg_ring, stride, R,
                       (const double*)ctx->cg_alpha_hist, flushed, (const int32_t*)ctx->d_flags, only_done ? 1 : 0, opts->zero_guess ? 0 : 1,
                       unscale ? (const double*)A->d_s : (const double*)nullptr, x->d);
  };
  const int gv = vec_grid(ctx, n);
  const int gs = femo_spmv_grid(m);
  int32_t* h_flags = FlagPoll::host_words(ctx);
  double* P = ctx->d_partials;
  double* S = ctx->d_scal;
  const uint8_t* mask = A->pc_has_mask ? A->d_pcmask : nullptr;
  FemoZeroExtra ze;
  ze.count = 0;
  if (m->n_vert > n) {
    const int64_t tail = ctx->cg_n - n;                          // (ensure_work: vectors of max(n_rows, n_vert) + 2 entries)
    ze.p[ze.count] = w.p + n; ze.n[ze.count++] = tail;
    ze.p[ze.count] = w.r + n; ze.n[ze.count++] = tail;
  }
  if (opts->zero_guess && x->n > n) { ze.p[ze.count] = x->d + n; ze.n[ze.count++] = x->n - n; }   // ghost tail of the solution, as the classic loop leaves it
  FEMO_TRY(femo_pc_merged_begin(m, A->d_s, mask, &ze, femo_pc_weights_key(A), &A->pc_wt));
  const double* q0;
  FEMO_TRY(initial_guess(A, A->d_vals, x, opts->zero_guess, /*clear_x=*/false, w.q, &q0));
  double* const p0 = R ? slot(0) : w.p;
  hipLaunchKernelGGL(k_cg_init, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, b->d, q0, A->d_s, w.r, p0, w.xh, P, A->has_idrows ? A->d_idrows : nullptr);
  const double atol2 = opts->atol * opts->atol;
  if (multi) {
    FEMO_TRY(femo_launch_fold(1024, gv, 2, P + FEMO_MAX_PARTIALS, S + MS_RED, st));
    FEMO_TRY(femo_coll_allreduce(ctx, S + MS_RED, 2, st));
    hipLaunchKernelGGL(k_pcg_setup, dim3(1), dim3(1024), 0, st, 0, P + FEMO_MAX_PARTIALS, S, opts->rtol * opts->rtol, atol2, ctx->d_flags);
  } else {
    hipLaunchKernelGGL(k_pcg_setup, dim3(1), dim3(1024), 0, st, gv, P + FEMO_MAX_PARTIALS, S, opts->rtol * opts->rtol, atol2, ctx->d_flags);
  }
  FemoPcgStop stop;
  stop.rtol2_factor = 0.0;                       // read from S[MS_FACTOR] on the device
  stop.atol_pc2 = opts->atol_pc * opts->atol_pc;
  stop.tolg2 = S + MS_TOLG;
  stop.flags = ctx->d_flags;
  stop.it = -1;
  FemoMergedVecs V;
  V.x = w.xh; V.r = w.r; V.p = p0; V.q = nullptr; V.n = n; V.cur = 0; V.gv = gv; V.atol2 = 0.0;
  V.nb_q[0] = V.nb_q[1] = 0; V.Pq[0] = V.Pq[1] = nullptr;
  FEMO_TRY(femo_pc_merged_apply(m, mask, A->pc_key, V, S, ctx->d_flags, &stop));
  FEMO_HIP_CHECK(hipGetLastError());
  // The one synchronisation before the loop: rho0, bb, gamma0 and the flag.  x of a solve that does not iterate (the
  // identity rows, solved by k_cg_init) is written speculatively in front of it -- 6 us that save such a solve (Newton's
  // later passes) a second stream drain; an iterating solve overwrites it at the end.
  const bool spec_x = n > 0 && opts->zero_guess;
  if (spec_x) hipLaunchKernelGGL(k_unscale_done, dim3(2048), dim3(256), 0, st, n, 0, A->d_s, w.xh, x->d, ctx->d_flags);   // (only if the flag says so: an iterating solve skips the 44 us at C4)
  FEMO_TRY(read_back(ctx, ctx->ev1));
  const double rho0 = ctx->h_scal[MS_RR], bb = ctx->h_scal[MS_BB], gamma0 = ctx->h_scal[MS_GAMMA];
  info->rhs_norm = std::sqrt(bb);
  const int max_it = opts->max_it > 0 ? opts->max_it : 10000;
  info->spmv_ms = 0.0; info->spmv_samples = 0;
  info->pc_rhs_norm = std::sqrt(gamma0 * (rho0 > 0.0 ? bb / rho0 : 1.0));
  if (h_flags[0]) {                               // below the absolute tolerance (k_pcg_setup) or below atol_pc (first apply)
    info->pc_residual_norm = std::sqrt(gamma0);
    if (!spec_x && n > 0) FEMO_TRY(unscale_x(A, w.xh, x, opts->zero_guess));
    femo_mat_compact_settle(A);
    return fill_info(ctx, ctx->ev1, info, 0, (h_flags[2] || !(rho0 == rho0)) ? -1 : 1, rho0);
  }
  FEMO_TRY(femo_mat_ensure_scaled(A, false));

  SpmvSamples spmv(ctx, 2);
  // Batches: with a prediction (the smaller of the last two counts on this mesh) exactly that many iterations first, then
  // 2, 3, 4, 6, 8, 8 ... -- each batch polled synchronously (a solve that follows a short one paid a
  // blocking poll every second iteration).  Without a prediction: 8 at a time.
  const int batch = opts->check_every > 0 ? std::min(opts->check_every, 8) : 8;
  // Round 5: the prediction follows the REDUCTION this solve needs, ln(gamma_0 / threshold), at the rate the last solve on
  // this mesh converged with (ln of its reduction per iteration).  The smaller of the last two counts mispredicted whenever a
  // short solve (Newton's second pass: one iteration) sat between two long ones: the long solve after it was polled after
  // 1, 3, 6, 10, 16 ... iterations, ~35 us of idle device per poll.
  int predicted = 0;
  {
    const double tolg = ctx->h_scal[MS_TOLG];
    if (m->pcg_rate > 0.0 && gamma0 > 0.0 && tolg > 0.0 && gamma0 > tolg) {
      const double need = std::log(gamma0 / tolg);
      predicted = (int)std::ceil(need / m->pcg_rate) + 1;
      predicted = std::max(1, std::min(predicted, 4 * std::max(m->pcg_last_iters, 8)));
    } else if (m->pcg_rate <= 0.0) {
      const int last2 = std::min(m->pcg_last_iters, m->pcg_prev_iters);
      predicted = last2 > 0 ? last2 : 0;
    }
  }
  int it = 0, grow = 2;
  bool done = false;
  const int64_t ar0 = ctx->n_allreduce;
  double* Pq_int = P + 4 * FEMO_MAX_PARTIALS;     // triples [p.q | q.q | r.q]: interior / only launch, boundary launch
  double* Pq_bnd = P + 7 * FEMO_MAX_PARTIALS;
  V.q = w.q; V.atol2 = atol2;
  // q = Ah p: N ranks with the triple the one all-reduce carries, the ghosts of p refreshed by whoever sends them (the
  // prolongation of the apply before, or the product itself); one rank with p.q alone
  const FemoSpmv Ap_multi = {.vals = A->d_valsS, .unit = true, .dots = FEMO_DOTS_TRIPLE, .partials = Pq_int, .dvec = w.r, .done = ctx->d_flags};
  const FemoSpmv Ap_one = {.vals = A->d_valsS, .unit = true, .dots = FEMO_DOTS_DAX, .partials = Pq_int, .done = ctx->d_flags};
  const bool inflight = multi && femo_pc_merged_sends_halo(m);
  while (!done) {
    int this_batch = batch;
    if (predicted > 0) {
      if (it == 0) this_batch = predicted;
      else { this_batch = grow; grow = std::min(8, grow + (grow + 1) / 2); }
    }
    const int it_end = it + this_batch < max_it ? it + this_batch : max_it;
    for (; it < it_end; ++it) {
      if (R) {
        // the ring is full: this iteration's prolongation writes the slot of direction `flushed` -- directions up to it - 1
        // (their alphas are known) go to x^ first
        if (it + 1 - flushed == R) { flush(false, false); flushed = it; }
        V.p = slot(it); V.p_next = slot(it + 1); V.alpha_out = ctx->cg_alpha_hist + it % R;
      }
      FEMO_TRY(spmv.begin(it));
      int g1 = gs, g2 = 0;
      if (multi) FEMO_TRY(femo_halo_spmv(A, w.p, w.q, Ap_multi, &g1, &g2, inflight));
      else FEMO_TRY(femo_launch_spmv(A, V.p, w.q, Ap_one));
      FEMO_TRY(spmv.end());
      stop.it = it;
      V.cur = it & 1;
      V.nb_q[0] = g1; V.nb_q[1] = g2; V.Pq[0] = Pq_int; V.Pq[1] = Pq_bnd;
      FEMO_TRY(femo_pc_merged_apply(m, mask, A->pc_key, V, S, ctx->d_flags, &stop));
    }
    FEMO_HIP_CHECK(hipGetLastError());
    // the poll carries everything the end of a converged solve needs: x (unscaled on the device only if the flag is set),
    // the flags and the scalars -- the batch that converges costs ONE host round trip, not two (round 6)
    // (kept directions: the same launch adds those not yet in x^ first -- like k_unscale_done, nothing unless the flag is set)
    if (R) flush(true, true);
    else if (n > 0) hipLaunchKernelGGL(k_unscale_done, dim3(2048), dim3(256), 0, st, n, opts->zero_guess ? 0 : 1, A->d_s, w.xh, x->d, ctx->d_flags);
    // a consumer of the device-initiated ghost refresh that gave up waiting (4 s) must not pass for a result: its flag
    // travels in the spare word of the poll
    if (femo_halo_direct_ready(m)) FEMO_HIP_CHECK(hipMemcpyAsync(ctx->d_flags + 3, m->hd->d_err, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    FEMO_TRY(read_back(ctx, ctx->ev_pool[POLL_EV]));
    FEMO_REQUIRE(!(femo_halo_direct_ready(m) && h_flags[3] != 0),
                 "ghost refresh: a consumer waited 4 s for a neighbour's stores and gave up (rank %d of %d) -- the solve is void", ctx->rank, ctx->nranks);
    if (h_flags[0] || it >= max_it) done = true;
  }
  info->loop_allreduces = (int32_t)(ctx->n_allreduce - ar0);
  const hipEvent_t end = h_flags[0] ? ctx->ev_pool[POLL_EV] : ctx->ev1;
  if (!h_flags[0]) {
    // not converged within max_it: x of the last iterate, the final scalars and the time with one more synchronisation
    if (R) flush(false, true);
    else if (n > 0) hipLaunchKernelGGL(k_unscale, dim3(2048), dim3(256), 0, st, n, opts->zero_guess ? 0 : 1, A->d_s, w.xh, x->d);
    FEMO_TRY(read_back(ctx, ctx->ev1));
  }
  const int iters = h_flags[1];
  const int conv = h_flags[0] ? (h_flags[2] ? -1 : 1) : 0;
  if (conv == 1 && iters > 0) { m->pcg_prev_iters = m->pcg_last_iters; m->pcg_last_iters = iters; }
  if (conv == 1 && iters >= 4) {
    const double g_end = ctx->h_scal[MS_GAMMA + (iters & 1)];
    if (g_end > 0.0 && gamma0 > g_end) m->pcg_rate = std::log(gamma0 / g_end) / iters;
  }
  FEMO_TRY(spmv.report(info));
  femo_mat_compact_settle(A);                    // (the last poll waited for everything this solve enqueued)
  info->pc_residual_norm = std::sqrt(ctx->h_scal[MS_GAMMA + (iters & 1)]);
  return fill_info(ctx, end, info, iters, conv, ctx->h_scal[MS_RR]);
}

// CG with the auxiliary-lattice BPX preconditioner.  Same scaled system, same stopping norm
// (sqrt(rh.rh) = sqrt(r^T D^-1 r)) as the Jacobi path; scalars live on the device and are
// all-reduced there when the mesh is partitioned.
static int solve_pcg_bpx(femo_mat* A, int transpose, const femo_vec* b, femo_vec* x,
                         const femo_solver_opts* opts, femo_solve_info* info) {
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  const int64_t n = m->n_rows;
  FEMO_REQUIRE(A->bpx_ok, "the BPX preconditioner needs an operator assembled from a Poisson-type form");
  FEMO_REQUIRE(!transpose, "the BPX preconditioner is for symmetric operators");
  hipStream_t st = ctx->stream;
  // (not multi_path: FEMO_FORCE_MULTI on one rank keeps the classic loop, whose all-reduce path it tests)
  if (!(ctx->comm != nullptr && ctx->nranks == 1 && femo_env_flag("FEMO_FORCE_MULTI")) && femo_pc_merged_ok(m))
    return solve_pcg_bpx_merged(A, b, x, opts, info);
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev0, st));
  FEMO_TRY(femo_mat_ensure_s(A));
  FEMO_TRY(femo_pc_build(m));
  CgWork w;
  const bool multi = multi_path(ctx);
  FEMO_TRY(ensure_work(ctx, n, m->n_vert, w, 1));
  const int gv = vec_grid(ctx, n);
  const int gs = femo_spmv_grid(m);
  FlagPoll poll(ctx);
  int32_t* h_flags = poll.h_flags;
  double* P = ctx->d_partials;
  double* S = ctx->d_scal;
  const uint8_t* mask = A->pc_has_mask ? A->d_pcmask : nullptr;
  FEMO_TRY(femo_pc_begin(m, A->d_s, mask, femo_pc_weights_key(A), &A->pc_wt));
  auto allreduce1 = [&](double* d) -> int {
    if (multi) FEMO_TRY(femo_coll_allreduce(ctx, d, 1, st));
    return 0;
  };

  FEMO_HIP_CHECK(hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int32_t), st));
  const double* q0;
  FEMO_TRY(initial_guess(A, A->d_vals, x, opts->zero_guess, /*clear_x=*/true, w.q, &q0));
  hipLaunchKernelGGL(k_cg_init, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, b->d, q0, A->d_s, w.r, w.p, w.xh, P, A->has_idrows ? A->d_idrows : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  double rho0, bb;
  FEMO_TRY(initial_norms(ctx, multi, gv, P + FEMO_MAX_PARTIALS, S, &rho0, &bb));
  // Stopping rule: relative in the norm of the preconditioner, sqrt(r^T M^-1 r) <= rtol sqrt(b^T M^-1 b)
  // (tested inside femo_pc_apply, where gamma = r^T M^-1 r becomes known), absolute in the Jacobi norm,
  // sqrt(r^T D^-1 r) <= atol (Newton's rounding-floor rule is stated in that norm; tested by k_pcg_check).
  const double bnorm = std::sqrt(bb);
  const double tol = opts->atol;
  info->rhs_norm = bnorm;
  const int max_it = opts->max_it > 0 ? opts->max_it : 10000;
  if (!(std::sqrt(rho0) > tol) || rho0 == 0.0) return finish_solve(A, w.xh, x, opts->zero_guess, info, 0, rho0 == rho0 ? 1 : -1, rho0);

  double hs[FEMO_NSCAL] = {0};
  hs[S_TOL2] = tol * tol;
  hs[S_RHO] = rho0;
  memcpy(ctx->h_scal, hs, sizeof hs);
  FEMO_HIP_CHECK(hipMemcpyAsync(S, ctx->h_scal, sizeof hs, hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  // ph0 = zh0 = M^-1 rh0, gamma0 = rh0.zh0 = rho0 + g_L.e_L (lattice dot: global on every rank, no all-reduce);
  // the same launch stores the threshold max(rtol^2 gamma_0 bb/rho0, atol_pc^2) (relative to the right-hand
  // side, not to r0) and tests gamma_0 against it
  FemoPcgStop stop;
  stop.rtol2_factor = opts->rtol * opts->rtol * (rho0 > 0.0 ? bb / rho0 : 1.0);
  stop.atol_pc2 = opts->atol_pc * opts->atol_pc;
  stop.tolg2 = S + S_TOLG;
  stop.flags = ctx->d_flags;
  stop.it = -1;
  FemoPcApply pc = {.rh = w.r, .out = w.p, .mode = 2, .rho = S + S_RHO, .gamma_cur = S + S_GAMMA + 1, .gamma_nxt = S + S_GAMMA,
                    .done = ctx->d_flags, .gv = gv, .stop = &stop};
  FEMO_TRY(femo_pc_apply(m, mask, A->pc_key, pc));
  pc.mode = 1;                                  // from here on: the next direction, zh + beta ph
  FEMO_TRY(read_back(ctx, nullptr));
  const double gamma0 = ctx->h_scal[S_GAMMA];
  info->pc_rhs_norm = std::sqrt(gamma0 * (rho0 > 0.0 ? bb / rho0 : 1.0));
  info->pc_residual_norm = std::sqrt(gamma0);
  if (h_flags[0]) return finish_solve(A, w.xh, x, opts->zero_guess, info, 0, gamma0 == gamma0 ? 1 : -1, rho0);   // below atol_pc before the first iteration
  FEMO_TRY(femo_mat_ensure_scaled(A, false));   // the iteration's operator S A S (the apply above only needed S)

  SpmvSamples spmv(ctx, 2);
  const bool local_scalars = !multi && m->n_nbr == 0;
  const bool piggyback = multi && femo_pc_can_piggyback(m);
  // x += alpha p inside the preconditioner's single-workgroup launch (the first apply, above, has settled whether the
  // fused lattice cycle runs on this mesh)
  const bool carry_x = local_scalars && femo_pc_carries_xupdate(m);
  const bool use_atol = opts->atol > 0.0;
  // Iterations are enqueued in batches and the host polls the "done" stamp; launches behind the converged iteration
  // return at once but still cost ~5 us each (6 per iteration).  Round 1: fixed batches of 8, polled two deep -- a
  // solve that converges at iteration 28 enqueued 40 (12 dead iterations).  Round 2: first batch = the count of
  // earlier solves on this mesh + 1, then batches of 3, still two deep: 4 dead iterations per solve (12 % of the
  // SpMV launches in the kernel trace were early exits).  Round 3: with a prediction the first batch is exactly the
  // earlier count (BPX counts repeat from solve to solve: 28, 28, 28 ...) and the host waits for its stamp before it
  // enqueues anything else; beyond the prediction two iterations at a time (a host round trip of ~30 us per pair,
  // at most one dead iteration).  Without a prediction: batches of 8, two deep, as before.
  const int batch = opts->check_every > 0 ? std::min(opts->check_every, 8) : 8;
  double* r_cur = w.r;
  // (the smaller of the last two counts: Newton's later solves need far fewer iterations than its first)
  const int last2 = std::min(m->pcg_last_iters, m->pcg_prev_iters);
  const int predicted = last2 > 0 ? last2 : 0;
  int it = 0;
  bool done = false;
  const int64_t ar0 = ctx->n_allreduce;
  const FemoSpmv Ap = {.vals = A->d_valsS, .unit = true, .dots = FEMO_DOTS_DAX, .partials = P + P_DELTA * FEMO_MAX_PARTIALS, .done = ctx->d_flags};
  while (!done) {
    const int this_batch = predicted > 0 ? (it == 0 ? predicted : 2) : batch;
    const int it_end = it + this_batch < max_it ? it + this_batch : max_it;
    for (; it < it_end; ++it) {
      const int cur = it & 1, nxt = cur ^ 1;
      FEMO_TRY(spmv.begin(it));
      int g1 = gs, g2 = 0;
      FEMO_TRY(femo_halo_spmv(A, w.p, w.q, Ap, &g1, &g2));
      FEMO_TRY(spmv.end());
      double* Pd = P + P_DELTA * FEMO_MAX_PARTIALS;
      double* Pr = P + 1 * FEMO_MAX_PARTIALS;
      double* Pg = P + 2 * FEMO_MAX_PARTIALS;   // boundary-slice partials of the overlapped SpMV
      stop.it = it;
      FemoPcApply a = pc;                         // this iteration's apply: the branches below add what differs
      a.gamma_cur = S + S_GAMMA + cur; a.gamma_nxt = S + S_GAMMA + nxt;
      if (local_scalars) {
        // single GPU: the consumers fold the per-block partials themselves
        // ph = M^-1 rh + beta ph in one pass: rh.zh = rho + g_L.e_L is known before the mesh prolongation, and
        // with it the stopping test.  The Jacobi-norm test runs only when an absolute tolerance is set.
        if (use_atol) {
          hipLaunchKernelGGL(k_pcg_xr, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, cur, g1, Pd, S, w.q, w.p, (const double*)r_cur, r_cur, w.xh, Pr, ctx->d_flags);
          hipLaunchKernelGGL(k_pcg_check, dim3(1), dim3(1024), 0, st, it, gv, Pr, S, ctx->d_flags);
          FEMO_TRY(femo_pc_apply(m, mask, A->pc_key, a));
        } else if (carry_x) {
          hipLaunchKernelGGL(k_pcg_xr, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, cur, g1, Pd, S, w.q, w.p, (const double*)r_cur, r_cur, w.xh, Pr, ctx->d_flags, 1);
          const FemoXUpdate xu = {w.xh, w.p, S + S_ALPHA, n};
          a.nb_rho = gv; a.rho_partials = Pr; a.xupdate = &xu;
          FEMO_TRY(femo_pc_apply(m, mask, A->pc_key, a));
        } else {
          hipLaunchKernelGGL(k_pcg_xr, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, cur, g1, Pd, S, w.q, w.p, (const double*)r_cur, r_cur, w.xh, Pr, ctx->d_flags);
          a.nb_rho = gv; a.rho_partials = Pr;
          FEMO_TRY(femo_pc_apply(m, mask, A->pc_key, a));
        }
      } else {
        FEMO_TRY(femo_launch_fold(1024, g1, 1, Pd, S + S_DELTA, st, ctx->d_flags, g2, Pg));
        FEMO_TRY(allreduce1(S + S_DELTA));
        hipLaunchKernelGGL(k_pcg_xr, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, cur, 0, Pd, S, w.q, w.p, (const double*)w.r, w.r, w.xh, Pr, ctx->d_flags);
        FEMO_TRY(femo_launch_fold(1024, gv, 1, Pr, S + S_RHO, st, ctx->d_flags));
        if (piggyback) {
          // the rank's part of rh.rh rides in the lattice all-reduce of the preconditioner; the stopping
          // test then runs after the apply (one wasted apply in the last iteration, one collective less in all)
          a.rho_is_partial = true;
          FEMO_TRY(femo_pc_apply(m, mask, A->pc_key, a));
          if (use_atol) hipLaunchKernelGGL(k_pcg_check, dim3(1), dim3(1024), 0, st, it, 0, Pr, S, ctx->d_flags);
        } else {
          FEMO_TRY(allreduce1(S + S_RHO));
          if (use_atol) hipLaunchKernelGGL(k_pcg_check, dim3(1), dim3(1024), 0, st, it, 0, Pr, S, ctx->d_flags);
          FEMO_TRY(femo_pc_apply(m, mask, A->pc_key, a));
        }
      }
    }
    FEMO_HIP_CHECK(hipGetLastError());
    FEMO_TRY(poll.after_batch(it >= max_it, /*sync=*/predicted > 0, &done));   // with a prediction: the batch just enqueued
  }
  info->loop_allreduces = (int32_t)(ctx->n_allreduce - ar0);
  FEMO_TRY(read_back(ctx, nullptr));
  const int iters = h_flags[1];
  const int conv = h_flags[0] ? (h_flags[2] ? -1 : 1) : 0;
  if (conv == 1 && iters > 0) { m->pcg_prev_iters = m->pcg_last_iters; m->pcg_last_iters = iters; }
  FEMO_TRY(spmv.report(info));
  info->pc_residual_norm = std::sqrt(ctx->h_scal[S_GAMMA + (iters & 1)]);
  return finish_solve(A, w.xh, x, opts->zero_guess, info, iters, conv, ctx->h_scal[S_RHO]);
}

// z = M^-1 r with the BPX preconditioner of A, in unscaled variables:
//   M^-1 = D^-1 + theta sum_l P_l C_l P_l^T   (oracle/bpx_oracle.py restates it; tests compare)
extern "C" int femo_mat_pc_apply(const femo_mat* A_, const femo_vec* r, femo_vec* z) {
  FEMO_REQUIRE(A_ && r && z, "null argument");
  femo_mat* A = const_cast<femo_mat*>(A_);
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  const int64_t n = m->n_rows;
  FEMO_REQUIRE(A->bpx_ok, "the BPX preconditioner needs an operator assembled from a Poisson-type form");
  FEMO_REQUIRE(r->n >= n && z->n >= n && r->d != z->d, "vector size mismatch in pc_apply");
  femo_vec_touch(z);
  hipStream_t st = ctx->stream;
  FEMO_TRY(femo_mat_ensure_s(A));
  FEMO_TRY(femo_pc_build(m));
  CgWork w;
  FEMO_TRY(ensure_work(ctx, n, m->n_vert, w, 1));
  const uint8_t* mask = A->pc_has_mask ? A->d_pcmask : nullptr;
  FEMO_TRY(femo_pc_begin(m, A->d_s, mask, femo_pc_weights_key(A), &A->pc_wt));
  const int gv = vec_grid(ctx, n);
  FEMO_HIP_CHECK(hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int32_t), st));
  if (n == 0) return 0;
  // rh = S r, zh = Mh^-1 rh, z = S zh
  hipLaunchKernelGGL(k_cg_init, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, r->d, (const double*)nullptr, A->d_s, w.r, w.p, w.xh, ctx->d_partials, (const uint8_t*)nullptr);
  FEMO_TRY(femo_pc_apply(m, mask, A->pc_key, FemoPcApply{.rh = w.r, .out = w.sv, .done = ctx->d_flags, .gv = gv}));
  hipLaunchKernelGGL(k_unscale, dim3(2048), dim3(256), 0, st, n, 0, A->d_s, w.sv, z->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int femo_solve_cg(const femo_mat* A_, int transpose, const femo_vec* b, femo_vec* x,
                             const femo_solver_opts* opts, femo_solve_info* info) {
  FEMO_REQUIRE(A_ && b && x && opts && info, "null argument");
  femo_mat* A = const_cast<femo_mat*>(A_);
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  const int64_t n = m->n_rows;
  FEMO_REQUIRE(b->n >= n && x->n >= m->n_vert, "vector size mismatch in solve_cg");
  FEMO_REQUIRE(b->d != x->d, "solve_cg cannot run in place");
  femo_vec_touch(x);
  memset(info, 0, sizeof *info);
  FEMO_REQUIRE(opts->pc == FEMO_PC_JACOBI || opts->pc == FEMO_PC_BPX, "unknown preconditioner %d", opts->pc);
  if (opts->pc == FEMO_PC_BPX) return solve_pcg_bpx(A, transpose, b, x, opts, info);
  hipStream_t st = ctx->stream;
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev0, st));
  FEMO_TRY(femo_mat_ensure_s(A));
  if (transpose && !opts->zero_guess) FEMO_TRY(femo_mat_ensure_transpose(A));
  CgWork w;
  const bool multi = multi_path(ctx);
  FEMO_TRY(ensure_work(ctx, n, m->n_vert, w, multi ? 1 : 0));
  const int gv = vec_grid(ctx, n);
  const int gs = femo_spmv_grid(m);
  FlagPoll poll(ctx);
  double* P = ctx->d_partials;

  FEMO_HIP_CHECK(hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int32_t), st));
  // r0 = b - A x0 with the unscaled operator; the iteration then solves for the correction
  const double* q0;
  FEMO_TRY(initial_guess(A, transpose ? A->d_valsT : A->d_vals, x, opts->zero_guess, /*clear_x=*/true, w.q, &q0));
  hipLaunchKernelGGL(k_cg_init, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, b->d, q0, A->d_s, w.r, w.p, w.xh, P, A->has_idrows ? A->d_idrows : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  // gamma0 and ||S b||^2: partial slots 1 and 2
  double gamma0, bb;
  FEMO_TRY(initial_norms(ctx, multi, gv, P + FEMO_MAX_PARTIALS, ctx->d_scal, &gamma0, &bb));
  const double bnorm = std::sqrt(bb);
  double tol = opts->rtol * bnorm;
  if (opts->atol > tol) tol = opts->atol;
  info->rhs_norm = bnorm;
  const int max_it = opts->max_it > 0 ? opts->max_it : 10000;
  if (!(std::sqrt(gamma0) > tol))   // converged at once, or NaN (reported as breakdown)
    return finish_solve(A, w.xh, x, opts->zero_guess, info, 0, gamma0 == gamma0 ? 1 : -1, gamma0);
  FEMO_TRY(femo_mat_ensure_scaled(A, transpose != 0));

  double hs[FEMO_NSCAL] = {0};
  if (multi) hs[M_TOL2] = tol * tol;
  else { hs[S_GAMMA + 0] = gamma0; hs[S_TOL2] = tol * tol; }
  memcpy(ctx->h_scal, hs, sizeof hs);
  FEMO_HIP_CHECK(hipMemcpyAsync(ctx->d_scal, ctx->h_scal, sizeof hs, hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));  // h_scal is reused below

  SpmvSamples spmv(ctx, 4);
  const FemoSpmv Ap = {.vals = A->d_valsS, .unit = true, .dots = FEMO_DOTS_DAX, .partials = P + P_DELTA * FEMO_MAX_PARTIALS, .done = ctx->d_flags};
  const FemoSpmv Ar = {.vals = A->d_valsS, .unit = true, .dots = FEMO_DOTS_DAX_XX, .partials = P, .done = ctx->d_flags};
  // w = Ah r with both dots, folded and all-reduced into the (delta, gamma) pair of `parity` (it < 0: not sampled)
  auto merged_spmv = [&](int parity, int it) -> int {
    int g1 = gs, g2 = 0;
    FEMO_TRY(spmv.begin(it));
    FEMO_TRY(femo_halo_spmv(A, w.r, w.q, Ar, &g1, &g2));
    FEMO_TRY(spmv.end());
    FEMO_TRY(femo_launch_fold(1024, g1, 2, P, ctx->d_scal + 2 * parity, st, ctx->d_flags, g2, P + 2 * FEMO_MAX_PARTIALS));
    FEMO_TRY(femo_coll_allreduce(ctx, ctx->d_scal + 2 * parity, 2, st));
    return 0;
  };
  if (multi) FEMO_TRY(merged_spmv(0, -1));

  const int batch = opts->check_every > 0 ? opts->check_every : 32;
  int it = 0;
  bool done = false;
  while (!done) {
    const int it_end = it + batch < max_it ? it + batch : max_it;
    for (; it < it_end; ++it) {
      const int cur = it & 1, nxt = cur ^ 1;
      if (multi) {
        // single-reduction CG: update from the reduced (delta, gamma) of parity cur, then the next SpMV
        hipLaunchKernelGGL(k_cgm_update, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, it, ctx->d_scal, w.q, w.r, w.p, w.sv, w.xh, ctx->d_flags);
        FEMO_TRY(merged_spmv(nxt, it));
      } else {
        FEMO_TRY(spmv.begin(it));
        FEMO_TRY(femo_launch_spmv(A, w.p, w.q, Ap));
        FEMO_TRY(spmv.end());
        hipLaunchKernelGGL(k_cg_update_r, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, cur, gs, gv, P, ctx->d_scal, w.q, w.r, ctx->d_flags);
        hipLaunchKernelGGL(k_cg_update_xp, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, cur, it, gs, gv, P, ctx->d_scal, w.r, w.p, w.xh, ctx->d_flags);
      }
    }
    FEMO_HIP_CHECK(hipGetLastError());
    FEMO_TRY(poll.after_batch(it >= max_it, /*sync=*/false, &done));
  }
  // final scalars: gamma of the last completed iteration sits in the (iters & 1) slot
  int32_t* h_flags = poll.h_flags;
  FEMO_HIP_CHECK(hipMemcpyAsync(h_flags, ctx->d_flags, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  const int iters = h_flags[1];
  const int conv = h_flags[0] ? (h_flags[2] ? -1 : 1) : 0;
  double gamma_f = 0.0;
  if (multi) {
    FEMO_HIP_CHECK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal, FEMO_NSCAL * sizeof(double), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    gamma_f = ctx->h_scal[2 * (iters & 1) + 1];
  } else {
    FEMO_TRY(femo_launch_fold(1024, gv, 1, P + (P_GAMMA + (iters & 1)) * FEMO_MAX_PARTIALS, ctx->d_scal + 8, st));
    FEMO_HIP_CHECK(hipMemcpyAsync(ctx->h_scal, ctx->d_scal + 8, sizeof(double), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    gamma_f = ctx->h_scal[0];
  }
  FEMO_TRY(spmv.report(info));
  return finish_solve(A, w.xh, x, opts->zero_guess, info, iters, conv, gamma_f);
}


// ------------------------------------------------------------- BiCGSTAB ------
extern "C" int femo_solve_bicgstab(const femo_mat* A_, int transpose, const femo_vec* b, femo_vec* x,
                                   const femo_solver_opts* opts, femo_solve_info* info) {
  FEMO_REQUIRE(A_ && b && x && opts && info, "null argument");
  femo_mat* A = const_cast<femo_mat*>(A_);
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  const int64_t n = m->n_rows;
  FEMO_REQUIRE(b->n >= n && x->n >= m->n_vert, "vector size mismatch in solve_bicgstab");
  FEMO_REQUIRE(b->d != x->d, "solve_bicgstab cannot run in place");
  femo_vec_touch(x);
  memset(info, 0, sizeof *info);
  hipStream_t st = ctx->stream;
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev0, st));
  // transposed operator of a partitioned mesh: applied by scatter + reverse halo add from the untransposed values
  const bool scatter_T = transpose != 0 && !femo_transpose_is_local(m);
  FEMO_TRY(femo_mat_ensure_scaled(A, transpose != 0 && !scatter_T));
  CgWork w;
  FEMO_TRY(ensure_work(ctx, n, m->n_vert, w, 2));
  const bool multi = multi_path(ctx);
  const int gv = vec_grid(ctx, n);
  const int gs = femo_spmv_grid(m);
  double* P = ctx->d_partials;
  double* S = ctx->d_scal;
  int32_t* h_flags = FlagPoll::host_words(ctx);
  FEMO_HIP_CHECK(hipMemsetAsync(ctx->d_flags, 0, 4 * sizeof(int32_t), st));
  FEMO_HIP_CHECK(hipMemsetAsync(w.sv, 0, ctx->cg_n * sizeof(double), st));   // sv, p: gathered incl. ghosts
  const double* q0;
  if (scatter_T && !opts->zero_guess) {
    FEMO_TRY(femo_spmv_transposed_scatter(A, A->d_vals, false, x->d, w.q, nullptr));
    q0 = w.q;
  } else {
    FEMO_TRY(initial_guess(A, transpose ? A->d_valsT : A->d_vals, x, opts->zero_guess, /*clear_x=*/true, w.q, &q0));
  }
  hipLaunchKernelGGL(k_bi_init, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, b->d, q0, A->d_s, w.r, w.r0, w.p, w.q, w.xh, P);
  FEMO_HIP_CHECK(hipGetLastError());
  double rr0, bb;
  FEMO_TRY(initial_norms(ctx, multi, gv, P, S + 12, &rr0, &bb));
  const double bnorm = std::sqrt(bb);
  double tol = opts->rtol * bnorm;
  if (opts->atol > tol) tol = opts->atol;
  info->rhs_norm = bnorm;
  const int max_it = opts->max_it > 0 ? opts->max_it : 10000;
  if (!(std::sqrt(rr0) > tol)) return finish_solve(A, w.xh, x, opts->zero_guess, info, 0, rr0 == rr0 ? 1 : -1, rr0);
  double hs[FEMO_NSCAL] = {0};
  hs[B_RHO] = rr0; hs[B_RHO_OLD] = 1.0; hs[B_ALPHA] = 1.0; hs[B_OMEGA] = 1.0; hs[B_RR] = rr0; hs[B_TOL2] = tol * tol;
  memcpy(ctx->h_scal, hs, sizeof hs);
  FEMO_HIP_CHECK(hipMemcpyAsync(S, ctx->h_scal, sizeof hs, hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));

  const int batch = opts->check_every > 0 ? opts->check_every : 32;
  int it = 0;
  bool done = false;
  const FemoSpmv Ap = {.vals = A->d_valsS, .unit = true, .dots = FEMO_DOTS_DAX, .partials = P, .dvec = w.r0, .done = ctx->d_flags};
  const FemoSpmv As = {.vals = A->d_valsS, .unit = true, .dots = FEMO_DOTS_DAX_AXAX, .partials = P, .done = ctx->d_flags};
  while (!done) {
    const int it_end = it + batch < max_it ? it + batch : max_it;
    for (; it < it_end; ++it) {
      hipLaunchKernelGGL(k_bi_check, dim3(1), dim3(1), 0, st, it, S, ctx->d_flags);
      hipLaunchKernelGGL(k_bi_p, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, it, S, w.r, w.q, w.p, ctx->d_flags);
      if (scatter_T) {
        FEMO_TRY(femo_spmv_transposed_scatter(A, A->d_valsS, true, w.p, w.q, ctx->d_flags));                       // v
        hipLaunchKernelGGL(k_dot, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, w.r0, w.q, P);                            // (r0, v)
      } else {
        if (m->n_nbr > 0) FEMO_TRY(femo_halo_raw(m, w.p, st));
        FEMO_TRY(femo_launch_spmv(A, w.p, w.q, Ap));   // v, (r0, v)
      }
      FEMO_TRY(femo_launch_fold(1024, scatter_T ? gv : gs, 1, P, S + B_R0V, st, ctx->d_flags));
      if (multi) FEMO_TRY(femo_coll_allreduce(ctx, S + B_R0V, 1, st));
      hipLaunchKernelGGL(k_bi_s, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, S, w.r, w.q, w.sv, ctx->d_flags);
      if (scatter_T) {
        FEMO_TRY(femo_spmv_transposed_scatter(A, A->d_valsS, true, w.sv, w.t, ctx->d_flags));                      // t
        hipLaunchKernelGGL(k_dot, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, w.sv, w.t, P);                            // (s, t)
        hipLaunchKernelGGL(k_dot, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, w.t, w.t, P + FEMO_MAX_PARTIALS);         // (t, t)
      } else {
        if (m->n_nbr > 0) FEMO_TRY(femo_halo_raw(m, w.sv, st));
        FEMO_TRY(femo_launch_spmv(A, w.sv, w.t, As));  // t, (s,t), (t,t)
      }
      FEMO_TRY(femo_launch_fold(1024, scatter_T ? gv : gs, 2, P, S + B_TS, st, ctx->d_flags));
      if (multi) FEMO_TRY(femo_coll_allreduce(ctx, S + B_TS, 2, st));
      hipLaunchKernelGGL(k_bi_xr, dim3(gv), dim3(FEMO_BLOCK), 0, st, n, it, S, w.p, w.sv, w.t, w.r0, w.xh, w.r, P, ctx->d_flags);
      FEMO_TRY(femo_launch_fold(1024, gv, 2, P, S + 12, st, ctx->d_flags));
      if (multi) FEMO_TRY(femo_coll_allreduce(ctx, S + 12, 2, st));
      hipLaunchKernelGGL(k_bi_set_rho, dim3(1), dim3(1), 0, st, S + 12, S, ctx->d_flags);
    }
    hipLaunchKernelGGL(k_bi_check, dim3(1), dim3(1), 0, st, it, S, ctx->d_flags);
    FEMO_HIP_CHECK(hipGetLastError());
    FEMO_HIP_CHECK(hipMemcpyAsync(h_flags, ctx->d_flags, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    if (h_flags[0] || it >= max_it) done = true;
  }
  FEMO_HIP_CHECK(hipMemcpyAsync(ctx->h_scal, S, FEMO_NSCAL * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  const int conv = h_flags[0] ? (h_flags[2] ? -1 : 1) : 0;
  const int iters = h_flags[0] ? h_flags[1] : it;
  return finish_solve(A, w.xh, x, opts->zero_guess, info, iters, conv, ctx->h_scal[B_RR]);
}
