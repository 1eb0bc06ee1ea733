// SIMP topology optimisation: harmonic response of the linear elasticity, (K(rho) - omega^2 M(rho)) u = F, undamped and in
// real arithmetic (C-ABI in include/femo_hip.h: femo_elast_mass_assemble, femo_elast_dyn_apply_multi,
// femo_elast_dyn_solve_multi, femo_elast_mass_drho_multi).
//
//   M(rho) = rho0 sum_e m(rho_e) M0_e,   M0_e[(a,i),(b,j)] = delta_ij |T_e| (1 + delta_ab) / ((d+1)(d+2))   (consistent P1)
//
// M is a SCALAR matrix on the mesh's SELL pattern times I_d: one double per pattern entry (mvals, in the slots K uses) and one
// per row (mdiag), against d^2 doubles per entry of K.  It is assembled vertex-centric like K (k_elast_assemble): one writer
// per entry, the cells around a vertex in ascending order, the cell weight formed from `conn` in its own vertex order, so
// entry (v, w) and entry (w, v) are sums of the same numbers in the same order -- M is symmetric bit for bit.
//
// Layout as in elast_solve.hip: column l at l * n_dof, 1 <= L <= FEMO_ELAST_MAX_COLS.  Column l carries its own shift
// sigma_l = omega_l^2 >= 0; the shifts travel by value as a struct of FEMO_ELAST_MAX_COLS doubles.
//
// The product k_elast_dyn_spmv_multi is k_elast_spmv_multi with a second accumulator per column and component for M x: the
// block, its column index, the fixed bytes AND the mass scalar of an entry are read once for the columns of a chunk, and
// y_l = a (K x_l - sigma_l M x_l) + b f_l.  With sigma_l = 0 it gives the bits of k_elast_spmv_multi.  It keeps a row walk of
// its own, in the order of elast_row_walk (elast_internal.h) with MASS: through the shared walk the MINRES iteration at four
// columns measured 1 to 2 % slower (70.2 to 71.2 against 69.8 us, DESIGN_LOG.md R24).
//
// The solve is Paige & Saunders' MINRES with the SPD preconditioners of the static solve (block-Jacobi or multilevel, both
// built from the masked, UNSHIFTED K): above the first resonance K - sigma M is indefinite, where PCG breaks down.  One
// iteration issues these launches, each with a column dimension in its grid:
//
//   q_l = S_l v_l, partial v_l.q_l          k_elast_dyn_spmv_multi
//   alfa_l                                  k_minres_scalar (mode 1)    one workgroup per column
//   r' = q - (alfa/beta) r2 - (beta/oldb) r1, r1 <- r2, r2 <- r', z = M^-1 r2, partial r2.z
//                                           k_minres_lanczos (block-Jacobi in the same launch), or k_minres_lanczos and
//                                           the four launches of femo_elast_pc_step(update = false)
//   beta_l, the Givens rotation, phi, phibar, convergence of column l
//                                           k_minres_scalar (mode 2)
//   w = (v - oldeps w1 - delta w2) / gamma, x += phi w, v = z / beta
//                                           k_minres_x
//
// Column l owns its MINRES scalars at ms + l * MS_STRIDE (EMS_STRIDE is too small for them), the flags of the PCG loop at
// flag + l * EMF_STRIDE (0 done, 1 iterations, 2 non-finite, 3 converged) and its own slab of partials.  A column whose flag[0]
// is set is frozen: every block of it returns early, and its x is never written again.  The x update of an iteration depends
// on the rotation of the same iteration, so k_minres_x runs for the columns whose iteration count equals the iteration being
// issued -- the column that has just finished included -- and for no other.  Both dots are per-block partials folded in a
// fixed order: no float atomics, and a column has the same bits whatever L is.
//
// It stops on phibar <= max(rtol beta1, atol), beta1 = sqrt(b . M^-1 b) of the first residual: phibar is the recurrence's
// estimate of the preconditioned residual norm sqrt(r . M^-1 r), the norm the PCG tests.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

// MINRES device scalars of a column
enum { MS_BETA1 = 0, MS_BETA, MS_OLDB, MS_ALFA, MS_DBAR, MS_EPSLN, MS_OLDEPS, MS_DELTA, MS_GAMMA, MS_CS, MS_SN, MS_PHI,
       MS_PHIBAR, MS_TOL };
constexpr int MS_STRIDE = FEMO_ELAST_HARM_SCALARS;

// ---------------------------------------------------------------------------------------------- mass assembly ----
// One thread per vertex row on the shared visit walk (elast_visits), as k_elast_assemble.  A visit of cell c as its vertex a adds
// w_c = rho0 m(rho_c) |T_c| / ((d+1)(d+2)) to the entries (a, b), b != a, and 2 w_c to the diagonal.
template <int D>
__global__ __launch_bounds__(EB) void k_elast_mass_assemble(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell,
    const uint32_t* __restrict__ visit_slots, const int64_t* __restrict__ mptr, const int32_t* __restrict__ rowlen,
    const int32_t* __restrict__ conn, const double* __restrict__ x, const double* __restrict__ rho, int law, double rho0,
    double* __restrict__ mvals, double* __restrict__ mdiag) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t slice = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t mb = mptr[slice];
  const int len = rowlen[row];
  for (int k = 0; k < len; ++k) mvals[femo_sell_index(mb, k, lane)] = 0.0;
  double dg = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    const uint32_t sl = visit_slots[t.vi];
    const double w = mass_weight<D>(rho0 * mass_law(law, rho[t.c]), elast_cell_volume<D>(conn, x, t.c).vol);
#pragma unroll
    for (int b = 0; b <= D; ++b) {
      if (b == t.a) dg += w + w;
      else mvals[femo_sell_index(mb, slot_pos(sl, t.a, b), lane)] += w;
    }
  }
  mdiag[row] = dg;
}

// ------------------------------------------------------------------------------------------- shifted product ----
// y_l = a (K - sg_l M) x_l + b f_l (+ partial dot(x_l, y_l) per block and column when part != null) for the columns
// c0 = MC * blockIdx.y ... min(c0 + MC, n_cols) - 1: k_elast_spmv_multi with the mass scalar of every entry and a second
// accumulator.  MASKED: identity rows / columns on fixed dofs, as for the masked A.  done != null: a column whose
// done[l * EMF_STRIDE] is set is skipped.  vs: column stride of the vectors, ps: of the partials.
template <int D, bool MASKED, int MC>
__global__ __launch_bounds__(EB) void k_elast_dyn_spmv_multi(
    int64_t n_rows, const int64_t* __restrict__ mptr, const int32_t* __restrict__ cols, const int32_t* __restrict__ rowlen,
    const double* __restrict__ vals, const double* __restrict__ diag, const double* __restrict__ mvals,
    const double* __restrict__ mdiag, const uint8_t* __restrict__ fixed, int n_cols, int64_t vs, ColScalars sig, double a,
    const double* __restrict__ x, double b, const double* __restrict__ f, double* __restrict__ y, double* __restrict__ part,
    int64_t ps, const int32_t* __restrict__ done) {
  constexpr int DD = D * D;
  __shared__ double lds[EB / 64];
  const int c0 = (int)blockIdx.y * MC;
  bool on[MC];          // uniform over the block
  double sg[MC];
  bool any = false;
#pragma unroll
  for (int c = 0; c < MC; ++c) {
    on[c] = c0 + c < n_cols && !(done && done[(c0 + c) * EMF_STRIDE]);
    sg[c] = c0 + c < n_cols ? sig.v[c0 + c] : 0.0;
    any = any || on[c];
  }
  if (!any) return;
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  double dotv[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) dotv[c] = 0.0;
  if (row < n_rows) {
    const int64_t slice = row >> 6;
    const int lane = (int)(row & 63);
    const int64_t mb = mptr[slice];
    const int len = rowlen[row];
    double acc[MC][D], accm[MC][D], xo[MC][D];
    uint8_t fo[D];
#pragma unroll
    for (int r = 0; r < D; ++r) fo[r] = MASKED ? fixed[row * D + r] : 0;
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
      for (int r = 0; r < D; ++r) xo[c][r] = on[c] ? x[(c0 + c) * vs + row * D + r] : 0.0;
    {
      double dg[DD];
#pragma unroll
      for (int q = 0; q < DD; ++q) dg[q] = diag[row * DD + q];
      const double md = mdiag[row];
#pragma unroll
      for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int r = 0; r < D; ++r) {
          double s = 0.0;
#pragma unroll
          for (int cc = 0; cc < D; ++cc) s += dg[r * D + cc] * (fo[cc] ? 0.0 : xo[c][cc]);
          acc[c][r] = s;
          accm[c][r] = md * (fo[r] ? 0.0 : xo[c][r]);
        }
    }
    for (int k = 0; k < len; ++k) {
      const int64_t e = femo_sell_index(mb, k, lane);
      const int64_t col = cols[e];
      double blk[DD];
#pragma unroll
      for (int q = 0; q < DD; ++q) blk[q] = vals[e * DD + q];
      const double mv = mvals[e];
      uint8_t fc[D];
#pragma unroll
      for (int cc = 0; cc < D; ++cc) fc[cc] = MASKED ? fixed[col * D + cc] : 0;
#pragma unroll
      for (int c = 0; c < MC; ++c) {
        if (!on[c]) continue;
        double xc[D];
#pragma unroll
        for (int cc = 0; cc < D; ++cc) {
          xc[cc] = x[(c0 + c) * vs + col * D + cc];
          if (MASKED && fc[cc]) xc[cc] = 0.0;
        }
#pragma unroll
        for (int r = 0; r < D; ++r) {
#pragma unroll
          for (int cc = 0; cc < D; ++cc) acc[c][r] += blk[r * D + cc] * xc[cc];
          accm[c][r] += mv * xc[r];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      if (!on[c]) continue;
#pragma unroll
      for (int r = 0; r < D; ++r) {
        double o = MASKED && fo[r] ? xo[c][r] : acc[c][r] - sg[c] * accm[c][r];
        o = a * o;
        if (f) o += b * f[(c0 + c) * vs + row * D + r];
        y[(c0 + c) * vs + row * D + r] = o;
        dotv[c] += xo[c][r] * o;
      }
    }
  }
  if (part) {
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      if (!on[c]) continue;
      const double s = femo_block_sum<EB>(dotv[c], lds);
      if (threadIdx.x == 0) part[(c0 + c) * ps + blockIdx.x] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- MINRES ----
// blockIdx.y (k_minres_scalar: blockIdx.x) is the column.
// STEP: the Lanczos update r' = q - (alfa / beta) r2 - (beta / oldb) r1 (the last term from the second iteration on),
// r1 <- r2, r2 <- r'; a frozen column is skipped.  JACOBI: z = Dinv r2 (block) and the partial r2.z per block as well.
template <int D, bool STEP, bool JACOBI>
__global__ __launch_bounds__(EB) void k_minres_lanczos(int64_t n_rows, const double* __restrict__ dinv, double* __restrict__ r1,
                                                       double* __restrict__ r2, const double* __restrict__ q,
                                                       double* __restrict__ z, const double* __restrict__ ms,
                                                       double* __restrict__ part, int64_t ps, const int32_t* __restrict__ flag) {
  constexpr int DD = D * D;
  __shared__ double lds[EB / 64];
  flag += blockIdx.y * EMF_STRIDE;
  ms += blockIdx.y * MS_STRIDE;
  if (STEP && flag[0]) return;
  const int64_t colv = (int64_t)blockIdx.y * n_rows * D;
  r1 += colv; r2 += colv; q += colv; z += colv; part += blockIdx.y * ps;
  double ca = 0.0, cb = 0.0;
  if (STEP) {
    ca = ms[MS_ALFA] / ms[MS_BETA];
    cb = flag[1] >= 1 ? ms[MS_BETA] / ms[MS_OLDB] : 0.0;
  }
  double dotv = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * EB) {
    double rr[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int64_t o = row * D + i;
      double ri = r2[o];
      if (STEP) {
        double t = q[o] - ca * ri;
        if (cb != 0.0) t -= cb * r1[o];
        r1[o] = ri;
        r2[o] = t;
        ri = t;
      }
      rr[i] = ri;
    }
    if (JACOBI) {
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double zi = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) zi += dinv[row * DD + i * D + k] * rr[k];
        z[row * D + i] = zi;
        dotv += rr[i] * zi;
      }
    }
  }
  if (JACOBI) {
    const double t = femo_block_sum<EB>(dotv, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
  }
}

// mode 0: beta1 = sqrt(r.z) of the first residual, the start values and the stopping level.  mode 1: alfa = v.q.
// mode 2: beta = sqrt(r2.z), the rotation, phi and phibar, the stopping test.  One workgroup per column.
__global__ __launch_bounds__(1024) void k_minres_scalar(int mode, const double* __restrict__ part, int64_t ps, int np, double rtol,
                                                        double atol, int max_it, double* __restrict__ ms,
                                                        int32_t* __restrict__ flag) {
  __shared__ double lds[16];
  part += blockIdx.x * ps;
  ms += blockIdx.x * MS_STRIDE;
  flag += blockIdx.x * EMF_STRIDE;
  if (mode != 0 && flag[0]) return;
  const double v = femo_fold_partials<1024>(part, np, lds);
  if (threadIdx.x != 0) return;
  if (mode == 0) {
    const double beta1 = sqrt(v);
    const double tol = fmax(rtol * beta1, atol);
    ms[MS_BETA1] = beta1; ms[MS_BETA] = beta1; ms[MS_OLDB] = 0.0; ms[MS_ALFA] = 0.0; ms[MS_DBAR] = 0.0; ms[MS_EPSLN] = 0.0;
    ms[MS_OLDEPS] = 0.0; ms[MS_DELTA] = 0.0; ms[MS_GAMMA] = 0.0; ms[MS_CS] = -1.0; ms[MS_SN] = 0.0; ms[MS_PHI] = 0.0;
    ms[MS_PHIBAR] = beta1; ms[MS_TOL] = tol;
    flag[0] = 0; flag[1] = 0; flag[2] = 0; flag[3] = 0;
    if (!is_finite(beta1)) { flag[0] = 1; flag[2] = 1; }                                  // v < 0 included
    else if (beta1 <= tol) { flag[0] = 1; flag[3] = 1; }                                  // a zero right-hand side included
  } else if (mode == 1) {
    if (!is_finite(v)) { flag[0] = 1; flag[2] = 1; return; }
    ms[MS_ALFA] = v;
  } else {
    flag[1] += 1;
    const double beta = sqrt(v), alfa = ms[MS_ALFA];
    const double cs = ms[MS_CS], sn = ms[MS_SN], dbar = ms[MS_DBAR];
    const double delta = cs * dbar + sn * alfa;
    const double gbar = sn * dbar - cs * alfa;
    double gamma = sqrt(gbar * gbar + beta * beta);
    gamma = fmax(gamma, 2.220446049250313e-16);
    const double cn = gbar / gamma, snn = beta / gamma;
    const double phi = cn * ms[MS_PHIBAR], phibar = snn * ms[MS_PHIBAR];
    if (!is_finite(beta) || !is_finite(phi) || !is_finite(delta)) { flag[0] = 1; flag[2] = 1; return; }
    ms[MS_OLDEPS] = ms[MS_EPSLN];
    ms[MS_DELTA] = delta;
    ms[MS_EPSLN] = sn * beta;
    ms[MS_DBAR] = -cs * beta;
    ms[MS_GAMMA] = gamma;
    ms[MS_CS] = cn; ms[MS_SN] = snn;
    ms[MS_PHI] = phi; ms[MS_PHIBAR] = phibar;
    ms[MS_OLDB] = ms[MS_BETA];
    ms[MS_BETA] = beta;
    if (phibar <= ms[MS_TOL] || beta == 0.0) { flag[0] = 1; flag[3] = 1; }                // beta = 0: an invariant subspace
    else if (flag[1] >= max_it) flag[0] = 1;
  }
}

// STEP (iteration `it` of the loop): for a column whose iteration count is `it` -- active, or finished in this very
// iteration -- w = (v - oldeps w1 - delta w2) / gamma, w1 <- w2, w2 <- w, x += phi w; and v = z / beta unless it has
// finished.  Otherwise (the start): v = z / beta1, w1 = w2 = 0 for the columns that are not done at iteration 0.
template <bool STEP>
__global__ __launch_bounds__(EB) void k_minres_x(int64_t n, int it, double* __restrict__ x, double* __restrict__ v,
                                                 const double* __restrict__ z, double* __restrict__ w1, double* __restrict__ w2,
                                                 const double* __restrict__ ms, const int32_t* __restrict__ flag) {
  flag += blockIdx.y * EMF_STRIDE;
  ms += blockIdx.y * MS_STRIDE;
  if (STEP ? (flag[1] != it || flag[2] != 0) : flag[0] != 0) return;
  const int64_t colv = (int64_t)blockIdx.y * n;
  x += colv; v += colv; z += colv; w1 += colv; w2 += colv;
  const bool go_on = flag[0] == 0;
  const double beta = ms[MS_BETA];
  if (!STEP) {
    for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EB) {
      v[i] = z[i] / beta;
      w1[i] = 0.0;
      w2[i] = 0.0;
    }
    return;
  }
  const double oldeps = ms[MS_OLDEPS], delta = ms[MS_DELTA], gamma = ms[MS_GAMMA], phi = ms[MS_PHI];
  for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EB) {
    const double wo = w2[i];
    const double w = (v[i] - oldeps * w1[i] - delta * wo) / gamma;
    w1[i] = wo;
    w2[i] = w;
    x[i] += phi * w;
    if (go_on) v[i] = z[i] / beta;
  }
}

// ----------------------------------------------------------------------------------------- mass part of dR/drho ----
// rev: y_c (+)= sum_l s_l rho0 m'(rho_c) x_{l,c}^T M0_c u_{l,c}, one thread per cell, the columns in ascending order
template <int D>
__global__ __launch_bounds__(EB) void k_elast_mass_drho_T(int64_t n_cell, int64_t n_dof, const int32_t* __restrict__ conn,
                                                          const double* __restrict__ xv, const double* __restrict__ rho, int law,
                                                          double rho0, int n_cols, ColScalars sc, const double* __restrict__ u,
                                                          const double* __restrict__ x, double* __restrict__ y, int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= n_cell) return;
  const ElastCellVolume<D> K = elast_cell_volume<D>(conn, xv, c);
  const double dM = mass_weight<D>(rho0 * mass_law_d(law, rho[c]), K.vol);
  double acc = 0.0;
  for (int l = 0; l < n_cols; ++l) {
    const double* __restrict__ ul = u + (int64_t)l * n_dof;
    const double* __restrict__ xl = x + (int64_t)l * n_dof;
    double mm = 0.0;         // sum_i (sx su + xu): not the order of the mass part of k_elast_eig_drho
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double su = 0.0, sx = 0.0, xu = 0.0;
#pragma unroll
      for (int b = 0; b <= D; ++b) {
        const double ub = ul[(int64_t)K.v[b] * D + i], xb = xl[(int64_t)K.v[b] * D + i];
        su += ub; sx += xb; xu += xb * ub;
      }
      mm += sx * su + xu;
    }
    acc += sc.v[l] * (dM * mm);
  }
  y[c] = accumulate ? y[c] + acc : acc;
}

// fwd: y_l[(v, i)] (+)= s_l sum over the cells c around v of rho0 m'(rho_c) dr_c (M0_c u_{l,c})[(v, i)]; one thread per vertex
// row on the shared visit walk (elast_visits) with the mass row of k_elast_mass (mass_row_add), the geometry of a visit
// serving all columns
template <int D>
__global__ __launch_bounds__(EB) void k_elast_mass_drho_N(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, const double* __restrict__ rho, int law, double rho0, int n_cols, ColScalars sc,
    const double* __restrict__ u, const double* __restrict__ dr, double* __restrict__ y, int accumulate) {
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
    mass_row_add<D, false>(K.v, t.a, mass_weight<D>(rho0 * mass_law_d(law, rho[t.c]) * dr[t.c], K.vol), nullptr, n_cols, n_dof, u,
                           acc);
  }
#pragma unroll
  for (int l = 0; l < EMC; ++l) {
    if (l >= n_cols) break;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int64_t k = (int64_t)l * n_dof + row * D + i;
      const double t = sc.v[l] * acc[l][i];
      y[k] = accumulate ? y[k] + t : t;
    }
  }
}

// ----------------------------------------------------------------------------------------------- launches ----
// y_l = a (Op - sig_l M) x_l + b f_l on raw pointers, as femo_elast_spmv
int dyn_spmv(femo_elast* e, bool masked, int n_cols, const ColScalars& sig, double a, const double* x, double b, const double* f,
             double* y, double* part, int64_t ps, const int32_t* done) {
  femo_mesh* m = e->mesh;
  // one column: the MC = 1 instantiation, which carries no accumulators of absent columns
  const int mc = n_cols == 1 ? 1 : ELAST_CHUNK;
  elast_dispatch(e->d, masked, [&](auto dim, auto mask) {
    constexpr int D = decltype(dim)::value;
    constexpr bool MASKED = decltype(mask)::value;
    auto* kernel = n_cols == 1 ? k_elast_dyn_spmv_multi<D, MASKED, 1> : k_elast_dyn_spmv_multi<D, MASKED, ELAST_CHUNK>;
    hipLaunchKernelGGL(kernel, dim3(grid_of(m->n_rows), (unsigned)((n_cols + mc - 1) / mc)), dim3(EB), 0, m->ctx->stream, m->n_rows,
                       m->d_mptr, m->d_cols, m->d_rowlen, e->d_vals, e->d_diag, e->d_mvals, e->d_mdiag, e->d_fixed, n_cols,
                       m->n_rows * D, sig, a, x, b, f, y, part, ps, done);
  });
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

bool shifts_ok(int n_cols, const double* shifts, ColScalars& sig) {
  for (int l = 0; l < EMC; ++l) {
    sig.v[l] = l < n_cols ? shifts[l] : 0.0;
    if (!(sig.v[l] >= 0.0) || !std::isfinite(sig.v[l])) return false;
  }
  return true;
}

// the batched MINRES of femo_elast_dyn_solve_multi, which has checked its arguments
int minres_solve(femo_elast* e, int n_cols, const ColScalars& sig, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts,
                 femo_solve_info* info, const char* who) {
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d;
  const bool ml = opts->pc == FEMO_ELAST_PC_MULTILEVEL;
  hipStream_t st = m->ctx->stream;
  const bool masked = e->has_fixed;
  const int nps = (int)grid_of(m->n_rows);
  const unsigned L = (unsigned)n_cols, gp = (unsigned)PCG_GRID;
  // r2, z, v, q are the PCG's work vectors w_r, w_z, w_p, w_q; r1, w1, w2 lie behind one another in w_harm.  The loop
  // reserves them before start(), so every launch reads them from the handle when it runs
  auto harm = [&](int k) { return e->w_harm + k * n * n_cols; };
#define FEMO_LANCZOS(D, S, J) hipLaunchKernelGGL((k_minres_lanczos<D, S, J>), dim3(gp, L), dim3(EB), 0, st, m->n_rows, e->d_dinv, \
                                                 harm(0), e->w_r, e->w_q, e->w_z, e->w_ms, e->w_part, e->w_pstride, e->w_flag)
  // z = M^-1 r2 and the partials of r2.z: update = false reads neither s nor (for a frozen column) anything it may not
  auto precond = [&](bool step) -> int {
    if (ml) {
      if (step) { if (e->d == 2) FEMO_LANCZOS(2, true, false); else FEMO_LANCZOS(3, true, false); }
      return femo_elast_pc_step(e, false, n_cols, nullptr, e->w_r, nullptr, nullptr, e->w_z, nullptr, e->w_s, e->w_part, e->w_pstride,
                                e->w_flag,
                                e->d_dinv);
    }
    if (e->d == 2) { if (step) FEMO_LANCZOS(2, true, true); else FEMO_LANCZOS(2, false, true); }
    else { if (step) FEMO_LANCZOS(3, true, true); else FEMO_LANCZOS(3, false, true); }
    return 0;
  };
#undef FEMO_LANCZOS
#define FEMO_MINRES_SCALAR(MODE, NP) hipLaunchKernelGGL(k_minres_scalar, dim3(L), dim3(1024), 0, st, MODE, e->w_part, e->w_pstride, NP, \
                                                        opts->rtol, opts->atol, max_it, e->w_ms, e->w_flag)
  femo_elast_krylov loop = {who, n_cols, n_cols, 1, true};
  loop.start = [&](int max_it) -> int {
    FEMO_TRY(femo_elast_start_x(e, n_cols, opts->zero_guess, b->d, x->d));
    FEMO_TRY(dyn_spmv(e, masked, n_cols, sig, -1.0, x->d, 1.0, b->d, e->w_r, nullptr, 0, nullptr));             // r2 = b - S x
    FEMO_TRY(precond(false));
    FEMO_MINRES_SCALAR(0, PCG_GRID);
    hipLaunchKernelGGL(k_minres_x<false>, dim3(gp, L), dim3(EB), 0, st, n, 0, x->d, e->w_p, e->w_z, harm(1), harm(2), e->w_ms, e->w_flag);
    return 0;
  };
  loop.iterate = [&](int it, int max_it) -> int {
    FEMO_TRY(dyn_spmv(e, masked, n_cols, sig, 1.0, e->w_p, 0.0, nullptr, e->w_q, e->w_part, e->w_pstride, e->w_flag));   // q = S v, v.q
    FEMO_MINRES_SCALAR(1, nps);
    FEMO_TRY(precond(true));
    FEMO_MINRES_SCALAR(2, PCG_GRID);
    hipLaunchKernelGGL(k_minres_x<true>, dim3(gp, L), dim3(EB), 0, st, n, it + 1, x->d, e->w_p, e->w_z, harm(1), harm(2), e->w_ms, e->w_flag);
    return 0;
  };
#undef FEMO_MINRES_SCALAR
  loop.d_scal = &femo_elast::w_ms; loop.h_scal = &femo_elast::h_ms; loop.scal_stride = MS_STRIDE;
  loop.s_res = MS_PHIBAR; loop.s_rhs = MS_BETA1; loop.squared = false;
  return femo_elast_krylov_loop(e, b, x, opts, info, loop);
}

}  // namespace

int femo_elast_dyn_spmv(femo_elast* e, bool masked, int n_cols, double shift, double a, const double* x, double b, const double* f,
                        double* y, double* part, int64_t part_stride, const int32_t* done) {
  ColScalars sig;
  for (int l = 0; l < EMC; ++l) sig.v[l] = shift;
  return dyn_spmv(e, masked, n_cols, sig, a, x, b, f, y, part, part_stride, done);
}

// the three extra vectors of the MINRES loop (r1, w1, w2) for at least n_cols columns, its scalars and their pinned mirror
int femo_elast_harm_reserve(femo_elast* e, int n_cols, const char* who) {
  if (!e->w_ms) FEMO_TRY(dalloc(&e->w_ms, (int64_t)MS_STRIDE * EMC));
  if (!e->h_ms) FEMO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->h_ms), MS_STRIDE * EMC * sizeof(double)));
  if (e->w_harm_cols >= n_cols) return 0;
  const int64_t n = e->mesh->n_vert * e->d;
  double* w = nullptr;
  if (dalloc(&w, 3 * n * n_cols)) {
    femo_set_error("%s: device allocation failed", who);
    return 1;
  }
  FEMO_HIP_CHECK(hipStreamSynchronize(e->mesh->ctx->stream));
  hipFree(e->w_harm);
  e->w_harm = w;
  e->w_harm_cols = n_cols;
  return 0;
}

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_mass_assemble(femo_elast* e, int mass_law, double density, const femo_vec* rho) {
  FEMO_REQUIRE(e && rho, "null argument");
  FEMO_REQUIRE(mass_law == FEMO_ELAST_MASS_LINEAR || mass_law == FEMO_ELAST_MASS_DU_OLHOFF, "unknown mass law %d", mass_law);
  FEMO_REQUIRE(density >= 0.0 && std::isfinite(density), "femo_elast_mass_assemble: need a finite density >= 0");
  femo_mesh* m = e->mesh;
  FEMO_REQUIRE(rho->n >= m->n_cell, "density vector too small");
  if (!e->d_mvals) {
    double *mv = nullptr, *md = nullptr;
    if (dalloc(&mv, m->sell_entries) || dalloc(&md, m->n_rows)) {
      hipFree(mv);
      femo_set_error("femo_elast_mass_assemble: device allocation failed");
      return 1;
    }
    e->d_mvals = mv; e->d_mdiag = md;
  }
  FEMO_TRY(femo_vec_await(rho));
  FEMO_TRY(elast_dispatch_d(e->d, [&](auto dim) {
    return elast_launch_rows(e, k_elast_mass_assemble<decltype(dim)::value>, m->d_vptr, m->d_visit_cell, m->d_visit_slots, m->d_mptr,
                             m->d_rowlen, m->d_conn, m->d_x, rho->d, mass_law, density, e->d_mvals, e->d_mdiag);
  }));
  e->mass_assembled = true;
  return 0;
}

int femo_elast_dyn_apply_multi(femo_elast* e, int masked, int n_cols, const double* shifts, double a, const femo_vec* x, double b,
                               const femo_vec* f, femo_vec* y) {
  FEMO_REQUIRE(e && shifts && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_dyn_apply_multi: %d columns (1 to %d)", n_cols, EMC);
  FEMO_REQUIRE(e->assembled, "femo_elast_dyn_apply_multi: assemble K first");
  FEMO_REQUIRE(e->mass_assembled, "femo_elast_dyn_apply_multi: assemble M first (femo_elast_mass_assemble)");
  const int64_t n = e->mesh->n_vert * e->d * n_cols;
  FEMO_REQUIRE(x->n >= n && y->n >= n && (!f || f->n >= n),
               "vector size mismatch in femo_elast_dyn_apply_multi: %d columns need %lld entries", n_cols, (long long)n);
  FEMO_REQUIRE(!masked || e->has_fixed, "femo_elast_dyn_apply_multi: masked product without a fixed set");
  FEMO_REQUIRE(x != y, "femo_elast_dyn_apply_multi: x and y must differ");
  ColScalars sig;
  FEMO_REQUIRE(shifts_ok(n_cols, shifts, sig), "femo_elast_dyn_apply_multi: the shifts omega^2 must be finite and >= 0");
  FEMO_TRY(femo_vec_await(x));
  if (f) FEMO_TRY(femo_vec_await(f));
  femo_vec_touch(y);
  return dyn_spmv(e, masked != 0, n_cols, sig, a, x->d, b, f ? f->d : nullptr, y->d, nullptr, 0, nullptr);
}

int femo_elast_dyn_solve_multi(femo_elast* e, int n_cols, const double* shifts, const femo_vec* b, femo_vec* x,
                               const femo_solver_opts* opts, femo_solve_info* info) {
  FEMO_REQUIRE(e && shifts && b && x && opts, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_dyn_solve_multi: %d columns (1 to %d)", n_cols, EMC);
  FEMO_REQUIRE(e->assembled, "femo_elast_dyn_solve_multi: assemble K first");
  FEMO_REQUIRE(e->mass_assembled, "femo_elast_dyn_solve_multi: assemble M first (femo_elast_mass_assemble)");
  const int64_t n = e->mesh->n_vert * e->d * n_cols;
  FEMO_REQUIRE(b->n >= n && x->n >= n && b != x, "vector size mismatch in femo_elast_dyn_solve_multi: %d columns need %lld entries",
               n_cols, (long long)n);
  ColScalars sig;
  FEMO_REQUIRE(shifts_ok(n_cols, shifts, sig), "femo_elast_dyn_solve_multi: the shifts omega^2 must be finite and >= 0");
  return minres_solve(e, n_cols, sig, b, x, opts, info, "femo_elast_dyn_solve_multi");
}

int femo_elast_mass_drho_multi(femo_elast* e, int mass_law, double density, int transpose, int n_cols, const double* scales,
                               const femo_vec* rho, const femo_vec* u, const femo_vec* x, femo_vec* y, int accumulate) {
  FEMO_REQUIRE(e && scales && rho && u && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_mass_drho_multi: %d columns (1 to %d)", n_cols, EMC);
  FEMO_REQUIRE(mass_law == FEMO_ELAST_MASS_LINEAR || mass_law == FEMO_ELAST_MASS_DU_OLHOFF, "unknown mass law %d", mass_law);
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d, nl = n * n_cols;
  FEMO_REQUIRE(rho->n >= m->n_cell && u->n >= nl, "vector size mismatch in femo_elast_mass_drho_multi");
  FEMO_REQUIRE(transpose ? (x->n >= nl && y->n >= m->n_cell) : (x->n >= m->n_cell && y->n >= nl),
               "vector size mismatch in femo_elast_mass_drho_multi");
  FEMO_REQUIRE(y != x && y != u && y != rho, "femo_elast_mass_drho_multi: output aliases an input");
  ColScalars sc;
  for (int l = 0; l < EMC; ++l) sc.v[l] = l < n_cols ? scales[l] : 0.0;
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(u)); FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(y);
  return elast_dispatch_d(e->d, [&](auto dim) {
    constexpr int D = decltype(dim)::value;
    if (transpose)
      return elast_launch_cells(e, k_elast_mass_drho_T<D>, n, m->d_conn, m->d_x, rho->d, mass_law, density, n_cols, sc, u->d, x->d,
                                y->d, accumulate);
    return elast_launch_rows(e, k_elast_mass_drho_N<D>, m->d_vptr, m->d_visit_cell, m->d_conn, m->d_x, rho->d, mass_law, density,
                             n_cols, sc, u->d, x->d, y->d, accumulate);
  });
}

}  // extern "C"
