// SIMP topology optimisation: damped harmonic response of the linear elasticity in complex arithmetic (C-ABI in
// include/femo_hip.h: femo_elast_cdyn_apply_multi, femo_elast_cdyn_solve_multi),
//
//   Z_l u_l = F_l,   Z_l = (K - sigma_l M) + i (cK_l K + cM_l M),   sigma_l = omega_l^2,
//
// with the assembled K and the scalar mass matrix of femo_elast_mass_assemble (elast_harm.hip).  cK_l = eta + omega_l beta
// and cM_l = omega_l alpha hold a structural loss factor eta and Rayleigh damping alpha M + beta K; the library sees the two
// coefficients only.  Z is complex SYMMETRIC, not Hermitian.
//
// Layout: complex column l is the pair of real columns 2 l (Re) and 2 l + 1 (Im) of the layout of elast_solve.hip, so
// 1 <= L <= FEMO_ELAST_MAX_COLS / 2.  sigma, cK, cM travel by value, one per complex column.
//
// The product k_elast_cdyn_spmv_multi is k_elast_dyn_spmv_multi with four accumulators per complex column and component
// -- K x_re, M x_re, K x_im, M x_im -- from ONE read of the block, its column index, the fixed bytes and the mass scalar of
// an entry.  Two complex columns per thread (ELAST_CHUNK / 2) are the registers of the real kernel at four.  It keeps a row
// walk of its own, in the order of elast_row_walk (elast_internal.h) over the real columns 2 c + h: through the shared walk
// its <2, false, 2> instantiation changes occupancy (DESIGN_LOG.md R24).  Each part is formed as the real
// kernel forms it, (K x - sigma M x), and the damping term is subtracted (added) last: with cK = cM = 0 both parts have the
// bits of femo_elast_dyn_apply_multi.  conj = 1 gives conj(Z), the transpose of the real 2L-column operator.
//
// The solve is the preconditioned COCR of Sogabe & Zhang (2007): conjugate residuals with the unconjugated bilinear form
// x^T y, for which a complex symmetric Z is "self-adjoint", with the real SPD preconditioners of the static solve applied to
// both parts.  (The real-equivalent symmetric form [[A, -B], [-B, -A]] under MINRES has a spectrum symmetric about zero and
// takes 5 to 25 times the iterations: DESIGN.md.)  One iteration issues these launches, each with a column dimension:
//
//   w_l = Z_l z_l, partial z_l^T w_l                         k_elast_cdyn_spmv_multi
//   rho_l, beta_l = rho_l / rho_l(old)                       k_cocr_scalar (mode 1)      one workgroup per column
//   p = z + beta p, q = w + beta q, m = M^-1 q, partial q^T m
//                                                            k_cocr_dir (block-Jacobi in the same launch), or k_cocr_dir, the
//                                                            four launches of femo_elast_pc_step(update = false) on the 2 L
//                                                            real columns and k_cocr_dot
//   alpha_l = rho_l / (q^T m)                                k_cocr_scalar (mode 2)
//   x += alpha p, r -= alpha q, z -= alpha m, partial Re(r^H z)
//                                                            k_cocr_update
//   the iteration count and the convergence of column l      k_cocr_scalar (mode 3)
//
// z = M^-1 r is carried by its recurrence: one product and one preconditioner application per iteration, as in the MINRES.
// Complex column l owns its scalars at w_ms + l * CS_STRIDE and the flags of the PCG loop (0 done, 1 iterations, 2
// non-finite or zero denominator, 3 converged), written to BOTH of its real columns' slots, so that the preconditioner
// step sees them per real column.  A column whose flag[0] is set is frozen and never written again.  All dots are
// per-block partials folded in a fixed order: no float atomics, and a column has the same bits whatever L is.
//
// It stops on sqrt(Re(r^H M^-1 r)) <= max(rtol beta1, atol), beta1 that of the first residual: the norm the PCG tests.
#include "elast_internal.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;
constexpr int CMC = EMC / 2;          // complex columns at the most

// one value per complex column
struct CplxScalars { double v[CMC]; };

// COCR device scalars of a complex column
enum { CS_RHO_R = 0, CS_RHO_I, CS_ALPHA_R, CS_ALPHA_I, CS_BETA_R, CS_BETA_I, CS_BETA1, CS_TOL, CS_RES };
constexpr int CS_STRIDE = 16;
static_assert(CS_STRIDE * CMC <= FEMO_ELAST_HARM_SCALARS * EMC, "the COCR scalars live in the MINRES scalars");

// ------------------------------------------------------------------------------------------- complex product ----
// y_l = a Z_l x_l + b f_l (conj(Z_l) with cj = -1) for the complex columns c0 = MC * blockIdx.y ... min(c0 + MC, n_cols)
// - 1, + the partials of the unconjugated x_l^T y_l per block when part != null (Re in slab 2 l, Im in slab 2 l + 1).
// MASKED: identity rows / columns on the fixed dofs of both parts.  done != null: a column whose done[2 l * EMF_STRIDE] is
// set is skipped.  vs: stride of a REAL column of the vectors, ps: of a slab of partials.
template <int D, bool MASKED, int MC>
__global__ __launch_bounds__(EB) void k_elast_cdyn_spmv_multi(
    int64_t n_rows, const int64_t* __restrict__ mptr, const int32_t* __restrict__ cols, const int32_t* __restrict__ rowlen,
    const double* __restrict__ vals, const double* __restrict__ diag, const double* __restrict__ mvals,
    const double* __restrict__ mdiag, const uint8_t* __restrict__ fixed, int n_cols, int64_t vs, CplxScalars sig, CplxScalars ck,
    CplxScalars cm, double cj, double a, const double* __restrict__ x, double b, const double* __restrict__ f,
    double* __restrict__ y, double* __restrict__ part, int64_t ps, const int32_t* __restrict__ done) {
  constexpr int DD = D * D;
  __shared__ double lds[EB / 64];
  const int c0 = (int)blockIdx.y * MC;
  bool on[MC];          // uniform over the block
  double sg[MC], dk[MC], dm[MC];
  bool any = false;
#pragma unroll
  for (int c = 0; c < MC; ++c) {
    const bool in = c0 + c < n_cols;
    on[c] = in && !(done && done[2 * (c0 + c) * EMF_STRIDE]);
    sg[c] = in ? sig.v[c0 + c] : 0.0;
    dk[c] = in ? cj * ck.v[c0 + c] : 0.0;
    dm[c] = in ? cj * cm.v[c0 + c] : 0.0;
    any = any || on[c];
  }
  if (!any) return;
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  double dotr[MC], doti[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) dotr[c] = doti[c] = 0.0;
  if (row < n_rows) {
    const int64_t slice = row >> 6;
    const int lane = (int)(row & 63);
    const int64_t mb = mptr[slice];
    const int len = rowlen[row];
    // [c][part][component]
    double acc[MC][2][D], accm[MC][2][D], xo[MC][2][D];
    uint8_t fo[D];
#pragma unroll
    for (int r = 0; r < D; ++r) fo[r] = MASKED ? fixed[row * D + r] : 0;
#pragma unroll
    for (int c = 0; c < MC; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < D; ++r) xo[c][h][r] = on[c] ? x[(2 * (c0 + c) + h) * vs + row * D + r] : 0.0;
    {
      double dg[DD];
#pragma unroll
      for (int q = 0; q < DD; ++q) dg[q] = diag[row * DD + q];
      const double md = mdiag[row];
#pragma unroll
      for (int c = 0; c < MC; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int r = 0; r < D; ++r) {
            double s = 0.0;
#pragma unroll
            for (int cc = 0; cc < D; ++cc) s += dg[r * D + cc] * (fo[cc] ? 0.0 : xo[c][h][cc]);
            acc[c][h][r] = s;
            accm[c][h][r] = md * (fo[r] ? 0.0 : xo[c][h][r]);
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
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          double xc[D];
#pragma unroll
          for (int cc = 0; cc < D; ++cc) {
            xc[cc] = x[(2 * (c0 + c) + h) * vs + col * D + cc];
            if (MASKED && fc[cc]) xc[cc] = 0.0;
          }
#pragma unroll
          for (int r = 0; r < D; ++r) {
#pragma unroll
            for (int cc = 0; cc < D; ++cc) acc[c][h][r] += blk[r * D + cc] * xc[cc];
            accm[c][h][r] += mv * xc[r];
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      if (!on[c]) continue;
#pragma unroll
      for (int r = 0; r < D; ++r) {
        // the undamped parts exactly as k_elast_dyn_spmv_multi forms them, the damping term last
        double o_r = MASKED && fo[r] ? xo[c][0][r] : acc[c][0][r] - sg[c] * accm[c][0][r];
        double o_i = MASKED && fo[r] ? xo[c][1][r] : acc[c][1][r] - sg[c] * accm[c][1][r];
        if (!(MASKED && fo[r])) {
          o_r -= dk[c] * acc[c][1][r] + dm[c] * accm[c][1][r];
          o_i += dk[c] * acc[c][0][r] + dm[c] * accm[c][0][r];
        }
        o_r = a * o_r;
        o_i = a * o_i;
        if (f) {
          o_r += b * f[(2 * (c0 + c)) * vs + row * D + r];
          o_i += b * f[(2 * (c0 + c) + 1) * vs + row * D + r];
        }
        y[(2 * (c0 + c)) * vs + row * D + r] = o_r;
        y[(2 * (c0 + c) + 1) * vs + row * D + r] = o_i;
        dotr[c] += xo[c][0][r] * o_r - xo[c][1][r] * o_i;
        doti[c] += xo[c][0][r] * o_i + xo[c][1][r] * o_r;
      }
    }
  }
  if (part) {
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      if (!on[c]) continue;
      const double sr = femo_block_sum<EB>(dotr[c], lds);
      const double si = femo_block_sum<EB>(doti[c], lds);
      if (threadIdx.x == 0) {
        part[(2 * (c0 + c)) * ps + blockIdx.x] = sr;
        part[(2 * (c0 + c) + 1) * ps + blockIdx.x] = si;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------ COCR ----
// blockIdx.y (k_cocr_scalar: blockIdx.x) is the complex column; its parts are the real columns 2 l and 2 l + 1.
//
// STEP: p = z + beta p, q = w + beta q (p = z, q = w in the first iteration); a frozen column is skipped.  JACOBI: out =
// Dinv src on both parts (src = q with STEP, the residual without) and the partials per block: of the unconjugated
// src^T out with STEP (Re, Im), of Re(src^H out) without (Re only).
template <int D, bool STEP, bool JACOBI>
__global__ __launch_bounds__(EB) void k_cocr_dir(int64_t n_rows, const double* __restrict__ dinv, const double* __restrict__ src,
                                                 const double* __restrict__ w, double* __restrict__ p, double* __restrict__ q,
                                                 double* __restrict__ out, const double* __restrict__ cs,
                                                 double* __restrict__ part, int64_t ps, const int32_t* __restrict__ flag) {
  constexpr int DD = D * D;
  __shared__ double lds[EB / 64];
  flag += 2 * blockIdx.y * EMF_STRIDE;
  cs += blockIdx.y * CS_STRIDE;
  if (flag[0]) return;
  const int64_t n = n_rows * D;
  const int64_t colv = 2 * (int64_t)blockIdx.y * n;
  src += colv; w += colv; p += colv; q += colv; out += colv; part += 2 * blockIdx.y * ps;
  const bool first = flag[1] == 0;
  const double br = STEP && !first ? cs[CS_BETA_R] : 0.0, bi = STEP && !first ? cs[CS_BETA_I] : 0.0;
  double dr = 0.0, di = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * EB) {
    double vr[D], vi[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int64_t o = row * D + i;
      if (STEP) {
        double pr = src[o], pi = src[n + o], qr = w[o], qi = w[n + o];
        if (!first) {
          const double pr0 = p[o], pi0 = p[n + o], qr0 = q[o], qi0 = q[n + o];
          pr += br * pr0 - bi * pi0;
          pi += br * pi0 + bi * pr0;
          qr += br * qr0 - bi * qi0;
          qi += br * qi0 + bi * qr0;
        }
        p[o] = pr; p[n + o] = pi; q[o] = qr; q[n + o] = qi;
        vr[i] = qr; vi[i] = qi;
      } else {
        vr[i] = src[o]; vi[i] = src[n + o];
      }
    }
    if (JACOBI) {
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double zr = 0.0, zi = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double dv = dinv[row * DD + i * D + k];
          zr += dv * vr[k];
          zi += dv * vi[k];
        }
        out[row * D + i] = zr;
        out[n + row * D + i] = zi;
        if (STEP) {
          dr += vr[i] * zr - vi[i] * zi;
          di += vr[i] * zi + vi[i] * zr;
        } else {
          dr += vr[i] * zr + vi[i] * zi;
        }
      }
    }
  }
  if (JACOBI) {
    const double tr = femo_block_sum<EB>(dr, lds);
    const double ti = STEP ? femo_block_sum<EB>(di, lds) : 0.0;
    if (threadIdx.x == 0) {
      part[blockIdx.x] = tr;
      if (STEP) part[ps + blockIdx.x] = ti;
    }
  }
}

// The partials of k_cocr_dir behind a preconditioner that does not form them: HERM ? Re(u^H v) : u^T v (Re, Im)
template <bool HERM>
__global__ __launch_bounds__(EB) void k_cocr_dot(int64_t n, const double* __restrict__ u, const double* __restrict__ v,
                                                 double* __restrict__ part, int64_t ps, const int32_t* __restrict__ flag) {
  __shared__ double lds[EB / 64];
  if (flag[2 * blockIdx.y * EMF_STRIDE]) return;
  const int64_t colv = 2 * (int64_t)blockIdx.y * n;
  u += colv; v += colv; part += 2 * blockIdx.y * ps;
  double dr = 0.0, di = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EB) {
    const double ur = u[i], ui = u[n + i], wr = v[i], wi = v[n + i];
    if (HERM) {
      dr += ur * wr + ui * wi;
    } else {
      dr += ur * wr - ui * wi;
      di += ur * wi + ui * wr;
    }
  }
  const double tr = femo_block_sum<EB>(dr, lds);
  const double ti = HERM ? 0.0 : femo_block_sum<EB>(di, lds);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = tr;
    if (!HERM) part[ps + blockIdx.x] = ti;
  }
}

// x += alpha p, r -= alpha q, z -= alpha m, and the partials of Re(r^H z) per block; a frozen column is skipped
__global__ __launch_bounds__(EB) void k_cocr_update(int64_t n, double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                    const double* __restrict__ p, const double* __restrict__ q,
                                                    const double* __restrict__ m, const double* __restrict__ cs,
                                                    double* __restrict__ part, int64_t ps, const int32_t* __restrict__ flag) {
  __shared__ double lds[EB / 64];
  if (flag[2 * blockIdx.y * EMF_STRIDE]) return;
  cs += blockIdx.y * CS_STRIDE;
  const int64_t colv = 2 * (int64_t)blockIdx.y * n;
  x += colv; r += colv; z += colv; p += colv; q += colv; m += colv; part += 2 * blockIdx.y * ps;
  const double ar = cs[CS_ALPHA_R], ai = cs[CS_ALPHA_I];
  double dot = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EB) {
    const double pr = p[i], pi = p[n + i], qr = q[i], qi = q[n + i], mr = m[i], mi = m[n + i];
    x[i] += ar * pr - ai * pi;
    x[n + i] += ar * pi + ai * pr;
    const double rr = r[i] - (ar * qr - ai * qi), ri = r[n + i] - (ar * qi + ai * qr);
    const double zr = z[i] - (ar * mr - ai * mi), zi = z[n + i] - (ar * mi + ai * mr);
    r[i] = rr; r[n + i] = ri;
    z[i] = zr; z[n + i] = zi;
    dot += rr * zr + ri * zi;
  }
  const double t = femo_block_sum<EB>(dot, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// both real columns of a complex column see its flags
__device__ __forceinline__ void set_flag(int32_t* flag, int k, int32_t v) {
  flag[k] = v;
  flag[EMF_STRIDE + k] = v;
}

// mode 0: beta1 = sqrt(Re(r^H z)) of the first residual and the stopping level.  mode 1: rho = z^T w, and beta = rho /
// rho(old) from the second iteration on.  mode 2: alpha = rho / (q^T m).  mode 3: the iteration count, sqrt(Re(r^H z)) and
// the stopping test.  A zero denominator or a non-finite value ends the column (flag 2).  One workgroup per column.
__global__ __launch_bounds__(1024) void k_cocr_scalar(int mode, const double* __restrict__ part, int64_t ps, int np, double rtol,
                                                      double atol, int max_it, double* __restrict__ cs, int32_t* __restrict__ flag) {
  __shared__ double lds[16];
  part += 2 * blockIdx.x * ps;
  cs += blockIdx.x * CS_STRIDE;
  flag += 2 * blockIdx.x * EMF_STRIDE;
  if (mode != 0 && flag[0]) return;
  const double vr = femo_fold_partials<1024>(part, np, lds);
  const double vi = mode == 1 || mode == 2 ? femo_fold_partials<1024>(part + ps, np, lds) : 0.0;
  if (threadIdx.x != 0) return;
  if (mode == 0) {
    const double beta1 = sqrt(vr);
    const double tol = fmax(rtol * beta1, atol);
    for (int k = 0; k < CS_STRIDE; ++k) cs[k] = 0.0;
    cs[CS_BETA1] = beta1; cs[CS_TOL] = tol; cs[CS_RES] = beta1;
    for (int k = 0; k < 4; ++k) set_flag(flag, k, 0);
    if (!is_finite(beta1)) { set_flag(flag, 0, 1); set_flag(flag, 2, 1); }                // vr < 0 included
    else if (beta1 <= tol) { set_flag(flag, 0, 1); set_flag(flag, 3, 1); }                // a zero right-hand side included
  } else if (mode == 1) {
    bool ok = is_finite(vr) && is_finite(vi);
    if (ok && flag[1] >= 1) {
      const double orr = cs[CS_RHO_R], ori = cs[CS_RHO_I];
      const double den = orr * orr + ori * ori;
      const double br = (vr * orr + vi * ori) / den, bi = (vi * orr - vr * ori) / den;
      ok = den != 0.0 && is_finite(br) && is_finite(bi);
      cs[CS_BETA_R] = br; cs[CS_BETA_I] = bi;
    }
    if (!ok) { set_flag(flag, 0, 1); set_flag(flag, 2, 1); return; }
    cs[CS_RHO_R] = vr; cs[CS_RHO_I] = vi;
  } else if (mode == 2) {
    const double rr = cs[CS_RHO_R], ri = cs[CS_RHO_I];
    const double den = vr * vr + vi * vi;
    const double ar = (rr * vr + ri * vi) / den, ai = (ri * vr - rr * vi) / den;
    if (!(den != 0.0) || !is_finite(ar) || !is_finite(ai)) { set_flag(flag, 0, 1); set_flag(flag, 2, 1); return; }
    cs[CS_ALPHA_R] = ar; cs[CS_ALPHA_I] = ai;
  } else {
    const int32_t it = flag[1] + 1;
    set_flag(flag, 1, it);
    const double res = sqrt(vr);
    if (!is_finite(res)) { set_flag(flag, 0, 1); set_flag(flag, 2, 1); return; }
    cs[CS_RES] = res;
    if (res <= cs[CS_TOL]) { set_flag(flag, 0, 1); set_flag(flag, 3, 1); }
    else if (it >= max_it) set_flag(flag, 0, 1);
  }
}

struct Damping {
  CplxScalars sig, ck, cm;
  double cj;          // +1: Z, -1: conj(Z)
};

// y_l = a Z_l x_l + b f_l on raw pointers
int cdyn_spmv(femo_elast* e, bool masked, int n_cols, const Damping& z, double a, const double* x, double b, const double* f,
              double* y, double* part, int64_t ps, const int32_t* done) {
  femo_mesh* m = e->mesh;
  // one complex column: the MC = 1 instantiation; otherwise two per thread
  const int mc = n_cols == 1 ? 1 : ELAST_CHUNK / 2;
  elast_dispatch(e->d, masked, [&](auto dim, auto mask) {
    constexpr int D = decltype(dim)::value;
    constexpr bool MASKED = decltype(mask)::value;
    auto* kernel = n_cols == 1 ? k_elast_cdyn_spmv_multi<D, MASKED, 1> : k_elast_cdyn_spmv_multi<D, MASKED, ELAST_CHUNK / 2>;
    hipLaunchKernelGGL(kernel, dim3(grid_of(m->n_rows), (unsigned)((n_cols + mc - 1) / mc)), dim3(EB), 0, m->ctx->stream, m->n_rows,
                       m->d_mptr, m->d_cols, m->d_rowlen, e->d_vals, e->d_diag, e->d_mvals, e->d_mdiag, e->d_fixed, n_cols,
                       m->n_rows * D, z.sig, z.ck, z.cm, z.cj, a, x, b, f, y, part, ps, done);
  });
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

bool damping_ok(int n_cols, int conj, const double* shifts, const double* ck, const double* cm, Damping& z) {
  z.cj = conj ? -1.0 : 1.0;
  for (int l = 0; l < CMC; ++l) {
    z.sig.v[l] = l < n_cols ? shifts[l] : 0.0;
    z.ck.v[l] = l < n_cols ? ck[l] : 0.0;
    z.cm.v[l] = l < n_cols ? cm[l] : 0.0;
    for (double v : {z.sig.v[l], z.ck.v[l], z.cm.v[l]})
      if (!(v >= 0.0) || !std::isfinite(v)) return false;
  }
  return true;
}

// the batched COCR of femo_elast_cdyn_solve_multi, which has checked its arguments
int cocr_solve(femo_elast* e, int n_cols, const Damping& zd, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts,
               femo_solve_info* info, const char* who) {
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d;
  const int nr = 2 * n_cols;          // real columns
  const bool ml = opts->pc == FEMO_ELAST_PC_MULTILEVEL;
  hipStream_t st = m->ctx->stream;
  const bool masked = e->has_fixed;
  const int nps = (int)grid_of(m->n_rows);
  const unsigned L = (unsigned)n_cols, gp = (unsigned)PCG_GRID;
  // r, z, p, q are the PCG's work vectors w_r, w_z, w_p, w_q; w = Z z and mq = M^-1 q are the first two of the MINRES loop's
  // three in w_harm, the scalars those of the MINRES (w_ms).  The loop reserves them before start(), so every launch reads
  // them from the handle when it runs
  auto mq = [&]() { return e->w_harm + n * e->w_harm_cols; };
#define FEMO_COCR_DIR(D, S, J, SRC, OUT) hipLaunchKernelGGL((k_cocr_dir<D, S, J>), dim3(gp, L), dim3(EB), 0, st, m->n_rows, e->d_dinv, \
                                                            SRC, e->w_harm, e->w_p, e->w_q, OUT, e->w_ms, e->w_part, e->w_pstride, e->w_flag)
  // start: z = M^-1 r and the partials of Re(r^H z).  step: p, q, mq = M^-1 q and the partials of q^T mq
  auto precond = [&](bool step) -> int {
    if (ml) {
      if (step) { if (e->d == 2) FEMO_COCR_DIR(2, true, false, e->w_z, mq()); else FEMO_COCR_DIR(3, true, false, e->w_z, mq()); }
      FEMO_TRY(femo_elast_pc_step(e, false, nr, nullptr, step ? e->w_q : e->w_r, nullptr, nullptr, step ? mq() : e->w_z, nullptr,
                                  e->w_s, e->w_part, e->w_pstride, e->w_flag, e->d_dinv));
      if (step) hipLaunchKernelGGL(k_cocr_dot<false>, dim3(gp, L), dim3(EB), 0, st, n, e->w_q, mq(), e->w_part, e->w_pstride,
                                   e->w_flag);
      else hipLaunchKernelGGL(k_cocr_dot<true>, dim3(gp, L), dim3(EB), 0, st, n, e->w_r, e->w_z, e->w_part, e->w_pstride,
                              e->w_flag);
      return 0;
    }
    if (e->d == 2) { if (step) FEMO_COCR_DIR(2, true, true, e->w_z, mq()); else FEMO_COCR_DIR(2, false, true, e->w_r, e->w_z); }
    else { if (step) FEMO_COCR_DIR(3, true, true, e->w_z, mq()); else FEMO_COCR_DIR(3, false, true, e->w_r, e->w_z); }
    return 0;
  };
#undef FEMO_COCR_DIR
#define FEMO_COCR_SCALAR(MODE, NP) hipLaunchKernelGGL(k_cocr_scalar, dim3(L), dim3(1024), 0, st, MODE, e->w_part, e->w_pstride, NP, \
                                                      opts->rtol, opts->atol, max_it, e->w_ms, e->w_flag)
  femo_elast_krylov loop = {who, nr, n_cols, 2, true};
  loop.start = [&](int max_it) -> int {
    FEMO_TRY(femo_elast_start_x(e, nr, opts->zero_guess, b->d, x->d));
    FEMO_TRY(cdyn_spmv(e, masked, n_cols, zd, -1.0, x->d, 1.0, b->d, e->w_r, nullptr, 0, nullptr));              // r = b - Z x
    // the flags of the last solve may freeze a column before mode 0 has run: clear them first
    FEMO_HIP_CHECK(hipMemsetAsync(e->w_flag, 0, (size_t)nr * EMF_STRIDE * sizeof(int32_t), st));
    FEMO_TRY(precond(false));
    FEMO_COCR_SCALAR(0, PCG_GRID);
    return 0;
  };
  loop.iterate = [&](int, int max_it) -> int {
    FEMO_TRY(cdyn_spmv(e, masked, n_cols, zd, 1.0, e->w_z, 0.0, nullptr, e->w_harm, e->w_part, e->w_pstride, e->w_flag));   // w = Z z, z^T w
    FEMO_COCR_SCALAR(1, nps);
    FEMO_TRY(precond(true));
    FEMO_COCR_SCALAR(2, PCG_GRID);
    hipLaunchKernelGGL(k_cocr_update, dim3(gp, L), dim3(EB), 0, st, n, x->d, e->w_r, e->w_z, e->w_p, e->w_q, mq(), e->w_ms,
                       e->w_part, e->w_pstride, e->w_flag);
    FEMO_COCR_SCALAR(3, PCG_GRID);
    return 0;
  };
#undef FEMO_COCR_SCALAR
  loop.d_scal = &femo_elast::w_ms; loop.h_scal = &femo_elast::h_ms; loop.scal_stride = CS_STRIDE;
  loop.s_res = CS_RES; loop.s_rhs = CS_BETA1; loop.squared = false;
  return femo_elast_krylov_loop(e, b, x, opts, info, loop);
}

}  // namespace

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_cdyn_apply_multi(femo_elast* e, int masked, int conj, int n_cols, const double* shifts, const double* ck,
                                const double* cm, double a, const femo_vec* x, double b, const femo_vec* f, femo_vec* y) {
  FEMO_REQUIRE(e && shifts && ck && cm && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= CMC, "femo_elast_cdyn_apply_multi: %d complex columns (1 to %d)", n_cols, CMC);
  FEMO_REQUIRE(e->assembled, "femo_elast_cdyn_apply_multi: assemble K first");
  FEMO_REQUIRE(e->mass_assembled, "femo_elast_cdyn_apply_multi: assemble M first (femo_elast_mass_assemble)");
  const int64_t n = e->mesh->n_vert * e->d * 2 * n_cols;
  FEMO_REQUIRE(x->n >= n && y->n >= n && (!f || f->n >= n),
               "vector size mismatch in femo_elast_cdyn_apply_multi: %d complex columns need %lld entries", n_cols, (long long)n);
  FEMO_REQUIRE(!masked || e->has_fixed, "femo_elast_cdyn_apply_multi: masked product without a fixed set");
  FEMO_REQUIRE(x != y, "femo_elast_cdyn_apply_multi: x and y must differ");
  Damping z;
  FEMO_REQUIRE(damping_ok(n_cols, conj, shifts, ck, cm, z),
               "femo_elast_cdyn_apply_multi: the shifts omega^2 and the damping coefficients must be finite and >= 0");
  FEMO_TRY(femo_vec_await(x));
  if (f) FEMO_TRY(femo_vec_await(f));
  femo_vec_touch(y);
  return cdyn_spmv(e, masked != 0, n_cols, z, a, x->d, b, f ? f->d : nullptr, y->d, nullptr, 0, nullptr);
}

int femo_elast_cdyn_solve_multi(femo_elast* e, int conj, int n_cols, const double* shifts, const double* ck, const double* cm,
                                const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info) {
  FEMO_REQUIRE(e && shifts && ck && cm && b && x && opts, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= CMC, "femo_elast_cdyn_solve_multi: %d complex columns (1 to %d)", n_cols, CMC);
  FEMO_REQUIRE(e->assembled, "femo_elast_cdyn_solve_multi: assemble K first");
  FEMO_REQUIRE(e->mass_assembled, "femo_elast_cdyn_solve_multi: assemble M first (femo_elast_mass_assemble)");
  const int64_t n = e->mesh->n_vert * e->d * 2 * n_cols;
  FEMO_REQUIRE(b->n >= n && x->n >= n && b != x,
               "vector size mismatch in femo_elast_cdyn_solve_multi: %d complex columns need %lld entries", n_cols, (long long)n);
  Damping z;
  FEMO_REQUIRE(damping_ok(n_cols, conj, shifts, ck, cm, z),
               "femo_elast_cdyn_solve_multi: the shifts omega^2 and the damping coefficients must be finite and >= 0");
  return cocr_solve(e, n_cols, z, b, x, opts, info, "femo_elast_cdyn_solve_multi");
}

}  // extern "C"
