// Block product and PCG of the SIMP elasticity, for one right-hand side or several load cases in one batched loop (C-ABI in
// include/femo_hip.h: femo_elast_solve, femo_elast_solve_multi, femo_elast_apply_multi; femo_elast_spmv serves the rest).
//
// Layout.  L columns (1 <= L <= FEMO_ELAST_MAX_COLS) one after the other in one vector: column l starts at l * n_dof and
// keeps the blocked layout d * vertex + component.  K(rho), the fixed set and the preconditioner are shared.  The
// single-column entry points are this loop with L = 1.
//
// An iteration issues these launches, each with a column dimension in its grid:
//
//   q_l = A p_l, partial p_l.q_l       k_elast_spmv_multi   up to MC columns per thread: a d x d block, its column index
//                                                           and the fixed bytes are read once for them (elast_row_walk);
//                                                           pass blockIdx.y covers columns MC * blockIdx.y ...  One column
//                                                           runs the MC = 1 instantiation, several run ELAST_CHUNK
//   alpha_l                            k_pcg_scalar         one workgroup per column
//   x, r update, z_l = M^-1 r_l        k_pcg_precond, or the four launches of femo_elast_pc_step
//   beta_l, convergence of column l    k_pcg_scalar
//   p_l = z_l + beta_l p_l             k_pcg_p
//
// Column l owns s[] at s + l * EMS_STRIDE, flag[] at flag + l * EMF_STRIDE and its own slab of partials.  Once flag[0] of
// a column is set (converged, breakdown, or the stopping test met at iteration 0) every block of that column returns
// early, so its x, r and p are never written again and a stale alpha does no harm.  Within a column every sum runs in the
// same order whatever L is: no float atomics, the same bits on every call.
//
// The host side of the loop -- reserve, start, bursts of iterations between polls of the flags, read-back -- is
// femo_elast_krylov_loop, which the MINRES of elast_harm.hip and the COCR of elast_damp.hip run as well.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

// y_l = a Op x_l + b f_l (+ partial dot(x_l, y_l) per block and column when part != null) for the columns
// c0 = MC * blockIdx.y ... min(c0 + MC, n_cols) - 1.  done != null: a column whose done[l * EMF_STRIDE] is set is skipped.
// vs: column stride of the vectors, ps: of the partials.
template <int D, bool MASKED, int MC>
__global__ __launch_bounds__(EB) void k_elast_spmv_multi(
    int64_t n_rows, const int64_t* __restrict__ mptr, const int32_t* __restrict__ cols, const int32_t* __restrict__ rowlen,
    const double* __restrict__ vals, const double* __restrict__ diag, const uint8_t* __restrict__ fixed, int n_cols, int64_t vs,
    double a, const double* __restrict__ x, double b, const double* __restrict__ f, double* __restrict__ y,
    double* __restrict__ part, int64_t ps, const int32_t* __restrict__ done) {
  __shared__ double lds[EB / 64];
  const int c0 = (int)blockIdx.y * MC;
  bool on[MC];          // uniform over the block
  bool any = false;
#pragma unroll
  for (int c = 0; c < MC; ++c) {
    on[c] = c0 + c < n_cols && !(done && done[(c0 + c) * EMF_STRIDE]);
    any = any || on[c];
  }
  if (!any) return;
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  double dotv[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) dotv[c] = 0.0;
  if (row < n_rows) {
    ElastRowIn<MC> in;
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      in.x[c] = x + (c0 + c) * vs;
      in.on[c] = on[c];
    }
    const auto w = elast_row_walk<D, MASKED, MC, false>(row, mptr, cols, rowlen, vals, diag, fixed, nullptr, nullptr, in);
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      if (!on[c]) continue;
#pragma unroll
      for (int r = 0; r < D; ++r) {
        double o = MASKED && w.fo[r] ? w.xo[c][r] : w.acc[c][r];
        o = a * o;
        if (f) o += b * f[(c0 + c) * vs + row * D + r];
        y[(c0 + c) * vs + row * D + r] = o;
        dotv[c] += w.xo[c][r] * o;
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

// ------------------------------------------------------------------------------------------------ PCG ----
// Device scalars s[] and flag[]: elast_internal.h.  blockIdx.y (k_pcg_scalar: blockIdx.x) is the column.
__global__ void k_pcg_start_x(int64_t n, int zero_guess, const uint8_t* __restrict__ fixed, const double* __restrict__ b,
                              double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  b += blockIdx.y * n; x += blockIdx.y * n;
  double v = zero_guess ? 0.0 : x[i];
  if (fixed && fixed[i]) v = b[i];
  x[i] = v;
}

// z = Dinv r (block), optional x += alpha p, r -= alpha q first; partial r.z per block; INIT: p = z as well
template <int D, bool UPDATE, bool INIT>
__global__ __launch_bounds__(EB) void k_pcg_precond(int64_t n_rows, const double* __restrict__ dinv, double* __restrict__ x,
                                                    double* __restrict__ r, const double* __restrict__ p,
                                                    const double* __restrict__ q, double* __restrict__ z,
                                                    double* __restrict__ pinit, const double* __restrict__ s,
                                                    double* __restrict__ part, int64_t ps, const int32_t* __restrict__ flag) {
  constexpr int DD = D * D;
  __shared__ double lds[EB / 64];
  flag += blockIdx.y * EMF_STRIDE;
  s += blockIdx.y * EMS_STRIDE;
  if (UPDATE && flag[0]) return;
  const int64_t colv = (int64_t)blockIdx.y * n_rows * D;
  x += colv; r += colv; p += colv; q += colv; z += colv; part += blockIdx.y * ps;
  if (INIT) pinit += colv;
  double dotv = 0.0;
  const double alpha = UPDATE ? s[S_ALPHA] : 0.0;
  for (int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * EB) {
    double rr[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int64_t o = row * D + i;
      double ri = r[o];
      if (UPDATE) {
        x[o] += alpha * p[o];
        ri -= alpha * q[o];
        r[o] = ri;
      }
      rr[i] = ri;
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double zi = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) zi += dinv[row * DD + i * D + k] * rr[k];
      z[row * D + i] = zi;
      if (INIT) pinit[row * D + i] = zi;
      dotv += rr[i] * zi;
    }
  }
  const double t = femo_block_sum<EB>(dotv, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// mode 0: initial rz.  mode 1: alpha = rz / pq.  mode 2: rz' -> beta, convergence.  One workgroup per column.
__global__ __launch_bounds__(1024) void k_pcg_scalar(int mode, const double* __restrict__ part, int64_t ps, int np,
                                                     double rtol2, double atol2, int max_it, double* __restrict__ s,
                                                     int32_t* __restrict__ flag) {
  __shared__ double lds[16];
  part += blockIdx.x * ps;
  s += blockIdx.x * EMS_STRIDE;
  flag += blockIdx.x * EMF_STRIDE;
  if (mode != 0 && flag[0]) return;
  const double v = femo_fold_partials<1024>(part, np, lds);
  if (threadIdx.x != 0) return;
  if (mode == 0) {
    s[S_RZ] = v; s[S_RZ0] = v;
    const double tol2 = fmax(rtol2 * v, atol2);
    s[S_TOL2] = tol2;
    flag[0] = 0; flag[1] = 0; flag[2] = 0; flag[3] = 0;
    if (!(v == v)) { flag[0] = 1; flag[2] = 1; }
    else if (v <= tol2) { flag[0] = 1; flag[3] = 1; }
  } else if (mode == 1) {
    if (!(v > 0.0) || !(v == v)) { flag[0] = 1; flag[2] = 1; return; }
    s[S_ALPHA] = s[S_RZ] / v;
  } else {
    flag[1] += 1;
    if (!(v == v)) { flag[0] = 1; flag[2] = 1; return; }
    s[S_BETA] = v / s[S_RZ];
    s[S_RZ] = v;
    if (v <= s[S_TOL2]) { flag[0] = 1; flag[3] = 1; }
    else if (flag[1] >= max_it) flag[0] = 1;
  }
}

__global__ void k_pcg_p(int64_t n, const double* __restrict__ z, double* __restrict__ p, const double* __restrict__ s,
                        const int32_t* __restrict__ flag) {
  if (flag[blockIdx.y * EMF_STRIDE]) return;
  const double beta = s[blockIdx.y * EMS_STRIDE + S_BETA];
  z += blockIdx.y * n; p += blockIdx.y * n;
  for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n; i += (int64_t)gridDim.x * EB) p[i] = z[i] + beta * p[i];
}

// the PCG of femo_elast_solve (one column) and femo_elast_solve_multi, which have checked their arguments; who: the entry
// point, for the error texts.  info: n_cols records, or null.
// op: K (null), or K + sigma M with its own inverse diagonal blocks for the Jacobi term.
int pcg_solve(femo_elast* e, int n_cols, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info,
              const char* who, const femo_elast_op* op = nullptr) {
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d;
  const bool ml = opts->pc == FEMO_ELAST_PC_MULTILEVEL;
  hipStream_t st = m->ctx->stream;
  const uint8_t* fx = e->has_fixed ? e->d_fixed : nullptr;
  const double rtol2 = opts->rtol * opts->rtol, atol2 = opts->atol * opts->atol;
  const int nps = (int)grid_of(m->n_rows);
  const unsigned L = (unsigned)n_cols, gp = (unsigned)PCG_GRID;
  const double* dinv = op ? op->dinv : e->d_dinv;
  // y = a A x + b f of the chosen operator: the block product of K, or the shifted product with the shift -sigma
  auto product = [&](double a, const double* xx, double bb, const double* f, double* y, double* part, const int32_t* done) -> int {
    if (op) return femo_elast_dyn_spmv(e, fx != nullptr, n_cols, -op->sigma, a, xx, bb, f, y, part, e->w_pstride, done);
    return femo_elast_spmv(e, fx != nullptr, n_cols, a, xx, bb, f, y, part, e->w_pstride, done);
  };
#define FEMO_PRECOND(D, U, I) hipLaunchKernelGGL((k_pcg_precond<D, U, I>), dim3(gp, L), dim3(EB), 0, st, m->n_rows, dinv, x->d, \
                                                 e->w_r, e->w_p, e->w_q, e->w_z, e->w_p, e->w_s, e->w_part, e->w_pstride, e->w_flag)
#define FEMO_PCG_SCALAR(MODE, NP) hipLaunchKernelGGL(k_pcg_scalar, dim3(L), dim3(1024), 0, st, MODE, e->w_part, e->w_pstride, NP, \
                                                     rtol2, atol2, max_it, e->w_s, e->w_flag)
  femo_elast_krylov loop = {who, n_cols, n_cols, 1, false};
  loop.start = [&](int max_it) -> int {
    hipLaunchKernelGGL(k_pcg_start_x, dim3(grid_of(n), L), dim3(EB), 0, st, n, opts->zero_guess, fx, b->d, x->d);
    FEMO_TRY(product(-1.0, x->d, 1.0, b->d, e->w_r, nullptr, nullptr));                                         // r = b - A x
    if (ml) FEMO_TRY(femo_elast_pc_step(e, false, n_cols, x->d, e->w_r, e->w_p, e->w_q, e->w_z, e->w_p, e->w_s, e->w_part, e->w_pstride, e->w_flag, dinv));
    else if (e->d == 2) FEMO_PRECOND(2, false, true); else FEMO_PRECOND(3, false, true);
    FEMO_PCG_SCALAR(0, PCG_GRID);
    return 0;
  };
  loop.iterate = [&](int, int max_it) -> int {
    FEMO_TRY(product(1.0, e->w_p, 0.0, nullptr, e->w_q, e->w_part, e->w_flag));                                 // q = A p, p.q
    FEMO_PCG_SCALAR(1, nps);
    if (ml) FEMO_TRY(femo_elast_pc_step(e, true, n_cols, x->d, e->w_r, e->w_p, e->w_q, e->w_z, nullptr, e->w_s, e->w_part, e->w_pstride, e->w_flag, dinv));
    else if (e->d == 2) FEMO_PRECOND(2, true, false); else FEMO_PRECOND(3, true, false);
    FEMO_PCG_SCALAR(2, PCG_GRID);
    hipLaunchKernelGGL(k_pcg_p, dim3(gp, L), dim3(EB), 0, st, n, e->w_z, e->w_p, e->w_s, e->w_flag);
    return 0;
  };
#undef FEMO_PRECOND
#undef FEMO_PCG_SCALAR
  loop.d_scal = &femo_elast::w_s; loop.h_scal = &femo_elast::h_s; loop.scal_stride = EMS_STRIDE;
  loop.s_res = S_RZ; loop.s_rhs = S_RZ0; loop.squared = true;                                                   // r.z of the last and the first residual
  return femo_elast_krylov_loop(e, b, x, opts, info, loop);
}

// the product of femo_elast_apply (one column) and femo_elast_apply_multi, which have checked their arguments
int apply_cols(femo_elast* e, int masked, int n_cols, double a, const femo_vec* x, double b, const femo_vec* f, femo_vec* y) {
  FEMO_TRY(femo_vec_await(x));
  if (f) FEMO_TRY(femo_vec_await(f));
  femo_vec_touch(y);
  return femo_elast_spmv(e, masked != 0, n_cols, a, x->d, b, f ? f->d : nullptr, y->d, nullptr, 0, nullptr);
}

}  // namespace

int femo_elast_spmv(femo_elast* e, bool masked, int n_cols, double a, const double* x, double b, const double* f, double* y,
                    double* part, int64_t part_stride, const int32_t* done) {
  femo_mesh* m = e->mesh;
  // one column: the MC = 1 instantiation, which carries no accumulators of absent columns
  const int mc = n_cols == 1 ? 1 : ELAST_CHUNK;
  elast_dispatch(e->d, masked, [&](auto dim, auto mask) {
    constexpr int D = decltype(dim)::value;
    constexpr bool MASKED = decltype(mask)::value;
    auto* kernel = n_cols == 1 ? k_elast_spmv_multi<D, MASKED, 1> : k_elast_spmv_multi<D, MASKED, ELAST_CHUNK>;
    hipLaunchKernelGGL(kernel, dim3(grid_of(m->n_rows), (unsigned)((n_cols + mc - 1) / mc)), dim3(EB), 0, m->ctx->stream, m->n_rows,
                       m->d_mptr, m->d_cols, m->d_rowlen, e->d_vals, e->d_diag, e->d_fixed, n_cols, m->n_rows * D, a, x, b, f, y,
                       part, part_stride, done);
  });
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_elast_krylov_loop(femo_elast* e, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info,
                           const femo_elast_krylov& loop) {
  femo_mesh* m = e->mesh;
  const bool ml = opts->pc == FEMO_ELAST_PC_MULTILEVEL;
  FEMO_REQUIRE(!ml || e->pc, "%s: pc = multilevel without femo_elast_pc_setup", loop.who);
  FEMO_TRY(femo_vec_await(b));
  femo_vec_touch(x);
  hipStream_t st = m->ctx->stream;
  if (ml) FEMO_TRY(femo_elast_pc_ensure(e));
  FEMO_TRY(femo_elast_work_reserve(e, loop.real_cols, loop.who));
  if (loop.harm) FEMO_TRY(femo_elast_harm_reserve(e, loop.real_cols, loop.who));
  const int check = opts->check_every > 0 ? opts->check_every : (ml ? 8 : 32);
  const int max_it = opts->max_it > 0 ? opts->max_it : 100000;
  hipEvent_t e0 = m->ctx->ev0, e1 = m->ctx->ev1;
  FEMO_HIP_CHECK(hipEventRecord(e0, st));
  FEMO_TRY(loop.start(max_it));
  FEMO_HIP_CHECK(hipGetLastError());
  int it_issued = 0;
  for (;;) {
    FEMO_HIP_CHECK(hipMemcpyAsync(e->h_flag, e->w_flag, (size_t)loop.real_cols * EMF_STRIDE * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    bool all_done = true;
    for (int l = 0; l < loop.n_cols; ++l) all_done = all_done && e->h_flag[loop.flag_stride * l * EMF_STRIDE] != 0;
    if (all_done || it_issued >= max_it) break;
    for (int k = 0; k < check && it_issued < max_it; ++k, ++it_issued) FEMO_TRY(loop.iterate(it_issued, max_it));
    FEMO_HIP_CHECK(hipGetLastError());
  }
  FEMO_HIP_CHECK(hipEventRecord(e1, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(e->*loop.h_scal, e->*loop.d_scal, (size_t)loop.n_cols * loop.scal_stride * sizeof(double),
                                hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  if (info) {
    float ms = 0.0f;
    const bool timed = hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    for (int l = 0; l < loop.n_cols; ++l) {
      const int32_t* fl = e->h_flag + loop.flag_stride * l * EMF_STRIDE;
      const double* s = e->*loop.h_scal + l * loop.scal_stride;
      femo_solve_info* o = info + l;
      std::memset(o, 0, sizeof(*o));
      o->iterations = fl[1];
      o->converged = fl[2] ? -1 : (fl[3] ? 1 : 0);
      o->residual_norm = loop.squared ? std::sqrt(std::fabs(s[loop.s_res])) : s[loop.s_res];
      o->rhs_norm = loop.squared ? std::sqrt(std::fabs(s[loop.s_rhs])) : s[loop.s_rhs];
      o->pc_residual_norm = o->residual_norm;
      o->pc_rhs_norm = o->rhs_norm;
      if (timed) o->solve_ms = ms;
    }
  }
  return 0;
}

int femo_elast_pcg(femo_elast* e, int n_cols, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info,
                   const char* who, const femo_elast_op* op) {
  return pcg_solve(e, n_cols, b, x, opts, info, who, op);
}

int femo_elast_start_x(femo_elast* e, int n_cols, int zero_guess, const double* b, double* x) {
  const int64_t n = e->mesh->n_vert * e->d;
  hipLaunchKernelGGL(k_pcg_start_x, dim3(grid_of(n), (unsigned)n_cols), dim3(EB), 0, e->mesh->ctx->stream, n, zero_guess,
                     e->has_fixed ? e->d_fixed : nullptr, b, x);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_elast_work_reserve(femo_elast* e, int n_cols, const char* who) {
  if (e->w_cols >= n_cols) return 0;
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d, ps = std::max<int64_t>(PCG_GRID, grid_of(m->n_rows));
  double* w[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // r, z, p, q, part: the old ones stay until all five exist
  int rc = 0;
  for (int k = 0; k < 5; ++k) rc |= dalloc(&w[k], (k < 4 ? n : ps) * n_cols);
  if (rc) {
    for (double* v : w) hipFree(v);
    femo_set_error("%s: device allocation failed", who);
    return 1;
  }
  FEMO_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  hipFree(e->w_r); hipFree(e->w_z); hipFree(e->w_p); hipFree(e->w_q); hipFree(e->w_part);
  e->w_r = w[0]; e->w_z = w[1]; e->w_p = w[2]; e->w_q = w[3]; e->w_part = w[4];
  e->w_pstride = ps;
  e->w_cols = n_cols;
  return 0;
}

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_apply(femo_elast* e, int masked, double a, const femo_vec* x, double b, const femo_vec* f, femo_vec* y) {
  FEMO_REQUIRE(e && x && y, "null argument");
  FEMO_REQUIRE(e->assembled, "femo_elast_apply: assemble K first");
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(x->n >= n && y->n >= n && (!f || f->n >= n), "vector size mismatch in femo_elast_apply");
  FEMO_REQUIRE(!masked || e->has_fixed, "femo_elast_apply: masked product without a fixed set");
  FEMO_REQUIRE(x != y, "femo_elast_apply: x and y must differ");
  return apply_cols(e, masked, 1, a, x, b, f, y);
}

int femo_elast_apply_multi(femo_elast* e, int masked, int n_cols, double a, const femo_vec* x, double b, const femo_vec* f,
                           femo_vec* y) {
  FEMO_REQUIRE(e && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_apply_multi: %d columns (1 to %d)", n_cols, EMC);
  FEMO_REQUIRE(e->assembled, "femo_elast_apply_multi: assemble K first");
  const int64_t n = e->mesh->n_vert * e->d * n_cols;
  FEMO_REQUIRE(x->n >= n && y->n >= n && (!f || f->n >= n), "vector size mismatch in femo_elast_apply_multi: %d columns need %lld entries",
               n_cols, (long long)n);
  FEMO_REQUIRE(!masked || e->has_fixed, "femo_elast_apply_multi: masked product without a fixed set");
  FEMO_REQUIRE(x != y, "femo_elast_apply_multi: x and y must differ");
  return apply_cols(e, masked, n_cols, a, x, b, f, y);
}

int femo_elast_solve(femo_elast* e, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info) {
  FEMO_REQUIRE(e && b && x && opts, "null argument");
  FEMO_REQUIRE(e->assembled, "femo_elast_solve: assemble K first");
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(b->n >= n && x->n >= n && b != x, "vector size mismatch in femo_elast_solve");
  return pcg_solve(e, 1, b, x, opts, info, "femo_elast_solve");
}

int femo_elast_solve_multi(femo_elast* e, int n_cols, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts,
                           femo_solve_info* info) {
  FEMO_REQUIRE(e && b && x && opts, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_solve_multi: %d columns (1 to %d)", n_cols, EMC);
  FEMO_REQUIRE(e->assembled, "femo_elast_solve_multi: assemble K first");
  const int64_t n = e->mesh->n_vert * e->d * n_cols;
  FEMO_REQUIRE(b->n >= n && x->n >= n && b != x, "vector size mismatch in femo_elast_solve_multi: %d columns need %lld entries",
               n_cols, (long long)n);
  return pcg_solve(e, n_cols, b, x, opts, info, "femo_elast_solve_multi");
}

}  // extern "C"
