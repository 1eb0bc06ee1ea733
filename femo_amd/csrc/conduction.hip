// Heat conduction with a penalised conductivity, the second physics of the SIMP track (C-ABI in include/femo_hip.h,
// "Heat conduction"; tests/thermal_ref.py restates it with SciPy):
//   K_theta(rho) = sum_c k(rho_c) |T_c| grad phi_a . grad phi_b,   k(rho) = k_min + (k_0 - k_min) C(rho),
// C the SIMP or RAMP law of the elasticity, on the mesh's scalar SELL pattern in a femo_mat.
//
// Layout.  k_cond_assemble is k_pde_assemble (pde_filter.hip) with the cell's conductivity in place of rt^2 and no mass:
// vertex-centric on the shared visit walk, the thread of row v zeroes its slots, walks its cells in ascending order and adds
// k_c |T_c| g_a . g_b, formed from `conn` in the cell's own vertex order with explicit fma in ascending k, contraction off.  No
// float atomics.  Entry (v, w) and entry (w, v) see the same cells in the same order and the same products, so K_theta is
// symmetric bit for bit and has the same bits on every build.  With a Dirichlet set the same launch writes a second matrix,
// the eliminated one: zero rows and columns and a unit diagonal on the fixed vertices; it records its identity rows as
// note_pinned_vertices (api.hip) does, so femo_solve_cg solves them up front as it does for Poisson.  bpx_ok stays false: the
// solve is the Jacobi-scaled femo_solve_cg (an auxiliary-lattice preconditioner for this operator is out of scope).
//
// The two density products are exact transposes in exact arithmetic:
//   forward  (dR/drho d)_v = sum_{c around v} k'(rho_c) d_c |T_c| grad phi_v . grad T_c     vertex walk, cells ascending
//   reverse  y_c = k'(rho_c) |T_c| grad x_c . grad T_c                                        one thread per cell
//
// Non-finite input: a NaN or an infinity in rho reaches the diagonal of its vertices, the Jacobi norm of the right-hand side
// is then non-finite, which the solve reports before it iterates; the call is refused.  A non-finite right-hand side is
// refused the same way.  The handle keeps no state of a refused call.
#include <cmath>

#include "elast_internal.h"

struct femo_cond {
  femo_ctx* ctx = nullptr;
  femo_mesh* mesh = nullptr;
  femo_mat* K = nullptr;        // plain: the residual and the lifting
  femo_mat* A = nullptr;        // eliminated with the Dirichlet set of the last assembly (valid when has_fixed)
  bool assembled = false, has_fixed = false;
  femo_solve_info last = {};
};

namespace {

__device__ __forceinline__ double conductivity(int method, double k0, double kmin, double r) {
  return kmin + (k0 - kmin) * penal(method, r);
}

// fixed != null: valsA / diagA receive the eliminated matrix beside the plain one
template <int D>
__global__ __launch_bounds__(EB) void k_cond_assemble(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell,
    const uint32_t* __restrict__ visit_slots, const int64_t* __restrict__ mptr, const int32_t* __restrict__ rowlen,
    const int32_t* __restrict__ conn, const double* __restrict__ x, int method, double k0, double kmin,
    const double* __restrict__ rho, const uint8_t* __restrict__ fixed, double* __restrict__ vals, double* __restrict__ diag,
    double* __restrict__ valsA, double* __restrict__ diagA) {
#pragma clang fp contract(off)
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t slice = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t mb = mptr[slice];
  const int len = rowlen[row];
  for (int k = 0; k < len; ++k) {
    vals[femo_sell_index(mb, k, lane)] = 0.0;
    if (fixed) valsA[femo_sell_index(mb, k, lane)] = 0.0;
  }
  const bool own_fixed = fixed && fixed[row];
  double dg = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    const uint32_t sl = visit_slots[t.vi];
    const int a = t.a;
    int32_t v[D + 1];
    double p[D + 1][D], g[D + 1][D], vol;
    load_cell<D>(conn, x, t.c, v, p);
    simplex_grads<D>(p, g, vol);
    // g_a by selection: a run-time index would send g through scratch memory
    double ga[D];
#pragma unroll
    for (int k = 0; k < D; ++k) ga[k] = g[0][k];
#pragma unroll
    for (int b = 1; b <= D; ++b)
      if (a == b) {
#pragma unroll
        for (int k = 0; k < D; ++k) ga[k] = g[b][k];
      }
    const double kk = conductivity(method, k0, kmin, rho[t.c]) * vol;
#pragma unroll
    for (int b = 0; b <= D; ++b) {
      double gab = ga[0] * g[b][0];
#pragma unroll
      for (int k = 1; k < D; ++k) gab = fma(ga[k], g[b][k], gab);
      const double stiff = kk * gab;
      if (b == a) dg += stiff;
      else {
        const int64_t e = femo_sell_index(mb, slot_pos(sl, a, b), lane);
        vals[e] += stiff;
        if (fixed && !own_fixed && !fixed[v[b]]) valsA[e] += stiff;
      }
    }
  }
  diag[row] = dg;
  if (fixed) diagA[row] = own_fixed ? 1.0 : dg;
}

// forward: y_v = (accumulate ? y_v : 0) + a sum_c k'(rho_c) d_c |T_c| g_v . grad T_c
template <int D>
__global__ __launch_bounds__(EB) void k_cond_drho_N(int64_t n_rows, const int64_t* __restrict__ vptr,
                                                    const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
                                                    const double* __restrict__ xv, int method, double dk,
                                                    const double* __restrict__ rho, const double* __restrict__ T,
                                                    const double* __restrict__ dr, double a, double* __restrict__ y,
                                                    int accumulate) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  double acc = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    int32_t v[D + 1];
    double p[D + 1][D], g[D + 1][D], vol;
    load_cell<D>(conn, xv, t.c, v, p);
    simplex_grads<D>(p, g, vol);
    double ga[D];
#pragma unroll
    for (int k = 0; k < D; ++k) ga[k] = g[0][k];
#pragma unroll
    for (int b = 1; b <= D; ++b)
      if (t.a == b) {
#pragma unroll
        for (int k = 0; k < D; ++k) ga[k] = g[b][k];
      }
    double gT[D];
#pragma unroll
    for (int k = 0; k < D; ++k) gT[k] = 0.0;
#pragma unroll
    for (int b = 0; b <= D; ++b) {
      const double Tb = T[v[b]];
#pragma unroll
      for (int k = 0; k < D; ++k) gT[k] += g[b][k] * Tb;
    }
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) dot += ga[k] * gT[k];
    acc += (dk * penal_d(method, rho[t.c])) * dr[t.c] * vol * dot;
  }
  const double val = a * acc;
  y[row] = accumulate ? y[row] + val : val;
}

// reverse: y_c = (accumulate ? y_c : 0) + a k'(rho_c) |T_c| grad x_c . grad T_c
template <int D>
__global__ __launch_bounds__(EB) void k_cond_drho_T(int64_t n_cell, const int32_t* __restrict__ conn, const double* __restrict__ xv,
                                                    int method, double dk, const double* __restrict__ rho,
                                                    const double* __restrict__ T, const double* __restrict__ x, double a,
                                                    double* __restrict__ y, int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= n_cell) return;
  const ElastCell<D> K = elast_cell<D>(conn, xv, c);
  double gT[D], gx[D];
#pragma unroll
  for (int k = 0; k < D; ++k) gT[k] = gx[k] = 0.0;
#pragma unroll
  for (int b = 0; b <= D; ++b) {
    const double Tb = T[K.v[b]], xb = x[K.v[b]];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      gT[k] += K.g[b][k] * Tb;
      gx[k] += K.g[b][k] * xb;
    }
  }
  double dot = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) dot += gx[k] * gT[k];
  const double val = a * ((dk * penal_d(method, rho[c])) * K.vol * dot);
  y[c] = accumulate ? y[c] + val : val;
}

// the lifted right-hand side: b = g on the fixed vertices, q - (K g) elsewhere (kg == null: g = 0 off the set, b = q there)
__global__ __launch_bounds__(EB) void k_cond_lift(int64_t n, const uint8_t* __restrict__ fixed, const double* __restrict__ q,
                                                  const double* __restrict__ g, const double* __restrict__ kg,
                                                  double* __restrict__ b) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  if (fixed[i]) b[i] = g ? g[i] : 0.0;
  else b[i] = kg ? q[i] - kg[i] : q[i];
}

bool cond_method_ok(int method) { return method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP; }

bool cond_law_ok(double k0, double kmin) { return std::isfinite(k0) && std::isfinite(kmin) && kmin >= 0.0 && k0 > kmin; }

void cond_mark(femo_mat* A) {
  A->valsT_valid = false; A->scaled_valid = false; A->s_valid = false; femo_mat_touch(A);
  A->bpx_ok = false;
}

}  // namespace

extern "C" int femo_cond_destroy(femo_cond* c) {
  if (!c) return 0;
  femo_mat_destroy(c->K);
  femo_mat_destroy(c->A);
  delete c;
  return 0;
}

extern "C" int femo_cond_create(femo_mesh* mesh, femo_cond** out) {
  FEMO_REQUIRE(mesh && out, "null argument");
  *out = nullptr;
  FEMO_REQUIRE(mesh->tdim == 2 || mesh->tdim == 3, "conduction: a mesh of triangles or tetrahedra is needed (tdim = %d)", mesh->tdim);
  FEMO_REQUIRE(mesh->ctx->nranks == 1 && mesh->n_nbr == 0 && mesh->n_rows == mesh->n_vert,
               "conduction: one rank only (partitioned meshes are out of scope)");
  FEMO_REQUIRE(mesh->n_cell >= 1 && mesh->n_rows >= 1, "conduction: the mesh has no cells");
  femo_cond* c = new femo_cond;
  c->ctx = mesh->ctx; c->mesh = mesh;
  int rc;
  if ((rc = femo_mat_create(mesh, &c->K)) || (rc = femo_mat_create(mesh, &c->A))) {
    femo_cond_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

extern "C" int femo_cond_assemble(femo_cond* c, int method, double k0, double k_min, const femo_vec* rho, const femo_bc* bc) {
  FEMO_REQUIRE(c && rho, "null argument");
  FEMO_REQUIRE(cond_method_ok(method), "conduction: unknown method %d", method);
  FEMO_REQUIRE(cond_law_ok(k0, k_min), "conduction: k0 = %g, k_min = %g: finite values with 0 <= k_min < k0 are needed", k0, k_min);
  femo_mesh* m = c->mesh;
  FEMO_REQUIRE(rho->n >= m->n_cell, "conduction: the density is shorter than n_cell");
  FEMO_REQUIRE(bc == nullptr || bc->mesh == m, "conduction: the Dirichlet set belongs to another mesh");
  FEMO_TRY(femo_vec_await(rho));
  const bool fx = bc != nullptr && bc->n > 0;
  cond_mark(c->K);
  c->K->has_idrows = false;
  if (fx) {
    femo_mat* A = c->A;
    cond_mark(A);
    if (A->idrows_uid != bc->uid) {
      const int64_t nb = std::max<int64_t>(m->n_vert, 1) + 64;
      if (!A->d_idrows) FEMO_HIP_CHECK(hipMalloc(&A->d_idrows, nb));
      FEMO_HIP_CHECK(hipMemcpyAsync(A->d_idrows, bc->d_mask, nb, hipMemcpyDeviceToDevice, m->ctx->stream));
      A->idrows_uid = bc->uid;
    }
    A->has_idrows = true;
  }
  c->has_fixed = fx;
  c->assembled = false;
  const dim3 g(grid_of(m->n_rows)), b(EB);
#define COND_ASM(DIM)                                                                                                          \
  hipLaunchKernelGGL((k_cond_assemble<DIM>), g, b, 0, c->ctx->stream, m->n_rows, m->d_vptr, m->d_visit_cell, m->d_visit_slots, \
                     m->d_mptr, m->d_rowlen, m->d_conn, m->d_x, method, k0, k_min, rho->d,                                     \
                     fx ? (const uint8_t*)c->A->d_idrows : (const uint8_t*)nullptr, c->K->d_vals, c->K->d_diag,                \
                     fx ? c->A->d_vals : (double*)nullptr, fx ? c->A->d_diag : (double*)nullptr)
  if (m->tdim == 2) COND_ASM(2); else COND_ASM(3);
#undef COND_ASM
  FEMO_HIP_CHECK(hipGetLastError());
  c->assembled = true;
  return 0;
}

extern "C" int femo_cond_apply(femo_cond* c, int eliminated, const femo_vec* x, femo_vec* y) {
  FEMO_REQUIRE(c && x && y, "null argument");
  FEMO_REQUIRE(c->assembled, "conduction: apply before femo_cond_assemble");
  FEMO_REQUIRE(!eliminated || c->has_fixed, "conduction: the eliminated operator needs a Dirichlet set at the assembly");
  FEMO_REQUIRE(x->n >= c->mesh->n_vert && y->n >= c->mesh->n_rows && x != y, "conduction: vector size mismatch or aliasing in apply");
  return femo_mat_spmv(eliminated ? c->A : c->K, 0, x, y);
}

extern "C" int femo_cond_lift(femo_cond* c, const femo_vec* q, const femo_vec* g, femo_vec* work, femo_vec* b) {
  FEMO_REQUIRE(c && q && b, "null argument");
  FEMO_REQUIRE(c->assembled && c->has_fixed, "conduction: the lifting needs an assembly with a Dirichlet set");
  femo_mesh* m = c->mesh;
  FEMO_REQUIRE(q->n >= m->n_rows && b->n >= m->n_rows && (!g || (g->n >= m->n_vert && work && work->n >= m->n_rows)),
               "conduction: vector size mismatch in lift (values g need a work vector)");
  FEMO_REQUIRE(!g || (b != g && b != work && work != g && work != q), "conduction: lift: a vector aliases another");
  FEMO_TRY(femo_vec_await(q));
  if (g) FEMO_TRY(femo_mat_spmv(c->K, 0, g, work));
  femo_vec_touch(b);
  hipLaunchKernelGGL(k_cond_lift, dim3(grid_of(m->n_rows)), dim3(EB), 0, c->ctx->stream, m->n_rows, (const uint8_t*)c->A->d_idrows, q->d,
                     g ? g->d : (const double*)nullptr, g ? work->d : (const double*)nullptr, b->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int femo_cond_solve(femo_cond* c, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info) {
  FEMO_REQUIRE(c && b && x, "null argument");
  FEMO_REQUIRE(c->assembled, "conduction: solve before femo_cond_assemble");
  FEMO_REQUIRE(b->n >= c->mesh->n_rows && x->n >= c->mesh->n_vert && b != x, "conduction: vector size mismatch or aliasing in solve");
  femo_solver_opts o = {};
  if (opts) o = *opts;
  else { o.rtol = 1e-13; o.check_every = 8; o.zero_guess = 1; }
  FEMO_REQUIRE(o.pc == FEMO_PC_JACOBI, "conduction: the solve is Jacobi-preconditioned CG (pc = %d)", o.pc);
  FEMO_REQUIRE(std::isfinite(o.rtol) && o.rtol >= 0.0 && std::isfinite(o.atol) && o.atol >= 0.0, "conduction: bad tolerances");
  femo_solve_info si = {};
  FEMO_TRY(femo_solve_cg(c->has_fixed ? c->A : c->K, 0, b, x, &o, &si));
  c->last = si;
  if (info) *info = si;
  FEMO_REQUIRE(std::isfinite(si.rhs_norm) && si.converged != -1,
               "conduction: the density or the right-hand side is not finite (load norm %g after %d iterations)", si.rhs_norm,
               (int)si.iterations);
  return 0;
}

extern "C" int femo_cond_drho(femo_cond* c, int method, double k0, double k_min, int transpose, double a, const femo_vec* rho,
                              const femo_vec* T, const femo_vec* x, femo_vec* y, int accumulate) {
  FEMO_REQUIRE(c && rho && T && x && y, "null argument");
  FEMO_REQUIRE(cond_method_ok(method), "conduction: unknown method %d", method);
  FEMO_REQUIRE(cond_law_ok(k0, k_min), "conduction: k0 = %g, k_min = %g: finite values with 0 <= k_min < k0 are needed", k0, k_min);
  femo_mesh* m = c->mesh;
  FEMO_REQUIRE(rho->n >= m->n_cell && T->n >= m->n_vert &&
                   (transpose ? (x->n >= m->n_vert && y->n >= m->n_cell) : (x->n >= m->n_cell && y->n >= m->n_rows)),
               "conduction: vector size mismatch in drho");
  FEMO_REQUIRE(y != x && y != rho && y != T, "conduction: drho: output aliases an input");
  FEMO_TRY(femo_vec_await(rho));
  FEMO_TRY(femo_vec_await(T));
  FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(y);
  const double dk = k0 - k_min;
  hipStream_t st = c->ctx->stream;
  if (transpose) {
    const dim3 g(grid_of(m->n_cell)), b(EB);
    if (m->tdim == 2) hipLaunchKernelGGL(k_cond_drho_T<2>, g, b, 0, st, m->n_cell, m->d_conn, m->d_x, method, dk, rho->d, T->d, x->d, a, y->d, accumulate);
    else hipLaunchKernelGGL(k_cond_drho_T<3>, g, b, 0, st, m->n_cell, m->d_conn, m->d_x, method, dk, rho->d, T->d, x->d, a, y->d, accumulate);
  } else {
    const dim3 g(grid_of(m->n_rows)), b(EB);
    if (m->tdim == 2) hipLaunchKernelGGL(k_cond_drho_N<2>, g, b, 0, st, m->n_rows, m->d_vptr, m->d_visit_cell, m->d_conn, m->d_x, method, dk, rho->d, T->d, x->d, a, y->d, accumulate);
    else hipLaunchKernelGGL(k_cond_drho_N<3>, g, b, 0, st, m->n_rows, m->d_vptr, m->d_visit_cell, m->d_conn, m->d_x, method, dk, rho->d, T->d, x->d, a, y->d, accumulate);
  }
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

extern "C" int femo_cond_export_csr(const femo_cond* c, int eliminated, int64_t* rowptr, int32_t* col, double* val) {
  FEMO_REQUIRE(c, "null argument");
  FEMO_REQUIRE(c->assembled, "conduction: export before femo_cond_assemble");
  FEMO_REQUIRE(!eliminated || c->has_fixed, "conduction: the eliminated operator needs a Dirichlet set at the assembly");
  return femo_mat_export_csr(eliminated ? c->A : c->K, rowptr, col, val);
}
