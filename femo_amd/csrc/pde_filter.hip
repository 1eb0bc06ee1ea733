// Helmholtz (PDE) density filter of Lazarov & Sigmund (2011) on the mesh's own pattern: xt = W x for a DG0 field x,
//   W = V^-1 T^T A^-1 T,   A = rt^2 L + M,   rt = r / (2 sqrt 3),
// L the P1 stiffness, M the lumped or consistent P1 mass, T[v,c] = |T_c| / (d+1), V = diag |T_c| (include/femo_hip.h,
// "Helmholtz density filter", states it; tests/pde_filter_ref.py restates it with SciPy).  W^T = V W V^-1 is the same
// pipeline with 1 / |T_c| on the way in and |T_c| on the way out: one operator, one solve path.
//
// Layout.  A is a femo_mat: k_pde_assemble fills it once per handle, vertex-centric on the shared visit walk
// (elast_visits) as k_elast_mass_assemble does -- the thread of row v zeroes its slots, walks its cells in ascending order
// and adds rt^2 |T_c| g_a . g_b plus the mass term, both formed from `conn` in the cell's own vertex order.  No float
// atomics.  Entry (v, w) and entry (w, v) see the same cells in the same order and the same products (g_a . g_b is formed
// with explicit fma in ascending k, contraction off around it), so A is symmetric bit for bit and has the same bits on
// every build.  An application is three steps, the first and the last being the arithmetic of femo_dRdf_cell_apply on a
// vector of per-cell weights, so they ARE that entry point's launches:
//   load   b_v = sum_{c around v} cv_c x_c        one writer per vertex, cells ascending (k_mul_into + k_load_walk)
//   solve  A p = b                                femo_solve_cg, Jacobi, rtol 1e-13 from the zero guess by default
//   mean   y_c = cv'_c sum_a p[v_a]               one thread per cell (k_dRdf_cell_apply_T)
// with (cv, cv') = (|T_c| / (d+1), 1 / (d+1)) for W and the two swapped for W^T.  femo_pde_filter_project (project.hip)
// replaces the mean by k_p_mean, which applies the Heaviside map to the mean in registers.
//
// Non-finite input: the load of a NaN or an infinity makes the Jacobi norm of b non-finite, which the solve reports before
// it iterates (femo_solve_info.rhs_norm); the call is then refused.  y may have been written; the handle keeps no state of a
// refused call (a warm start is dropped), so the next call gives the clean result.
#include <cmath>

#include "elast_internal.h"

namespace {

// A visit of cell c as its vertex a adds rt^2 |T_c| g_a . g_b + m_ab to the entries (a, b); m_ab = delta_ab |T_c| / (d+1)
// (LUMPED) or |T_c| (1 + delta_ab) / ((d+1)(d+2)).
template <int D, bool LUMPED>
__global__ __launch_bounds__(EB) void k_pde_assemble(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell,
    const uint32_t* __restrict__ visit_slots, const int64_t* __restrict__ mptr, const int32_t* __restrict__ rowlen,
    const int32_t* __restrict__ conn, const double* __restrict__ x, double rt2, double* __restrict__ vals,
    double* __restrict__ diag) {
#pragma clang fp contract(off)
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t slice = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t mb = mptr[slice];
  const int len = rowlen[row];
  for (int k = 0; k < len; ++k) vals[femo_sell_index(mb, k, lane)] = 0.0;
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
    const double kk = rt2 * vol;
    const double m_off = LUMPED ? 0.0 : vol * (1.0 / ((D + 1) * (D + 2)));
    const double m_own = LUMPED ? vol * (1.0 / (D + 1)) : m_off + m_off;
#pragma unroll
    for (int b = 0; b <= D; ++b) {
      double gab = ga[0] * g[b][0];
#pragma unroll
      for (int k = 1; k < D; ++k) gab = fma(ga[k], g[b][k], gab);
      const double stiff = kk * gab;
      if (b == a) dg += stiff + m_own;
      else vals[femo_sell_index(mb, slot_pos(sl, a, b), lane)] += stiff + m_off;
    }
  }
  diag[row] = dg;
}

int pde_assemble(femo_pde_filter* f) {
  femo_mesh* m = f->mesh;
  femo_mat* A = f->A;
  const double rt = f->radius / (2.0 * std::sqrt(3.0));
  const double rt2 = rt * rt;
  A->valsT_valid = false; A->scaled_valid = false; A->s_valid = false; femo_mat_touch(A);
  A->has_idrows = false; A->bpx_ok = false;
  const dim3 g(grid_of(m->n_rows)), b(EB);
  hipStream_t st = f->ctx->stream;
#define PDE_ASM(DIM, LUMPED)                                                                                                  \
  hipLaunchKernelGGL((k_pde_assemble<DIM, LUMPED>), g, b, 0, st, m->n_rows, m->d_vptr, m->d_visit_cell, m->d_visit_slots, m->d_mptr, \
                     m->d_rowlen, m->d_conn, m->d_x, rt2, A->d_vals, A->d_diag)
  if (m->tdim == 2) { if (f->lumped) PDE_ASM(2, true); else PDE_ASM(2, false); }
  else { if (f->lumped) PDE_ASM(3, true); else PDE_ASM(3, false); }
#undef PDE_ASM
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

bool pde_overlap(const femo_vec* a, const femo_vec* b, int64_t n) {
  return a == b || (a->d < b->d + n && b->d < a->d + n);
}

}  // namespace

extern "C" int femo_pde_filter_destroy(femo_pde_filter* f) {
  if (!f) return 0;
  femo_mat_destroy(f->A);
  femo_vec_destroy(f->cv_vol); femo_vec_destroy(f->cv_one); femo_vec_destroy(f->b); femo_vec_destroy(f->p); femo_vec_destroy(f->pT);
  delete f;
  return 0;
}

extern "C" int femo_pde_filter_create(femo_mesh* mesh, double radius, int lumped, femo_pde_filter** out) {
  FEMO_REQUIRE(mesh && out, "null argument");
  *out = nullptr;
  femo_ctx* ctx = mesh->ctx;
  FEMO_REQUIRE(mesh->tdim == 2 || mesh->tdim == 3, "pde_filter: a mesh of triangles or tetrahedra is needed (tdim = %d)", mesh->tdim);
  FEMO_REQUIRE(ctx->nranks == 1 && mesh->n_nbr == 0 && mesh->n_rows == mesh->n_vert,
               "pde_filter: one rank only (partitioned meshes are out of scope)");
  FEMO_REQUIRE(std::isfinite(radius) && radius > 0.0, "pde_filter: radius = %g, must be finite and > 0", radius);
  FEMO_REQUIRE(mesh->n_cell >= 1 && mesh->n_rows >= 1, "pde_filter: the mesh has no cells");
  femo_pde_filter* f = new femo_pde_filter;
  f->ctx = ctx; f->mesh = mesh; f->n = mesh->n_cell; f->radius = radius; f->lumped = lumped != 0;
  auto fail = [&](int rc) { femo_pde_filter_destroy(f); return rc; };
  int rc;
  if ((rc = femo_mat_create(mesh, &f->A)) || (rc = femo_vec_create(ctx, f->n, &f->cv_vol)) ||
      (rc = femo_vec_create(ctx, f->n, &f->cv_one)) || (rc = femo_vec_create(ctx, mesh->n_rows, &f->b)) ||
      (rc = femo_vec_create(ctx, mesh->n_vert, &f->p)) || (rc = femo_vec_create(ctx, mesh->n_vert, &f->pT)))
    return fail(rc);
  // cv_vol = |T_c| / (d+1): the compact dR/df of the Poisson forms with its sign turned; cv_one = 1 / (d+1)
  if ((rc = femo_launch_dRdf_cell(mesh, f->cv_vol->d)) || (rc = femo_launch_scale(f->cv_vol->d, -1.0, f->cv_vol->d, f->n, ctx->stream)) ||
      (rc = femo_launch_fill(f->cv_one->d, 1.0 / (mesh->tdim + 1), f->n, ctx->stream)) || (rc = pde_assemble(f)))
    return fail(rc);
  *out = f;
  return 0;
}

extern "C" int femo_pde_filter_set(femo_pde_filter* f, double rtol, int warm_start) {
  FEMO_REQUIRE(f, "null argument");
  FEMO_REQUIRE(std::isfinite(rtol) && rtol > 0.0, "pde_filter: rtol = %g, must be finite and > 0", rtol);
  f->rtol = rtol;
  f->warm_start = warm_start != 0;
  f->have_guess = false;
  return 0;
}

extern "C" int femo_pde_filter_bytes(const femo_pde_filter* f, int64_t* bytes) {
  FEMO_REQUIRE(f && bytes, "null argument");
  const femo_mesh* m = f->mesh;
  const femo_mat* A = f->A;
  const int64_t nd = m->n_slices * FEMO_WAVE, ne = m->sell_entries;
  int64_t t = 8 * (nd + ne);                                     // diagonal and values
  if (A->d_valsS) t += 8 * ne;                                   // S A S
  if (A->d_valsT) t += 8 * ne;
  if (A->d_s) t += 8 * m->n_vert;
  if (A->d_valsC) t += 8 * ne + 4 * m->n_slices * ((int64_t)m->sdelta_stride + 1);
  t += 8 * (2 * f->n + m->n_rows + 2 * m->n_vert);               // cv_vol, cv_one, b, p, pT
  *bytes = t;
  return 0;
}

extern "C" int femo_pde_filter_export_csr(const femo_pde_filter* f, int64_t* rowptr, int32_t* col, double* val) {
  FEMO_REQUIRE(f, "null argument");
  return femo_mat_export_csr(f->A, rowptr, col, val);
}

int femo_pde_filter_nodal(femo_pde_filter* f, int transpose, const femo_vec* x, const femo_solver_opts* opts,
                          femo_solve_info* info, const femo_vec** nodal) {
  femo_mesh* m = f->mesh;
  femo_solver_opts o = {};
  if (opts) o = *opts;
  else { o.rtol = f->rtol; o.check_every = 8; }
  FEMO_REQUIRE(o.pc == FEMO_PC_JACOBI, "pde_filter: the solve is Jacobi-preconditioned CG (pc = %d)", o.pc);
  FEMO_REQUIRE(std::isfinite(o.rtol) && o.rtol >= 0.0 && std::isfinite(o.atol) && o.atol >= 0.0, "pde_filter: bad tolerances");
  // the first guess is the handle's business: zero, or the last forward field under warm_start; the transpose never warm-starts
  const bool warm = f->warm_start && !transpose && f->have_guess;
  o.zero_guess = warm ? 0 : 1;
  femo_vec* p = transpose ? f->pT : f->p;
  if (!transpose) f->have_guess = false;
  FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(f->b);
  FEMO_TRY(femo_launch_dRdf_cell_apply(m, (transpose ? f->cv_one : f->cv_vol)->d, 0, x->d, f->b->d, 0));
  femo_solve_info si = {};
  FEMO_TRY(femo_solve_cg(f->A, 0, f->b, p, &o, &si));
  f->last = si;
  if (info) *info = si;
  FEMO_REQUIRE(std::isfinite(si.rhs_norm) && si.converged != -1, "pde_filter: the input is not finite (load norm %g after %d iterations)",
               si.rhs_norm, (int)si.iterations);
  if (si.converged != 1) {
    femo_set_error("pde_filter: the solve did not converge in %d iterations (residual %.3e, load %.3e, rtol %.1e)",
                   (int)si.iterations, si.residual_norm, si.rhs_norm, o.rtol);
    return 1;
  }
  if (!transpose && f->warm_start) f->have_guess = true;
  *nodal = p;
  return 0;
}

extern "C" int femo_pde_filter_apply(femo_pde_filter* f, int transpose, const femo_vec* x, femo_vec* y,
                                     const femo_solver_opts* opts, femo_solve_info* info) {
  FEMO_REQUIRE(f && x && y, "null argument");
  FEMO_REQUIRE(x->n >= f->n && y->n >= f->n, "pde_filter: a vector is shorter than n = %lld", (long long)f->n);
  FEMO_REQUIRE(!pde_overlap(x, y, f->n), "pde_filter: x overlaps y");
  const femo_vec* p = nullptr;
  FEMO_TRY(femo_pde_filter_nodal(f, transpose, x, opts, info, &p));
  femo_vec_touch(y);
  return femo_launch_dRdf_cell_apply(f->mesh, (transpose ? f->cv_vol : f->cv_one)->d, 1, p->d, y->d, 0);
}
