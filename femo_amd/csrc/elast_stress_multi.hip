// The aggregated von Mises stress of the SIMP elasticity over several load cases in one pass (C-ABI in include/femo_hip.h,
// "femo_elast_pnorm_stress_multi", "femo_elast_von_mises_multi").
//
//   J_l = 1/alpha sum_e |T_e| (m_l rho_e^q sigma_vm,e(u_l))^p,     J = sum_l w_l J_l
//
// Layout as in elast_solve.hip: L columns (1 <= L <= FEMO_ELAST_MAX_COLS), column l of the state and of dJ/du at l * n_dof.
// The arithmetic of a column is that of k_elast_stress_cell / k_elast_stress_du (elasticity.hip); what the columns share
// -- the cell's vertices, the gradients of its barycentric coordinates, its volume and rho^q -- is computed once per cell
// (cell kernel) and once per cell visit (dJ/du kernel), not once per column.  m, w and the field scales travel as
// by-value structs of FEMO_ELAST_MAX_COLS doubles.  No float atomics: one writer per cell and per vertex, the per-column
// partials folded in a fixed order, so every call gives the same bits.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

struct ColScalars { double v[EMC]; };

// columns per thread of the dJ/du kernel: D accumulators and one deviator per column in registers
template <int D>
struct StressChunk { static constexpr int value = 4; };

inline unsigned grid_of(int64_t n, int64_t cap = 1 << 20) {
  int64_t g = (n + EB - 1) / EB;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

// One thread per cell; the geometry once, then the columns one after the other.  Every output optional by null pointer:
//   part[l * ps + block] = sum over the block of J_{l,c} = |T_c| / alpha (m_l rho_c^q sigma_vm(u_l))^p
//   drho[c] (+)= sum_l w_l p q / rho_c J_{l,c}, summed in ascending l
//   field[c] = max_l s_l rho_c^q sigma_vm(u_l) (column < 0: the envelope), or s_column rho_c^q sigma_vm(u_column)
// rho == null reads as q = 0.  The zero-stress guard of k_elast_stress_cell holds per (cell, column).
template <int D>
__global__ __launch_bounds__(EB) void k_elast_stress_cell_multi(
    int64_t n_cell, const int32_t* __restrict__ conn, const double* __restrict__ xv, const double* __restrict__ rho,
    const double* __restrict__ u, int64_t vs, int n_cols, double mu, ColScalars m, ColScalars w, ColScalars sc, double p,
    double q, double inv_alpha, int column, double* __restrict__ field, double* __restrict__ part, int64_t ps,
    double* __restrict__ drho, int accumulate) {
  __shared__ double lds[EB / 64];
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  const bool live = c < n_cell;
  int32_t v[D + 1];
  double g[D + 1][D], vol = 0.0, r = 1.0, rq = 1.0;
  if (live) {
    double pt[D + 1][D];
    load_cell<D>(conn, xv, c, v, pt);
    simplex_grads<D>(pt, g, vol);
    r = rho ? rho[c] : 1.0;
    rq = rho && q != 0.0 ? pow(r, q) : 1.0;
  } else {
#pragma unroll
    for (int b = 0; b <= D; ++b) {
      v[b] = 0;
#pragma unroll
      for (int i = 0; i < D; ++i) g[b][i] = 0.0;
    }
  }
  const bool sums = part || drho;
  const int l0 = field && !sums && column >= 0 ? column : 0;          // a single field: that column only
  const int l1 = field && !sums && column >= 0 ? column + 1 : n_cols;
  double dsum = 0.0, fmax_ = 0.0;
  for (int l = l0; l < l1; ++l) {
    double Jc = 0.0;
    if (live) {
      double s[D][D];
      const double vm = cell_von_mises<D>(g, v, u + l * vs, mu, s);
      const double relaxed = rq * vm;
      if (field && (column < 0 || column == l)) fmax_ = fmax(fmax_, sc.v[l] * relaxed);
      if (sums) {
        Jc = vm > 0.0 ? vol * inv_alpha * pow(m.v[l] * relaxed, p) : 0.0;
        if (drho && q != 0.0 && Jc != 0.0 && w.v[l] != 0.0) dsum += w.v[l] * (p * q / r * Jc);
      }
    }
    if (part) {
      const double t = femo_block_sum<EB>(Jc, lds);
      if (threadIdx.x == 0) part[l * ps + blockIdx.x] = t;
    }
  }
  if (live) {
    if (field) field[c] = fmax_;
    if (drho) drho[c] = accumulate ? drho[c] + dsum : dsum;
  }
}

// dJ/du: one thread per vertex row with the visit walk of k_elast_stress_du, for the columns c0 = MC * blockIdx.y ...
// min(c0 + MC, n_cols) - 1.  Column l of y (+)= w_l dJ_l/du_l.  The geometry and rho^q once per visited cell, D accumulators
// per column.  A column with w_l = 0 takes no part in the walk: it is written as zeros (left alone with accumulate).
template <int D, int MC>
__global__ __launch_bounds__(EB) void k_elast_stress_du_multi(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, const double* __restrict__ rho, const double* __restrict__ u, int64_t vs, int n_cols,
    double mu, ColScalars m, ColScalars w, double p, double q, double inv_alpha, double* __restrict__ y, int accumulate) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int c0 = (int)blockIdx.y * MC;
  bool on[MC], act[MC];      // uniform over the block
  double mm[MC], ww[MC];
  bool any = false;
#pragma unroll
  for (int cc = 0; cc < MC; ++cc) {
    on[cc] = c0 + cc < n_cols;
    mm[cc] = on[cc] ? m.v[c0 + cc] : 1.0;
    ww[cc] = on[cc] ? w.v[c0 + cc] : 0.0;
    act[cc] = on[cc] && ww[cc] != 0.0;
    any = any || act[cc];
  }
  double acc[MC][D];
#pragma unroll
  for (int cc = 0; cc < MC; ++cc)
#pragma unroll
    for (int i = 0; i < D; ++i) acc[cc][i] = 0.0;
  if (any) {
    const int64_t slice = row >> 6;
    const int lane = (int)(row & 63);
    const int64_t vb = vptr[slice];
    const int nvis = (int)((vptr[slice + 1] - vb) >> 6);
    for (int k = 0; k < nvis; ++k) {
      const int32_t ca = visit_cell[vb + (int64_t)k * 64 + lane];
      if (ca < 0) continue;
      const int64_t c = ca >> 2;
      const int a = ca & 3;
      int32_t v[D + 1];
      double pt[D + 1][D], g[D + 1][D], vol;
      load_cell<D>(conn, xv, c, v, pt);
      simplex_grads<D>(pt, g, vol);
      const double rq = q != 0.0 ? pow(rho[c], q) : 1.0;
      double ga[D];
#pragma unroll
      for (int j = 0; j < D; ++j) ga[j] = g[a][j];
      const double base = 3.0 * mu * p * vol * inv_alpha;
#pragma unroll
      for (int cc = 0; cc < MC; ++cc) {
        if (!act[cc]) continue;
        double s[D][D];
        const double vm = cell_von_mises<D>(g, v, u + (c0 + cc) * vs, mu, s);
        if (!(vm > 0.0)) continue;
        const double mr = mm[cc] * rq;
        const double wt = ww[cc] * (base * mr * pow(mr * vm, p - 1.0));
        if (wt == 0.0) continue;
#pragma unroll
        for (int i = 0; i < D; ++i) {
          double t = 0.0;
#pragma unroll
          for (int j = 0; j < D; ++j) t += (s[i][j] / vm) * ga[j];
          acc[cc][i] += wt * t;
        }
      }
    }
  }
#pragma unroll
  for (int cc = 0; cc < MC; ++cc) {
    if (!on[cc] || (accumulate && !act[cc])) continue;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int64_t o = (c0 + cc) * vs + row * D + i;
      y[o] = accumulate ? y[o] + acc[cc][i] : acc[cc][i];
    }
  }
}

template <typename T>
int dalloc(T** p, int64_t n) {
  FEMO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), (size_t)std::max<int64_t>(n, 1) * sizeof(T)));
  return 0;
}

int cell_launch(femo_elast* e, int nc, const double* rho, const double* u, const ColScalars& m, const ColScalars& w,
                const ColScalars& sc, double p, double q, double inv_alpha, int column, double* field, double* part, int64_t ps,
                double* drho, int accumulate) {
  femo_mesh* mh = e->mesh;
  const unsigned g = grid_of(mh->n_cell);
  FEMO_REQUIRE((int64_t)g * EB >= mh->n_cell, "too many cells for one launch");
  const int64_t vs = mh->n_vert * e->d;
  if (e->d == 2)
    hipLaunchKernelGGL(k_elast_stress_cell_multi<2>, dim3(g), dim3(EB), 0, mh->ctx->stream, mh->n_cell, mh->d_conn, mh->d_x, rho,
                       u, vs, nc, e->mu0, m, w, sc, p, q, inv_alpha, column, field, part, ps, drho, accumulate);
  else
    hipLaunchKernelGGL(k_elast_stress_cell_multi<3>, dim3(g), dim3(EB), 0, mh->ctx->stream, mh->n_cell, mh->d_conn, mh->d_x, rho,
                       u, vs, nc, e->mu0, m, w, sc, p, q, inv_alpha, column, field, part, ps, drho, accumulate);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

template <int D>
void du_launch(femo_elast* e, int nc, const double* rho, const double* u, const ColScalars& m, const ColScalars& w, double p,
               double q, double inv_alpha, double* y, int accumulate) {
  constexpr int MC = StressChunk<D>::value;
  femo_mesh* mh = e->mesh;
  hipLaunchKernelGGL((k_elast_stress_du_multi<D, MC>), dim3(grid_of(mh->n_rows), (unsigned)((nc + MC - 1) / MC)), dim3(EB), 0,
                     mh->ctx->stream, mh->n_rows, mh->d_vptr, mh->d_visit_cell, mh->d_conn, mh->d_x, rho, u, mh->n_vert * D, nc,
                     e->mu0, m, w, p, q, inv_alpha, y, accumulate);
}

}  // namespace

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_pnorm_stress_multi(femo_elast* e, int n_cols, const femo_vec* rho, const femo_vec* u, const double* m,
                                  const double* w, double p, double q, double alpha, double* values, femo_vec* grad_u,
                                  femo_vec* grad_rho, int accumulate) {
  FEMO_REQUIRE(e && rho && u && m, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_pnorm_stress_multi: %d columns (1 to %d)", n_cols, EMC);
  femo_mesh* mh = e->mesh;
  const int64_t n = mh->n_vert * e->d, nl = n * n_cols;
  FEMO_REQUIRE(rho->n >= mh->n_cell && u->n >= nl && (!grad_u || grad_u->n >= nl) && (!grad_rho || grad_rho->n >= mh->n_cell),
               "vector size mismatch in femo_elast_pnorm_stress_multi: %d columns need %lld entries", n_cols, (long long)nl);
  FEMO_REQUIRE(p >= 1.0 && q >= 0.0 && alpha > 0.0 && std::isfinite(p) && std::isfinite(q) && std::isfinite(alpha),
               "bad parameters of the stress aggregate: need m > 0, p >= 1, q >= 0, alpha > 0");
  ColScalars ms, ws, ones;
  for (int l = 0; l < EMC; ++l) {
    ms.v[l] = l < n_cols ? m[l] : 1.0;
    ws.v[l] = l < n_cols ? (w ? w[l] : 1.0) : 0.0;
    ones.v[l] = 1.0;
    FEMO_REQUIRE(ms.v[l] > 0.0 && std::isfinite(ms.v[l]), "bad parameters of the stress aggregate: need m > 0 (load case %d)", l);
    FEMO_REQUIRE(ws.v[l] >= 0.0 && std::isfinite(ws.v[l]), "bad parameters of the stress aggregate: need a weight >= 0 (load case %d)", l);
  }
  FEMO_REQUIRE(grad_u != u && grad_u != rho && grad_rho != rho && grad_rho != u && (!grad_u || grad_u != grad_rho),
               "femo_elast_pnorm_stress_multi: output aliases an input");
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(u));
  hipStream_t st = mh->ctx->stream;
  const int nb = (int)grid_of(mh->n_cell);
  // one fold for all columns while a slab fits the fold's slot, one fold per column beyond that
  const int64_t ps = std::max<int64_t>(nb, FEMO_MAX_PARTIALS);
  if (values && !e->w_smpart) FEMO_TRY(dalloc(&e->w_smpart, ps * EMC + EMC));
  const double inv_alpha = 1.0 / alpha;
  if (grad_rho) femo_vec_touch(grad_rho);
  if (values || grad_rho)
    FEMO_TRY(cell_launch(e, n_cols, rho->d, u->d, ms, ws, ones, p, q, inv_alpha, -1, nullptr, values ? e->w_smpart : nullptr, ps,
                         grad_rho ? grad_rho->d : nullptr, accumulate));
  if (grad_u) {
    femo_vec_touch(grad_u);
    if (e->d == 2) du_launch<2>(e, n_cols, rho->d, u->d, ms, ws, p, q, inv_alpha, grad_u->d, accumulate);
    else du_launch<3>(e, n_cols, rho->d, u->d, ms, ws, p, q, inv_alpha, grad_u->d, accumulate);
    FEMO_HIP_CHECK(hipGetLastError());
  }
  if (values) {
    double* out = e->w_smpart + ps * EMC;
    if (ps == FEMO_MAX_PARTIALS) FEMO_TRY(femo_launch_fold(1024, nb, n_cols, e->w_smpart, out, st));
    else
      for (int l = 0; l < n_cols; ++l) FEMO_TRY(femo_launch_fold(1024, nb, 1, e->w_smpart + l * ps, out + l, st));
    FEMO_HIP_CHECK(hipMemcpyAsync(e->h_s, out, (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    for (int l = 0; l < n_cols; ++l) values[l] = e->h_s[l];
  }
  return 0;
}

int femo_elast_von_mises_multi(femo_elast* e, int n_cols, const femo_vec* rho, const femo_vec* u, const double* scale, double q,
                               int column, femo_vec* out_cells) {
  FEMO_REQUIRE(e && u && out_cells, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_von_mises_multi: %d columns (1 to %d)", n_cols, EMC);
  FEMO_REQUIRE(column >= -1 && column < n_cols, "femo_elast_von_mises_multi: column %d of %d (-1: the envelope)", column, n_cols);
  FEMO_REQUIRE(q >= 0.0 && std::isfinite(q), "femo_elast_von_mises_multi: need q >= 0");
  FEMO_REQUIRE(rho || q == 0.0, "femo_elast_von_mises_multi: q > 0 needs the density");
  femo_mesh* mh = e->mesh;
  const int64_t nl = mh->n_vert * e->d * n_cols;
  FEMO_REQUIRE(u->n >= nl && out_cells->n >= mh->n_cell && (!rho || rho->n >= mh->n_cell),
               "vector size mismatch in femo_elast_von_mises_multi: %d columns need %lld entries", n_cols, (long long)nl);
  FEMO_REQUIRE(out_cells != u && out_cells != rho, "femo_elast_von_mises_multi: output aliases an input");
  ColScalars sc, ones;
  for (int l = 0; l < EMC; ++l) {
    sc.v[l] = l < n_cols && scale ? scale[l] : 1.0;
    ones.v[l] = 1.0;
    FEMO_REQUIRE(sc.v[l] > 0.0 && std::isfinite(sc.v[l]), "femo_elast_von_mises_multi: need a scale > 0 (load case %d)", l);
  }
  FEMO_TRY(femo_vec_await(u));
  if (rho) FEMO_TRY(femo_vec_await(rho));
  femo_vec_touch(out_cells);
  return cell_launch(e, n_cols, rho ? rho->d : nullptr, u->d, ones, ones, sc, 1.0, q, 1.0, column, out_cells->d, nullptr, 0,
                     nullptr, 0);
}

}  // extern "C"
