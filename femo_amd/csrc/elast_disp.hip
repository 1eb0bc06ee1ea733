// The aggregated nodal displacement of the SIMP elasticity, for one load case or several in one pass (C-ABI in
// include/femo_hip.h: "femo_elast_pnorm_disp_multi"): the smooth stand-in for "no vertex of this region moves more than delta".
//
//   J_l = 1/alpha sum_v a_v (m_l |u_{l,v}|)^p,     J = sum_l w_l J_l,     |u_v| the Euclidean norm of the vertex's d components
//
// Layout and conventions as in elast_stress.hip: L columns (1 <= L <= FEMO_ELAST_MAX_COLS), column l of the state and of
// dJ/du at l * n_dof; m and w travel as by-value structs.  One kernel, one thread per vertex, the columns in ascending order:
// the vertex weight is read once for all of them.  No float atomics: one writer per gradient entry, the per-column partials
// (wave sum -> LDS -> one per block and column) folded in a fixed order, so every call gives the same bits and column l does
// not depend on the number of columns.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int EMC = FEMO_ELAST_MAX_COLS;

// Every output optional by null pointer:
//   part[l * ps + block] = sum over the block of J_{l,v} = a_v / alpha (m_l |u_{l,v}|)^p
//   y[l * vs + d v + i] (+)= w_l p a_v / alpha m_l (m_l |u_v|)^(p-1) u_{v,i} / |u_v|
// (no negative power of |u_v| for p >= 1).  A vertex with a_v == 0 is skipped without reading u (a documented skip: what u
// holds there cannot show).  A vertex with |u_v| == 0 gives exact zeros; the guard is a test for == 0, so a non-finite |u_v|
// is no zero: it shows in the value and in all d gradient entries of its vertex (also where p = 1 would leave the other
// components finite).  A column with w_l = 0 takes no part in y: it is written as zeros (left alone with accumulate).
template <int D>
__global__ __launch_bounds__(EB) void k_elast_disp_multi(int64_t n_vert, const double* __restrict__ a,
                                                         const double* __restrict__ u, int64_t vs, int n_cols, ColScalars m,
                                                         ColScalars w, double p, double inv_alpha, double* __restrict__ part,
                                                         int64_t ps, double* __restrict__ y, int accumulate) {
  __shared__ double lds[EB / 64];
  const int64_t v = (int64_t)blockIdx.x * EB + threadIdx.x;
  const bool live = v < n_vert;              // a thread past the last vertex stays for the block sums
  const double av = live ? a[v] : 0.0;
  for (int l = 0; l < n_cols; ++l) {
    const bool act = y && w.v[l] != 0.0;
    double Jv = 0.0, g[D];
#pragma unroll
    for (int i = 0; i < D; ++i) g[i] = 0.0;
    if (live && av != 0.0 && (part || act)) {
      double uu[D], ss = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        uu[i] = u[l * vs + v * D + i];
        ss += uu[i] * uu[i];
      }
      const double nrm = sqrt(ss);
      if (nrm != 0.0) {                      // exactly zero only: a NaN goes on
        const double mn = m.v[l] * nrm;
        if (part) Jv = av * inv_alpha * pow(mn, p);
        if (act) {
          double wt = w.v[l] * (p * av * inv_alpha * m.v[l] * pow(mn, p - 1.0));
          if (!is_finite(nrm)) wt = nrm - nrm;          // NaN: pow(inf, 0) = 1 would hide it at p = 1
#pragma unroll
          for (int i = 0; i < D; ++i) g[i] = wt * (uu[i] / nrm);
        }
      }
    }
    if (part) {
      const double t = femo_block_sum<EB>(Jv, lds);
      if (threadIdx.x == 0) part[l * ps + blockIdx.x] = t;
    }
    if (live && y && !(accumulate && !act)) {
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const int64_t o = l * vs + v * D + i;
        y[o] = accumulate ? y[o] + g[i] : g[i];
      }
    }
  }
}

}  // namespace

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_pnorm_disp_multi(femo_elast* e, int n_cols, const femo_vec* u, const femo_vec* a, const double* m, const double* w,
                                double p, double alpha, double* values, femo_vec* grad_u, int accumulate) {
  FEMO_REQUIRE(e && u && a && m, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= EMC, "femo_elast_pnorm_disp_multi: %d columns (1 to %d)", n_cols, EMC);
  femo_mesh* mh = e->mesh;
  const int64_t nv = mh->n_vert, n = nv * e->d, nl = n * n_cols;
  FEMO_REQUIRE(u->n >= nl && a->n >= nv && (!grad_u || grad_u->n >= nl),
               "vector size mismatch in femo_elast_pnorm_disp_multi: %d columns need %lld entries", n_cols, (long long)nl);
  FEMO_REQUIRE(p >= 1.0 && std::isfinite(p) && std::isfinite(alpha),
               "bad parameters of the displacement aggregate: need m > 0, p >= 1, a finite alpha");
  FEMO_REQUIRE(grad_u != u && grad_u != a, "femo_elast_pnorm_disp_multi: output aliases an input");
  ColScalars ms, ws;
  for (int l = 0; l < EMC; ++l) {
    ms.v[l] = l < n_cols ? m[l] : 1.0;
    ws.v[l] = l < n_cols ? (w ? w[l] : 1.0) : 0.0;
    FEMO_REQUIRE(ms.v[l] > 0.0 && std::isfinite(ms.v[l]), "bad parameters of the displacement aggregate: need m > 0 (load case %d)", l);
    FEMO_REQUIRE(ws.v[l] >= 0.0 && std::isfinite(ws.v[l]),
                 "bad parameters of the displacement aggregate: need a weight >= 0 (load case %d)", l);
  }
  FEMO_TRY(femo_vec_await(u)); FEMO_TRY(femo_vec_await(a));
  hipStream_t st = mh->ctx->stream;
  // the weights are checked, and summed for alpha <= 0, on the host: n_vert doubles, once per call
  std::vector<double> ah((size_t)nv);
  FEMO_HIP_CHECK(hipMemcpyAsync(ah.data(), a->d, (size_t)nv * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  double asum = 0.0;
  for (int64_t v = 0; v < nv; ++v) {
    FEMO_REQUIRE(std::isfinite(ah[v]) && ah[v] >= 0.0, "femo_elast_pnorm_disp_multi: the weight of vertex %lld is %g (need finite, >= 0)",
                 (long long)v, ah[v]);
    asum += ah[v];
  }
  if (!(alpha > 0.0)) alpha = asum;
  FEMO_REQUIRE(alpha > 0.0 && std::isfinite(alpha), "femo_elast_pnorm_disp_multi: the weights sum to %g (need alpha > 0)", alpha);
  const int nb = (int)grid_of(nv);
  FEMO_REQUIRE((int64_t)nb * EB >= nv, "too many vertices for one launch");
  // one fold for all columns while a slab fits the fold's slot, one fold per column beyond that
  const int64_t ps = std::max<int64_t>(nb, FEMO_MAX_PARTIALS);
  if (values && !e->w_dpart) FEMO_TRY(dalloc(&e->w_dpart, ps * EMC + EMC));
  if (grad_u) femo_vec_touch(grad_u);
  if (values || grad_u)
    FEMO_TRY(elast_dispatch_d(e->d, [&](auto dim) {
      constexpr int D = decltype(dim)::value;
      return elast_launch(e, nv, 1u, k_elast_disp_multi<D>, a->d, u->d, n, n_cols, ms, ws, p, 1.0 / alpha,
                          values ? e->w_dpart : nullptr, ps, grad_u ? grad_u->d : nullptr, accumulate);
    }));
  if (values) {
    double* out = e->w_dpart + ps * EMC;
    if (ps == FEMO_MAX_PARTIALS) FEMO_TRY(femo_launch_fold(1024, nb, n_cols, e->w_dpart, out, st));
    else
      for (int l = 0; l < n_cols; ++l) FEMO_TRY(femo_launch_fold(1024, nb, 1, e->w_dpart + l * ps, out + l, st));
    FEMO_HIP_CHECK(hipMemcpyAsync(e->h_s, out, (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    for (int l = 0; l < n_cols; ++l) values[l] = e->h_s[l];
  }
  return 0;
}

}  // extern "C"
