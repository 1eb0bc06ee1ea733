// SIMP topology optimisation: vector CG1 linear elasticity with a DG0 density, and the DG0 density filter
// (examples/beam_topo_opt; C-ABI in include/femo_hip.h, "SIMP topology optimisation").
//
// Layout.  The state has d = tdim dofs per vertex (dof = d * vertex + component).  K(rho) lives on the mesh's SCALAR SELL
// pattern: SELL entry e holds one d x d block at vals[e * d^2 + r * d + c] (r: row component, c: column component), the
// diagonal blocks at diag[v * d^2 + ...].  Per block one 4-byte column index serves 8 d^2 bytes of values.
//
// The stress aggregate is in elast_stress.hip, the product and the solve in elast_solve.hip.
//
// Assembly walks the vertex -> cell incidence like assemble.hip: the thread of row v visits the cells around v and adds
// C(rho_c) |T_c| B_v^T D_0 B_w to its blocks (v, w).  No float atomics: every block has one writer, the visits come in
// ascending cell order, and the cell geometry is formed from `conn` in its own vertex order, so block (v, w) and block
// (w, v)^T are sums of the same numbers in the same order -- K is symmetric entry for entry.
#include "elast_internal.h"
#include "filter_grid.h"

#include <algorithm>
#include <cmath>

namespace {

// ----------------------------------------------------------------------------------------------- assembly ----
template <int D>
__global__ __launch_bounds__(EB) void k_elast_assemble(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell,
    const uint32_t* __restrict__ visit_slots, const int64_t* __restrict__ mptr, const int32_t* __restrict__ rowlen,
    const int32_t* __restrict__ conn, const double* __restrict__ x, const double* __restrict__ rho, int method,
    double lam, double mu, const uint8_t* __restrict__ fixed, double* __restrict__ vals, double* __restrict__ diag,
    double* __restrict__ dinv) {
  constexpr int DD = D * D;
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t slice = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t mb = mptr[slice];
  const int len = rowlen[row];
  for (int k = 0; k < len; ++k) {
    const int64_t e = femo_sell_index(mb, k, lane);
#pragma unroll
    for (int q = 0; q < DD; ++q) vals[e * DD + q] = 0.0;
  }
  double dg[DD];
#pragma unroll
  for (int q = 0; q < DD; ++q) dg[q] = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    const uint32_t sl = visit_slots[t.vi];
    const int64_t c = t.c;
    const int a = t.a;
    // g is indexed by the run-time a: an array of its own, which a member of the cell record could not be split into
    int32_t v[D + 1];
    double p[D + 1][D], g[D + 1][D], vol;
    load_cell<D>(conn, x, c, v, p);
    simplex_grads<D>(p, g, vol);
    const double coef = penal(method, rho[c]) * vol;
#pragma unroll
    for (int b = 0; b <= D; ++b) {
      const double gab = dotg<D>(g, a, b);
      if (b == a) {
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
          for (int cc = 0; cc < D; ++cc) dg[r * D + cc] += coef * kblock<D>(g, a, b, r, cc, lam, mu, gab);
      } else {
        const int64_t e = femo_sell_index(mb, slot_pos(sl, a, b), lane);
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
          for (int cc = 0; cc < D; ++cc) vals[e * DD + r * D + cc] += coef * kblock<D>(g, a, b, r, cc, lam, mu, gab);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < DD; ++q) diag[row * DD + q] = dg[q];
  // block-Jacobi: inverse of the diagonal block, fixed components as identity rows / columns
  double B[DD], Bi[DD];
#pragma unroll
  for (int q = 0; q < DD; ++q) B[q] = dg[q];
  block_inverse_fixed<D>(B, fixed ? fixed + row * D : nullptr, Bi);
#pragma unroll
  for (int q = 0; q < DD; ++q) dinv[row * DD + q] = Bi[q];
}

// Elastic supports: K_s = K + diag(k).  After k_elast_assemble, and only when springs are set: the thread of a row with a
// non-zero spring adds k[d row + r] to entry (r, r) of its diagonal block and recomputes the block's inverse (the fixed byte
// first, as in the assembly: a spring on a fixed dof stays in the unmasked operator and out of the masked one).  One writer
// per entry, no atomics.  A row without springs is not touched.
template <int D>
__global__ __launch_bounds__(EB) void k_elast_springs(int64_t n_rows, const double* __restrict__ k,
                                                      const uint8_t* __restrict__ fixed, double* __restrict__ diag,
                                                      double* __restrict__ dinv) {
  constexpr int DD = D * D;
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  double kr[D];
  bool any = false;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    kr[r] = k[row * D + r];
    any = any || kr[r] != 0.0;
  }
  if (!any) return;
  double B[DD], Bi[DD];
#pragma unroll
  for (int q = 0; q < DD; ++q) B[q] = diag[row * DD + q];
#pragma unroll
  for (int r = 0; r < D; ++r) {
    B[r * D + r] += kr[r];
    diag[row * DD + r * D + r] = B[r * D + r];
  }
  block_inverse_fixed<D>(B, fixed ? fixed + row * D : nullptr, Bi);
#pragma unroll
  for (int q = 0; q < DD; ++q) dinv[row * DD + q] = Bi[q];
}

// ---------------------------------------------------------------------------------------------- dR/drho ----
// rev: y_c (+)= C'(rho_c) |T| (lam div w div u + 2 mu eps(w) : eps(u)) = C'(rho_c) w_c^T K0_c u_c
template <int D>
__global__ __launch_bounds__(EB) void k_elast_drho_T(int64_t n_cell, const int32_t* __restrict__ conn,
                                                     const double* __restrict__ xv, const double* __restrict__ rho, int method,
                                                     double lam, double mu, const double* __restrict__ u,
                                                     const double* __restrict__ w, double* __restrict__ y, int accumulate) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= n_cell) return;
  const ElastCell<D> K = elast_cell<D>(conn, xv, c);
  double Gu[D][D], Gw[D][D];
  cell_gradient<D>(K.g, K.v, u, Gu);
  cell_gradient<D>(K.g, K.v, w, Gw);
  const double val = penal_d(method, rho[c]) * K.vol * elastic_form<D>(Gu, Gw, lam, mu);
  y[c] = accumulate ? y[c] + val : val;
}

// fwd: y_v (+)= sum over the cells c around v of C'(rho_c) dr_c |T| sigma_0(u_c) grad(phi_v)
template <int D>
__global__ __launch_bounds__(EB) void k_elast_drho_N(
    int64_t n_rows, const int64_t* __restrict__ vptr, const int32_t* __restrict__ visit_cell, const int32_t* __restrict__ conn,
    const double* __restrict__ xv, const double* __restrict__ rho, int method, double lam, double mu,
    const double* __restrict__ u, const double* __restrict__ dr, double* __restrict__ y, int accumulate) {
  const int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (row >= n_rows) return;
  double acc[D];
#pragma unroll
  for (int r = 0; r < D; ++r) acc[r] = 0.0;
  const ElastVisits V = elast_visits(row, vptr);
  for (int s = 0; s < V.n; ++s) {
    const ElastVisit t = elast_visit(V, visit_cell, s);
    if (!t.live) continue;
    const int64_t c = t.c;
    const int a = t.a;
    int32_t v[D + 1];        // g[a]: an array of its own, as in k_elast_assemble
    double p[D + 1][D], g[D + 1][D], vol, Gu[D][D];
    load_cell<D>(conn, xv, c, v, p);
    simplex_grads<D>(p, g, vol);
    cell_gradient<D>(g, v, u, Gu);
    double divu = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) divu += Gu[i][i];
    const double coef = penal_d(method, rho[c]) * dr[c] * vol;
    // lam div g_a first, then the shear terms in ascending k: not the order of a stress tensor times g_a
#pragma unroll
    for (int r = 0; r < D; ++r) {
      double sg = lam * divu * g[a][r];
#pragma unroll
      for (int k = 0; k < D; ++k) sg += mu * (Gu[r][k] + Gu[k][r]) * g[a][k];
      acc[r] += coef * sg;
    }
  }
#pragma unroll
  for (int r = 0; r < D; ++r) y[row * D + r] = accumulate ? y[row * D + r] + acc[r] : acc[r];
}

// ------------------------------------------------------------------------------------------- traction ----
template <int D>
__global__ __launch_bounds__(EB) void k_elast_load(int64_t n_vert, const int64_t* __restrict__ fptr,
                                                   const int32_t* __restrict__ flist, const int32_t* __restrict__ fverts,
                                                   const double* __restrict__ x, double t0, double t1, double t2,
                                                   double* __restrict__ F) {
  const int64_t v = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (v >= n_vert) return;
  double w = 0.0;
  for (int64_t k = fptr[v]; k < fptr[v + 1]; ++k) {
    const int64_t f = flist[k];
    double p[D][D];
#pragma unroll
    for (int b = 0; b < D; ++b)
#pragma unroll
      for (int i = 0; i < D; ++i) p[b][i] = x[(int64_t)fverts[f * D + b] * D + i];
    double meas;
    if constexpr (D == 2) {
      meas = sqrt((p[1][0] - p[0][0]) * (p[1][0] - p[0][0]) + (p[1][1] - p[0][1]) * (p[1][1] - p[0][1]));
    } else {
      const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
      const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
      const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
      meas = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
    }
    w += meas / D;
  }
  const double t[3] = {t0, t1, t2};
#pragma unroll
  for (int i = 0; i < D; ++i) F[v * D + i] = t[i] * w;
}

// --------------------------------------------------------------------------------------------- export ----
template <int D>
__global__ void k_elast_export(int64_t n_rows, const int64_t* __restrict__ mptr, const int32_t* __restrict__ cols,
                               const int32_t* __restrict__ rowlen, const uint32_t* __restrict__ rowreal,
                               const double* __restrict__ diag, const double* __restrict__ vals,
                               const int64_t* __restrict__ rowptr, int32_t* __restrict__ ocol, double* __restrict__ oval) {
  constexpr int DD = D * D;
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t base = mptr[row >> 6];
  const int lane = (int)(row & 63);
  const int len = rowlen[row];
  int64_t o = rowptr[row];
  bool placed = false;
  const uint32_t real = rowreal[row];
  for (int k = 0; k < len; ++k) {
    if (k < 32 && !((real >> k) & 1u)) continue;
    const int64_t e = femo_sell_index(base, k, lane);
    const int32_t c = cols[e];
    if (!placed && c > row) {
      ocol[o] = (int32_t)row;
      for (int q = 0; q < DD; ++q) oval[o * DD + q] = diag[row * DD + q];
      ++o; placed = true;
    }
    ocol[o] = c;
    for (int q = 0; q < DD; ++q) oval[o * DD + q] = vals[e * DD + q];
    ++o;
  }
  if (!placed) {
    ocol[o] = (int32_t)row;
    for (int q = 0; q < DD; ++q) oval[o * DD + q] = diag[row * DD + q];
  }
}

// --------------------------------------------------------------------------------------------- filter ----
using Grid = FilterGrid;      // filter_grid.h: the host plans it, the kernels below index with it

template <int D>
__device__ __forceinline__ int64_t grid_cell(const Grid& G, const double* p, int64_t (&ijk)[3]) {
  int64_t id = 0, stride = 1;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    int64_t q = (int64_t)floor((p[k] - G.lo[k]) / G.h);
    q = q < 0 ? 0 : (q >= G.n[k] ? G.n[k] - 1 : q);
    ijk[k] = q;
    id += q * stride;
    stride *= G.n[k];
  }
  return id;
}

template <int D>
__global__ void k_f_bin(int64_t n, const double* __restrict__ x, Grid G, int64_t* __restrict__ cid,
                        unsigned long long* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  int64_t ijk[3];
  const int64_t c = grid_cell<D>(G, x + i * D, ijk);
  cid[i] = c;
  atomicAdd(&count[c], 1ull);
}

// exclusive scan of n counts into out[0..n] (one workgroup, chunk by chunk; build-time only)
__global__ __launch_bounds__(1024) void k_scan(int64_t n, const unsigned long long* __restrict__ in, int64_t* __restrict__ out) {
  __shared__ int64_t buf[1024];
  __shared__ int64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < n ? (int64_t)in[i] : 0;
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int64_t t = threadIdx.x >= (unsigned)off ? buf[threadIdx.x - off] : 0;
      __syncthreads();
      buf[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < n) out[i] = carry + buf[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += buf[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[n] = carry;
}

__global__ void k_f_fill(int64_t n, const int64_t* __restrict__ cid, const int64_t* __restrict__ start,
                         unsigned long long* __restrict__ cursor, int32_t* __restrict__ bucket) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cid[i];
  const unsigned long long k = atomicAdd(&cursor[c], 1ull);
  bucket[start[c] + (int64_t)k] = (int32_t)i;
}

// each grid cell's points in ascending order: the walks below visit candidates deterministically
__global__ void k_f_sort_buckets(int64_t ncell, const int64_t* __restrict__ start, int32_t* __restrict__ bucket) {
  const int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (c >= ncell) return;
  const int64_t b = start[c], e = start[c + 1];
  for (int64_t i = b + 1; i < e; ++i) {
    const int32_t v = bucket[i];
    int64_t j = i - 1;
    while (j >= b && bucket[j] > v) { bucket[j + 1] = bucket[j]; --j; }
    bucket[j + 1] = v;
  }
}

__device__ __forceinline__ double dist_sym(const double* a, const double* b, int D) {
  double s = 0.0;
  for (int k = 0; k < D; ++k) { const double t = a[k] - b[k]; s += t * t; }
  return sqrt(s);
}

// PASS 0: count the neighbours of every point.  PASS 1: write (column, r - d) into the row, then sort it by column.
template <int D, int PASS>
__global__ void k_f_rows(int64_t n, const double* __restrict__ x, Grid G, double radius, const int64_t* __restrict__ start,
                         const int32_t* __restrict__ bucket, unsigned long long* __restrict__ rowcnt,
                         const int64_t* __restrict__ rowptr, int32_t* __restrict__ col, double* __restrict__ rd) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  int64_t ijk[3] = {0, 0, 0};
  grid_cell<D>(G, x + i * D, ijk);
  int64_t cnt = 0;
  const int64_t o = PASS == 1 ? rowptr[i] : 0;
  const int dz = D == 3 ? 1 : 0;
  for (int oz = -dz; oz <= dz; ++oz)
    for (int oy = -1; oy <= 1; ++oy)
      for (int ox = -1; ox <= 1; ++ox) {
        const int64_t cx = ijk[0] + ox, cy = ijk[1] + oy, cz = ijk[2] + oz;
        if (cx < 0 || cx >= G.n[0] || cy < 0 || cy >= G.n[1]) continue;
        if (D == 3 && (cz < 0 || cz >= G.n[2])) continue;
        const int64_t c = cx + G.n[0] * (cy + (D == 3 ? G.n[1] * cz : 0));
        for (int64_t k = start[c]; k < start[c + 1]; ++k) {
          const int32_t j = bucket[k];
          const double d = dist_sym(x + i * D, x + (int64_t)j * D, D);
          if (d <= radius) {
            if (PASS == 1) { col[o + cnt] = j; rd[o + cnt] = radius - d; }
            ++cnt;
          }
        }
      }
  if (PASS == 0) {
    rowcnt[i] = (unsigned long long)cnt;
  } else {
    for (int64_t a = o + 1; a < o + cnt; ++a) {
      const int32_t cj = col[a];
      const double vj = rd[a];
      int64_t b = a - 1;
      while (b >= o && col[b] > cj) { col[b + 1] = col[b]; rd[b + 1] = rd[b]; --b; }
      col[b + 1] = cj; rd[b + 1] = vj;
    }
  }
}

__global__ void k_f_rowsum(int64_t n, const int64_t* __restrict__ rowptr, const double* __restrict__ rd, double* __restrict__ S) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) s += rd[e];
  S[i] = s;
}

// W_ij = (r - d_ij) / S_i;  (W^T)_ij = W_ji = (r - d_ij) / S_j on the same pattern (d_ij = d_ji bit for bit)
__global__ void k_f_weights(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                            const double* __restrict__ S, double* __restrict__ val, double* __restrict__ valT) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  const double si = S[i];
  for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
    const double r = valT[e];
    val[e] = r / si;
    valT[e] = r / S[col[e]];
  }
}

__global__ void k_f_apply(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                          const double* __restrict__ val, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) s += val[e] * x[col[e]];
  y[i] = s;
}

// The launches of dR/drho for one column on raw pointers.
int drho_launch(femo_elast* e, int method, int transpose, const double* rho, const double* u, const double* x, double* y,
                int accumulate) {
  femo_mesh* m = e->mesh;
  return elast_dispatch_d(e->d, [&](auto dim) {
    constexpr int D = decltype(dim)::value;
    if (transpose)
      return elast_launch_cells(e, k_elast_drho_T<D>, m->d_conn, m->d_x, rho, method, e->lam0, e->mu0, u, x, y, accumulate);
    return elast_launch_rows(e, k_elast_drho_N<D>, m->d_vptr, m->d_visit_cell, m->d_conn, m->d_x, rho, method, e->lam0, e->mu0, u,
                             x, y, accumulate);
  });
}

// dR/drho of femo_elast_drho (one column) and femo_elast_drho_multi, which have checked their sizes; who: the entry point,
// for the error texts.  The transpose sums the columns into y in ascending order.
int drho_cols(femo_elast* e, int method, int transpose, int n_cols, const femo_vec* rho, const femo_vec* u, const femo_vec* x,
              femo_vec* y, int accumulate, const char* who) {
  FEMO_REQUIRE(method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP, "unknown penalisation method %d", method);
  FEMO_REQUIRE(y != x && y != u && y != rho, "%s: output aliases an input", who);
  FEMO_TRY(femo_vec_await(rho)); FEMO_TRY(femo_vec_await(u)); FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(y);
  const int64_t n = e->mesh->n_vert * e->d;
  for (int l = 0; l < n_cols; ++l) {
    if (transpose) FEMO_TRY(drho_launch(e, method, 1, rho->d, u->d + l * n, x->d + l * n, y->d, accumulate || l > 0));
    else FEMO_TRY(drho_launch(e, method, 0, rho->d, u->d + l * n, x->d, y->d + l * n, accumulate));
  }
  return 0;
}

}  // namespace

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_create(femo_mesh* m, double E, double nu, femo_elast** out) {
  FEMO_REQUIRE(m && out, "null argument");
  FEMO_REQUIRE(m->tdim == 2 || m->tdim == 3, "elasticity needs a 2-D or 3-D simplex mesh");
  FEMO_REQUIRE(m->n_nbr == 0 && m->n_rows == m->n_vert,
               "elasticity runs on one GPU: a partitioned mesh (halo set) is not supported");
  FEMO_REQUIRE(nu > -1.0 && nu < 0.5 && E > 0.0, "elasticity: need E > 0 and -1 < nu < 1/2");
  auto* e = new femo_elast();
  e->mesh = m;
  e->d = m->tdim;
  e->lam0 = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu));
  e->mu0 = E / (2.0 * (1.0 + nu));
  const int64_t dd = (int64_t)e->d * e->d;
  int rc = 0;
  rc |= dalloc(&e->d_vals, m->sell_entries * dd);
  rc |= dalloc(&e->d_diag, m->n_vert * dd);
  rc |= dalloc(&e->d_dinv, m->n_vert * dd);
  rc |= femo_elast_work_reserve(e, 1, "femo_elast_create");
  rc |= dalloc(&e->w_s, (int64_t)EMS_STRIDE * FEMO_ELAST_MAX_COLS);
  rc |= dalloc(&e->w_flag, (int64_t)EMF_STRIDE * FEMO_ELAST_MAX_COLS);
  if (rc == 0 && hipHostMalloc(reinterpret_cast<void**>(&e->h_flag), EMF_STRIDE * FEMO_ELAST_MAX_COLS * sizeof(int32_t)) != hipSuccess) rc = 1;
  if (rc == 0 && hipHostMalloc(reinterpret_cast<void**>(&e->h_s), EMS_STRIDE * FEMO_ELAST_MAX_COLS * sizeof(double)) != hipSuccess) rc = 1;
  if (rc) { femo_elast_destroy(e); femo_set_error("femo_elast_create: device allocation failed"); return 1; }
  *out = e;
  return 0;
}

int femo_elast_destroy(femo_elast* e) {
  if (!e) return 0;                    // hipFree waits for the device; the mesh may already be gone
  femo_elast_pc_free(e);
  hipFree(e->d_vals); hipFree(e->d_diag); hipFree(e->d_dinv); hipFree(e->d_fixed); hipFree(e->d_springs);
  hipFree(e->d_fverts); hipFree(e->d_fptr); hipFree(e->d_flist);
  hipFree(e->w_r); hipFree(e->w_z); hipFree(e->w_p); hipFree(e->w_q); hipFree(e->w_part); hipFree(e->w_s); hipFree(e->w_flag); hipFree(e->w_smpart); hipFree(e->w_dpart);
  hipFree(e->w_eig); hipFree(e->w_gram); hipFree(e->w_gstress);
  hipFree(e->d_mvals); hipFree(e->d_mdiag); hipFree(e->w_harm); hipFree(e->w_ms);
  hipFree(e->w_nm); hipFree(e->d_nm_dinv);
  if (e->h_ms) hipHostFree(e->h_ms);
  if (e->h_gram) hipHostFree(e->h_gram);
  if (e->h_flag) hipHostFree(e->h_flag);
  if (e->h_s) hipHostFree(e->h_s);
  delete e;
  return 0;
}

int femo_elast_info(const femo_elast* e, int64_t info[FEMO_ELAST_INFO_COUNT]) {
  FEMO_REQUIRE(e && info, "null argument");
  const femo_mesh* m = e->mesh;
  const int64_t d = e->d;
  info[FEMO_ELAST_INFO_DIM] = d;
  info[FEMO_ELAST_INFO_NDOF] = d * m->n_vert;
  info[FEMO_ELAST_INFO_NNZ] = m->nnz;
  info[FEMO_ELAST_INFO_SELL] = m->sell_entries;
  info[FEMO_ELAST_INFO_SPMV_BYTES] = m->nnz * (4 + 8 * d * d) + m->n_vert * 16 * d + (m->n_slices + 1) * 8 + m->n_vert * 4;
  return 0;
}

int femo_elast_set_fixed(femo_elast* e, const uint8_t* mask) {
  FEMO_REQUIRE(e, "null argument");
  const int64_t n = e->mesh->n_vert * e->d;
  hipStream_t st = e->mesh->ctx->stream;
  e->pc_dirty = true;
  if (!mask) { e->has_fixed = false; return 0; }
  if (!e->d_fixed) FEMO_TRY(dalloc(&e->d_fixed, n));
  FEMO_HIP_CHECK(hipMemcpyAsync(e->d_fixed, mask, n, hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  e->has_fixed = true;
  return 0;
}

int femo_elast_set_springs(femo_elast* e, const double* k) {
  FEMO_REQUIRE(e, "null argument");
  const int64_t n = e->mesh->n_vert * e->d;
  bool any = false;
  for (int64_t i = 0; k && i < n; ++i) {
    FEMO_REQUIRE(std::isfinite(k[i]) && k[i] >= 0.0, "femo_elast_set_springs: the stiffness of dof %lld is %g (need finite, >= 0)",
                 (long long)i, k[i]);
    any = any || k[i] != 0.0;
  }
  if (any) {
    hipStream_t st = e->mesh->ctx->stream;
    if (!e->d_springs) FEMO_TRY(dalloc(&e->d_springs, n));
    FEMO_HIP_CHECK(hipMemcpyAsync(e->d_springs, k, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
  }
  e->has_springs = any;
  e->assembled = false;            // the stored operator is that of the old supports: no product before the next assembly
  e->pc_dirty = true;
  return 0;
}

int femo_elast_set_facets(femo_elast* e, int64_t n_facets, const int32_t* fv) {
  FEMO_REQUIRE(e && (fv || n_facets == 0) && n_facets >= 0, "null argument");
  const femo_mesh* m = e->mesh;
  const int d = e->d;
  std::vector<int64_t> ptr(m->n_vert + 1, 0);
  for (int64_t f = 0; f < n_facets * d; ++f) {
    FEMO_REQUIRE(fv[f] >= 0 && fv[f] < m->n_vert, "facet vertex out of range");
    ++ptr[fv[f] + 1];
  }
  for (int64_t v = 0; v < m->n_vert; ++v) ptr[v + 1] += ptr[v];
  std::vector<int32_t> list(ptr[m->n_vert]);
  std::vector<int64_t> cur(ptr.begin(), ptr.end() - 1);
  for (int64_t f = 0; f < n_facets; ++f)               // ascending facet order per vertex
    for (int b = 0; b < d; ++b) list[cur[fv[f * d + b]]++] = (int32_t)f;
  hipStream_t st = m->ctx->stream;
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  hipFree(e->d_fverts); hipFree(e->d_fptr); hipFree(e->d_flist);
  e->d_fverts = nullptr; e->d_fptr = nullptr; e->d_flist = nullptr;
  FEMO_TRY(dalloc(&e->d_fverts, n_facets * d));
  FEMO_TRY(dalloc(&e->d_fptr, m->n_vert + 1));
  FEMO_TRY(dalloc(&e->d_flist, (int64_t)list.size()));
  if (n_facets) FEMO_HIP_CHECK(hipMemcpyAsync(e->d_fverts, fv, n_facets * d * sizeof(int32_t), hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(e->d_fptr, ptr.data(), ptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
  if (!list.empty()) FEMO_HIP_CHECK(hipMemcpyAsync(e->d_flist, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  e->n_facets = n_facets;
  return 0;
}

int femo_elast_assemble(femo_elast* e, int method, const femo_vec* rho) {
  FEMO_REQUIRE(e && rho, "null argument");
  FEMO_REQUIRE(method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP, "unknown penalisation method %d", method);
  femo_mesh* m = e->mesh;
  FEMO_REQUIRE(rho->n >= m->n_cell, "density vector too small");
  FEMO_TRY(femo_vec_await(rho));
  const uint8_t* fx = e->has_fixed ? e->d_fixed : nullptr;
  FEMO_TRY(elast_dispatch_d(e->d, [&](auto dim) {
    return elast_launch_rows(e, k_elast_assemble<decltype(dim)::value>, m->d_vptr, m->d_visit_cell, m->d_visit_slots, m->d_mptr,
                             m->d_rowlen, m->d_conn, m->d_x, rho->d, method, e->lam0, e->mu0, fx, e->d_vals, e->d_diag, e->d_dinv);
  }));
  if (e->has_springs)
    FEMO_TRY(elast_dispatch_d(e->d, [&](auto dim) {
      return elast_launch_rows(e, k_elast_springs<decltype(dim)::value>, e->d_springs, fx, e->d_diag, e->d_dinv);
    }));
  e->assembled = true;
  e->pc_dirty = true;
  e->method = method;
  e->rho_uid = rho->uid;
  e->rho_gen = rho->gen;
  // wrapped memory cannot be recognised later: with a lattice plan in place its blocks are built now
  if (e->pc && rho->uid == 0) FEMO_TRY(femo_elast_pc_build(e, rho->d));
  return 0;
}

int femo_elast_load(femo_elast* e, const double* t, femo_vec* F) {
  FEMO_REQUIRE(e && t && F, "null argument");
  femo_mesh* m = e->mesh;
  FEMO_REQUIRE(F->n >= m->n_vert * e->d, "load vector too small");
  FEMO_REQUIRE(e->d_fptr, "femo_elast_load: no tagged facets (femo_elast_set_facets)");
  femo_vec_touch(F);
  const double t2 = e->d == 3 ? t[2] : 0.0;
  return elast_dispatch_d(e->d, [&](auto dim) {      // n_vert = n_rows on the one GPU the elasticity runs on
    return elast_launch_rows(e, k_elast_load<decltype(dim)::value>, e->d_fptr, e->d_flist, e->d_fverts, m->d_x, t[0], t[1], t2, F->d);
  });
}

int femo_elast_drho(femo_elast* e, int method, int transpose, const femo_vec* rho, const femo_vec* u, const femo_vec* x,
                    femo_vec* y, int accumulate) {
  FEMO_REQUIRE(e && rho && u && x && y, "null argument");
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d;
  FEMO_REQUIRE(rho->n >= m->n_cell && u->n >= n, "vector size mismatch in femo_elast_drho");
  FEMO_REQUIRE(transpose ? (x->n >= n && y->n >= m->n_cell) : (x->n >= m->n_cell && y->n >= n), "vector size mismatch in femo_elast_drho");
  return drho_cols(e, method, transpose, 1, rho, u, x, y, accumulate, "femo_elast_drho");
}

int femo_elast_drho_multi(femo_elast* e, int method, int transpose, int n_cols, const femo_vec* rho, const femo_vec* u,
                          const femo_vec* x, femo_vec* y, int accumulate) {
  FEMO_REQUIRE(e && rho && u && x && y, "null argument");
  FEMO_REQUIRE(n_cols >= 1 && n_cols <= FEMO_ELAST_MAX_COLS, "femo_elast_drho_multi: %d columns (1 to %d)", n_cols,
               FEMO_ELAST_MAX_COLS);
  femo_mesh* m = e->mesh;
  const int64_t n = m->n_vert * e->d, nl = n * n_cols;
  FEMO_REQUIRE(rho->n >= m->n_cell && u->n >= nl, "vector size mismatch in femo_elast_drho_multi");
  FEMO_REQUIRE(transpose ? (x->n >= nl && y->n >= m->n_cell) : (x->n >= m->n_cell && y->n >= nl),
               "vector size mismatch in femo_elast_drho_multi");
  return drho_cols(e, method, transpose, n_cols, rho, u, x, y, accumulate, "femo_elast_drho_multi");
}

int femo_elast_export_csr(const femo_elast* e, int64_t* rowptr, int32_t* col, double* val) {
  FEMO_REQUIRE(e && rowptr && col && val, "null argument");
  FEMO_REQUIRE(e->assembled, "femo_elast_export_csr: assemble K first");
  const femo_mesh* m = e->mesh;
  FEMO_TRY(femo_mesh_pattern_csr(m, rowptr, col));
  const int64_t dd = (int64_t)e->d * e->d;
  hipStream_t st = m->ctx->stream;
  int64_t* d_rp = nullptr; int32_t* d_col = nullptr; double* d_val = nullptr;
  FEMO_TRY(dalloc(&d_rp, m->n_rows + 1));
  FEMO_TRY(dalloc(&d_col, m->nnz));
  FEMO_TRY(dalloc(&d_val, m->nnz * dd));
  FEMO_HIP_CHECK(hipMemcpyAsync(d_rp, rowptr, (m->n_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  FEMO_TRY(elast_dispatch_d(e->d, [&](auto dim) {
    return elast_launch_rows(e, k_elast_export<decltype(dim)::value>, m->d_mptr, m->d_cols, m->d_rowlen, m->d_rowreal, e->d_diag,
                             e->d_vals, d_rp, d_col, d_val);
  }));
  FEMO_HIP_CHECK(hipMemcpyAsync(col, d_col, m->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(val, d_val, m->nnz * dd * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  hipFree(d_rp); hipFree(d_col); hipFree(d_val);
  return 0;
}

int femo_elast_bench_spmv(femo_elast* e, const femo_vec* x, femo_vec* y, int reps, double* ms) {
  FEMO_REQUIRE(e && x && y && ms && reps > 0, "null argument");
  FEMO_REQUIRE(e->assembled, "femo_elast_bench_spmv: assemble K first");
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(x->n >= n && y->n >= n && x != y, "vector size mismatch in femo_elast_bench_spmv");
  hipStream_t st = e->mesh->ctx->stream;
  femo_vec_touch(y);
  FEMO_TRY(femo_elast_spmv(e, false, 1, 1.0, x->d, 0.0, nullptr, y->d, nullptr, 0, nullptr));     // warm-up
  FEMO_HIP_CHECK(hipEventRecord(e->mesh->ctx->ev0, st));
  for (int k = 0; k < reps; ++k) FEMO_TRY(femo_elast_spmv(e, false, 1, 1.0, x->d, 0.0, nullptr, y->d, nullptr, 0, nullptr));
  FEMO_HIP_CHECK(hipEventRecord(e->mesh->ctx->ev1, st));
  FEMO_HIP_CHECK(hipEventSynchronize(e->mesh->ctx->ev1));
  float t = 0.0f;
  FEMO_HIP_CHECK(hipEventElapsedTime(&t, e->mesh->ctx->ev0, e->mesh->ctx->ev1));
  *ms = t / reps;
  return 0;
}

// ------------------------------------------------------------------------------------------------ filter ----
int femo_filter_create(femo_ctx* ctx, int dim, int64_t n, const double* coords, double radius, femo_filter** out) {
  FEMO_REQUIRE(ctx && coords && out, "null argument");
  FEMO_REQUIRE(dim == 2 || dim == 3, "filter: dim must be 2 or 3");
  FEMO_REQUIRE(n > 0 && n < INT32_MAX, "filter: bad point count");
  FEMO_REQUIRE(radius > 0.0 && std::isfinite(radius), "filter: radius must be positive");
  // uniform grid, cell size >= r (the 3^d cells around a point hold every neighbour), at most ~ 4 n + 1024 cells
  Grid G{};
  int64_t ncell = 1;
  FEMO_REQUIRE(filter_grid_plan(dim, n, coords, radius, &G, &ncell) == FILTER_GRID_OK, "filter: coordinates must be finite");
  hipStream_t st = ctx->stream;
  auto* F = new femo_filter();
  F->ctx = ctx;
  F->n = n;
  double* d_x = nullptr; int64_t* d_cid = nullptr; unsigned long long* d_cnt = nullptr; int64_t* d_start = nullptr;
  int32_t* d_bucket = nullptr; double* d_S = nullptr;
  auto fail = [&](int rc) { hipFree(d_x); hipFree(d_cid); hipFree(d_cnt); hipFree(d_start); hipFree(d_bucket); hipFree(d_S);
                            femo_filter_destroy(F); return rc; };
  if (dalloc(&d_x, n * dim) || dalloc(&d_cid, n) || dalloc(&d_cnt, std::max(ncell, n)) || dalloc(&d_start, std::max(ncell, n) + 1) ||
      dalloc(&d_bucket, n) || dalloc(&d_S, n) || dalloc(&F->d_rowptr, n + 1))
    return fail(1);
  if (hipMemcpyAsync(d_x, coords, n * dim * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(d_cnt, 0, ncell * sizeof(unsigned long long), st) != hipSuccess) {
    femo_set_error("femo_filter_create: copy failed"); return fail(1);
  }
  const unsigned gn = grid_of(n), gc = grid_of(ncell);
  if (dim == 2) hipLaunchKernelGGL(k_f_bin<2>, dim3(gn), dim3(EB), 0, st, n, d_x, G, d_cid, d_cnt);
  else hipLaunchKernelGGL(k_f_bin<3>, dim3(gn), dim3(EB), 0, st, n, d_x, G, d_cid, d_cnt);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, ncell, d_cnt, d_start);
  hipMemsetAsync(d_cnt, 0, ncell * sizeof(unsigned long long), st);
  hipLaunchKernelGGL(k_f_fill, dim3(gn), dim3(EB), 0, st, n, d_cid, d_start, d_cnt, d_bucket);
  hipLaunchKernelGGL(k_f_sort_buckets, dim3(gc), dim3(EB), 0, st, ncell, d_start, d_bucket);
  // rows: count, scan, fill + sort
  unsigned long long* d_rowcnt = d_cnt;      // reused (n entries fit: allocated max(ncell, n))
  if (dim == 2) hipLaunchKernelGGL((k_f_rows<2, 0>), dim3(gn), dim3(EB), 0, st, n, d_x, G, radius, d_start, d_bucket, d_rowcnt, nullptr, nullptr, nullptr);
  else hipLaunchKernelGGL((k_f_rows<3, 0>), dim3(gn), dim3(EB), 0, st, n, d_x, G, radius, d_start, d_bucket, d_rowcnt, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, n, d_rowcnt, F->d_rowptr);
  if (hipGetLastError() != hipSuccess ||
      hipMemcpyAsync(&F->nnz, F->d_rowptr + n, sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    femo_set_error("femo_filter_create: grid passes failed"); return fail(1);
  }
  if (dalloc(&F->d_col, F->nnz) || dalloc(&F->d_val, F->nnz) || dalloc(&F->d_valT, F->nnz)) return fail(1);
  if (dim == 2) hipLaunchKernelGGL((k_f_rows<2, 1>), dim3(gn), dim3(EB), 0, st, n, d_x, G, radius, d_start, d_bucket, nullptr, F->d_rowptr, F->d_col, F->d_valT);
  else hipLaunchKernelGGL((k_f_rows<3, 1>), dim3(gn), dim3(EB), 0, st, n, d_x, G, radius, d_start, d_bucket, nullptr, F->d_rowptr, F->d_col, F->d_valT);
  hipLaunchKernelGGL(k_f_rowsum, dim3(gn), dim3(EB), 0, st, n, F->d_rowptr, F->d_valT, d_S);
  hipLaunchKernelGGL(k_f_weights, dim3(gn), dim3(EB), 0, st, n, F->d_rowptr, F->d_col, d_S, F->d_val, F->d_valT);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    femo_set_error("femo_filter_create: row passes failed"); return fail(1);
  }
  hipFree(d_x); hipFree(d_cid); hipFree(d_cnt); hipFree(d_start); hipFree(d_bucket); hipFree(d_S);
  *out = F;
  return 0;
}

int femo_filter_destroy(femo_filter* f) {
  if (!f) return 0;
  hipFree(f->d_rowptr); hipFree(f->d_col); hipFree(f->d_val); hipFree(f->d_valT);
  delete f;
  return 0;
}

int femo_filter_nnz(const femo_filter* f, int64_t* nnz) {
  FEMO_REQUIRE(f && nnz, "null argument");
  *nnz = f->nnz;
  return 0;
}

int femo_filter_apply(femo_filter* f, int transpose, const femo_vec* x, femo_vec* y) {
  FEMO_REQUIRE(f && x && y, "null argument");
  FEMO_REQUIRE(x->n >= f->n && y->n >= f->n && x != y, "vector size mismatch in femo_filter_apply");
  FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(y);
  hipLaunchKernelGGL(k_f_apply, dim3(grid_of(f->n)), dim3(EB), 0, f->ctx->stream, f->n, f->d_rowptr, f->d_col,
                     transpose ? f->d_valT : f->d_val, x->d, y->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_filter_export_csr(const femo_filter* f, int transpose, int64_t* rowptr, int32_t* col, double* val) {
  FEMO_REQUIRE(f && rowptr && col && val, "null argument");
  hipStream_t st = f->ctx->stream;
  FEMO_HIP_CHECK(hipMemcpyAsync(rowptr, f->d_rowptr, (f->n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(col, f->d_col, f->nnz * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(val, transpose ? f->d_valT : f->d_val, f->nnz * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"
