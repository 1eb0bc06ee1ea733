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
// note_pinned_vertices (api.hip) does, so femo_solve_cg solves them up front as it does for Poisson.
//
// Solves.  The default is the Jacobi-scaled femo_solve_cg.  With pc = FEMO_PC_BPX the solve runs the auxiliary-lattice BPX of
// bpx.hip with level weights taken from this operator (tests/cond_pc_ref.py restates them):
//   C_l[I] = keep_l[I] theta / G_l[I],   G_l[I] = (Pt_l^T A Pt_l)_II = sum_c k(rho_c) |T_c| | sum_{a in c} w_aI free_a grad lambda_a |^2,
// Pt_l the multilinear interpolation from lattice l straight to the vertices in fp64, zero rows on the fixed vertices.  The stock
// weights are the unit Laplacian's; k(rho) ranges over three decades.  The assembly records the fixed set for the
// preconditioner as note_pinned_vertices does and sets bpx_ok; k_cond_pc_diag forms G of every level once per assembly, inside
// the first BPX solve (or pc_apply / export) behind it, so the state and the adjoint solve of a cycle share one build.  G lives
// in the handle and is named by the generation of the matrix it was formed from: the coefficient arrays of the mesh's
// hierarchy are cached under that generation (bpx.hip: pc_prepare), a refused call leaves nothing behind that the next
// assembly would read.  The sums of G are fp64 atomics: the weights, and a solution through them, repeat to rounding, not
// bit for bit.
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
  // Galerkin diagonals of all lattice levels (layout of the hierarchy's coefficient arrays), formed from the matrix of
  // generation G_gen with the law and density of the last assembly
  double* d_G = nullptr;
  int64_t G_n = 0;
  uint64_t G_gen = 0;
  int64_t G_builds = 0;
  int method = 0;
  double k0 = 0.0, kmin = 0.0;
  const double* d_rho = nullptr;   // the density of the last assembly: read again by the first BPX solve behind it
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

// ---- level weights of the lattice preconditioner -----------------------------------------------------------------------
constexpr int CPC_LDS_DOUBLES = 2048;      // 16 KiB of accumulators per workgroup: levels of at most this many nodes
constexpr int CPC_LDS_GRID = 256;          // workgroups (= flushes) of an LDS-accumulated level

// G_l[I] += k(rho_c) |T_c| |g_I|^2, g_I = sum_a w_aI free_a grad lambda_a, for the nodes I of the cell's bin range on level
// l (jittered cells straddle lattice lines: the range is not 2^D nodes).  One thread per cell.  The hats are evaluated from
// the bin and fraction of each vertex on THIS level, in fp64 from the coordinates.  LDS: the level fits in the workgroup's
// accumulators, flushed once per workgroup -- 400 k cells adding into a six-node lattice must not serialise on six addresses.
template <int D, bool LDS>
__global__ __launch_bounds__(EB) void k_cond_pc_diag(int64_t n_cell, const int32_t* __restrict__ conn, const double* __restrict__ x,
                                                     int method, double k0, double kmin, const double* __restrict__ rho,
                                                     const uint8_t* __restrict__ fixed, FemoLattice L, double* __restrict__ G) {
  extern __shared__ double acc[];
  if (LDS) {
    for (int64_t i = threadIdx.x; i < L.nodes; i += EB) acc[i] = 0.0;
    __syncthreads();
  }
  double* dst = LDS ? acc : G;
  for (int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x; c < n_cell; c += (int64_t)gridDim.x * EB) {
    int32_t v[D + 1];
    double p[D + 1][D], g[D + 1][D], vol;
    load_cell<D>(conn, x, c, v, p);
    simplex_grads<D>(p, g, vol);
    const double kk = conductivity(method, k0, kmin, rho[c]) * vol;
    int bin[D + 1][D];
    double t[D + 1][D], fr[D + 1];
    int ilo[3] = {0, 0, 0}, ihi[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < D; ++k) {
#pragma unroll
      for (int a = 0; a <= D; ++a) {
        const double s = (p[a][k] - L.lo[k]) * L.inv_h[k];
        int b = (int)floor(s);
        b = b < 0 ? 0 : (b > L.n[k] - 1 ? L.n[k] - 1 : b);
        const double f = s - b;
        bin[a][k] = b;
        t[a][k] = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
        ilo[k] = a == 0 ? b : min(ilo[k], b);
        ihi[k] = a == 0 ? b + 1 : max(ihi[k], b + 1);
      }
    }
#pragma unroll
    for (int a = 0; a <= D; ++a) fr[a] = (fixed && fixed[v[a]]) ? 0.0 : 1.0;
    for (int i2 = ilo[2]; i2 <= ihi[2]; ++i2)
      for (int i1 = ilo[1]; i1 <= ihi[1]; ++i1)
        for (int i0 = ilo[0]; i0 <= ihi[0]; ++i0) {
          const int ijk[3] = {i0, i1, i2};
          double gI[D];
#pragma unroll
          for (int k = 0; k < D; ++k) gI[k] = 0.0;
#pragma unroll
          for (int a = 0; a <= D; ++a) {
            double w = fr[a];
#pragma unroll
            for (int k = 0; k < D; ++k) w *= ijk[k] == bin[a][k] ? 1.0 - t[a][k] : (ijk[k] == bin[a][k] + 1 ? t[a][k] : 0.0);
#pragma unroll
            for (int k = 0; k < D; ++k) gI[k] += w * g[a][k];
          }
          double gg = 0.0;
#pragma unroll
          for (int k = 0; k < D; ++k) gg += gI[k] * gI[k];
          if (gg == 0.0) continue;
          atomicAdd(&dst[((int64_t)i2 * (L.n[1] + 1) + i1) * (L.n[0] + 1) + i0], kk * gg);
        }
  }
  if (LDS) {
    __syncthreads();
    for (int64_t i = threadIdx.x; i < L.nodes; i += EB) {
      const double a = acc[i];
      if (a != 0.0) atomicAdd(&G[i], a);
    }
  }
}

bool cond_method_ok(int method) { return method == FEMO_ELAST_SIMP || method == FEMO_ELAST_RAMP; }

bool cond_law_ok(double k0, double kmin) { return std::isfinite(k0) && std::isfinite(kmin) && kmin >= 0.0 && k0 > kmin; }

void cond_mark(femo_mat* A) {
  A->valsT_valid = false; A->scaled_valid = false; A->s_valid = false; femo_mat_touch(A);
  A->bpx_ok = true;
  A->pc_wt = FemoPcWeighted{};             // the weights of the new content are formed by the first solve that asks for them
}

// the pinned vertices of the preconditioner, as note_pinned_vertices (api.hip) records them for a strong Dirichlet set
int cond_note_pinned(femo_mat* A, const femo_bc* bc) {
  femo_mesh* m = A->mesh;
  const bool strong = bc != nullptr && bc->n > 0;
  const uint64_t key = 1 + (strong ? bc->uid << 20 : 0);
  if (A->pc_key == key) return 0;
  A->pc_has_mask = strong;
  if (strong) {
    const int64_t nb = std::max<int64_t>(m->n_vert, 1) + 64;
    if (!A->d_pcmask) FEMO_HIP_CHECK(hipMalloc(&A->d_pcmask, nb));
    FEMO_HIP_CHECK(hipMemcpyAsync(A->d_pcmask, bc->d_mask, nb, hipMemcpyDeviceToDevice, m->ctx->stream));
  }
  A->pc_key = key;
  return 0;
}

femo_mat* cond_solved(femo_cond* c) { return c->has_fixed ? c->A : c->K; }

// G of every level for the matrix the solves use, once per assembly
int cond_ensure_weights(femo_cond* c) {
  femo_mat* A = cond_solved(c);
  femo_mesh* m = c->mesh;
  if (c->G_gen == A->gen && A->pc_wt.G != nullptr) return 0;
  FEMO_TRY(femo_pc_build(m));
  FemoLattice L;
  FEMO_TRY(femo_pc_lattice(m, 0, &L));
  if (c->G_n < L.total) {
    if (c->d_G) FEMO_HIP_CHECK(hipFree(c->d_G));
    c->d_G = nullptr; c->G_n = 0;
    FEMO_HIP_CHECK(hipMalloc(&c->d_G, (size_t)L.total * sizeof(double)));
    c->G_n = L.total;
  }
  hipStream_t st = c->ctx->stream;
  FEMO_HIP_CHECK(hipMemsetAsync(c->d_G, 0, (size_t)L.total * sizeof(double), st));
  const uint8_t* fixed = c->has_fixed ? (const uint8_t*)A->d_idrows : (const uint8_t*)nullptr;
  int nl = 0;
  int64_t finest = 0;
  FEMO_TRY(femo_pc_levels(m, &nl, &finest));
  for (int l = 0; l < nl; ++l) {
    FEMO_TRY(femo_pc_lattice(m, l, &L));
    double* G = c->d_G + L.offset;
#define COND_DIAG(DIM)                                                                                                          \
  if (L.nodes <= CPC_LDS_DOUBLES)                                                                                               \
    hipLaunchKernelGGL((k_cond_pc_diag<DIM, true>), dim3(std::min<unsigned>(grid_of(m->n_cell), CPC_LDS_GRID)), dim3(EB),       \
                       (size_t)L.nodes * sizeof(double), st, m->n_cell, m->d_conn, m->d_x, c->method, c->k0, c->kmin, c->d_rho, \
                       fixed, L, G);                                                                                            \
  else                                                                                                                          \
    hipLaunchKernelGGL((k_cond_pc_diag<DIM, false>), dim3(grid_of(m->n_cell)), dim3(EB), 0, st, m->n_cell, m->d_conn, m->d_x,   \
                       c->method, c->k0, c->kmin, c->d_rho, fixed, L, G)
    if (m->tdim == 2) { COND_DIAG(2); } else { COND_DIAG(3); }
#undef COND_DIAG
  }
  FEMO_HIP_CHECK(hipGetLastError());
  c->G_gen = A->gen;
  ++c->G_builds;
  A->pc_wt.G = c->d_G;
  A->pc_wt.gen = A->gen;
  return 0;
}

}  // namespace

extern "C" int femo_cond_destroy(femo_cond* c) {
  if (!c) return 0;
  femo_mat_destroy(c->K);
  femo_mat_destroy(c->A);
  (void)hipFree(c->d_G);
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
  FEMO_TRY(cond_note_pinned(fx ? c->A : c->K, fx ? bc : nullptr));
  c->has_fixed = fx;
  c->assembled = false;
  c->method = method; c->k0 = k0; c->kmin = k_min; c->d_rho = rho->d;
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
  FEMO_REQUIRE(o.pc == FEMO_PC_JACOBI || o.pc == FEMO_PC_BPX, "conduction: unknown preconditioner %d (FEMO_PC_JACOBI or FEMO_PC_BPX)", o.pc);
  FEMO_REQUIRE(std::isfinite(o.rtol) && o.rtol >= 0.0 && std::isfinite(o.atol) && o.atol >= 0.0, "conduction: bad tolerances");
  if (o.pc == FEMO_PC_BPX) {
    FEMO_REQUIRE(std::isfinite(o.atol_pc) && o.atol_pc >= 0.0, "conduction: bad tolerances");
    FEMO_TRY(cond_ensure_weights(c));
  }
  femo_solve_info si = {};
  FEMO_TRY(femo_solve_cg(cond_solved(c), 0, b, x, &o, &si));
  c->last = si;
  if (info) *info = si;
  FEMO_REQUIRE(std::isfinite(si.rhs_norm) && si.converged != -1,
               "conduction: the density or the right-hand side is not finite (load norm %g after %d iterations)", si.rhs_norm,
               (int)si.iterations);
  return 0;
}

extern "C" int femo_cond_pc_apply(femo_cond* c, const femo_vec* r, femo_vec* z) {
  FEMO_REQUIRE(c && r && z, "null argument");
  FEMO_REQUIRE(c->assembled, "conduction: pc_apply before femo_cond_assemble");
  FEMO_REQUIRE(r->n >= c->mesh->n_rows && z->n >= c->mesh->n_rows && r != z, "conduction: vector size mismatch or aliasing in pc_apply");
  FEMO_TRY(femo_vec_await(r));
  FEMO_TRY(cond_ensure_weights(c));
  return femo_mat_pc_apply(cond_solved(c), r, z);
}

extern "C" int femo_cond_pc_info(femo_cond* c, int64_t* out, int count) {
  FEMO_REQUIRE(c && out && count >= 2, "null argument");
  FEMO_TRY(femo_pc_build(c->mesh));
  int nl = 0;
  int64_t finest = 0;
  FEMO_TRY(femo_pc_levels(c->mesh, &nl, &finest));
  out[0] = nl;
  out[1] = c->G_builds;
  for (int l = 0; l < nl && 2 + l < count; ++l) {
    FemoLattice L;
    FEMO_TRY(femo_pc_lattice(c->mesh, l, &L));
    out[2 + l] = L.nodes;
  }
  return 0;
}

extern "C" int femo_cond_pc_export_level(femo_cond* c, int level, double* coef) {
  FEMO_REQUIRE(c && coef, "null argument");
  FEMO_REQUIRE(c->assembled, "conduction: pc_export_level before femo_cond_assemble");
  FEMO_TRY(cond_ensure_weights(c));
  femo_mat* A = cond_solved(c);
  femo_mesh* m = c->mesh;
  // the coefficient arrays as a solve of this operator finds them: the begin of a solve names the operator
  FEMO_TRY(femo_mat_ensure_s(A));
  const uint8_t* mask = A->pc_has_mask ? A->d_pcmask : nullptr;
  FEMO_TRY(femo_pc_begin(m, A->d_s, mask, femo_pc_weights_key(A), &A->pc_wt));
  const double* d = nullptr;
  int64_t n = 0;
  FEMO_TRY(femo_pc_level_coef(m, mask, A->pc_key, level, &d, &n));
  FEMO_HIP_CHECK(hipMemcpyAsync(coef, d, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->ctx->stream));
  FEMO_HIP_CHECK(hipStreamSynchronize(c->ctx->stream));
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
