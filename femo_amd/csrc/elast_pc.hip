// Additive multilevel preconditioner of the SIMP elasticity solves (C-ABI in include/femo_hip.h, "femo_elast_pc_*"):
//
//   M^-1 = D_blk^-1 + sum_l P_l C_l P_l^T,      C_l = blockdiag_d(P_l^T A P_l)^-1
//
// Lattices.  Level 0 has one bin along the shortest axis of the mesh's bounding box, level l + 1 halves the spacing of
// level l, so the lattices are nested and P_l = P_L T_{L->l} with L the finest level and T the multilinear transfer
// between lattices.  The apply therefore touches mesh-sized data on the finest lattice only:
//
//   g_L = P_L^T r                     k_pc_restrict_mesh   node-centric gather over a (node -> vertex, weight) CSR built at
//                                                          set-up, a group of lanes per node, fixed-order sums: no atomics
//   s_L = C_L g_L, g_L-1 = T^T g_L    k_pc_lat_restrict    one thread per lattice node
//   levels L-1 .. 0 down, scale, up   k_pc_coarse          ONE workgroup, a barrier between levels (the lattices below the
//                                                          finest hold a few thousand nodes)
//   z = D^-1 r + P_L s_L + P_L-1 e    k_pc_final           the x / r update, p = z on the first call and the partial r.z of
//                                                          k_pcg_precond, plus two multilinear gathers per vertex
//
// The four kernels carry a column in the grid -- blockIdx.y, for k_pc_coarse one workgroup per column -- so one step serves
// the L load cases of a batched solve (femo_elast_pc_step) on L copies of the lattice work vectors; a single solve and
// femo_elast_pc_apply are the step with L = 1.  The Galerkin blocks are shared.
//
// A vertex keeps its finest-lattice bin (int32 per axis) and fraction (fp64 per axis); the bin and fraction on level L - 1
// follow exactly (bin >> 1, (frac + (bin & 1)) / 2).  The restriction CSR carries the products of the same fractions, so
// the restriction is the exact transpose of the gather.
//
// Galerkin blocks (k_pc_blocks, once per assembled K, fixed set or set of springs; with elastic supports k_pc_springs adds
// P_l^T diag(k) P_l behind it).  With g_r = sum_a w_aI m_ar grad(lambda_a) -- w_aI the
// hat of node I at vertex a, m_ar = 0 on a fixed dof -- cell e adds C(rho_e) |T_e| (lam0 g_r[r] g_c[c] + mu0 (g_r[c] g_c[r]
// + delta_rc g_r . g_c)) to entry (r, c) of the block of node I.  The hats are evaluated at the nodes of the cell's bin
// range, so a cell that straddles bins needs no de-duplication.  Fine levels add with fp64 atomics straight into the
// lattice; levels of at most PC_LDS_DOUBLES / d^2 nodes accumulate per workgroup in LDS and flush once per workgroup.
#include "elast_internal.h"

#include <algorithm>
#include <cmath>

constexpr int PC_ML = FEMO_ELAST_PC_MAX_LEVELS;
constexpr int PC_LDS_DOUBLES = 2048;       // 16 KiB of block accumulators per workgroup
constexpr int PC_LDS_GRID = 256;           // workgroups (= flushes) of an LDS-accumulated level
constexpr int PC_COARSE_NT = 1024;
constexpr int64_t PC_COARSE_MAX_NODES = 1 << 18;   // largest second-finest lattice the one-workgroup sweep is asked to carry
constexpr double PC_DEFAULT_SPACING = 2.0;
constexpr double PC_SNAP = 1e-9;           // finest-lattice coordinates this close to a lattice line are moved onto it

struct PcLat {
  int n[3];              // bins per axis (0 along z in 2-D: one node)
  int64_t nodes;
  double inv_h;
};
struct PcLevels {
  int n_levels;
  PcLat lat[PC_ML];
  int64_t off[PC_ML + 1];   // first node of each level in the concatenated arrays
  double lo[3];
};

struct femo_elast_pc {
  PcLevels P{};
  double H[PC_ML] = {};
  double* d_G = nullptr;        // total nodes * d^2: Galerkin blocks
  double* d_C = nullptr;        // total nodes * d^2: their inverses
  double* d_g = nullptr;        // cols * total nodes * d: restricted residual, one column after the other
  double* d_e = nullptr;        // cols * total nodes * d: corrections
  int cols = 0;                 // one from femo_elast_pc_setup, grown by the step
  int32_t* d_vbin = nullptr;    // n_vert * d
  double* d_vfrac = nullptr;    // n_vert * d
  int64_t* d_rptr = nullptr;    // finest nodes + 1
  int32_t* d_rvert = nullptr;
  double* d_rw = nullptr;
  int64_t r_entries = 0;
  int64_t bytes = 0, builds = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {

inline unsigned pc_grid(int64_t n, int nt = EB) {
  int64_t g = (n + nt - 1) / nt;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(g, 1 << 20));
}

template <typename T>
int pc_alloc(T** p, int64_t n) {
  FEMO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), (size_t)std::max<int64_t>(n, 1) * sizeof(T)));
  return 0;
}

// Coordinate of a point on the finest lattice, in bins.  A vertex a round-off away from a lattice line must not reach the
// nodes beyond the line with a weight of 1e-17: such a node would get a block, and a correction, made of noise.
__host__ __device__ inline double pc_coord(double x, double lo, double inv_h, int n) {
  double t = (x - lo) * inv_h;
  const double tr = rint(t);
  if (fabs(t - tr) < PC_SNAP) t = tr;
  return t < 0.0 ? 0.0 : (t > (double)n ? (double)n : t);
}

__host__ __device__ inline int64_t pc_node(const PcLat& L, int i0, int i1, int i2) {
  return i0 + (int64_t)(L.n[0] + 1) * (i1 + (int64_t)(L.n[1] + 1) * i2);
}

// ------------------------------------------------------------------------------------------- Galerkin blocks ----
template <int D, bool LDS>
__global__ __launch_bounds__(EB) void k_pc_blocks(int64_t n_cell, const int32_t* __restrict__ conn, const double* __restrict__ x,
                                                  const double* __restrict__ rho, int method, double lam, double mu,
                                                  const uint8_t* __restrict__ fixed, PcLat L, PcLat F, double to_level, double lo0,
                                                  double lo1, double lo2, double* __restrict__ G) {
  constexpr int DD = D * D;
  extern __shared__ double acc[];
  const int64_t nacc = L.nodes * DD;
  if (LDS) {
    for (int64_t i = threadIdx.x; i < nacc; i += EB) acc[i] = 0.0;
    __syncthreads();
  }
  double* dst = LDS ? acc : G;
  const double lo[3] = {lo0, lo1, lo2};
  for (int64_t c = (int64_t)blockIdx.x * EB + threadIdx.x; c < n_cell; c += (int64_t)gridDim.x * EB) {
    int32_t v[D + 1];
    double p[D + 1][D], g[D + 1][D], vol;
    load_cell<D>(conn, x, c, v, p);
    simplex_grads<D>(p, g, vol);
    const double coef = penal(method, rho[c]) * vol;
    double t[D + 1][D], m[D + 1][D];
    int ilo[3] = {0, 0, 0}, ihi[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double tmin = 0.0, tmax = 0.0;
#pragma unroll
      for (int a = 0; a <= D; ++a) {
        const double s = pc_coord(p[a][k], lo[k], F.inv_h, F.n[k]) * to_level;     // a power of two: exact
        t[a][k] = s;
        tmin = a == 0 ? s : fmin(tmin, s);
        tmax = a == 0 ? s : fmax(tmax, s);
      }
      ilo[k] = (int)floor(tmin);
      ihi[k] = min(L.n[k], (int)floor(tmax) + 1);
    }
#pragma unroll
    for (int a = 0; a <= D; ++a)
#pragma unroll
      for (int r = 0; r < D; ++r) m[a][r] = (fixed && fixed[(int64_t)v[a] * D + r]) ? 0.0 : 1.0;
    for (int i2 = ilo[2]; i2 <= ihi[2]; ++i2)
      for (int i1 = ilo[1]; i1 <= ihi[1]; ++i1)
        for (int i0 = ilo[0]; i0 <= ihi[0]; ++i0) {
          const int ijk[3] = {i0, i1, i2};
          double w[D + 1], wsum = 0.0;
#pragma unroll
          for (int a = 0; a <= D; ++a) {
            double ww = 1.0;
#pragma unroll
            for (int k = 0; k < D; ++k) ww *= fmax(0.0, 1.0 - fabs(t[a][k] - (double)ijk[k]));
            w[a] = ww;
            wsum += ww;
          }
          if (wsum == 0.0) continue;
          double Gr[D][D];       // Gr[r][k] = k-th component of g_r
#pragma unroll
          for (int r = 0; r < D; ++r)
#pragma unroll
            for (int k = 0; k < D; ++k) {
              double s = 0.0;
#pragma unroll
              for (int a = 0; a <= D; ++a) s += w[a] * m[a][r] * g[a][k];
              Gr[r][k] = s;
            }
          const int64_t node = pc_node(L, i0, i1, i2);
#pragma unroll
          for (int r = 0; r < D; ++r)
#pragma unroll
            for (int cc = r; cc < D; ++cc) {
              double val = lam * Gr[r][r] * Gr[cc][cc] + mu * Gr[r][cc] * Gr[cc][r];
              if (r == cc) {
#pragma unroll
                for (int k = 0; k < D; ++k) val += mu * Gr[r][k] * Gr[r][k];
              }
              val *= coef;
              if (val != 0.0) atomicAdd(&dst[node * DD + r * D + cc], val);
            }
        }
  }
  if (LDS) {
    __syncthreads();
    for (int64_t i = threadIdx.x; i < nacc; i += EB) {
      const double a = acc[i];
      if (a != 0.0) atomicAdd(&G[i], a);
    }
  }
}

// Elastic supports in the blocks: P_l^T diag(k) P_l adds w_vI^2 k[d v + r] to entry (r, r) of the block of every node I under
// whose hat vertex v lies (fixed dofs skipped: their row of P_l is zero).  One thread per vertex; the bin and fraction on
// level L - shift follow from the finest ones as in k_pc_final, one halving per level, so P_l is that of the apply.  fp64
// atomics like k_pc_blocks, behind its launches on the same stream: straight into the lattice on fine levels, per workgroup in
// LDS with one flush on the levels that fit (a foundation under every vertex would otherwise send n_vert 2^d d atomics to the
// handful of addresses of the coarsest levels).
template <int D, bool LDS>
__global__ __launch_bounds__(EB) void k_pc_springs(int64_t n_vert, const double* __restrict__ k, const uint8_t* __restrict__ fixed,
                                                   const int32_t* __restrict__ vbin, const double* __restrict__ vfrac, PcLat L,
                                                   int shift, double* __restrict__ G) {
  constexpr int DD = D * D;
  extern __shared__ double acc[];
  const int64_t nacc = L.nodes * DD;
  if (LDS) {
    for (int64_t i = threadIdx.x; i < nacc; i += EB) acc[i] = 0.0;
    __syncthreads();
  }
  double* dst = LDS ? acc : G;
  for (int64_t v = (int64_t)blockIdx.x * EB + threadIdx.x; v < n_vert; v += (int64_t)gridDim.x * EB) {
    double kr[D];
    bool any = false;
#pragma unroll
    for (int r = 0; r < D; ++r) {
      kr[r] = (fixed && fixed[v * D + r]) ? 0.0 : k[v * D + r];
      any = any || kr[r] != 0.0;
    }
    if (!any) continue;
    int b[D];
    double f[D];
#pragma unroll
    for (int i = 0; i < D; ++i) { b[i] = vbin[v * D + i]; f[i] = vfrac[v * D + i]; }
    for (int s = 0; s < shift; ++s) {
#pragma unroll
      for (int i = 0; i < D; ++i) { f[i] = 0.5 * (f[i] + (double)(b[i] & 1)); b[i] >>= 1; }
    }
    for (int corner = 0; corner < (1 << D); ++corner) {
      int ijk[3] = {0, 0, 0};
      double w = 1.0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const int up = (corner >> i) & 1;
        ijk[i] = b[i] + up;
        w *= up ? f[i] : 1.0 - f[i];
      }
      if (w == 0.0) continue;
      const int64_t node = pc_node(L, ijk[0], ijk[1], ijk[2]);
#pragma unroll
      for (int r = 0; r < D; ++r)
        if (kr[r] != 0.0) atomicAdd(&dst[node * DD + r * D + r], w * w * kr[r]);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int64_t i = threadIdx.x; i < nacc; i += EB) {
      const double a = acc[i];
      if (a != 0.0) atomicAdd(&G[i], a);
    }
  }
}

// upper triangle -> full block, and its inverse; a component with a zero diagonal (no free dof touches it) gets a zero
// row and column
template <int D>
__global__ __launch_bounds__(EB) void k_pc_invert(int64_t n_nodes, double* __restrict__ G, double* __restrict__ C) {
  constexpr int DD = D * D;
  for (int64_t i = (int64_t)blockIdx.x * EB + threadIdx.x; i < n_nodes; i += (int64_t)gridDim.x * EB) {
  double B[DD], W[DD], Wi[DD];
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c) B[r * D + c] = G[i * DD + (r <= c ? r * D + c : c * D + r)];
  bool dead[D];
#pragma unroll
  for (int r = 0; r < D; ++r) dead[r] = B[r * D + r] == 0.0;
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c) W[r * D + c] = (dead[r] || dead[c]) ? (r == c ? 1.0 : 0.0) : B[r * D + c];
  block_inverse<D>(W, Wi);
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c) {
      G[i * DD + r * D + c] = B[r * D + c];
      C[i * DD + r * D + c] = (dead[r] || dead[c]) ? 0.0 : Wi[r * D + c];
    }
  }
}

// ------------------------------------------------------------------------------------------------- apply ----
// blockIdx.y of the kernels below is the column (k_pc_coarse: blockIdx.x).  vs: column stride of the mesh vectors, ls: of
// the lattice vectors, ps: of the partials.
// g_L[node] = sum over the vertices under the node's hat of w (r - alpha q), fixed dofs skipped.  GL lanes per node.
template <int D, int GL, bool UPDATE>
__global__ __launch_bounds__(EB) void k_pc_restrict_mesh(int64_t nodes, const int64_t* __restrict__ rptr,
                                                         const int32_t* __restrict__ rvert, const double* __restrict__ rw,
                                                         const double* __restrict__ r, const double* __restrict__ q,
                                                         const double* __restrict__ s, const uint8_t* __restrict__ fixed,
                                                         const int32_t* __restrict__ flag, double* __restrict__ g,
                                                         int64_t vs, int64_t ls) {
  const int64_t col = blockIdx.y;
  r += col * vs; s += col * EMS_STRIDE; flag += col * EMF_STRIDE; g += col * ls;
  if (UPDATE) q += col * vs;
  if (UPDATE && flag[0]) return;
  const double alpha = UPDATE ? s[S_ALPHA] : 0.0;
  const int lane = threadIdx.x % GL;
  const int64_t per_grid = (int64_t)gridDim.x * (EB / GL);
  // every thread makes the same number of trips, so the shuffles below always see whole groups
  for (int64_t base = 0; base < nodes; base += per_grid) {
  const int64_t node = base + ((int64_t)blockIdx.x * EB + threadIdx.x) / GL;
  double acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.0;
  if (node < nodes) {
    const int64_t e1 = rptr[node + 1];
    for (int64_t k = rptr[node] + lane; k < e1; k += GL) {
      const int64_t v = rvert[k];
      const double w = rw[k];
#pragma unroll
      for (int c = 0; c < D; ++c) {
        double val = r[v * D + c];
        if (UPDATE) val = fma(-alpha, q[v * D + c], val);
        if (fixed && fixed[v * D + c]) val = 0.0;
        acc[c] += w * val;
      }
    }
  }
#pragma unroll
  for (int off = GL / 2; off > 0; off >>= 1)
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] += __shfl_xor(acc[c], off, GL);
  if (node < nodes && lane == 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) g[node * D + c] = acc[c];
  }
  }
}

template <int D>
__device__ __forceinline__ void pc_decode(const PcLat& L, int64_t idx, int (&ijk)[3]) {
  ijk[0] = (int)(idx % (L.n[0] + 1));
  const int64_t t = idx / (L.n[0] + 1);
  ijk[1] = (int)(t % (L.n[1] + 1));
  ijk[2] = (int)(t / (L.n[1] + 1));
}

// coarse node J <- the 3^d fine nodes 2J + delta, weight 1/2 per off-centre axis
template <int D>
__device__ __forceinline__ void pc_restrict_node(const PcLat& F, const PcLat& Cc, int64_t idx, const double* gF, double* gC) {
  int J[3];
  pc_decode<D>(Cc, idx, J);
  double acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.0;
  const int dz = D == 3 ? 1 : 0;
  for (int o2 = -dz; o2 <= dz; ++o2)
    for (int o1 = -1; o1 <= 1; ++o1)
      for (int o0 = -1; o0 <= 1; ++o0) {
        const int f0 = 2 * J[0] + o0, f1 = 2 * J[1] + o1, f2 = 2 * J[2] + o2;
        if (f0 < 0 || f0 > F.n[0] || f1 < 0 || f1 > F.n[1] || f2 < 0 || f2 > F.n[2]) continue;
        const double w = (o0 ? 0.5 : 1.0) * (o1 ? 0.5 : 1.0) * (o2 ? 0.5 : 1.0);
        const int64_t nf = pc_node(F, f0, f1, f2);
#pragma unroll
        for (int c = 0; c < D; ++c) acc[c] += w * gF[nf * D + c];
      }
#pragma unroll
  for (int c = 0; c < D; ++c) gC[idx * D + c] = acc[c];
}

// e_F[i] = C_F g_F[i] + (T e_C)[i]; eC == null: no coarser level
template <int D>
__device__ __forceinline__ void pc_prolong_node(const PcLat& F, const PcLat& Cc, int64_t idx, const double* __restrict__ CF,
                                                const double* gF, const double* eC, double* eF) {
  constexpr int DD = D * D;
  double out[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s += CF[idx * DD + i * D + k] * gF[idx * D + k];
    out[i] = s;
  }
  if (eC) {
    int I[3];
    pc_decode<D>(F, idx, I);
    for (int corner = 0; corner < (1 << D); ++corner) {
      int J[3] = {0, 0, 0};
      double w = 1.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const int up = (corner >> k) & 1;
        if (I[k] & 1) { J[k] = (I[k] >> 1) + up; w *= 0.5; }
        else { J[k] = I[k] >> 1; if (up) w = 0.0; }
      }
      if (w == 0.0) continue;
      const int64_t nc = pc_node(Cc, J[0], J[1], J[2]);
#pragma unroll
      for (int i = 0; i < D; ++i) out[i] += w * eC[nc * D + i];
    }
  }
#pragma unroll
  for (int i = 0; i < D; ++i) eF[idx * D + i] = out[i];
}

// finest level: s_L = C_L g_L (into e_L) and g_L-1 = T^T g_L
template <int D, bool UPDATE>
__global__ __launch_bounds__(EB) void k_pc_lat_restrict(PcLat F, PcLat Cc, int has_coarse, const double* __restrict__ CF,
                                                        const double* __restrict__ gF, double* __restrict__ sF,
                                                        double* __restrict__ gC, const int32_t* __restrict__ flag, int64_t ls) {
  const int64_t col = blockIdx.y;
  gF += col * ls; sF += col * ls; flag += col * EMF_STRIDE;
  if (has_coarse) gC += col * ls;
  if (UPDATE && flag[0]) return;
  for (int64_t idx = (int64_t)blockIdx.x * EB + threadIdx.x; idx < F.nodes; idx += (int64_t)gridDim.x * EB) {
    pc_prolong_node<D>(F, Cc, idx, CF, gF, nullptr, sF);
    if (has_coarse && idx < Cc.nodes) pc_restrict_node<D>(F, Cc, idx, gF, gC);
  }
}

// levels top .. 0 in one workgroup: restrict down from g_top, e_0 = C_0 g_0, e_l = C_l g_l + T e_l-1 up to top.  One
// workgroup per column (blockIdx.x), all of them at once; the Galerkin blocks C are shared
template <int D, bool UPDATE>
__global__ __launch_bounds__(PC_COARSE_NT) void k_pc_coarse(PcLevels P, int top, const double* __restrict__ C, double* g, double* e,
                                                            const int32_t* __restrict__ flag, int64_t ls) {
  constexpr int DD = D * D;
  const int64_t col = blockIdx.x;
  g += col * ls; e += col * ls; flag += col * EMF_STRIDE;
  if (UPDATE && flag[0]) return;
  for (int l = top - 1; l >= 0; --l) {
    for (int64_t idx = threadIdx.x; idx < P.lat[l].nodes; idx += PC_COARSE_NT)
      pc_restrict_node<D>(P.lat[l + 1], P.lat[l], idx, g + P.off[l + 1] * D, g + P.off[l] * D);
    __syncthreads();
  }
  for (int l = 0; l <= top; ++l) {
    for (int64_t idx = threadIdx.x; idx < P.lat[l].nodes; idx += PC_COARSE_NT)
      pc_prolong_node<D>(P.lat[l], P.lat[l > 0 ? l - 1 : 0], idx, C + P.off[l] * DD, g + P.off[l] * D,
                         l > 0 ? e + P.off[l - 1] * D : nullptr, e + P.off[l] * D);
    __syncthreads();
  }
}

template <int D>
__device__ __forceinline__ void pc_gather(const PcLat& L, const int (&b)[D], const double (&f)[D], const double* __restrict__ e,
                                          double (&out)[D]) {
  for (int corner = 0; corner < (1 << D); ++corner) {
    int ijk[3] = {0, 0, 0};
    double w = 1.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const int up = (corner >> k) & 1;
      ijk[k] = b[k] + up;
      w *= up ? f[k] : 1.0 - f[k];
    }
    const int64_t node = pc_node(L, ijk[0], ijk[1], ijk[2]);
#pragma unroll
    for (int i = 0; i < D; ++i) out[i] += w * e[node * D + i];
  }
}

// k_pcg_precond with z = D^-1 r + P_L s_L + P_L-1 e_L-1 (free dofs)
template <int D, bool UPDATE, bool INIT>
__global__ __launch_bounds__(EB) void k_pc_final(int64_t n_rows, const double* __restrict__ dinv, double* __restrict__ x,
                                                 double* __restrict__ r, const double* __restrict__ p,
                                                 const double* __restrict__ q, double* __restrict__ z, double* __restrict__ pinit,
                                                 const double* __restrict__ s, double* __restrict__ part,
                                                 const int32_t* __restrict__ flag, const uint8_t* __restrict__ fixed,
                                                 const int32_t* __restrict__ vbin, const double* __restrict__ vfrac, PcLat F,
                                                 const double* __restrict__ sF, PcLat Cc, const double* __restrict__ eC,
                                                 int64_t vs, int64_t ls, int64_t ps) {
  constexpr int DD = D * D;
  __shared__ double lds[EB / 64];
  const int64_t col = blockIdx.y;
  r += col * vs; z += col * vs; s += col * EMS_STRIDE; part += col * ps; flag += col * EMF_STRIDE; sF += col * ls;
  if (UPDATE) { x += col * vs; p += col * vs; q += col * vs; }
  if (INIT) pinit += col * vs;
  if (eC) eC += col * ls;
  if (UPDATE && flag[0]) return;
  double dotv = 0.0;
  const double alpha = UPDATE ? s[S_ALPHA] : 0.0;
  for (int64_t row = (int64_t)blockIdx.x * EB + threadIdx.x; row < n_rows; row += (int64_t)gridDim.x * EB) {
    double rr[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double ri = r[row * D + i];
      if (UPDATE) {
        x[row * D + i] += alpha * p[row * D + i];
        ri = fma(-alpha, q[row * D + i], ri);
        r[row * D + i] = ri;
      }
      rr[i] = ri;
    }
    int b[D];
    double f[D], corr[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { b[k] = vbin[row * D + k]; f[k] = vfrac[row * D + k]; corr[k] = 0.0; }
    pc_gather<D>(F, b, f, sF, corr);
    if (eC) {
#pragma unroll
      for (int k = 0; k < D; ++k) { f[k] = 0.5 * (f[k] + (double)(b[k] & 1)); b[k] >>= 1; }
      pc_gather<D>(Cc, b, f, eC, corr);
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double zi = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) zi += dinv[row * DD + i * D + k] * rr[k];
      if (!(fixed && fixed[row * D + i])) zi += corr[i];
      z[row * D + i] = zi;
      if (INIT) pinit[row * D + i] = zi;
      dotv += rr[i] * zi;
    }
  }
  const double t = femo_block_sum<EB>(dotv, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

template <int D>
int pc_build_blocks(femo_elast* e, const double* rho) {
  constexpr int DD = D * D;
  femo_elast_pc* pc = e->pc;
  femo_mesh* m = e->mesh;
  hipStream_t st = m->ctx->stream;
  const PcLevels& P = pc->P;
  const int64_t total = P.off[P.n_levels];
  const uint8_t* fx = e->has_fixed ? e->d_fixed : nullptr;
  FEMO_HIP_CHECK(hipEventRecord(pc->ev0, st));
  FEMO_HIP_CHECK(hipMemsetAsync(pc->d_G, 0, (size_t)total * DD * sizeof(double), st));
  for (int l = 0; l < P.n_levels; ++l) {
    double* G = pc->d_G + P.off[l] * DD;
    const PcLat& F = P.lat[P.n_levels - 1];
    const double to_level = 1.0 / (double)(1 << (P.n_levels - 1 - l));
    if (P.lat[l].nodes * DD <= PC_LDS_DOUBLES)
      hipLaunchKernelGGL((k_pc_blocks<D, true>), dim3(std::min<unsigned>(pc_grid(m->n_cell), PC_LDS_GRID)), dim3(EB),
                         (size_t)P.lat[l].nodes * DD * sizeof(double), st, m->n_cell, m->d_conn, m->d_x, rho, e->method,
                         e->lam0, e->mu0, fx, P.lat[l], F, to_level, P.lo[0], P.lo[1], P.lo[2], G);
    else
      hipLaunchKernelGGL((k_pc_blocks<D, false>), dim3(pc_grid(m->n_cell)), dim3(EB), 0, st, m->n_cell, m->d_conn, m->d_x,
                         rho, e->method, e->lam0, e->mu0, fx, P.lat[l], F, to_level, P.lo[0], P.lo[1], P.lo[2], G);
  }
  if (e->has_springs)
    for (int l = 0; l < P.n_levels; ++l) {
      double* G = pc->d_G + P.off[l] * DD;
      const int shift = P.n_levels - 1 - l;
      if (P.lat[l].nodes * DD <= PC_LDS_DOUBLES)
        hipLaunchKernelGGL((k_pc_springs<D, true>), dim3(std::min<unsigned>(pc_grid(m->n_vert), PC_LDS_GRID)), dim3(EB),
                           (size_t)P.lat[l].nodes * DD * sizeof(double), st, m->n_vert, e->d_springs, fx, pc->d_vbin, pc->d_vfrac,
                           P.lat[l], shift, G);
      else
        hipLaunchKernelGGL((k_pc_springs<D, false>), dim3(pc_grid(m->n_vert)), dim3(EB), 0, st, m->n_vert, e->d_springs, fx,
                           pc->d_vbin, pc->d_vfrac, P.lat[l], shift, G);
    }
  hipLaunchKernelGGL(k_pc_invert<D>, dim3(pc_grid(total)), dim3(EB), 0, st, total, pc->d_G, pc->d_C);
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_HIP_CHECK(hipEventRecord(pc->ev1, st));
  return 0;
}

template <int D, bool UPDATE>
int pc_step(femo_elast* e, int nc, double* x, double* r, const double* p, const double* q, double* z, double* pinit,
            const double* s, double* part, int64_t ps, const int32_t* flag, const double* dinv) {
  constexpr int GL = D == 2 ? 8 : 64;
  femo_elast_pc* pc = e->pc;
  femo_mesh* m = e->mesh;
  hipStream_t st = m->ctx->stream;
  const PcLevels& P = pc->P;
  const int L = P.n_levels - 1;
  const PcLat& F = P.lat[L];
  const PcLat& Cc = P.lat[L > 0 ? L - 1 : 0];
  const uint8_t* fx = e->has_fixed ? e->d_fixed : nullptr;
  const int64_t vs = m->n_rows * D, ls = P.off[P.n_levels] * D;
  double* gF = pc->d_g + P.off[L] * D;
  double* sF = pc->d_e + P.off[L] * D;
  double* gC = L > 0 ? pc->d_g + P.off[L - 1] * D : nullptr;
  const double* eC = L > 0 ? pc->d_e + P.off[L - 1] * D : nullptr;
  const unsigned cols = (unsigned)nc;
  hipLaunchKernelGGL((k_pc_restrict_mesh<D, GL, UPDATE>), dim3(pc_grid(F.nodes * GL), cols), dim3(EB), 0, st, F.nodes,
                     pc->d_rptr, pc->d_rvert, pc->d_rw, r, q, s, fx, flag, gF, vs, ls);
  hipLaunchKernelGGL((k_pc_lat_restrict<D, UPDATE>), dim3(pc_grid(F.nodes), cols), dim3(EB), 0, st, F, Cc, L > 0 ? 1 : 0,
                     pc->d_C + P.off[L] * D * D, gF, sF, gC, flag, ls);
  if (L > 0)
    hipLaunchKernelGGL((k_pc_coarse<D, UPDATE>), dim3(cols), dim3(PC_COARSE_NT), 0, st, P, L - 1, pc->d_C, pc->d_g,
                       pc->d_e, flag, ls);
  if (pinit)
    hipLaunchKernelGGL((k_pc_final<D, UPDATE, true>), dim3(PCG_GRID, cols), dim3(EB), 0, st, m->n_rows, dinv, x, r, p, q,
                       z, pinit, s, part, flag, fx, pc->d_vbin, pc->d_vfrac, F, sF, Cc, eC, vs, ls, ps);
  else
    hipLaunchKernelGGL((k_pc_final<D, UPDATE, false>), dim3(PCG_GRID, cols), dim3(EB), 0, st, m->n_rows, dinv, x, r, p, q,
                       z, pinit, s, part, flag, fx, pc->d_vbin, pc->d_vfrac, F, sF, Cc, eC, vs, ls, ps);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

void femo_elast_pc_free(femo_elast* e) {
  femo_elast_pc* pc = e ? e->pc : nullptr;
  if (!pc) return;
  hipFree(pc->d_G); hipFree(pc->d_C); hipFree(pc->d_g); hipFree(pc->d_e); hipFree(pc->d_vbin); hipFree(pc->d_vfrac);
  hipFree(pc->d_rptr); hipFree(pc->d_rvert); hipFree(pc->d_rw);
  if (pc->ev0) hipEventDestroy(pc->ev0);
  if (pc->ev1) hipEventDestroy(pc->ev1);
  delete pc;
  e->pc = nullptr;
}

int femo_elast_pc_ensure(femo_elast* e) {
  FEMO_REQUIRE(e && e->pc, "multilevel preconditioner: femo_elast_pc_setup first");
  FEMO_REQUIRE(e->assembled, "multilevel preconditioner: assemble K first");
  if (!e->pc_dirty) return 0;
  const femo_vec* rho = femo_vec_live(e->rho_uid);
  FEMO_REQUIRE(rho && rho->gen == e->rho_gen && rho->n >= e->mesh->n_cell,
               "multilevel preconditioner: the density vector of femo_elast_assemble is gone or was written since; assemble again");
  return femo_elast_pc_build(e, rho->d);
}

int femo_elast_pc_build(femo_elast* e, const double* rho) {
  FEMO_TRY(e->d == 2 ? pc_build_blocks<2>(e, rho) : pc_build_blocks<3>(e, rho));
  e->pc_dirty = false;
  ++e->pc->builds;
  return 0;
}

int femo_elast_pc_step(femo_elast* e, bool update, int n_cols, double* x, double* r, const double* p, const double* q,
                       double* z, double* pinit, const double* s, double* part, int64_t part_stride, const int32_t* flag,
                       const double* dinv) {
  femo_elast_pc* pc = e->pc;
  FEMO_REQUIRE(pc && n_cols >= 1 && n_cols <= FEMO_ELAST_MAX_COLS, "femo_elast_pc_step: bad column count %d", n_cols);
  if (pc->cols < n_cols) {                       // the old pair stays until the new one exists
    const int64_t per = pc->P.off[pc->P.n_levels] * e->d;
    double *g = nullptr, *c = nullptr;
    if (pc_alloc(&g, per * n_cols) || pc_alloc(&c, per * n_cols)) { hipFree(g); return 1; }
    FEMO_HIP_CHECK(hipStreamSynchronize(e->mesh->ctx->stream));
    hipFree(pc->d_g); hipFree(pc->d_e);
    pc->d_g = g; pc->d_e = c;
    pc->bytes += 2 * per * (n_cols - pc->cols) * (int64_t)sizeof(double);
    pc->cols = n_cols;
  }
#define FEMO_PC_STEP(D, U) pc_step<D, U>(e, n_cols, x, r, p, q, z, pinit, s, part, part_stride, flag, dinv)
  if (e->d == 2) return update ? FEMO_PC_STEP(2, true) : FEMO_PC_STEP(2, false);
  return update ? FEMO_PC_STEP(3, true) : FEMO_PC_STEP(3, false);
#undef FEMO_PC_STEP
}

// ===================================================================================================== C-ABI ====
extern "C" {

int femo_elast_pc_setup(femo_elast* e, double spacing_factor) {
  FEMO_REQUIRE(e, "null argument");
  FEMO_REQUIRE(spacing_factor >= 0.0 && std::isfinite(spacing_factor), "femo_elast_pc_setup: bad spacing factor");
  femo_mesh* m = e->mesh;
  const int d = e->d;
  const int nv = d + 1;
  hipStream_t st = m->ctx->stream;
  std::vector<double> x((size_t)m->n_vert * d);
  std::vector<int32_t> conn((size_t)m->n_cell * nv);
  FEMO_HIP_CHECK(hipMemcpyAsync(x.data(), m->d_x, x.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(conn.data(), m->d_conn, conn.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  // mean edge length: over the cells, all their edges
  double tot = 0.0;
  for (int64_t c = 0; c < m->n_cell; ++c)
    for (int a = 0; a < nv; ++a)
      for (int b = a + 1; b < nv; ++b) {
        double s = 0.0;
        for (int k = 0; k < d; ++k) {
          const double t = x[(size_t)conn[c * nv + a] * d + k] - x[(size_t)conn[c * nv + b] * d + k];
          s += t * t;
        }
        tot += std::sqrt(s);
      }
  const double h = tot / ((double)m->n_cell * (nv * d / 2));
  double lo[3] = {0, 0, 0}, ext[3] = {0, 0, 0};
  double lmin = 0.0;
  for (int k = 0; k < d; ++k) {
    lo[k] = m->bbox_lo[k];
    ext[k] = m->bbox_hi[k] - m->bbox_lo[k];
    lmin = k == 0 ? ext[k] : std::min(lmin, ext[k]);
  }
  FEMO_REQUIRE(h > 0.0 && lmin > 0.0, "femo_elast_pc_setup: degenerate mesh");
  const double f = spacing_factor > 0.0 ? spacing_factor : PC_DEFAULT_SPACING;
  int nl = 1 + (int)std::floor(std::log2(lmin / (f * h)) + 0.5);
  nl = std::min(std::max(nl, 1), PC_ML);
  auto* pc = new femo_elast_pc();
  PcLevels& P = pc->P;
  P.n_levels = nl;
  int64_t n0[3] = {0, 0, 0};
  for (int k = 0; k < d; ++k) n0[k] = std::max<int64_t>(1, (int64_t)std::ceil(ext[k] / lmin - 1e-9));
  P.off[0] = 0;
  for (int l = 0; l < nl; ++l) {
    PcLat& L = P.lat[l];
    int64_t nodes = 1;
    for (int k = 0; k < 3; ++k) {
      const int64_t nk = k < d ? n0[k] << l : 0;
      if (nk + 1 > (1 << 20) || nodes * (nk + 1) > (int64_t)1 << 28) {
        delete pc;
        femo_set_error("femo_elast_pc_setup: lattice too large");
        return 2;
      }
      L.n[k] = (int)nk;
      nodes *= nk + 1;
    }
    L.nodes = nodes;
    pc->H[l] = lmin / (double)(1 << l);
    L.inv_h = 1.0 / pc->H[l];
    P.off[l + 1] = P.off[l] + nodes;
  }
  for (int k = 0; k < 3; ++k) P.lo[k] = lo[k];
  if (nl > 1 && P.lat[nl - 2].nodes > PC_COARSE_MAX_NODES) {
    const long long n2 = (long long)P.lat[nl - 2].nodes;
    delete pc;
    femo_set_error("femo_elast_pc_setup: the second-finest lattice would have %lld nodes; the lattices below the finest are "
                   "swept by one workgroup (at most %lld): use a larger spacing factor", n2, (long long)PC_COARSE_MAX_NODES);
    return 2;
  }
  // per vertex: bin and fraction on the finest lattice; node -> (vertex, weight) lists in ascending vertex order
  const PcLat& F = P.lat[nl - 1];
  std::vector<int32_t> vbin((size_t)m->n_vert * d);
  std::vector<double> vfrac((size_t)m->n_vert * d);
  for (int64_t v = 0; v < m->n_vert; ++v)
    for (int k = 0; k < d; ++k) {
      const double t = pc_coord(x[(size_t)v * d + k], lo[k], F.inv_h, F.n[k]);
      int64_t b = (int64_t)std::floor(t);
      b = b < 0 ? 0 : (b > F.n[k] - 1 ? F.n[k] - 1 : b);
      double fr = t - (double)b;
      fr = fr < 0.0 ? 0.0 : (fr > 1.0 ? 1.0 : fr);
      vbin[(size_t)v * d + k] = (int32_t)b;
      vfrac[(size_t)v * d + k] = fr;
    }
  std::vector<int64_t> rptr(F.nodes + 1, 0);
  auto corner_of = [&](int64_t v, int corner, double& w) {
    int ijk[3] = {0, 0, 0};
    w = 1.0;
    for (int k = 0; k < d; ++k) {
      const int up = (corner >> k) & 1;
      ijk[k] = vbin[(size_t)v * d + k] + up;
      w *= up ? vfrac[(size_t)v * d + k] : 1.0 - vfrac[(size_t)v * d + k];
    }
    return pc_node(F, ijk[0], ijk[1], ijk[2]);
  };
  for (int64_t v = 0; v < m->n_vert; ++v)
    for (int corner = 0; corner < (1 << d); ++corner) {
      double w;
      const int64_t node = corner_of(v, corner, w);
      if (w != 0.0) ++rptr[node + 1];
    }
  for (int64_t i = 0; i < F.nodes; ++i) rptr[i + 1] += rptr[i];
  pc->r_entries = rptr[F.nodes];
  std::vector<int32_t> rvert((size_t)pc->r_entries);
  std::vector<double> rw((size_t)pc->r_entries);
  {
    std::vector<int64_t> cur(rptr.begin(), rptr.end() - 1);
    for (int64_t v = 0; v < m->n_vert; ++v)
      for (int corner = 0; corner < (1 << d); ++corner) {
        double w;
        const int64_t node = corner_of(v, corner, w);
        if (w == 0.0) continue;
        rvert[(size_t)cur[node]] = (int32_t)v;
        rw[(size_t)cur[node]++] = w;
      }
  }
  const int64_t total = P.off[nl], dd = (int64_t)d * d;
  int rc = 0;
  rc |= pc_alloc(&pc->d_G, total * dd); rc |= pc_alloc(&pc->d_C, total * dd);
  rc |= pc_alloc(&pc->d_g, total * d); rc |= pc_alloc(&pc->d_e, total * d);
  rc |= pc_alloc(&pc->d_vbin, m->n_vert * d); rc |= pc_alloc(&pc->d_vfrac, m->n_vert * d);
  rc |= pc_alloc(&pc->d_rptr, F.nodes + 1); rc |= pc_alloc(&pc->d_rvert, pc->r_entries); rc |= pc_alloc(&pc->d_rw, pc->r_entries);
  if (rc == 0 && (hipEventCreate(&pc->ev0) != hipSuccess || hipEventCreate(&pc->ev1) != hipSuccess)) rc = 1;
  femo_elast_pc* old = e->pc;
  e->pc = pc;
  if (rc) { femo_elast_pc_free(e); e->pc = old; femo_set_error("femo_elast_pc_setup: device allocation failed"); return 1; }
  e->pc = old;
  femo_elast_pc_free(e);
  e->pc = pc;
  e->pc_dirty = true;
  pc->cols = 1;
  pc->bytes = total * (2 * dd + 2 * d) * (int64_t)sizeof(double);
  FEMO_HIP_CHECK(hipMemcpyAsync(pc->d_vbin, vbin.data(), vbin.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(pc->d_vfrac, vfrac.data(), vfrac.size() * sizeof(double), hipMemcpyHostToDevice, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(pc->d_rptr, rptr.data(), rptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
  if (pc->r_entries) {
    FEMO_HIP_CHECK(hipMemcpyAsync(pc->d_rvert, rvert.data(), rvert.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    FEMO_HIP_CHECK(hipMemcpyAsync(pc->d_rw, rw.data(), rw.size() * sizeof(double), hipMemcpyHostToDevice, st));
  }
  FEMO_HIP_CHECK(hipStreamSynchronize(st));     // the host arrays go out of scope
  return 0;
}

int femo_elast_pc_info(const femo_elast* e, int64_t info[FEMO_ELAST_PC_INFO_COUNT]) {
  FEMO_REQUIRE(e && info, "null argument");
  FEMO_REQUIRE(e->pc, "femo_elast_pc_info: femo_elast_pc_setup first");
  const femo_elast_pc* pc = e->pc;
  for (int i = 0; i < FEMO_ELAST_PC_INFO_COUNT; ++i) info[i] = 0;
  info[FEMO_ELAST_PC_INFO_LEVELS] = pc->P.n_levels;
  info[FEMO_ELAST_PC_INFO_BYTES] = pc->bytes;
  info[FEMO_ELAST_PC_INFO_BUILDS] = pc->builds;
  if (pc->builds > 0) {
    float ms = 0.0f;
    FEMO_HIP_CHECK(hipEventSynchronize(pc->ev1));
    if (hipEventElapsedTime(&ms, pc->ev0, pc->ev1) == hipSuccess) info[FEMO_ELAST_PC_INFO_BUILD_US] = (int64_t)std::llround(ms * 1e3);
  }
  for (int l = 0; l < pc->P.n_levels; ++l) info[FEMO_ELAST_PC_INFO_NODES + l] = pc->P.lat[l].nodes;
  return 0;
}

int femo_elast_pc_export_level(femo_elast* e, int level, double* blocks) {
  FEMO_REQUIRE(e && blocks, "null argument");
  FEMO_TRY(femo_elast_pc_ensure(e));
  const femo_elast_pc* pc = e->pc;
  FEMO_REQUIRE(level >= 0 && level < pc->P.n_levels, "femo_elast_pc_export_level: no level %d", level);
  const int64_t dd = (int64_t)e->d * e->d;
  hipStream_t st = e->mesh->ctx->stream;
  FEMO_HIP_CHECK(hipMemcpyAsync(blocks, pc->d_G + pc->P.off[level] * dd, (size_t)pc->P.lat[level].nodes * dd * sizeof(double),
                                hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

int femo_elast_pc_apply(femo_elast* e, const femo_vec* r, femo_vec* z) {
  FEMO_REQUIRE(e && r && z, "null argument");
  const int64_t n = e->mesh->n_vert * e->d;
  FEMO_REQUIRE(r->n >= n && z->n >= n && r != z, "vector size mismatch in femo_elast_pc_apply");
  FEMO_TRY(femo_elast_pc_ensure(e));
  FEMO_TRY(femo_vec_await(r));
  femo_vec_touch(z);
  return femo_elast_pc_step(e, false, 1, nullptr, const_cast<double*>(r->d) /* read only without the update */, nullptr, nullptr, z->d, nullptr, e->w_s, e->w_part, e->w_pstride, e->w_flag, e->d_dinv);
}

}  // extern "C"
