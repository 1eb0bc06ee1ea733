// Reissner-Mindlin shell: the exact solve on the coarsest lattice level kept.  The Galerkin operator P^T K P of the
// level is formed as a dense matrix (three kernels: trilinear spaces, Hermite-type spaces with LDS atomics, Hermite-type
// spaces on the fp64 matrix cores), factorised (tiled Cholesky, level-wise triangular inverse) and applied as
// L^-T L^-1 in two products per iteration (shell_internal.h has the overview).
#include "shell_internal.h"

namespace {

// Dense Galerkin operator of one coarse lattice level c: A[a, b] = sum_{i, j free} P[i, a] K[i, j] P[j, b], 6 n_c x 6 n_c.
// One workgroup per item = points (256 by default) of one coarse cell and one field group (displacements of P2 nodes /
// rotations of vertices): they share the cell's eight nodes a, and the eight nodes of any j they couple to lie in the
// 4 x 4 x 4 node neighbourhood of the cell (an element is smaller than a coarse cell; info[1] reports otherwise).  The
// sums over the item never leave the workgroup: table[3 x 6 components][64 neighbourhood nodes][8 a] in LDS (72 KB),
// flushed to the dense matrix once (item_nbr: the neighbourhood's level-local node numbers, -1 where the surface does
// not touch the lattice).  The item's 3 x 3 blocks are staged through LDS 256 at a time, one block per thread (values
// with the Dirichlet mask applied, the column's eight weights, its cell offset); then a wave takes one staged block
// per step, its 64 lanes being the 8 x 8 pairs (cell node a, corner k' of the column's cell), and adds the nine
// products with ds_add_f64.  History at 1.97 M dofs (12 M blocks): all threads following one block through global
// memory, sums in registers of the thread that owns (a, neighbourhood node): 27 ms; blocks staged through LDS, same
// ownership (one (thread, block) pair in eight has work): 20 ms whatever the item size; LDS table with a 16-way bank
// conflict: 16.4 ms; this layout: 8.1 ms.
constexpr int CG_MAXPTS = 256;
constexpr int CG_TABLE = 8 * 64 * 18;                     // doubles
constexpr size_t CG_LDS = (size_t)CG_TABLE * 8 + 256 * 9 * 8 + 256 * 8 * 8 + CG_MAXPTS * 8 * 8 + 256 * 4 + (CG_MAXPTS + 1) * 4 + CG_MAXPTS * 4 * 2;
__global__ __launch_bounds__(256) void k_pc_coarse_galerkin(int c, int width, int64_t off_c, int64_t lda, int64_t n_unode,
                                                            const int64_t* __restrict__ item_ptr, const int32_t* __restrict__ item_pts,
                                                            const int32_t* __restrict__ item_nbr, const int32_t* __restrict__ node_xyz,
                                                            const int32_t* __restrict__ pcell, const int64_t* __restrict__ brow,
                                                            const int32_t* __restrict__ bcols, const double* __restrict__ vals,
                                                            const uint8_t* __restrict__ fixed, const int32_t* __restrict__ ell_idx,
                                                            const double* __restrict__ ell_w, double* __restrict__ A, int32_t* __restrict__ info) {
  extern __shared__ double cg_lds[];
  double* table = cg_lds;                                                  // [3 fa][6][64 bl][8 a]
  double (*s_val)[9] = reinterpret_cast<double (*)[9]>(table + CG_TABLE);  // staged 3 x 3 blocks, Dirichlet mask applied
  double (*s_wb)[8] = reinterpret_cast<double (*)[8]>(s_val + 256);        // the column's weights on its cell's nodes
  double (*s_wpt)[8] = reinterpret_cast<double (*)[8]>(s_wb + 256);        // the item's points: weights on the cell's nodes
  int32_t* s_meta = reinterpret_cast<int32_t*>(s_wpt + CG_MAXPTS);         // ox | oy << 2 | oz << 4 | gj << 6 | q << 8, or -1
  int32_t* s_scan = s_meta + 256;                                          // blocks before point q of the chunk
  int32_t* s_k0 = s_scan + CG_MAXPTS + 1;
  int32_t* s_fi = s_k0 + CG_MAXPTS;
  const int64_t item = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t pbeg = item_ptr[item], pend = item_ptr[item + 1];
  const int32_t pfirst = item_pts[pbeg];
  const int gi = pfirst >= n_unode ? 1 : 0;
  const int64_t e0 = (int64_t)(3 * pfirst) * width + 8 * c;
  const int32_t pk0 = pcell[pfirst];
  const int bx = pk0 & 1023, by = (pk0 >> 10) & 1023, bz = pk0 >> 20;
  for (int idx = t; idx < CG_TABLE; idx += 256) table[idx] = 0.0;
  int far = 0;
  const int wv = t >> 6, la = t & 7, lk = (t >> 3) & 7;                     // wave, cell node a, corner k' of the column's cell
  for (int64_t p0 = pbeg; p0 < pend; p0 += CG_MAXPTS) {
    const int npts = (int)min((int64_t)CG_MAXPTS, pend - p0);
    __syncthreads();
    if (t < npts) {
      const int32_t i = item_pts[p0 + t];
      const int64_t k0 = brow[i];
      s_k0[t] = (int32_t)k0;
      s_scan[t + 1] = (int32_t)(brow[i + 1] - k0);
      s_fi[t] = fixed == nullptr ? 0 : (fixed[3 * i] ? 1 : 0) | (fixed[3 * i + 1] ? 2 : 0) | (fixed[3 * i + 2] ? 4 : 0);
    }
    for (int idx = t; idx < npts * 8; idx += 256) {
      const int32_t i = item_pts[p0 + (idx >> 3)];
      s_wpt[idx >> 3][idx & 7] = ell_w[(int64_t)(3 * i) * width + 8 * c + (idx & 7)];
    }
    __syncthreads();
    if (t == 0) {
      int32_t run = 0;
      s_scan[0] = 0;
      for (int q = 0; q < npts; ++q) { run += s_scan[q + 1]; s_scan[q + 1] = run; }
    }
    __syncthreads();
    const int B = s_scan[npts];
    for (int base = 0; base < B; base += 256) {
      const int f = base + t;
      if (f < B) {
        int lo = 0, hi = npts - 1;                         // largest q with s_scan[q] <= f
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (s_scan[mid] <= f) lo = mid; else hi = mid - 1;
        }
        const int q = lo, lkk = f - s_scan[q];
        const int64_t k0 = s_k0[q];
        const int64_t len = 3 * (int64_t)(s_scan[q + 1] - s_scan[q]);
        const int32_t cj = bcols[k0 + lkk];
        const int32_t pk = pcell[cj / 3];
        const int ox = (pk & 1023) - bx + 1, oy = ((pk >> 10) & 1023) - by + 1, oz = (pk >> 20) - bz + 1;
        if ((unsigned)ox > 2u || (unsigned)oy > 2u || (unsigned)oz > 2u) {
          far = 1;
          s_meta[t] = -1;
        } else {
          s_meta[t] = ox | (oy << 2) | (oz << 4) | ((cj >= 3 * n_unode ? 1 : 0) << 6) | (q << 8);
          const double* v = vals + 9 * k0 + 3 * lkk;
          const int fi = s_fi[q];
          const int fj = fixed == nullptr ? 0 : (fixed[cj] ? 1 : 0) | (fixed[cj + 1] ? 2 : 0) | (fixed[cj + 2] ? 4 : 0);
#pragma unroll
          for (int fa = 0; fa < 3; ++fa)
#pragma unroll
            for (int fb = 0; fb < 3; ++fb) s_val[t][3 * fa + fb] = ((fi >> fa) & 1) || ((fj >> fb) & 1) ? 0.0 : v[fa * len + fb];
          const double* wj = ell_w + (int64_t)cj * width + 8 * c;
#pragma unroll
          for (int b = 0; b < 8; ++b) s_wb[t][b] = wj[b];
        }
      }
      __syncthreads();
      const int cnt = min(256, B - base);
      for (int e = wv; e < cnt; e += 4) {                  // one staged block per wave and step
        const int32_t m = s_meta[e];
        if (m < 0) continue;
        const int ox = m & 3, oy = (m >> 2) & 3, oz = (m >> 4) & 3, gj = (m >> 6) & 1, q = m >> 8;
        const double ww = s_wpt[q][la] * s_wb[e][lk];
        const int bl = (ox + (lk & 1)) + 4 * (oy + ((lk >> 1) & 1)) + 16 * (oz + (lk >> 2));
        // table[component][bl][a], a fastest: the 64 lanes of an update spread over all banks (4 lanes per 8-byte
        // bank pair, the minimum); with [a][bl][component] the eight a and the two z corners shared a bank, a 16-way
        // conflict on every ds_add_f64 (16.4 ms at 1.97 M dofs)
        double* dst = table + ((3 * gj) * 64 + bl) * 8 + la;
#pragma unroll
        for (int fa = 0; fa < 3; ++fa)
#pragma unroll
          for (int fb = 0; fb < 3; ++fb)
            __hip_atomic_fetch_add(dst + (6 * fa + fb) * 512, ww * s_val[e][3 * fa + fb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      __syncthreads();
    }
  }
  if (far && info != nullptr) atomicOr(&info[1], 1);
  __syncthreads();
  // flush: thread t owns node a = t & 7 against neighbourhood nodes t >> 3 and (t >> 3) + 32
  {
    const int a = t & 7, blq = t >> 3;
    const int64_t na = ell_idx[e0 + a] / 6 - off_c;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int bl = blq + 32 * s;
      const int32_t nb = item_nbr[item * 64 + bl];
      if (nb < 0) continue;
      const double* src = table + bl * 8 + a;
#pragma unroll
      for (int fa = 0; fa < 3; ++fa)
#pragma unroll
        for (int f = 0; f < 6; ++f) {
          const double v = src[(6 * fa + f) * 512];
          if (v != 0.0) atomicAdd(&A[(6 * na + 3 * gi + fa) * lda + 6 * (int64_t)nb + f], v);
        }
    }
  }
}

// Dense Galerkin operator of the coarse-solve level for the Hermite-type spaces: A[6 a + f, 6 b + f'] with the composed
// (alpha, sigma) of that level.  Organisation of k_pc_coarse_galerkin (items = points of one coarse cell and one field
// group; the item's 3 x 3 blocks staged through LDS; a wave per staged block, lanes = (cell node a, corner k' of the
// column's cell); sums in an LDS table, flushed once).  pass 0: rows U of the displacement items against all six columns,
// T[fa][f] += alpha_p (K W_q)[fa][f]; pass 1: rows Theta against the Theta columns only -- [sigma_p]x K W_q^Theta for a
// displacement item, w_p K W_q^Theta for a rotation item; the (Theta, U) quadrant is the transpose of (U, Theta)
// (k_pc_coarse_mirror_tu): 27 LDS atomics per (block, a, k') in place of 36.
constexpr int CGH_CHUNK = 128;
constexpr size_t CGH_LDS = (size_t)CG_TABLE * 8 + CGH_CHUNK * 9 * 8 + CGH_CHUNK * 8 * 16 + CGH_CHUNK * 8 * 16 + CGH_CHUNK * 4 + (CGH_CHUNK + 1) * 4 + CGH_CHUNK * 4 * 2;
__global__ __launch_bounds__(256) void k_pc_coarse_galerkin_h(int pass, int c, int width, int64_t off_c, int64_t lda, int64_t n_unode,
                                                              const int64_t* __restrict__ item_ptr, const int32_t* __restrict__ item_pts,
                                                              const int32_t* __restrict__ item_nbr, const int32_t* __restrict__ pcell,
                                                              const int64_t* __restrict__ brow, const int32_t* __restrict__ bcols,
                                                              const double* __restrict__ vals, const uint8_t* __restrict__ fixed,
                                                              const int32_t* __restrict__ ell_idx, const float4* __restrict__ cs_w4,
                                                              double* __restrict__ A, int32_t* __restrict__ info) {
  extern __shared__ double cg_lds[];
  double* table = cg_lds;                                                  // [3 rows][6 cols][64 bl][8 a]
  double (*s_val)[9] = reinterpret_cast<double (*)[9]>(table + CG_TABLE);
  float4 (*s_wb)[8] = reinterpret_cast<float4 (*)[8]>(s_val + CGH_CHUNK);
  float4 (*s_wpt)[8] = reinterpret_cast<float4 (*)[8]>(s_wb + CGH_CHUNK);
  int32_t* s_meta = reinterpret_cast<int32_t*>(s_wpt + CGH_CHUNK);
  int32_t* s_scan = s_meta + CGH_CHUNK;
  int32_t* s_k0 = s_scan + CGH_CHUNK + 1;
  int32_t* s_fi = s_k0 + CGH_CHUNK;
  const int64_t item = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t pbeg = item_ptr[item], pend = item_ptr[item + 1];
  const int32_t pfirst = item_pts[pbeg];
  const int gi = pfirst >= n_unode ? 1 : 0;
  if (pass == 0 && gi == 1) return;                                        // rotation points have no U rows
  const int64_t e0 = (int64_t)(3 * pfirst) * width + 8 * c;
  const int32_t pk0 = pcell[pfirst];
  const int bx = pk0 & 1023, by = (pk0 >> 10) & 1023, bz = pk0 >> 20;
  for (int idx = t; idx < CG_TABLE; idx += 256) table[idx] = 0.0;
  int far = 0;
  const int wv = t >> 6, la = t & 7, lk = (t >> 3) & 7;
  for (int64_t p0 = pbeg; p0 < pend; p0 += CGH_CHUNK) {
    const int npts = (int)min((int64_t)CGH_CHUNK, pend - p0);
    __syncthreads();
    if (t < npts) {
      const int32_t i = item_pts[p0 + t];
      const int64_t k0 = brow[i];
      s_k0[t] = (int32_t)k0;
      s_scan[t + 1] = (int32_t)(brow[i + 1] - k0);
      s_fi[t] = fixed == nullptr ? 0 : (fixed[3 * i] ? 1 : 0) | (fixed[3 * i + 1] ? 2 : 0) | (fixed[3 * i + 2] ? 4 : 0);
    }
    for (int idx = t; idx < npts * 8; idx += 256) {
      const int32_t i = item_pts[p0 + (idx >> 3)];
      s_wpt[idx >> 3][idx & 7] = cs_w4[(int64_t)i * 8 + (idx & 7)];
    }
    __syncthreads();
    if (t == 0) {
      int32_t run = 0;
      s_scan[0] = 0;
      for (int q = 0; q < npts; ++q) { run += s_scan[q + 1]; s_scan[q + 1] = run; }
    }
    __syncthreads();
    const int B = s_scan[npts];
    for (int base = 0; base < B; base += CGH_CHUNK) {
      const int f = base + t;
      if (t < CGH_CHUNK && f < B) {
        int lo = 0, hi = npts - 1;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (s_scan[mid] <= f) lo = mid; else hi = mid - 1;
        }
        const int q = lo, lkk = f - s_scan[q];
        const int64_t k0 = s_k0[q];
        const int64_t len = 3 * (int64_t)(s_scan[q + 1] - s_scan[q]);
        const int32_t cj = bcols[k0 + lkk];
        const int32_t pk = pcell[cj / 3];
        const int ox = (pk & 1023) - bx + 1, oy = ((pk >> 10) & 1023) - by + 1, oz = (pk >> 20) - bz + 1;
        if ((unsigned)ox > 2u || (unsigned)oy > 2u || (unsigned)oz > 2u) {
          far = 1;
          s_meta[t] = -1;
        } else {
          s_meta[t] = ox | (oy << 2) | (oz << 4) | ((cj >= 3 * n_unode ? 1 : 0) << 6) | (q << 8);
          const double* v = vals + 9 * k0 + 3 * lkk;
          const int fi = s_fi[q];
          const int fj = fixed == nullptr ? 0 : (fixed[cj] ? 1 : 0) | (fixed[cj + 1] ? 2 : 0) | (fixed[cj + 2] ? 4 : 0);
#pragma unroll
          for (int fa = 0; fa < 3; ++fa)
#pragma unroll
            for (int fb = 0; fb < 3; ++fb) s_val[t][3 * fa + fb] = ((fi >> fa) & 1) || ((fj >> fb) & 1) ? 0.0 : v[fa * len + fb];
          const float4* wj = cs_w4 + (int64_t)(cj / 3) * 8;
#pragma unroll
          for (int b = 0; b < 8; ++b) s_wb[t][b] = wj[b];
        }
      }
      __syncthreads();
      const int cnt = min(CGH_CHUNK, B - base);
      for (int e = wv; e < cnt; e += 4) {
        const int32_t m = s_meta[e];
        if (m < 0) continue;
        const int ox = m & 3, oy = (m >> 2) & 3, oz = (m >> 4) & 3, gj = (m >> 6) & 1, q = m >> 8;
        const float4 wp = s_wpt[q][la], wq = s_wb[e][lk];
        const int bl = (ox + (lk & 1)) + 4 * (oy + ((lk >> 1) & 1)) + 16 * (oz + (lk >> 2));
        const double* K = s_val[e];
        // M = K W_q (3 x 6): U columns alpha_q K (displacement column), Theta columns -K [sigma_q]x or w_q K
        double MU[3][3], MT[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double k0v = K[3 * i], k1v = K[3 * i + 1], k2v = K[3 * i + 2];
          if (gj == 0) {
            MU[i][0] = (double)wq.x * k0v; MU[i][1] = (double)wq.x * k1v; MU[i][2] = (double)wq.x * k2v;
            // -(K [s]x)[i][.]:  (K[s]x)[i][0] = k1 s2 - k2 s1, [i][1] = k2 s0 - k0 s2, [i][2] = k0 s1 - k1 s0
            MT[i][0] = -(k1v * (double)wq.w - k2v * (double)wq.z);
            MT[i][1] = -(k2v * (double)wq.y - k0v * (double)wq.w);
            MT[i][2] = -(k0v * (double)wq.z - k1v * (double)wq.y);
          } else {
            MU[i][0] = MU[i][1] = MU[i][2] = 0.0;
            MT[i][0] = (double)wq.x * k0v; MT[i][1] = (double)wq.x * k1v; MT[i][2] = (double)wq.x * k2v;
          }
        }
        double* dst = table + bl * 8 + la;
        if (pass == 0) {
          const double ap = (double)wp.x;
#pragma unroll
          for (int fa = 0; fa < 3; ++fa) {
#pragma unroll
            for (int fb = 0; fb < 3; ++fb) {
              if (gj == 0) __hip_atomic_fetch_add(dst + (6 * fa + fb) * 512, ap * MU[fa][fb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              __hip_atomic_fetch_add(dst + (6 * fa + 3 + fb) * 512, ap * MT[fa][fb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
        } else {
          // Theta rows against the Theta columns: R = [sigma_p]x MT (displacement item) or w_p MT (rotation item)
          double R[3][3];
          if (gi == 0) {
            const double s0 = (double)wp.y, s1 = (double)wp.z, s2 = (double)wp.w;
#pragma unroll
            for (int fb = 0; fb < 3; ++fb) {
              R[0][fb] = -s2 * MT[1][fb] + s1 * MT[2][fb];
              R[1][fb] = s2 * MT[0][fb] - s0 * MT[2][fb];
              R[2][fb] = -s1 * MT[0][fb] + s0 * MT[1][fb];
            }
          } else {
#pragma unroll
            for (int fa = 0; fa < 3; ++fa)
#pragma unroll
              for (int fb = 0; fb < 3; ++fb) R[fa][fb] = (double)wp.x * MT[fa][fb];
          }
#pragma unroll
          for (int fa = 0; fa < 3; ++fa)
#pragma unroll
            for (int fb = 0; fb < 3; ++fb)
              __hip_atomic_fetch_add(dst + (6 * fa + 3 + fb) * 512, R[fa][fb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      __syncthreads();
    }
  }
  if (far && info != nullptr) atomicOr(&info[1], 1);
  __syncthreads();
  {
    const int a = t & 7, blq = t >> 3;
    const int64_t na = ell_idx[e0 + a] / 6 - off_c;
    const int row0 = pass == 0 ? 0 : 3;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int bl = blq + 32 * s;
      const int32_t nb = item_nbr[item * 64 + bl];
      if (nb < 0) continue;
      const double* src = table + bl * 8 + a;
#pragma unroll
      for (int fa = 0; fa < 3; ++fa)
#pragma unroll
        for (int f = (pass == 0 ? 0 : 3); f < 6; ++f) {
          const double v = src[(6 * fa + f) * 512];
          if (v != 0.0) atomicAdd(&A[(6 * na + row0 + fa) * lda + 6 * (int64_t)nb + f], v);
        }
    }
  }
}

// Dense Galerkin operator of the coarse-solve level on the fp64 matrix cores (round 4).  A = P_c^T (K P_c) is GEMM shaped:
// all points of an item (one coarse cell, one field group) share the cell's 8 nodes a -- the 48 rows (f, a) of their
// P_c^T -- and every column point of their blocks has its 8 nodes in the 4 x 4 x 4 node window of the cell -- the 384
// columns (f', bl) of Y = K P_c restricted to the item's rows.  Per chunk of MM_PTS points:
//   1. the chunk's 3 x 3 blocks are staged in LDS (one per thread: masked values, the column point's 8 weights, its cell
//      offset), as in k_pc_coarse_galerkin_h;
//   2. Y[(p, fa)][(f', bl)] += (K_pq W_q,k')[fa][f']: one wave per point walks its blocks, lanes = (f', k'), plain LDS
//      read-modify-writes (a wave's LDS operations execute in order, the rows of a point belong to one wave);
//   3. W^T[(f, a)][(p, fa)] = W_p,a[fa][f];
//   4. D[(f, a)][(f', bl)] += W^T Y with v_mfma_f64_16x16x4 (K = 3 MM_PTS = 24: six steps), accumulators in registers across
//      the chunks of the item: 3 x 24 tiles of 16 x 16, nine per wave.
// The tiles (Theta_1/2 rows, U columns) are not formed: k_pc_coarse_mirror_tu fills the (Theta, U) quadrant from (U, Theta).
// LDS atomics of the version before (k_pc_coarse_galerkin_h, 15 G of them at 1.97 M dofs): 18.7 ms; this kernel 6.9 ms as first
// written, 5.5 with the item's row extents loaded once and the next chunk's column indices and values prefetched under the
// MFMA phase, the operands of block e + 1 fetched before the read-modify-writes of block e, and the f' blocks of Y 66
// doubles apart.  Phase times at 248 k dofs (0.92 ms): step 2 0.49, MFMA 0.19, staging 0.12 -- step 2 is bound by the LDS
// instruction rate (per block and wave: 13 operand reads, 9 of them broadcasts of the block's values, and 6 for Y).
constexpr int MM_PTS = 8, MM_K = 3 * MM_PTS, MM_YP = 400, MM_YF = 66, MM_WP = 25, MM_STAGE = 256, MM_THREADS = 512, MM_ITEM = 256;
constexpr size_t MM_LDS = (size_t)MM_K * MM_YP * 8 + 48 * MM_WP * 8 + MM_STAGE * 9 * 8 + MM_STAGE * 8 * 16 + MM_STAGE * 4 + MM_PTS * 8 * 16 +
                          4 * (MM_ITEM + 1) + 4 * MM_ITEM * 2 + MM_ITEM + 64;
__global__ __launch_bounds__(MM_THREADS) void k_pc_coarse_galerkin_mm(int c, int width, int64_t off_c, int64_t lda, int64_t n_unode,
                                                                      const int64_t* __restrict__ item_ptr, const int32_t* __restrict__ item_pts,
                                                                      const int32_t* __restrict__ item_nbr, const int32_t* __restrict__ pcell,
                                                                      const int64_t* __restrict__ brow, const int32_t* __restrict__ bcols,
                                                                      const double* __restrict__ vals, const uint8_t* __restrict__ fixed,
                                                                      const int32_t* __restrict__ ell_idx, const float4* __restrict__ cs_w4,
                                                                      double* __restrict__ A, int32_t* __restrict__ info) {
  extern __shared__ double mm_lds[];
  double (*Y)[MM_YP] = reinterpret_cast<double (*)[MM_YP]>(mm_lds);                         // [3 pl + fa][MM_YF f' + bl]
  double (*Wt)[MM_WP] = reinterpret_cast<double (*)[MM_WP]>(mm_lds + MM_K * MM_YP);          // [8 f + a][3 pl + fa]
  double (*s_val)[9] = reinterpret_cast<double (*)[9]>(&Wt[48][0]);
  float4 (*s_wb)[8] = reinterpret_cast<float4 (*)[8]>(s_val + MM_STAGE);
  int32_t* s_meta = reinterpret_cast<int32_t*>(s_wb + MM_STAGE);
  float4 (*s_wpt)[8] = reinterpret_cast<float4 (*)[8]>(s_meta + MM_STAGE);
  int32_t* s_S = reinterpret_cast<int32_t*>(s_wpt + MM_PTS);               // blocks before point i of the item (MM_ITEM + 1 entries)
  int32_t* s_ik0 = s_S + MM_ITEM + 1;                                      // first block of point i
  int32_t* s_ipt = s_ik0 + MM_ITEM;                                        // point i of the item
  uint8_t* s_ifi = reinterpret_cast<uint8_t*>(s_ipt + MM_ITEM);            // its Dirichlet bits
  int32_t* s_wsum = reinterpret_cast<int32_t*>(s_ifi + MM_ITEM);           // scan scratch (4 waves)
  const int64_t item = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t pbeg = item_ptr[item], pend = item_ptr[item + 1];
  const int np = (int)(pend - pbeg);                                       // <= MM_ITEM (femo_shell_pc_coarse checks)
  const int32_t pfirst = item_pts[pbeg];
  const int gi = pfirst >= n_unode ? 1 : 0;                                // 0: displacement points (rows U and Theta), 1: rotation points (Theta)
  const int64_t e0 = (int64_t)(3 * pfirst) * width + 8 * c;
  const int32_t pk0 = pcell[pfirst];
  const int bx = pk0 & 1023, by = (pk0 >> 10) & 1023, bz = pk0 >> 20;
  const int li = lane & 15, lk = lane >> 4;
  // the item's points, their block rows and Dirichlet bits, once: two dependent loads per ITEM instead of per chunk
  {
    int32_t len = 0;
    if (t < MM_ITEM) {
      int32_t i = 0, k0 = 0, fi = 0;
      if (t < np) {
        i = item_pts[pbeg + t];
        const int64_t b0 = brow[i];
        k0 = (int32_t)b0; len = (int32_t)(brow[i + 1] - b0);
        fi = fixed == nullptr ? 0 : (fixed[3 * i] ? 1 : 0) | (fixed[3 * i + 1] ? 2 : 0) | (fixed[3 * i + 2] ? 4 : 0);
      }
      s_ipt[t] = i; s_ik0[t] = k0; s_ifi[t] = (uint8_t)fi;
      int32_t v = len;                                                     // inclusive scan within the wave
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const int32_t u = __shfl_up(v, d); if (lane >= d) v += u; }
      if (lane == 63) s_wsum[wv] = v;
      len = v;
    }
    __syncthreads();
    if (t < MM_ITEM) {
      int32_t base = 0;
      for (int w = 0; w < wv; ++w) base += s_wsum[w];
      s_S[t + 1] = base + len;
      if (t == 0) s_S[0] = 0;
    }
    __syncthreads();
  }
  // accumulators: N-tiles nt = wv + 8 j (j = 0..2), M-tiles mt = 0..2
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 acc[3][3];
#pragma unroll
  for (int mt = 0; mt < 3; ++mt)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[mt][j] = d4{0.0, 0.0, 0.0, 0.0};
  int far = 0;
  // block t of a chunk: which of its points, which block of that point's row
  auto locate = [&](int i0, int npts, int f, int& q, int& lkk) {
    q = 0;
#pragma unroll
    for (int qq = 1; qq < MM_PTS; ++qq) q += (qq < npts && s_S[i0 + qq] <= f) ? 1 : 0;
    lkk = f - s_S[i0 + q];
  };
  // prefetch registers: column index and values of this thread's block of the NEXT chunk (issued before the MFMA phase)
  int32_t pf_cj = 0;
  double pf_v[9];
  bool pf_ok = false;
  auto prefetch = [&](int i0) {
    pf_ok = false;
    if (i0 >= np || t >= MM_STAGE) return;
    const int npts = min(MM_PTS, np - i0);
    const int f = s_S[i0] + t;
    if (f >= s_S[i0 + npts]) return;
    int q, lkk;
    locate(i0, npts, f, q, lkk);
    const int64_t k0 = s_ik0[i0 + q];
    const int64_t len = 3 * (int64_t)(s_S[i0 + q + 1] - s_S[i0 + q]);
    pf_cj = bcols[k0 + lkk];
    const double* v = vals + 9 * k0 + 3 * lkk;
#pragma unroll
    for (int fa = 0; fa < 3; ++fa)
#pragma unroll
      for (int fb = 0; fb < 3; ++fb) pf_v[3 * fa + fb] = v[fa * len + fb];
    pf_ok = true;
  };
  prefetch(0);
  for (int i0 = 0; i0 < np; i0 += MM_PTS) {
    const int npts = min(MM_PTS, np - i0);
    __syncthreads();                                                       // the MFMA phase of the chunk before has read Y and Wt
    for (int idx = t; idx < MM_K * MM_YP; idx += MM_THREADS) (&Y[0][0])[idx] = 0.0;
    if (t >= 64 && t < 64 + MM_PTS * 8) {
      const int q = (t - 64) >> 3, a = (t - 64) & 7;
      s_wpt[q][a] = q < npts ? cs_w4[(int64_t)s_ipt[i0 + q] * 8 + a] : float4{0.f, 0.f, 0.f, 0.f};
    }
    const int S0 = s_S[i0], B = s_S[i0 + npts] - S0;
    for (int base = 0; base < B; base += MM_STAGE) {
      const int fblk = base + t;
      if (t < MM_STAGE && fblk < B) {
        int q, lkk;
        locate(i0, npts, S0 + fblk, q, lkk);
        int32_t cj;
        double v9[9];
        if (base == 0 && pf_ok) {
          cj = pf_cj;
#pragma unroll
          for (int k = 0; k < 9; ++k) v9[k] = pf_v[k];
        } else {                                                           // rounds beyond the first (rare): not prefetched
          const int64_t k0 = s_ik0[i0 + q];
          const int64_t len = 3 * (int64_t)(s_S[i0 + q + 1] - s_S[i0 + q]);
          cj = bcols[k0 + lkk];
          const double* v = vals + 9 * k0 + 3 * lkk;
#pragma unroll
          for (int fa = 0; fa < 3; ++fa)
#pragma unroll
            for (int fb = 0; fb < 3; ++fb) v9[3 * fa + fb] = v[fa * len + fb];
        }
        const int32_t pk = pcell[cj / 3];
        const int ox = (pk & 1023) - bx + 1, oy = ((pk >> 10) & 1023) - by + 1, oz = (pk >> 20) - bz + 1;
        if ((unsigned)ox > 2u || (unsigned)oy > 2u || (unsigned)oz > 2u) {
          far = 1;                                                         // flagged; contributes nothing here
          s_meta[t] = 1 | (1 << 2) | (1 << 4);
#pragma unroll
          for (int k = 0; k < 9; ++k) s_val[t][k] = 0.0;
#pragma unroll
          for (int b = 0; b < 8; ++b) s_wb[t][b] = float4{0.f, 0.f, 0.f, 0.f};
        } else {
          s_meta[t] = ox | (oy << 2) | (oz << 4) | ((cj >= 3 * n_unode ? 1 : 0) << 6) | (q << 8);
          const int fi = s_ifi[i0 + q];
          const int fj = fixed == nullptr ? 0 : (fixed[cj] ? 1 : 0) | (fixed[cj + 1] ? 2 : 0) | (fixed[cj + 2] ? 4 : 0);
          const float4* wj = cs_w4 + (int64_t)(cj / 3) * 8;
          float4 w8[8];
#pragma unroll
          for (int b = 0; b < 8; ++b) w8[b] = wj[b];
#pragma unroll
          for (int fa = 0; fa < 3; ++fa)
#pragma unroll
            for (int fb = 0; fb < 3; ++fb) s_val[t][3 * fa + fb] = ((fi >> fa) & 1) || ((fj >> fb) & 1) ? 0.0 : v9[3 * fa + fb];
#pragma unroll
          for (int b = 0; b < 8; ++b) s_wb[t][b] = w8[b];
        }
      }
      __syncthreads();
      // Y of point pl = wv: its staged blocks are the slots [S[i0 + wv], S[i0 + wv + 1]) - S0 of this round.  Software
      // pipelined: the meta words of up to 64 blocks sit in the lanes (readlane, no LDS round trip), the weight and the nine
      // values of block e + 1 are loaded before the three read-modify-writes of block e -- per block one LDS latency, not three
      if (wv < npts) {
        const int pl = wv;
        const int e_lo = max(s_S[i0 + pl] - S0, base) - base, e_hi = min(s_S[i0 + pl + 1] - S0, base + MM_STAGE) - base;
        const int kq = lane & 7, fc = lane >> 3;
        // column f' = fc of W_q,k' as a 3-vector u = (sg[k] w[ix[k]])_k, w = (alpha, sigma): displacement column fc < 3: alpha e_fc;
        // 3: (0, -s2, s1); 4: (s2, 0, -s0); 5: (-s1, s0, 0); rotation column: w e_(fc - 3)
        int ix0 = 0, ix1 = 0, ix2 = 0;
        double sg0 = 0.0, sg1 = 0.0, sg2 = 0.0, sr0 = 0.0, sr1 = 0.0, sr2 = 0.0;
        if (fc == 0) sg0 = 1.0; else if (fc == 1) sg1 = 1.0; else if (fc == 2) sg2 = 1.0;
        else if (fc == 3) { ix1 = 3; sg1 = -1.0; ix2 = 2; sg2 = 1.0; sr0 = 1.0; }
        else if (fc == 4) { ix0 = 3; sg0 = 1.0; ix2 = 1; sg2 = -1.0; sr1 = 1.0; }
        else if (fc == 5) { ix0 = 2; sg0 = -1.0; ix1 = 1; sg1 = 1.0; sr2 = 1.0; }
        const int fcl = fc < 6 ? fc : 0;
        double* y0 = &Y[3 * pl][MM_YF * fcl];      // f' blocks 66 apart: with 64 the six f' lanes of a corner share their LDS banks
        for (int eb = e_lo; eb < e_hi; eb += 64) {
          const int cnt = min(64, e_hi - eb);
          const int32_t my_m = lane < cnt ? s_meta[eb + lane] : 0;
          const float* wf = reinterpret_cast<const float*>(&s_wb[eb][kq]);
          float w0 = wf[ix0], w1 = wf[ix1], w2 = wf[ix2], wa = wf[0];
          double K[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) K[k] = s_val[eb][k];
          for (int e = 0; e < cnt; ++e) {
            const int32_t m = __builtin_amdgcn_readlane(my_m, e);
            const bool gj = (m >> 6) & 1;
            const double u0 = gj ? sr0 * (double)wa : sg0 * (double)w0, u1 = gj ? sr1 * (double)wa : sg1 * (double)w1,
                         u2 = gj ? sr2 * (double)wa : sg2 * (double)w2;
            const double c0 = K[0] * u0 + K[1] * u1 + K[2] * u2, c1 = K[3] * u0 + K[4] * u1 + K[5] * u2, c2 = K[6] * u0 + K[7] * u1 + K[8] * u2;
            if (e + 1 < cnt) {                                             // block e + 1's operands, before this block's read-modify-writes
              const float* wn = reinterpret_cast<const float*>(&s_wb[eb + e + 1][kq]);
              w0 = wn[ix0]; w1 = wn[ix1]; w2 = wn[ix2]; wa = wn[0];
#pragma unroll
              for (int k = 0; k < 9; ++k) K[k] = s_val[eb + e + 1][k];
            }
            const int ox = m & 3, oy = (m >> 2) & 3, oz = (m >> 4) & 3;
            const int bl = (ox + (kq & 1)) + 4 * (oy + ((kq >> 1) & 1)) + 16 * (oz + (kq >> 2));
            if (fc < 6) { y0[bl] += c0; y0[MM_YP + bl] += c1; y0[2 * MM_YP + bl] += c2; }
          }
        }
      }
      __syncthreads();
    }
    // W^T of the chunk: entry (m = 8 f + a, k = 3 pl + fa) = W_p,a[fa][f]
    for (int idx = t; idx < 48 * MM_K; idx += MM_THREADS) {
      const int m = idx / MM_K, k = idx - m * MM_K;
      const int f = m >> 3, a = m & 7, pl = k / 3, fa = k - 3 * pl;
      const float4 w = s_wpt[pl][a];
      double v = 0.0;
      if (gi == 0) {
        if (f < 3) v = f == fa ? (double)w.x : 0.0;
        else {
          // (-[sigma]x)[fa][j]: rows (0, s2, -s1), (-s2, 0, s0), (s1, -s0, 0)
          const int j = f - 3;
          const double s0 = (double)w.y, s1 = (double)w.z, s2 = (double)w.w;
          if (fa == 0) v = j == 1 ? s2 : (j == 2 ? -s1 : 0.0);
          else if (fa == 1) v = j == 0 ? -s2 : (j == 2 ? s0 : 0.0);
          else v = j == 0 ? s1 : (j == 1 ? -s0 : 0.0);
        }
      } else if (f >= 3) {
        v = (f - 3) == fa ? (double)w.x : 0.0;
      }
      Wt[m][k] = v;
    }
    prefetch(i0 + MM_PTS);                                                 // in flight during the MFMA phase
    __syncthreads();
    // D += W^T Y
#pragma unroll
    for (int ks = 0; ks < MM_K / 4; ++ks) {
      const int kk = 4 * ks + lk;
      double av[3];
#pragma unroll
      for (int mt = 0; mt < 3; ++mt) av[mt] = Wt[16 * mt + li][kk];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int nt = wv + 8 * j;
        const double bv = Y[kk][MM_YF * (nt >> 2) + 16 * (nt & 3) + li];
        if (gi == 0) acc[0][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv, acc[1][j], 0, 0, 0);
        if (nt >= 12) acc[2][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2], bv, acc[2][j], 0, 0, 0);
      }
    }
  }
  if (far && info != nullptr) atomicOr(&info[1], 1);
  // flush: lane holds D[16 mt + lk + 4 i][16 nt + li]
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int nt = wv + 8 * j;
    const int n = 16 * nt + li, fp = n >> 6, bl = n & 63;
    const int32_t nb = item_nbr[item * 64 + bl];
    if (nb < 0) continue;
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
      if (mt == 2 && nt < 12) continue;
      if (mt == 0 && gi == 1) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 16 * mt + lk + 4 * i, f = m >> 3, a = m & 7;
        const double v = acc[mt][j][i];
        if (v == 0.0) continue;
        const int64_t na = ell_idx[e0 + a] / 6 - off_c;
        atomicAdd(&A[(6 * na + f) * lda + 6 * (int64_t)nb + fp], v);
      }
    }
  }
}

// the (Theta, U) quadrant of every node pair = transpose of (U, Theta): A[6 a + 3 + i, 6 b + j] = A[6 b + j, 6 a + 3 + i]
__global__ void k_pc_coarse_mirror_tu(int64_t n, int64_t lda, double* __restrict__ A) {
  const int64_t r = blockIdx.y;
  if (r >= n || (r % 6) < 3) return;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x)
    if ((c % 6) < 3) A[r * lda + c] = A[c * lda + r];
}

// packed lattice coordinates of the level-c cell of every point (its first ELL node is the cell's corner)
__global__ void k_pc_coarse_cells(int64_t n_pts, int c, int width, int64_t off_c, const int32_t* __restrict__ ell_idx,
                                  const int32_t* __restrict__ node_xyz, int32_t* __restrict__ pcell) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  const int32_t nd = ell_idx[(3 * p) * width + 8 * c] / 6 - (int32_t)off_c;
  pcell[p] = node_xyz[3 * nd] | (node_xyz[3 * nd + 1] << 10) | (node_xyz[3 * nd + 2] << 20);
}

// ---- dense factorisation of the coarse operator (N = n padded to a multiple of 64, row-major, leading dimension N) ----
// Written here rather than taken from rocSOLVER: loading that library costs 80-450 s on a fresh machine (a 0.9 GB
// shared object read from a cold disk), for a 3000 x 3000 matrix whose factorisation takes milliseconds.
// Blocked right-looking Cholesky A = L L^T with 64 x 64 tiles (lower triangle), then W = L^-1 row of tiles by row of
// tiles, stored transposed in the upper triangle (= L^-T, which the second half of the apply reads along rows) and
// mirrored into the lower one at the end.  A^-1 = L^-T L^-1 is applied in this product form, never formed: W^T W is
// positive definite whatever the rounding in W.
constexpr int DT = 64;                                   // tile edge
constexpr int DP = DT + 1;                               // LDS row pitch

// unknowns no free dof touches have an empty row and column, and so have the padding rows: unit diagonal (their
// restricted residual is zero); a relative 1e-13 on the others keeps the factorisation away from round-off rank deficiency
__global__ void k_pc_coarse_fix_diag(int64_t N, double* __restrict__ A, double ridge) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  const double d = A[r * N + r];
  A[r * N + r] = d > 0.0 ? d * (1.0 + ridge) : 1.0;
}

__device__ __forceinline__ void tile_load(double (*s)[DP], const double* __restrict__ g, int64_t ld, bool transpose) {
  for (int idx = threadIdx.x; idx < DT * DT; idx += 256) {
    const int r = idx / DT, c = idx % DT;
    const double v = g[(int64_t)r * ld + c];
    if (transpose) s[c][r] = v; else s[r][c] = v;
  }
}

// C += A B^T for 64 x 64 tiles with both operands in LDS as [row][k], on the fp64 matrix cores: wave w owns the
// 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 tiles of v_mfma_f64_16x16x4_f64; per k-step of 4 a lane supplies
// A[l & 15][l >> 4] and B[l >> 4][l & 15] and holds D[(l >> 4) + 4 i][l & 15] in register i (the f64 map, not the
// f32 one).  16 k-steps x 4 MFMAs per wave and tile product (the scalar version: 1024 FMAs per thread, ~4 us).
typedef double v4d __attribute__((ext_vector_type(4)));
struct TileAcc {
  v4d v[2][2];
  __device__ TileAcc() {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) v[a][b] = v4d{0.0, 0.0, 0.0, 0.0};
  }
};

__device__ __forceinline__ void tile_mma(TileAcc& acc, const double (*sa)[DP], const double (*sb)[DP]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = 32 * (w >> 1), c0 = 32 * (w & 1), li = lane & 15, lk = lane >> 4;
#pragma unroll 4
  for (int k0 = 0; k0 < DT; k0 += 4) {
    const double a0 = sa[r0 + li][k0 + lk], a1 = sa[r0 + 16 + li][k0 + lk];
    const double b0 = sb[c0 + li][k0 + lk], b1 = sb[c0 + 16 + li][k0 + lk];
    acc.v[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.v[0][0], 0, 0, 0);
    acc.v[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.v[0][1], 0, 0, 0);
    acc.v[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.v[1][0], 0, 0, 0);
    acc.v[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.v[1][1], 0, 0, 0);
  }
}

// f(row, col, value) for the 16 elements of the tile this lane holds
template <class F>
__device__ __forceinline__ void tile_foreach(const TileAcc& acc, F f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = 32 * (w >> 1) + (lane >> 4), c0 = 32 * (w & 1) + (lane & 15);
#pragma unroll
  for (int sr = 0; sr < 2; ++sr)
#pragma unroll
    for (int sc = 0; sc < 2; ++sc)
#pragma unroll
      for (int i = 0; i < 4; ++i) f(r0 + 16 * sr + 4 * i, c0 + 16 * sc, acc.v[sr][sc][i]);
}

// diagonal tile kb: unblocked Cholesky in LDS, L_kk written back (lower part), its inverse (lower triangular, full
// 64 x 64 with zeros above) into dinv[kb]; info[2] = 1 if a pivot is not positive
// the diagonal tile in LDS `a` (all threads have passed a barrier after filling it): Cholesky factor in place, its inverse in
// `w`; L_kk goes to g (lower part), the inverse to dinv_k.  256 threads, ends without a barrier.
__device__ __forceinline__ void chol_diag_tile(double (*a)[DP], double (*w)[DP], double* __restrict__ g, int64_t N, double* __restrict__ dinv_k,
                                               int32_t* __restrict__ info) {
  // One wave factorises the tile column by column, lane r holding row r in registers (static indices: both loops
  // unrolled); the finished entries live in LDS as well, where the other lanes read row c as broadcasts:
  //   L[r][c] = (A[r][c] - sum_{k < c} L[r][k] L[c][k]) / L[c][c].
  // LDS operations of one wave execute in program order; the fences pin the compiler.  (History of this tile: three
  // workgroup barriers per column and the inverse through LDS 169 us, 8 of the factorisation's 10 ms; a wave working on
  // the LDS copy in place was slower (dependent read-modify-writes); a right-looking register version spilled 2 k
  // registers.)
#define FEMO_WAVE_SYNC() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier()
  if (threadIdx.x < DT) {
    const int r = threadIdx.x;
    double row[DT];
#pragma unroll
    for (int c = 0; c < DT; ++c) row[c] = a[r][c];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < DT; ++c) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < c; ++k) sum += row[k] * a[c][k];
      const double v = row[c] - sum;
      if (r == c) {
        if (!(v > 0.0)) bad = true;
        row[c] = sqrt(v > 0.0 ? v : 1.0);
        a[c][c] = row[c];
      }
      FEMO_WAVE_SYNC();
      if (r > c) {
        row[c] = v / a[c][c];
        a[r][c] = row[c];
      }
      FEMO_WAVE_SYNC();
    }
    if (bad) atomicOr(&info[2], 1);
  }
#undef FEMO_WAVE_SYNC
  __syncthreads();
  // inverse: thread c solves L x = e_c with its column in registers; the loops are uniform (entries above the
  // diagonal of the column are zeros), so every read of L is an LDS broadcast and the unrolled code has static
  // register indices
  if (threadIdx.x < DT) {
    const int c = threadIdx.x;
    double x[DT];
#pragma unroll
    for (int r = 0; r < DT; ++r) {
      double v = r == c ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < r; ++k) v -= a[r][k] * x[k];
      x[r] = r >= c ? v / a[r][r] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < DT; ++r) w[r][c] = x[r];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < DT * DT; idx += 256) {
    const int r = idx / DT, c = idx % DT;
    if (r >= c) g[(int64_t)r * N + c] = a[r][c];
    dinv_k[idx] = w[r][c];
  }
}

// diagonal tile kb: unblocked Cholesky in LDS, L_kk written back (lower part), its inverse (lower triangular, full
// 64 x 64 with zeros above) into dinv[kb]; info[2] = 1 if a pivot is not positive.  Launched for kb = 0 only: the later
// diagonal tiles are factorised by the workgroup of k_chol_update that completes them.
__global__ __launch_bounds__(256) void k_chol_diag(int64_t N, int kb, double* __restrict__ A, double* __restrict__ dinv, int32_t* __restrict__ info) {
  __shared__ double a[DT][DP];
  __shared__ double w[DT][DP];
  double* g = A + ((int64_t)kb * DT) * N + (int64_t)kb * DT;
  tile_load(a, g, N, false);
  __syncthreads();
  chol_diag_tile(a, w, g, N, dinv + (int64_t)kb * DT * DT, info);
}

// panel below the diagonal tile: L_ik = A_ik L_kk^-T = A_ik (dinv_k)^T, block rows i = kb + 1 + blockIdx.x
__global__ __launch_bounds__(256) void k_chol_panel(int64_t N, int kb, double* __restrict__ A, const double* __restrict__ dinv) {
  __shared__ double sa[DT][DP];
  __shared__ double sb[DT][DP];
  const int i = kb + 1 + blockIdx.x;
  double* g = A + ((int64_t)i * DT) * N + (int64_t)kb * DT;
  tile_load(sa, g, N, false);
  tile_load(sb, dinv + (int64_t)kb * DT * DT, DT, false);
  __syncthreads();
  TileAcc acc;
  tile_mma(acc, sa, sb);
  tile_foreach(acc, [&](int r, int c, double v) { g[(int64_t)r * N + c] = v; });
}

// trailing update: A_ij -= L_ik L_jk^T for kb < j <= i; blockIdx.x enumerates the pairs (i, j) of the trailing triangle
__global__ __launch_bounds__(256) void k_chol_update(int64_t N, int kb, double* __restrict__ A, double* __restrict__ dinv, int32_t* __restrict__ info) {
  __shared__ double sa[DT][DP];
  __shared__ double sb[DT][DP];
  // pair index -> (ii >= jj) in the triangle of edge m = nblk - kb - 1
  int ii = (int)((sqrt(8.0 * blockIdx.x + 1.0) - 1.0) * 0.5);
  while ((ii + 1) * (ii + 2) / 2 <= (int)blockIdx.x) ++ii;
  while (ii * (ii + 1) / 2 > (int)blockIdx.x) --ii;
  const int jj = blockIdx.x - ii * (ii + 1) / 2;
  const int i = kb + 1 + ii, j = kb + 1 + jj;
  tile_load(sa, A + ((int64_t)i * DT) * N + (int64_t)kb * DT, N, false);
  tile_load(sb, A + ((int64_t)j * DT) * N + (int64_t)kb * DT, N, false);
  __syncthreads();
  TileAcc acc;
  tile_mma(acc, sa, sb);
  double* g = A + ((int64_t)i * DT) * N + (int64_t)j * DT;
  if (blockIdx.x == 0) {
    // tile (kb + 1, kb + 1) is complete with this update: factorise it here, while the other workgroups update the rest of the
    // trailing matrix -- the next step then starts with its panel (the separate diagonal launch was 51 of a step's 92 us)
    __syncthreads();                                       // the products have read sa / sb
    tile_foreach(acc, [&](int r, int c, double v) { sa[r][c] = g[(int64_t)r * N + c] - v; });
    __syncthreads();
    chol_diag_tile(sa, sb, g, N, dinv + (int64_t)(kb + 1) * DT * DT, info);
    return;
  }
  tile_foreach(acc, [&](int r, int c, double v) { g[(int64_t)r * N + c] -= v; });
}

// W = L^-1 by recursive doubling (round 4): with the diagonal tiles inverted (dinv), level s joins pairs of inverted diagonal
// blocks of 2^s tiles, [W_CC 0; W_RC W_RR] with W_RC = -W_RR (L_RC W_CC) -- two launches of independent tile products per
// level, 2 x 6 launches for 48 tiles, where the row-by-row version it replaced was 47 dependent launches whose last ones
// looped over 47 tile products per workgroup (4.5 ms at n = 3060).  phase 0: T_ij = sum_{k = j .. c1 - 1} L_ik W_kj, stored
// TRANSPOSED in T (what phase 1 reads as its B operand); phase 1: W_ij = -sum_{k = r0 .. i} W_ik T_kj, stored transposed in
// the upper triangle of A like every finished tile of W.  Operands: L below the diagonal of A, finished W tiles (k, j), k > j,
// at tile (j, k) of A transposed, diagonal ones in dinv.
__global__ __launch_bounds__(256) void k_trinv_level(int64_t N, int nt, int B, int phase, double* __restrict__ A, const double* __restrict__ dinv,
                                                     double* __restrict__ T) {
  __shared__ double sa[DT][DP];
  __shared__ double sb[DT][DP];
  const int per = B * B;
  const int b = blockIdx.x / per, ij = blockIdx.x % per;
  const int c0 = 2 * b * B, r0 = c0 + B;
  const int i = r0 + ij / B, j = c0 + ij % B;
  if (i >= nt) return;
  const int k_lo = phase == 0 ? j : r0, k_hi = phase == 0 ? r0 : i + 1;          // [k_lo, k_hi)
  TileAcc acc;
  double ra[16], rb[16];
  // operand tiles of step k as [row][k] arrays: phase 0: a = L_ik (tile (i, k), direct), b^T = W_kj: tile (j, k) direct, or dinv_j transposed;
  // phase 1: a = W_ik: tile (k, i) transposed, or dinv_i direct; b^T = T_kj^T: tile (k, j) of T, direct
  auto fetch = [&](int k) {
    const double *ga, *gb;
    int64_t lda, ldb;
    if (phase == 0) {
      ga = A + ((int64_t)i * DT) * N + (int64_t)k * DT; lda = N;
      if (k == j) { gb = dinv + (int64_t)j * DT * DT; ldb = DT; } else { gb = A + ((int64_t)j * DT) * N + (int64_t)k * DT; ldb = N; }
    } else {
      if (k == i) { ga = dinv + (int64_t)i * DT * DT; lda = DT; } else { ga = A + ((int64_t)k * DT) * N + (int64_t)i * DT; lda = N; }
      gb = T + ((int64_t)k * DT) * N + (int64_t)j * DT; ldb = N;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int idx = threadIdx.x + 256 * q, r = idx / DT, c = idx % DT;
      ra[q] = ga[(int64_t)r * lda + c];
      rb[q] = gb[(int64_t)r * ldb + c];
    }
  };
  fetch(k_lo);
  for (int k = k_lo; k < k_hi; ++k) {
    __syncthreads();
    const bool ta = phase == 1 && k != i;                  // a arrives transposed
    const bool tb = phase == 0 && k == j;                  // b^T arrives transposed
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int idx = threadIdx.x + 256 * q, r = idx / DT, c = idx % DT;
      if (ta) sa[c][r] = ra[q]; else sa[r][c] = ra[q];
      if (tb) sb[c][r] = rb[q]; else sb[r][c] = rb[q];
    }
    __syncthreads();
    if (k + 1 < k_hi) fetch(k + 1);
    tile_mma(acc, sa, sb);
  }
  if (phase == 0) {
    double* g = T + ((int64_t)i * DT) * N + (int64_t)j * DT;                                     // T_ij^T: element (c, r)
    tile_foreach(acc, [&](int r, int c, double v) { g[(int64_t)c * N + r] = v; });
  } else {
    double* g = A + ((int64_t)j * DT) * N + (int64_t)i * DT;                                     // tile (j, i) = W_ij^T
    tile_foreach(acc, [&](int r, int c, double v) { g[(int64_t)c * N + r] = -v; });
  }
}

// diagonal tiles of the result: L_kk^-T above, L_kk^-1 below the diagonal
__global__ __launch_bounds__(256) void k_trinv_diag(int64_t N, double* __restrict__ A, const double* __restrict__ dinv) {
  const int kb = blockIdx.x;
  double* g = A + ((int64_t)kb * DT) * N + (int64_t)kb * DT;
  const double* d = dinv + (int64_t)kb * DT * DT;
  for (int idx = threadIdx.x; idx < DT * DT; idx += 256) {
    const int r = idx / DT, c = idx % DT;
    g[(int64_t)r * N + c] = r >= c ? d[r * DT + c] : d[c * DT + r];
  }
}

// off-diagonal part: the upper triangle holds L^-T; copy it transposed into the lower one (over L)
__global__ void k_pc_coarse_mirror(int64_t N, double* __restrict__ A) {
  const int64_t r = blockIdx.y, cidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cidx < N && cidx / DT > r / DT) A[cidx * N + r] = A[r * N + cidx];
}

// the factors of the coarse inverse as the iteration reads them: single precision (round 3).  M_c^-1 = B^T B with B = fl32(L^-1)
// is symmetric positive semi-definite whatever the rounding did, a relative 6e-8 away from the fp64 one -- nothing an
// iteration count sees --, and the two triangular products per iteration stream half the bytes (products and sums in fp64).
__global__ void k_pc_coarse_to_float(int64_t count, const double* __restrict__ A, float* __restrict__ Af, double scale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) Af[i] = (float)(scale * A[i]);
}

// one workgroup per row of the triangular factor: lower = 1: y = L^-1 x (entries 0 .. r of row r); 0: y = L^-T x (r .. n).
// (A wave per row took 25 us per pass at n = 3060: the long rows are 24 dependent rounds of loads for one wave.)
// The solver's x += alpha p carried by extra workgroups of the first coarse product (round 3, see FemoXUpdate in bpx.hip for
// the Poisson twin): the lattice kernels between the restriction and the prolongation are launch- and latency-bound, the
// update depends on nothing they compute, and it must only be done before the prolongation overwrites p.
struct ShellXCarry {
  double* x;
  const double* p;
  const double* alpha;
  int64_t n;
  int row_blocks;        // workgroups [0, row_blocks) do the product, the rest carry
};

__global__ __launch_bounds__(SH_BLOCK) void k_pc_coarse_apply(int64_t n, int64_t N, int lower, const float* __restrict__ W, const double* __restrict__ x,
                                                              double* __restrict__ y, const int32_t* __restrict__ done, ShellXCarry xc = {nullptr, nullptr, nullptr, 0, 0}) {
  if (done != nullptr && *done) return;
  if (xc.x != nullptr && (int)blockIdx.x >= xc.row_blocks) {
    const double alpha = *xc.alpha;
    const int64_t stride = (int64_t)(gridDim.x - xc.row_blocks) * SH_BLOCK;
    for (int64_t i = (int64_t)(blockIdx.x - xc.row_blocks) * SH_BLOCK + threadIdx.x; i < xc.n; i += stride) xc.x[i] += alpha * xc.p[i];
    return;
  }
  __shared__ double lds[SH_BLOCK / 64];
  // rows are paired long with short (r and n - 1 - r take n + 1 entries together): even work per workgroup
  const int64_t pair = blockIdx.x;
  for (int h = 0; h < 2; ++h) {
    const int64_t r = h == 0 ? pair : n - 1 - pair;
    if (h == 1 && r <= pair) break;
    const float* row = W + r * N;
    const int64_t k0 = lower ? 0 : r, k1 = lower ? r + 1 : n;
    double s = 0.0;
    for (int64_t k = k0 + threadIdx.x; k < k1; k += SH_BLOCK) s += (double)row[k] * x[k];
    __syncthreads();
    const double t = femo_block_sum<SH_BLOCK>(s, lds);
    if (threadIdx.x == 0) y[r] = t;
  }
}

}  // namespace

// relative weight of the coarse solve in the additive sum (femo_shell_pc_weights; the factor of the inverse is scaled once
// per stiffness)
static double shell_coarse_weight(const femo_shell* s) { return s->w_coarse; }

// Dense Galerkin operator of the coarse-solve level for the current stiffness and mask, and the factors of its inverse.
// On failure (a pivot not positive, an element larger than a coarse cell) the coarse solve is switched off and the
// diagonal levels take over: the preconditioner changes, the solution does not.
// node_blocks: FEMO_SHELL_NO_BLOCKS is not set (read once per set-up by the caller, which decides on the node blocks with it).
int shell_pc_coarse_setup(femo_shell* s, const femo_vec* vals, const uint8_t* d_fixed, bool node_blocks) {
  s->cs_ready = false;
  s->hermite_on = false;
  if (s->cs_level < 0 || s->d_brow == nullptr) return 0;
  hipStream_t st = s->ctx->stream;
  const int64_t n = s->cs_n, N = s->cs_N;
  const int nblk = (int)(N / DT);
  FEMO_HIP_CHECK(hipMemsetAsync(s->d_cs_A, 0, N * N * sizeof(double), st));
  FEMO_HIP_CHECK(hipMemsetAsync(s->d_cs_info, 0, 4 * sizeof(int32_t), st));
  if (s->hermite && s->d_lvl_node != nullptr && !femo_env_flag("FEMO_SHELL_TRILINEAR") && node_blocks) {
    if (femo_env_flag("FEMO_SHELL_CG_ATOMIC") || s->cs_max_item > MM_ITEM) {      // (items above 256 points: callers of the C ABI may pass them)
      for (int pass = 0; pass < 2; ++pass)
        hipLaunchKernelGGL(k_pc_coarse_galerkin_h, dim3((unsigned)s->cs_items), dim3(256), CGH_LDS, st, pass, s->cs_level, s->pc_width, s->level_off[s->cs_level], N,
                           s->n_unode, s->d_cs_ptr, s->d_cs_pts, s->d_cs_nbr, s->d_cs_pcell, s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_ell_idx,
                           s->d_cs_w4, s->d_cs_A, s->d_cs_info);
    } else {
      hipLaunchKernelGGL(k_pc_coarse_galerkin_mm, dim3((unsigned)s->cs_items), dim3(MM_THREADS), MM_LDS, st, s->cs_level, s->pc_width, s->level_off[s->cs_level], N,
                         s->n_unode, s->d_cs_ptr, s->d_cs_pts, s->d_cs_nbr, s->d_cs_pcell, s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_ell_idx,
                         s->d_cs_w4, s->d_cs_A, s->d_cs_info);
    }
    hipLaunchKernelGGL(k_pc_coarse_mirror_tu, dim3(sgrid(n, 256), (unsigned)n), dim3(256), 0, st, n, N, s->d_cs_A);
    s->hermite_on = true;
  } else {
    hipLaunchKernelGGL(k_pc_coarse_galerkin, dim3((unsigned)s->cs_items), dim3(256), CG_LDS, st, s->cs_level, s->pc_width, s->level_off[s->cs_level], N,
                       s->n_unode, s->d_cs_ptr, s->d_cs_pts, s->d_cs_nbr, s->d_cs_xyz, s->d_cs_pcell, s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_ell_idx,
                       s->d_ell_w, s->d_cs_A, s->d_cs_info);
    s->hermite_on = false;
  }
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_TRY(shell_allreduce(s, s->d_cs_A, N * N, st));      // partitioned: every rank formed P^T (its rows of K) P
  // Hermite-type spaces: the six unknowns of a node the surface barely touches are nearly dependent (a rotation about the
  // line through the few points that see the node moves nothing), the operator is semi-definite there up to rounding and
  // the order of the atomic sums decided whether a pivot came out positive -- a relative 1e-9 on the diagonal settles it
  // (the prototype used 1e-8; the iteration counts do not move)
  hipLaunchKernelGGL(k_pc_coarse_fix_diag, dim3(sgrid(N, 256)), dim3(256), 0, st, N, s->d_cs_A, s->hermite_on ? 1e-9 : 1e-13);
  FEMO_HIP_CHECK(hipGetLastError());
  for (int kb = 0; kb < nblk; ++kb) {
    if (kb == 0) hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), 0, st, N, kb, s->d_cs_A, s->d_cs_dinv, s->d_cs_info);
    const int m = nblk - kb - 1;
    if (m > 0) {
      hipLaunchKernelGGL(k_chol_panel, dim3(m), dim3(256), 0, st, N, kb, s->d_cs_A, s->d_cs_dinv);
      hipLaunchKernelGGL(k_chol_update, dim3(m * (m + 1) / 2), dim3(256), 0, st, N, kb, s->d_cs_A, s->d_cs_dinv, s->d_cs_info);   // also factorises tile kb + 1
    }
  }
  for (int B = 1; B < nblk; B *= 2) {
    const int nb = (nblk + 2 * B - 1) / (2 * B);
    for (int phase = 0; phase < 2; ++phase)
      hipLaunchKernelGGL(k_trinv_level, dim3((unsigned)(nb * B * B)), dim3(256), 0, st, N, nblk, B, phase, s->d_cs_A, s->d_cs_dinv, s->d_cs_T);
  }
  hipLaunchKernelGGL(k_trinv_diag, dim3(nblk), dim3(256), 0, st, N, s->d_cs_A, s->d_cs_dinv);
  hipLaunchKernelGGL(k_pc_coarse_mirror, dim3(sgrid(N, 256), (unsigned)N), dim3(256), 0, st, N, s->d_cs_A);
  hipLaunchKernelGGL(k_pc_coarse_to_float, dim3(2048), dim3(256), 0, st, N * N, s->d_cs_A, s->d_cs_Af, std::sqrt(shell_coarse_weight(s)));
  FEMO_HIP_CHECK(hipGetLastError());
  int32_t info[4] = {0, 0, 0, 0};
  FEMO_HIP_CHECK(hipMemcpyAsync(info, s->d_cs_info, sizeof info, hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  s->cs_ready = info[1] == 0 && info[2] == 0;
  if (s->d_owned != nullptr && s->ctx->nranks > 1) {
    // the ranks must take the same branch (the collectives of the iteration depend on it): the coarse solve is used only
    // if no rank saw a failure (the factorisation is replicated, `far` is a property of the rank's cells)
    const double bad = s->cs_ready ? 0.0 : 1.0;
    double all = 0.0;
    FEMO_HIP_CHECK(hipMemcpyAsync(s->d_cs_tmp, &bad, sizeof bad, hipMemcpyHostToDevice, st));
    FEMO_TRY(shell_allreduce(s, s->d_cs_tmp, 1, st));
    FEMO_HIP_CHECK(hipMemcpyAsync(&all, s->d_cs_tmp, sizeof all, hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    s->cs_ready = all == 0.0;
  }
  if (s->hermite_on && !s->cs_ready) {
    // said once per shell: bench and tests read the state back through femo_shell_pc_info
    fprintf(stderr, "[femo] warning: the Hermite-type coarse operator could not be factorised (far %d, pivot %d); this shell falls back to the trilinear hierarchy\n", info[1], info[2]);
    // the Hermite-type transfers need their own (composed) coarse operator: without it the trilinear hierarchy takes over,
    // whose dense operator is formed now (the preconditioner changes, the solution does not)
    s->hermite = false;
    return shell_pc_coarse_setup(s, vals, d_fixed, node_blocks);
  }
  return 0;
}

// e = A^-1 g on the coarse-solve level (g in d_t, e in d_e): the two triangular products, back to back.
// carry_x != nullptr: 1024 extra workgroups of the first product do the solver's x += alpha p (p = d_p, alpha at d_scal + 5)
void shell_coarse_apply(femo_shell* s, const int32_t* done, double* carry_x, hipStream_t st) {
  const int cs = s->cs_level;
  const unsigned gp = (unsigned)((s->cs_n + 1) / 2);
  ShellXCarry xc = {nullptr, nullptr, nullptr, 0, 0};
  unsigned g1 = gp;
  if (carry_x != nullptr) { xc = {carry_x, s->d_p, s->d_scal + 5, s->n_dof, (int)gp}; g1 = gp + 1024u; }
  hipLaunchKernelGGL(k_pc_coarse_apply, dim3(g1), dim3(SH_BLOCK), 0, st, s->cs_n, s->cs_N, 1, (const float*)s->d_cs_Af,
                     s->d_t + 6 * s->level_off[cs], s->d_cs_tmp, done, xc);
  hipLaunchKernelGGL(k_pc_coarse_apply, dim3(gp), dim3(SH_BLOCK), 0, st, s->cs_n, s->cs_N, 0, (const float*)s->d_cs_Af, s->d_cs_tmp,
                     s->d_e + 6 * s->level_off[cs], done);
}

// the Galerkin kernels of the Hermite-type spaces use more LDS than a kernel gets by default (femo_shell_pc_hermite)
int shell_coarse_hermite_lds() {
  FEMO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pc_coarse_galerkin_h), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CGH_LDS));
  FEMO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pc_coarse_galerkin_mm), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MM_LDS));
  return 0;
}

extern "C" {

int femo_shell_pc_coarse(femo_shell* s, int level, const int32_t* node_xyz, int64_t n_items, const int64_t* item_ptr,
                         const int32_t* item_pts, const int32_t* item_nbr, const int64_t* down_rowptr, const int32_t* down_cols,
                         const double* down_vals) {
  FEMO_REQUIRE(s && node_xyz && item_ptr && item_pts && item_nbr, "null argument");
  FEMO_REQUIRE(s->pc_width > 0, "femo_shell_pc_coarse needs femo_shell_pc_create first");
  FEMO_REQUIRE(level >= 0 && level < s->pc_levels - 1 && n_items > 0 && s->cs_level < 0, "bad coarse-solve level");
  FEMO_REQUIRE(s->d_brow != nullptr, "the coarse solve needs the node-block view of the pattern");
  hipStream_t st = s->ctx->stream;
  FEMO_HIP_CHECK(hipSetDevice(s->ctx->device));
  const int64_t nodes = s->level_off[level + 1] - s->level_off[level];
  const int64_t n = 6 * nodes;
  FEMO_REQUIRE(n <= 8192, "coarse-solve level too large for a dense inverse");
  s->cs_max_item = 0;
  for (int64_t it = 0; it < n_items; ++it) {
    FEMO_REQUIRE(item_ptr[it + 1] > item_ptr[it], "empty Galerkin item");
    s->cs_max_item = std::max<int64_t>(s->cs_max_item, item_ptr[it + 1] - item_ptr[it]);
  }
  FEMO_TRY(to_device(&s->d_cs_xyz, node_xyz, 3 * nodes, st));
  FEMO_TRY(to_device(&s->d_cs_ptr, item_ptr, n_items + 1, st));
  FEMO_TRY(to_device(&s->d_cs_pts, item_pts, item_ptr[n_items], st));
  FEMO_TRY(to_device(&s->d_cs_nbr, item_nbr, n_items * 64, st));
  const int64_t N = (n + DT - 1) / DT * DT;
  FEMO_HIP_CHECK(hipMalloc(&s->d_cs_A, N * N * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_cs_Af, N * N * sizeof(float)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_cs_tmp, N * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_cs_dinv, N * DT * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_cs_T, N * N * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_cs_info, 4 * sizeof(int32_t)));
  FEMO_REQUIRE(s->level_off[level + 1] - s->level_off[level] > 0 && (1 << 10) > (1 << (level + 1)), "lattice too fine for 10-bit coordinates");
  FEMO_HIP_CHECK(hipMalloc(&s->d_cs_pcell, (s->n_dof / 3) * sizeof(int32_t)));
  hipLaunchKernelGGL(k_pc_coarse_cells, dim3(sgrid(s->n_dof / 3, 256)), dim3(256), 0, st, s->n_dof / 3, level, s->pc_width, s->level_off[level],
                     s->d_ell_idx, s->d_cs_xyz, s->d_cs_pcell);
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  if (down_rowptr != nullptr && down_cols != nullptr && down_vals != nullptr) {
    // rows: the nodes of levels `level` .. L - 2 in their global order, columns: global node numbers of the finest lattice
    const int64_t rows = s->level_off[s->pc_levels - 1] - s->level_off[level];
    FEMO_TRY(to_device(&s->d_cd_rowptr, down_rowptr, rows + 1, st));
    FEMO_TRY(to_device(&s->d_cd_cols, down_cols, down_rowptr[rows], st));
    FEMO_TRY(to_device(&s->d_cd_vals, down_vals, down_rowptr[rows], st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
  }
  FEMO_TRY(shell_pc_compact_levels(s, level, st));
  FEMO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pc_coarse_galerkin), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CG_LDS));
  s->cs_level = level; s->cs_n = n; s->cs_N = N; s->cs_items = n_items;
  s->pc_vals_uid = 0; s->pc_vals_gen = 0;                 // next solve recomputes the preconditioner's numbers
  return 0;
}

// For tests: the dense coarse operator (inverse = 0) or the factors of its inverse (1: L^-T above, L^-1 below the
// diagonal) for `vals` and the mask, row-major n x n on the host; the unknown count through *n_out.
int femo_shell_pc_coarse_matrix(femo_shell* s, const femo_vec* vals, const uint8_t* fixed_host, int inverse, double* out, int64_t* n_out) {
  FEMO_REQUIRE(s && vals && n_out, "null argument");
  FEMO_REQUIRE(s->cs_level >= 0, "no coarse solve on this shell");
  hipStream_t st = s->ctx->stream;
  *n_out = s->cs_n;
  if (out == nullptr) return 0;
  uint8_t* d_fixed = nullptr;
  if (fixed_host != nullptr) FEMO_TRY(to_device(&d_fixed, fixed_host, s->n_dof, st));
  const int64_t n = s->cs_n, N = s->cs_N;
  if (inverse) {
    FEMO_TRY(shell_pc_coarse_setup(s, vals, d_fixed, !femo_env_flag("FEMO_SHELL_NO_BLOCKS")));
    FEMO_REQUIRE(s->cs_ready, "the coarse operator could not be factorised");
  } else {
    FEMO_HIP_CHECK(hipMemsetAsync(s->d_cs_A, 0, N * N * sizeof(double), st));
    FEMO_HIP_CHECK(hipMemsetAsync(s->d_cs_info, 0, 4 * sizeof(int32_t), st));
    if (s->hermite && !femo_env_flag("FEMO_SHELL_TRILINEAR")) {
      for (int pass = 0; pass < 2; ++pass)
        hipLaunchKernelGGL(k_pc_coarse_galerkin_h, dim3((unsigned)s->cs_items), dim3(256), CGH_LDS, st, pass, s->cs_level, s->pc_width, s->level_off[s->cs_level], N,
                           s->n_unode, s->d_cs_ptr, s->d_cs_pts, s->d_cs_nbr, s->d_cs_pcell, s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_ell_idx,
                           s->d_cs_w4, s->d_cs_A, s->d_cs_info);
      hipLaunchKernelGGL(k_pc_coarse_mirror_tu, dim3(sgrid(n, 256), (unsigned)n), dim3(256), 0, st, n, N, s->d_cs_A);
    } else {
      hipLaunchKernelGGL(k_pc_coarse_galerkin, dim3((unsigned)s->cs_items), dim3(256), CG_LDS, st, s->cs_level, s->pc_width, s->level_off[s->cs_level], N,
                         s->n_unode, s->d_cs_ptr, s->d_cs_pts, s->d_cs_nbr, s->d_cs_xyz, s->d_cs_pcell, s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_ell_idx,
                         s->d_ell_w, s->d_cs_A, s->d_cs_info);
    }
    FEMO_HIP_CHECK(hipGetLastError());
    s->cs_ready = false;
  }
  s->pc_vals_uid = 0; s->pc_vals_gen = 0;
  FEMO_HIP_CHECK(hipMemcpy2DAsync(out, n * sizeof(double), s->d_cs_A, N * sizeof(double), n * sizeof(double), n, hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  if (d_fixed) (void)hipFree(d_fixed);
  return 0;
}

}  // extern "C"

void shell_coarse_free(femo_shell* s) {
  hipFree(s->d_cs_xyz); hipFree(s->d_cs_ptr); hipFree(s->d_cs_pts); hipFree(s->d_cs_nbr); hipFree(s->d_cs_A); hipFree(s->d_cs_Af); hipFree(s->d_cs_tmp);
  hipFree(s->d_cs_dinv); hipFree(s->d_cs_T); hipFree(s->d_cs_info); hipFree(s->d_cs_pcell);
  hipFree(s->d_cd_rowptr); hipFree(s->d_cd_cols); hipFree(s->d_cd_vals);
}
