// Reissner-Mindlin shell: the nested-lattice preconditioner -- restriction, level and prolongation kernels of the
// trilinear and the Hermite-type spaces, the 6 x 6 Galerkin node blocks and 3 x 3 point blocks, their set-up for a
// stiffness and a Dirichlet set, and the apply (shell_internal.h has the overview; the dense solve on the coarsest
// level kept is shell_coarse.hip).  The file keeps the name of the unit the others were cut out of.
#include "shell_internal.h"

namespace {

// ------------------------------------------------------- lattice preconditioner ----
// M^-1 = D^-1 + sum_l P_l C_l P_l^T: P_l = trilinear interpolation from a lattice of spacing 2^-l x (bounding cube) to
// the dof nodes, component by component (3 displacement fields on the P2 nodes, 3 rotation fields on the vertices),
// C_l = 1 / diag(P_l^T K P_l) -- the Galerkin diagonal, which carries the h / h^3 scaling of the membrane and bending
// parts per component.  Measured with the oracle (Scordelis-Lo, rtol 1e-10): 979 / 1066 / 1149 iterations on
// 16^2 / 32^2 / 64^2 against 3171 / 7491 / 15139 for Jacobi -- nearly mesh independent where Jacobi grows like n.
// The lattices are nested (P_l = P_{l+1} T_l exactly), so only the finest one touches the dofs: g_L = P_L^T r, then
// g_l = T_l^T g_{l+1} down the hierarchy, e_0 = C_0 g_0, e_{l+1} = C_{l+1} g_{l+1} + T_l e_l up again, z = D^-1 r +
// P_L e_L.  (The first version applied every level's P_l directly: the rows of P_0^T have n_dof / 4 entries, 2.4 ms
// per iteration at 248 k dofs.)  P of every level is kept in ELL form for the Galerkin diagonals.

// diag[j] += sum_i sum_k P[i,j] K[i,k] P[k,j] over the free dofs: one thread per (row i, ELL slot a)
__global__ __launch_bounds__(SH_BLOCK) void k_pc_galerkin_diag(int64_t n, int width, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                               const double* __restrict__ vals, const uint8_t* __restrict__ fixed,
                                                               const int32_t* __restrict__ ell_idx, const double* __restrict__ ell_w,
                                                               double* __restrict__ diag, int first_slot) {
  // slots first_slot .. width - 1 of every row (the levels below belong to the coarse solve when there is one)
  const int wact = width - first_slot;
  const int64_t t = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  const int64_t i = t / wact;
  const int a = first_slot + (int)(t % wact);
  if (i >= n || (fixed != nullptr && fixed[i])) return;
  const double wi = ell_w[i * width + a];
  if (wi == 0.0) return;
  const int32_t j = ell_idx[i * width + a];
  const int lev8 = (a >> 3) << 3;
  double acc = 0.0;
  for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
    const int32_t k = cols[e];
    if (fixed != nullptr && fixed[k]) continue;
    const int32_t* ik = ell_idx + (int64_t)k * width + lev8;
    const double* wk = ell_w + (int64_t)k * width + lev8;
    double pk = 0.0;
#pragma unroll
    for (int b = 0; b < 8; ++b) pk += ik[b] == j ? wk[b] : 0.0;
    acc += vals[e] * pk;
  }
  atomicAdd(&diag[j], wi * acc);
}

// ---- Galerkin set-up for the Hermite-type lattice spaces ------------------------------------------------------------------
// W_p,n = [alpha I, -[sigma]x] (3 x 6) for a displacement point, [0, w I] for a rotation point: blk[n] = sum over the pairs
// of points (p, q) that both touch node n of W_p,n^T K_pq W_q,n.  Same organisation as k_pc_galerkin_blocks (a thread per
// (point, level, component fa), the row's sums against the point's eight nodes in registers), but a row dof of a
// displacement point now feeds three rows of the block (U_fa with alpha, two Theta rows with -+sigma), so the LDS table is
// keyed by node and holds whole 6 x 6 blocks (upper triangle used).
__global__ __launch_bounds__(SH_BLOCK) void k_pc_galerkin_blocks_h(int64_t n_pts, int64_t n_unode, const int64_t* __restrict__ brow,
                                                                   const int32_t* __restrict__ bcols, const double* __restrict__ vals,
                                                                   const uint8_t* __restrict__ fixed, const int32_t* __restrict__ lvl_node,
                                                                   const float4* __restrict__ lvl_w4, double* __restrict__ blk) {
  constexpr int HS = 256;
  __shared__ int32_t h_key[HS];
  __shared__ double h_val[HS][36];
  for (int i = threadIdx.x; i < HS; i += SH_BLOCK) h_key[i] = -1;
  for (int i = threadIdx.x; i < HS * 36; i += SH_BLOCK) (&h_val[0][0])[i] = 0.0;
  __syncthreads();
  const int fa = (int)(blockIdx.y % 3);
  const int32_t* ln = lvl_node + (int64_t)(blockIdx.y / 3) * n_pts * 8;
  const float4* lw = lvl_w4 + (int64_t)(blockIdx.y / 3) * n_pts * 8;
  const int64_t p = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  const bool active = p < n_pts && !(fixed != nullptr && fixed[3 * p + fa]);
  if (active) {
    int32_t nd[8];
    float4 wi[8];
    double acc[8][6];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      nd[a] = ln[p * 8 + a];
      wi[a] = lw[p * 8 + a];
      if (wi[a].x == 0.f && wi[a].y == 0.f && wi[a].z == 0.f && wi[a].w == 0.f) nd[a] = -1;
#pragma unroll
      for (int q = 0; q < 6; ++q) acc[a][q] = 0.0;
    }
    const bool pu = p < n_unode;
    const int64_t k0 = brow[p], k1 = brow[p + 1], len = 3 * (k1 - k0);
    const double* v = vals + 9 * k0 + fa * len;
    for (int64_t k = k0; k < k1; ++k) {
      const int32_t cj = bcols[k];
      const int32_t* ik = ln + (int64_t)(cj / 3) * 8;
      const float4* wk = lw + (int64_t)(cj / 3) * 8;
      const int64_t o = 3 * (k - k0);
      double m0 = v[o], m1 = v[o + 1], m2 = v[o + 2];
      if (fixed != nullptr) {
        if (fixed[cj]) m0 = 0.0;
        if (fixed[cj + 1]) m1 = 0.0;
        if (fixed[cj + 2]) m2 = 0.0;
      }
      const bool qu = cj < 3 * n_unode;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int32_t nb = ik[b];
        const float4 w = wk[b];
        // the row vector m (1 x 3) times W_q,b: [alpha m, sigma x m] for a displacement column, [0, w m] for a rotation column
        double c0, c1, c2, c3, c4, c5;
        if (qu) {
          c0 = (double)w.x * m0; c1 = (double)w.x * m1; c2 = (double)w.x * m2;
          c3 = (double)w.z * m2 - (double)w.w * m1; c4 = (double)w.w * m0 - (double)w.y * m2; c5 = (double)w.y * m1 - (double)w.z * m0;
        } else {
          c0 = c1 = c2 = 0.0;
          c3 = (double)w.x * m0; c4 = (double)w.x * m1; c5 = (double)w.x * m2;
        }
#pragma unroll
        for (int a = 0; a < 8; ++a) {
          const double on = nb == nd[a] ? 1.0 : 0.0;
          acc[a][0] += on * c0; acc[a][1] += on * c1; acc[a][2] += on * c2;
          acc[a][3] += on * c3; acc[a][4] += on * c4; acc[a][5] += on * c5;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      if (nd[a] < 0) continue;
      const int32_t key = nd[a];
      int h = (int)(((uint32_t)key * 2654435761u) >> 24) & (HS - 1);
      int slot = -1;
      for (int probe = 0; probe < 16; ++probe) {
        const int32_t seen = atomicCAS(&h_key[h], -1, key);
        if (seen == -1 || seen == key) { slot = h; break; }
        h = (h + 1) & (HS - 1);
      }
      // rows of the block this dof feeds: (row, coefficient)
      int rw[3];
      double cf[3];
      int nrow;
      if (pu) {
        const double sg[3] = {(double)wi[a].y, (double)wi[a].z, (double)wi[a].w};
        const int k1i = (fa + 1) % 3, k2i = (fa + 2) % 3;          // (Theta x sigma)_fa = Theta_k1 sigma_k2 - Theta_k2 sigma_k1
        rw[0] = fa; cf[0] = (double)wi[a].x;
        rw[1] = 3 + k1i; cf[1] = sg[k2i];
        rw[2] = 3 + k2i; cf[2] = -sg[k1i];
        nrow = 3;
      } else {
        rw[0] = 3 + fa; cf[0] = (double)wi[a].x;
        nrow = 1;
      }
      for (int rI = 0; rI < nrow; ++rI) {
        if (cf[rI] == 0.0) continue;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          if (q < rw[rI] || acc[a][q] == 0.0) continue;
          const double val = cf[rI] * acc[a][q];
          if (slot >= 0) __hip_atomic_fetch_add(&h_val[slot][6 * rw[rI] + q], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          else atomicAdd(&blk[36 * (int64_t)key + 6 * rw[rI] + q], val);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < HS * 36; i += SH_BLOCK) {
    const int32_t key = h_key[i / 36];
    if (key < 0) continue;
    const double val = (&h_val[0][0])[i];
    if (val != 0.0) atomicAdd(&blk[36 * (int64_t)key + (i % 36)], val);
  }
}

// 6 x 6 Galerkin node blocks of the levels above the coarse solve, Hermite-type spaces, second version (round 4).  The
// version above walks every row three times per level from a thread per (point, level, component): K was fetched nine
// times (9 GB at 1.97 M dofs, 10.5 ms).  Here a WAVE takes an item -- at most 64 points of one cell of one level, so that
// all of them share the cell's eight nodes -- with lanes = (node a of the cell, column f' of the block):
//   per point p: the lanes first fetch the point's column indices and the level-l cells of its column points (one per lane:
//   two dependent loads per POINT, not per block); then, block by block, M[fa] += (K_pq)[fa][.] . u with u the column f' of
//   W_q,b and b the corner of q's cell that IS node a (b = a - cell offset; no match: nothing) -- the weight gathers of
//   the blocks are independent of each other; last acc[r] += (W_p,a^T M)[r] (r = 0..5);
//   per item: one flush of the upper triangles with atomics (the items of a cell and the neighbouring cells share nodes).
// The cell offset of a column point is at most one cell per axis when elements are smaller than the cells of the finest
// lattice; a larger one sets info[1] bit 1 and the caller falls back to the kernel above.
__global__ void k_point_fixbits(int64_t n_pts, const uint8_t* __restrict__ fixed, uint8_t* __restrict__ bits) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  bits[p] = fixed == nullptr ? 0 : (uint8_t)((fixed[3 * p] ? 1 : 0) | (fixed[3 * p + 1] ? 2 : 0) | (fixed[3 * p + 2] ? 4 : 0));
}

__global__ __launch_bounds__(256) void k_pc_galerkin_blocks_w(int64_t n_items, int64_t n_pts, int64_t n_unode, const int64_t* __restrict__ item_ptr,
                                                              const int32_t* __restrict__ item_lvl, const int32_t* __restrict__ item_pts,
                                                              const int32_t* __restrict__ pcell, const int64_t* __restrict__ brow,
                                                              const int32_t* __restrict__ bcols, const double* __restrict__ vals,
                                                              const uint8_t* __restrict__ fixbits, const int32_t* __restrict__ lvl_node,
                                                              const float4* __restrict__ lvl_w4, double* __restrict__ blk, int32_t* __restrict__ info) {
  constexpr int EC = 32;                                                   // blocks staged per round
  __shared__ double s_K[4][3][3 * EC];                                     // rows fa of the staged blocks (columns of fixed dofs zeroed)
  __shared__ float4 s_W[4][EC * 8];                                        // [block e][node a of THIS cell]: weight of the corner of q's cell that is node a, or 0
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t item = (int64_t)blockIdx.x * 4 + wv;
  if (item >= n_items) return;
  const int a = lane & 7, fc = lane >> 3;                                  // node of the cell, column of the block (fc < 6)
  // column f' = fc of W_q,b as a 3-vector u = (sg[k] * w[ix[k]])_k with w = (alpha, sigma) of the corner: displacement column
  // fc < 3: alpha e_fc; fc = 3: (0, -s2, s1); 4: (s2, 0, -s0); 5: (-s1, s0, 0); rotation column: w e_(fc-3) for fc >= 3
  int ixu[3] = {0, 0, 0};
  double sgu[3] = {0.0, 0.0, 0.0}, sgr[3] = {0.0, 0.0, 0.0};
  if (fc < 3) sgu[fc] = 1.0;
  else if (fc == 3) { ixu[1] = 3; sgu[1] = -1.0; ixu[2] = 2; sgu[2] = 1.0; sgr[0] = 1.0; }
  else if (fc == 4) { ixu[0] = 3; sgu[0] = 1.0; ixu[2] = 1; sgu[2] = -1.0; sgr[1] = 1.0; }
  else if (fc == 5) { ixu[0] = 2; sgu[0] = -1.0; ixu[1] = 1; sgu[1] = 1.0; sgr[2] = 1.0; }
  const int64_t pbeg = item_ptr[item], pend = item_ptr[item + 1];
  const int lv = item_lvl[item];
  const int32_t* ln = lvl_node + (int64_t)lv * n_pts * 8;
  const float4* lw = lvl_w4 + (int64_t)lv * n_pts * 8;
  const int32_t* pc = pcell + (int64_t)lv * n_pts;
  const int32_t pfirst = item_pts[pbeg];
  const int32_t node_a = ln[(int64_t)pfirst * 8 + a];
  const int32_t ck = pc[pfirst];
  const int cx = ck & 1023, cy = (ck >> 10) & 1023, cz = ck >> 20;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int far = 0;
  double (*sK)[3 * EC] = s_K[wv];
  float4* sW = s_W[wv];
  const float* sWf = reinterpret_cast<const float*>(sW);
  // three-stage software pipeline over the item's points: every iteration issues ONE level of the chain point id -> row
  // extent (+ the point's own weights and Dirichlet bits) -> column indices for a later point, after the loads of the current
  // point, so that a point's round starts with its column indices in registers
  const int64_t npt = pend - pbeg;
  int32_t p_2 = npt > 2 ? item_pts[pbeg + 2] : 0;
  int32_t p_1 = npt > 1 ? item_pts[pbeg + 1] : 0;
  int64_t k0_1 = 0; int nb_1 = 0; float4 wp_1 = float4{0.f, 0.f, 0.f, 0.f}; int fi_1 = 0;
  if (npt > 1) {
    k0_1 = brow[p_1]; nb_1 = (int)(brow[p_1 + 1] - k0_1); wp_1 = lw[(int64_t)p_1 * 8 + a]; fi_1 = fixbits == nullptr ? 0 : fixbits[p_1];
  }
  int32_t p_0 = pfirst;
  int64_t k0_0 = brow[p_0];
  int nb_0 = (int)(brow[p_0 + 1] - k0_0);
  float4 wp_0 = lw[(int64_t)p_0 * 8 + a];
  int fi_0 = fixbits == nullptr ? 0 : fixbits[p_0];
  int32_t cj_0 = lane < min(EC, nb_0) ? bcols[k0_0 + lane] : 0;
  auto advance = [&](int64_t ip) {
    const int64_t left = pend - ip;
    cj_0 = left > 1 && lane < min(EC, nb_1) ? bcols[k0_1 + lane] : 0;
    p_0 = p_1; k0_0 = k0_1; nb_0 = nb_1; wp_0 = wp_1; fi_0 = fi_1;
    if (left > 2) {
      k0_1 = brow[p_2]; nb_1 = (int)(brow[p_2 + 1] - k0_1); wp_1 = lw[(int64_t)p_2 * 8 + a]; fi_1 = fixbits == nullptr ? 0 : fixbits[p_2];
    }
    p_1 = p_2;
    p_2 = left > 3 ? item_pts[ip + 3] : 0;
  };
  for (int64_t ip = pbeg; ip < pend; ++ip) {
    const int32_t p = p_0;
    const int64_t k0 = k0_0;
    const int nb = nb_0;
    const int64_t len = 3 * (int64_t)nb;
    const float4 wp = wp_0;
    const int fi = fi_0;
    const int32_t cj_first = cj_0;
    const bool pu = p < n_unode;
    double M0 = 0.0, M1 = 0.0, M2 = 0.0;
    if (nb == 0) advance(ip);
    for (int e0 = 0; e0 < nb; e0 += EC) {
      const int cnt = min(EC, nb - e0);
      // the round's loads, all issued before anything is used: the blocks' rows (3 x 3 cnt contiguous doubles), lane e < cnt the
      // column index of block e0 + e, then -- one dependent step -- its level-l cell and Dirichlet bits and the eight weights
      double kv[2][3];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int fa = 0; fa < 3; ++fa) {
          const int idx = lane + 64 * h;
          kv[h][fa] = idx < 3 * cnt ? vals[9 * k0 + fa * len + 3 * e0 + idx] : 0.0;
        }
      int32_t my_cj = cj_first, my_meta = -1;
      if (e0 > 0) my_cj = lane < cnt ? bcols[k0 + e0 + lane] : 0;
      float4 wl[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int idx = lane + 64 * h, e = idx >> 3;
        const int32_t cje = __shfl(my_cj, e);
        wl[h] = e < cnt ? lw[(int64_t)(cje / 3) * 8 + (idx & 7)] : float4{0.f, 0.f, 0.f, 0.f};
      }
      if (lane < cnt) {
        const int32_t q = my_cj / 3;
        const int32_t pk = pc[q];
        const int ox = (pk & 1023) - cx + 1, oy = ((pk >> 10) & 1023) - cy + 1, oz = (pk >> 20) - cz + 1;
        if ((unsigned)ox > 2u || (unsigned)oy > 2u || (unsigned)oz > 2u) far = 1;
        else my_meta = ox | (oy << 2) | (oz << 4) | ((fixbits == nullptr ? 0 : fixbits[q]) << 6) | ((my_cj < 3 * n_unode ? 1 : 0) << 9);
      }
      if (e0 == 0) advance(ip);                            // the pipeline's loads for the points after this one
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int idx = lane + 64 * h;
        const int32_t me = __shfl(my_meta, idx / 3);
        const bool off = idx >= 3 * cnt || me < 0 || ((me >> (6 + idx % 3)) & 1);       // column of a fixed dof
#pragma unroll
        for (int fa = 0; fa < 3; ++fa)
          if (idx < 3 * EC) sK[fa][idx] = off ? 0.0 : kv[h][fa];
      }
      // weights: entry (e, corner b of q's cell) goes to the slot of the node a = b + cell offset of THIS cell, if it is one
#pragma unroll
      for (int h = 0; h < 4; ++h) sW[lane + 64 * h] = float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int idx = lane + 64 * h, e = idx >> 3, b = idx & 7;
        const int32_t me = __shfl(my_meta, e);
        const int tx = (b & 1) + (me & 3) - 1, ty = ((b >> 1) & 1) + ((me >> 2) & 3) - 1, tz = (b >> 2) + ((me >> 4) & 3) - 1;
        if (e < cnt && me >= 0 && (unsigned)tx < 2u && (unsigned)ty < 2u && (unsigned)tz < 2u) sW[8 * e + tx + 2 * ty + 4 * tz] = wl[h];
      }
      const uint64_t qmask = __ballot(lane < cnt && my_meta >= 0 && ((my_meta >> 9) & 1));      // blocks with a displacement column
      // LDS only (the wave's LDS operations execute in order): a fence would also wait for the loads of the pipeline
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const float* wa = sWf + 4 * a;
#pragma unroll 2
      for (int e = 0; e < cnt; ++e) {
        const float* w = wa + 32 * e;
        double u0, u1, u2;
        if ((qmask >> e) & 1) { u0 = sgu[0] * (double)w[ixu[0]]; u1 = sgu[1] * (double)w[ixu[1]]; u2 = sgu[2] * (double)w[ixu[2]]; }
        else { const double al = (double)w[0]; u0 = sgr[0] * al; u1 = sgr[1] * al; u2 = sgr[2] * al; }
        const double* k = &sK[0][3 * e];
        M0 += k[0] * u0 + k[1] * u1 + k[2] * u2;
        M1 += k[3 * EC] * u0 + k[3 * EC + 1] * u1 + k[3 * EC + 2] * u2;
        M2 += k[6 * EC] * u0 + k[6 * EC + 1] * u1 + k[6 * EC + 2] * u2;
      }
      // LDS only (the wave's LDS operations execute in order): a fence would also wait for the loads of the pipeline
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (fi & 1) M0 = 0.0;
    if (fi & 2) M1 = 0.0;
    if (fi & 4) M2 = 0.0;
    if (pu) {
      const double al = (double)wp.x, s0 = (double)wp.y, s1 = (double)wp.z, s2 = (double)wp.w;
      acc[0] += al * M0; acc[1] += al * M1; acc[2] += al * M2;
      acc[3] += -s2 * M1 + s1 * M2;
      acc[4] += s2 * M0 - s0 * M2;
      acc[5] += -s1 * M0 + s0 * M1;
    } else {
      const double w = (double)wp.x;
      acc[3] += w * M0; acc[4] += w * M1; acc[5] += w * M2;
    }
  }
  if (far && info != nullptr) atomicOr(&info[1], 2);
  if (fc < 6 && node_a >= 0) {
#pragma unroll
    for (int r = 0; r < 6; ++r)
      if (r <= fc && acc[r] != 0.0) atomicAdd(&blk[36 * (int64_t)node_a + 6 * r + fc], acc[r]);
  }
}

__global__ void k_pc_invert(int64_t n, double* __restrict__ d) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    d[i] = d[i] > 0.0 ? 1.0 / d[i] : 0.0;
}

// The coarse end of the hierarchy in one single-workgroup launch: levels kc .. 0 down, then 0 .. kc up (a few
// thousand nodes; as separate launches each costs its ~5 us launch floor).  The levels communicate through global
// memory inside one workgroup: __syncthreads() drains the stores before the barrier.
struct LatLevels { int kc; int64_t off[18]; };
__global__ __launch_bounds__(1024) void k_lat_coarse_fused(LatLevels Lv, const int64_t* __restrict__ chi_rowptr, const int32_t* __restrict__ chi_cols,
                                                           const double* __restrict__ chi_vals, const int64_t* __restrict__ par_rowptr,
                                                           const int32_t* __restrict__ par_cols, const double* __restrict__ par_vals,
                                                           const double* __restrict__ coarse, double* g, double* e, const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  for (int l = Lv.kc; l >= 0; --l) {
    const int64_t n0 = Lv.off[l], cnt = (Lv.off[l + 1] - n0) * 6;
    for (int64_t t = threadIdx.x; t < cnt; t += 1024) {
      const int64_t node = n0 + t / 6;
      const int f = (int)(t % 6);
      double s = 0.0;
      for (int64_t k = chi_rowptr[node]; k < chi_rowptr[node + 1]; ++k) s += chi_vals[k] * g[6 * (int64_t)chi_cols[k] + f];
      g[6 * node + f] = s;
    }
    __syncthreads();
  }
  for (int l = 0; l <= Lv.kc; ++l) {
    const int64_t n0 = Lv.off[l], cnt = (Lv.off[l + 1] - n0) * 6;
    for (int64_t t = threadIdx.x; t < cnt; t += 1024) {
      const int64_t node = n0 + t / 6;
      const int f = (int)(t % 6);
      const int64_t u = 6 * node + f;
      double s = 0.0;
      for (int64_t k = par_rowptr[node]; k < par_rowptr[node + 1]; ++k) s += par_vals[k] * e[6 * (int64_t)par_cols[k] + f];
      e[u] = coarse[u] * g[u] + s;
    }
    __syncthreads();
  }
}

// g = P_L^T r on the finest lattice's nodes [m0, m1): one row per (node, field group) listing the points (first dof
// 3 p) that touch the node and their weights, SUB lanes per row, three components at a time
template <int SUB>
__global__ __launch_bounds__(SH_BLOCK) void k_pc_restrict(int64_t m0, int64_t m1, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                          const float* __restrict__ vals, const double* __restrict__ r, double* __restrict__ g,
                                                          const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  const int sl = threadIdx.x & (SUB - 1);
  const int64_t nsub = (int64_t)gridDim.x * (SH_BLOCK / SUB);
  const int64_t nrow = 2 * (m1 - m0);
  for (int64_t row = (int64_t)blockIdx.x * (SH_BLOCK / SUB) + (threadIdx.x / SUB); row < nrow; row += nsub) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int64_t e1 = rowptr[row + 1];
    for (int64_t e = rowptr[row] + sl; e < e1; e += SUB) {
      const int32_t c = cols[e];
      const double w = (double)vals[e];
      const Triple rc = *reinterpret_cast<const Triple*>(r + c);
      s0 += w * rc.a;
      s1 += w * rc.b;
      s2 += w * rc.c;
    }
#pragma unroll
    for (int off = SUB / 2; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off, 64);
      s1 += __shfl_xor(s1, off, 64);
      s2 += __shfl_xor(s2, off, 64);
    }
    if (sl < 3) g[6 * (m0 + (row >> 1)) + 3 * (row & 1) + sl] = sl == 0 ? s0 : (sl == 1 ? s1 : s2);
  }
}

// one lattice level, nodes [n0, n1), six fields per node (unknown 6 node + f), one thread per unknown:
//   down: g[u] = sum over the node's children c of w g[6 c + f]                       (T^T, <= 27 children)
//   up:   e[u] = C[u] g[u] + sum over the node's parents p of w e[6 p + f]           (T, <= 8 parents; none on level 0)
//   blocks != nullptr (up only): C is the node's 6 x 6 block (row f of blocks[36 node ..]) instead of the diagonal
__global__ __launch_bounds__(256) void k_lat_level(int64_t n0, int64_t n1, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                            const double* __restrict__ vals, const double* __restrict__ coarse, double* __restrict__ g,
                            double* __restrict__ e, int up, const int32_t* __restrict__ done, const double* __restrict__ blocks = nullptr,
                            double* __restrict__ dot_partials = nullptr) {
  if (done != nullptr && *done) return;
  // dot_partials (up, finest level only): per-block partial of e . g over the level -- with r . (B r) from the update
  // kernel it gives r . z before z exists (r . P e = (P^T r) . e), so the direction update is fused into the prolongation
  __shared__ double lds[256 / 64];
  double dot = 0.0;
  const int64_t total = (n1 - n0) * 6;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t node = n0 + t / 6;
    const int f = (int)(t % 6);
    const int64_t u = 6 * node + f;
    const double* src = up ? e : g;
    double s = 0.0;
    for (int64_t k = rowptr[node]; k < rowptr[node + 1]; ++k) s += vals[k] * src[6 * (int64_t)cols[k] + f];
    if (!up) { g[u] = s; continue; }
    if (blocks != nullptr) {
      const double* B = blocks + 36 * node + 6 * f;
      const double* gn = g + 6 * node;
#pragma unroll
      for (int q = 0; q < 6; ++q) s += B[q] * gn[q];
    } else {
      s += coarse[u] * g[u];
    }
    e[u] = s;
    dot += s * g[u];
  }
  if (dot_partials != nullptr) {
    const double tsum = femo_block_sum<256>(dot, lds);
    if (threadIdx.x == 0) dot_partials[blockIdx.x] = tsum;
  }
}

// per-point copies of the ELL entries of the levels first_slot / 8 and up (node = unknown / 6): [level][point][8]
__global__ void k_compact_levels(int64_t n_pts, int width, int first_slot, const int32_t* __restrict__ ell_idx,
                                 const double* __restrict__ ell_w, int32_t* __restrict__ node, double* __restrict__ w) {
  const int nlev = (width - first_slot) >> 3;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_pts * nlev * 8) return;
  const int a = (int)(t & 7);
  const int64_t p = (t >> 3) % n_pts;
  const int lv = (int)((t >> 3) / n_pts);
  const int64_t e = (3 * p) * width + first_slot + 8 * lv + a;
  node[t] = ell_idx[e] / 6;
  w[t] = ell_w[e];
}

// 6 x 6 Galerkin blocks of the lattice nodes, levels first_slot / 8 and up: blk[node][f][f'] = sum over free dofs i of
// field f and k of field f' that both touch the node of P[i, node] K[i, k] P[k, node].  One thread per (point, level,
// component fa of the point) over the node-block view of the matrix: it keeps the row's sums against the point's eight
// nodes of the level (8 x 6 registers), reads a column point's eight (node, weight) pairs of the level once per block
// and matches them against its own eight.  (A thread per (dof, slot) over the scalar rows took longer than the
// iterations the blocks save; a thread per (point, slot) re-read the column's pairs for every slot: 18 ms at 1.97 M
// dofs.)  The diagonal of a block is the scalar Galerkin diagonal.
__global__ __launch_bounds__(SH_BLOCK) void k_pc_galerkin_blocks(int64_t n_pts, int width, int64_t n_unode, const int64_t* __restrict__ brow,
                                                                 const int32_t* __restrict__ bcols, const double* __restrict__ vals,
                                                                 const uint8_t* __restrict__ fixed, const int32_t* __restrict__ lvl_node,
                                                                 const double* __restrict__ lvl_w, double* __restrict__ blk, int first_slot) {
  // A workgroup = 256 consecutive points, one level, one component (blockIdx.y = 3 level + fa): neighbouring points
  // touch the same few dozen lattice nodes, so their sums are combined in an LDS hash table (key = node and field
  // group) and leave the workgroup as one global atomic per entry -- the global atomics were three quarters of this
  // kernel's time (7.4 ms with, 1.75 without them at 988 k dofs).
  constexpr int HS = 512;
  __shared__ int32_t h_key[HS];
  __shared__ double h_val[HS][6];
  for (int i = threadIdx.x; i < HS; i += SH_BLOCK) {
    h_key[i] = -1;
#pragma unroll
    for (int q = 0; q < 6; ++q) h_val[i][q] = 0.0;
  }
  __syncthreads();
  const int fa = (int)(blockIdx.y % 3);
  const int32_t* ln = lvl_node + (int64_t)(blockIdx.y / 3) * n_pts * 8;          // this level's [point][8] tables
  const double* lw = lvl_w + (int64_t)(blockIdx.y / 3) * n_pts * 8;
  const int64_t p = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  const bool active = p < n_pts && !(fixed != nullptr && fixed[3 * p + fa]);
  if (active) {
    int32_t nd[8];
    double wi[8], acc[8][6];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      nd[a] = ln[p * 8 + a];
      wi[a] = lw[p * 8 + a];
      if (wi[a] == 0.0) nd[a] = -1;
#pragma unroll
      for (int q = 0; q < 6; ++q) acc[a][q] = 0.0;
    }
    const int gi = p >= n_unode ? 1 : 0;
    const int64_t k0 = brow[p], k1 = brow[p + 1], len = 3 * (k1 - k0);
    const double* v = vals + 9 * k0 + fa * len;
    for (int64_t k = k0; k < k1; ++k) {
      const int32_t cj = bcols[k];
      const int32_t* ik = ln + (int64_t)(cj / 3) * 8;
      const double* wk = lw + (int64_t)(cj / 3) * 8;
      const int64_t o = 3 * (k - k0);
      double m0 = v[o], m1 = v[o + 1], m2 = v[o + 2];
      if (fixed != nullptr) {
        if (fixed[cj]) m0 = 0.0;
        if (fixed[cj + 1]) m1 = 0.0;
        if (fixed[cj + 2]) m2 = 0.0;
      }
      const bool gj = cj >= 3 * n_unode;
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int32_t nb = ik[b];
        const double wb = wk[b];
#pragma unroll
        for (int a = 0; a < 8; ++a) {
          const double ww = nb == nd[a] ? wb : 0.0;
          if (gj) { acc[a][3] += ww * m0; acc[a][4] += ww * m1; acc[a][5] += ww * m2; }
          else { acc[a][0] += ww * m0; acc[a][1] += ww * m1; acc[a][2] += ww * m2; }
        }
      }
    }
    // upper triangle only (the block is symmetric; k_pc_invert_blocks mirrors it)
    const int fi = 3 * gi + fa;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
      if (nd[a] < 0) continue;
      const int32_t key = 2 * nd[a] + gi;
      int h = (int)(((uint32_t)key * 2654435761u) >> 23) & (HS - 1);
      int slot = -1;
      for (int probe = 0; probe < 16; ++probe) {
        const int32_t seen = atomicCAS(&h_key[h], -1, key);
        if (seen == -1 || seen == key) { slot = h; break; }
        h = (h + 1) & (HS - 1);
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        if (q < fi || acc[a][q] == 0.0) continue;
        const double val = wi[a] * acc[a][q];
        if (slot >= 0) __hip_atomic_fetch_add(&h_val[slot][q], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else atomicAdd(&blk[36 * (int64_t)nd[a] + 6 * fi + q], val);          // table full around this key: straight to memory
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < HS; i += SH_BLOCK) {
    const int32_t key = h_key[i];
    if (key < 0) continue;
    const int fi = 3 * (key & 1) + fa;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double val = h_val[i][q];
      if (q >= fi && val != 0.0) atomicAdd(&blk[36 * (int64_t)(key >> 1) + 6 * fi + q], val);
    }
  }
}

// inverse of the 3 x 3 diagonal block of every point (imposed dofs: unit row and column), the smoother of the finest
// level in place of 1 / diag: it sees the coupling of a node's three displacement (rotation) components
__global__ void k_pt_block_inv(int64_t n_pts, const int64_t* __restrict__ brow, const int32_t* __restrict__ bcols,
                               const double* __restrict__ vals, const uint8_t* __restrict__ fixed, float* __restrict__ dinv3,
                               double* __restrict__ dinv) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  const int64_t k0 = brow[p], k1 = brow[p + 1], len = 3 * (k1 - k0);
  double a[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int64_t k = k0; k < k1; ++k)
    if (bcols[k] == 3 * p) {
      const double* v = vals + 9 * k0 + 3 * (k - k0);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) a[i][j] = v[i * len + j];
      break;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if ((fixed != nullptr && fixed[3 * p + i]) || !(a[i][i] > 0.0)) {
#pragma unroll
      for (int j = 0; j < 3; ++j) { a[i][j] = 0.0; a[j][i] = 0.0; }
      a[i][i] = 1.0;
    }
  // 1 / diag as well (what k_csr_diag_inv computes by scanning whole scalar rows: 5.8 GB fetched at 1.97 M dofs)
#pragma unroll
  for (int i = 0; i < 3; ++i) dinv[3 * p + i] = 1.0 / a[i][i];
  // symmetric 3 x 3 inverse by cofactors
  const double s01 = 0.5 * (a[0][1] + a[1][0]), s02 = 0.5 * (a[0][2] + a[2][0]), s12 = 0.5 * (a[1][2] + a[2][1]);
  const double c00 = a[1][1] * a[2][2] - s12 * s12, c01 = s02 * s12 - s01 * a[2][2], c02 = s01 * s12 - s02 * a[1][1];
  const double c11 = a[0][0] * a[2][2] - s02 * s02, c12 = s01 * s02 - a[0][0] * s12, c22 = a[0][0] * a[1][1] - s01 * s01;
  const double det = a[0][0] * c00 + s01 * c01 + s02 * c02;
  float* B = dinv3 + 9 * p;
  if (det > 0.0 && c00 > 0.0 && c22 > 0.0) {
    const double id = 1.0 / det;
    B[0] = (float)(c00 * id); B[1] = (float)(c01 * id); B[2] = (float)(c02 * id);
    B[3] = (float)(c01 * id); B[4] = (float)(c11 * id); B[5] = (float)(c12 * id);
    B[6] = (float)(c02 * id); B[7] = (float)(c12 * id); B[8] = (float)(c22 * id);
  } else {                                                 // not positive definite in floating point: plain Jacobi for this point
    B[0] = (float)(1.0 / a[0][0]); B[1] = 0.f; B[2] = 0.f; B[3] = 0.f; B[4] = (float)(1.0 / a[1][1]); B[5] = 0.f; B[6] = 0.f; B[7] = 0.f; B[8] = (float)(1.0 / a[2][2]);
  }
}

// in-place inverse of every node's 6 x 6 block (symmetric positive definite on the fields that have free dofs; a field
// without any gets a zero row and column): Gauss-Jordan without pivoting on the symmetrised block
__global__ void k_pc_invert_blocks(int64_t node0, int64_t node1, double* __restrict__ blk, double scale) {
  const int64_t node = node0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= node1) return;
  double* B = blk + 36 * node;
  double a[6][6], inv[6][6];
  bool dead[6];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) { a[r][c] = r <= c ? B[6 * r + c] : B[6 * c + r]; inv[r][c] = r == c ? 1.0 : 0.0; }    // upper triangle holds the sums
#pragma unroll
  for (int r = 0; r < 6; ++r) dead[r] = !(a[r][r] > 0.0);
#pragma unroll
  for (int r = 0; r < 6; ++r)
    if (dead[r]) {
#pragma unroll
      for (int c = 0; c < 6; ++c) { a[r][c] = 0.0; a[c][r] = 0.0; }
      a[r][r] = 1.0;
    }
#pragma unroll
  for (int r = 0; r < 6; ++r) a[r][r] *= 1.0 + 1e-12;
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const double d = 1.0 / a[p][p];
#pragma unroll
    for (int c = 0; c < 6; ++c) { a[p][c] *= d; inv[p][c] *= d; }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      if (r == p) continue;
      const double m = a[r][p];
#pragma unroll
      for (int c = 0; c < 6; ++c) { a[r][c] -= m * a[p][c]; inv[r][c] -= m * inv[p][c]; }
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) B[6 * r + c] = (dead[r] || dead[c]) ? 0.0 : scale * 0.5 * (inv[r][c] + inv[c][r]);
}

// all levels between the coarse-solve level and the finest lattice at once: g[node] = sum over the finest lattice's
// nodes of the composite child transfer (T_l^T ... T_{F-1}^T, built on the host), one wave per node, six fields per lane
__global__ __launch_bounds__(SH_BLOCK) void k_lat_down_composite(int64_t row0, int64_t n_rows, const int64_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ cols, const double* __restrict__ vals,
                                                                 double* __restrict__ g, const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (SH_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t k = rowptr[row] + lane; k < rowptr[row + 1]; k += 64) {
    const double w = vals[k];
    const double* src = g + 6 * (int64_t)cols[k];
#pragma unroll
    for (int f = 0; f < 6; ++f) s[f] += w * src[f];
  }
#pragma unroll
  for (int f = 0; f < 6; ++f) s[f] = femo_wave_sum(s[f]);
  if (lane == 0) {
    double* dst = g + 6 * (row0 + row);
#pragma unroll
    for (int f = 0; f < 6; ++f) dst[f] = s[f];
  }
}

// ---- Hermite-type lattice spaces (round 4; fea/shell.py::hermite_lattice, oracle/shell_oracle.py::LatticePreconditioner) --
// The nodal rotations of a lattice are the slopes of its displacement interpolation:
//   displacement point:  u = sum_n [ alpha_n U_n + Theta_n x sigma_n ]        (w4 = (alpha, sigma), 8 nodes)
//   rotation point:      theta = sum_n w_n Theta_n                            (w4 = (w, 0, 0, 0))
//   lattice to lattice:  U_c = a U_p + Theta_p x b,   Theta_c = c Theta_p     (w5 = (a, b, c) per (child, parent))
// and the transposes  g_U[n] += alpha r,  g_Theta[n] += sigma x r  /  g_U[p] += a g_U[c],  g_Theta[p] += c g_Theta[c] + b x g_U[c].
// A bending mode (w quadratic, theta = grad w) is then reproduced by lattices far coarser than the shell is thick, where
// the trilinear spaces of rounds 2-3 lock: 253 -> ~130 iterations on the 362 x 362 roof at the same cost per iteration.
struct V3 { double x, y, z; };
__device__ __forceinline__ V3 cross3(const V3& a, const V3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// g = P_L^T r on the finest lattice's nodes [m0, m1): per node a row of displacement points (first dof 3 p, w4) and a row
// of rotation points; SUB lanes per node
template <int SUB>
__global__ __launch_bounds__(SH_BLOCK) void k_pc_restrict_h(int64_t m0, int64_t m1, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                            const float4* __restrict__ w4, const double* __restrict__ r, double* __restrict__ g,
                                                            const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  const int sl = threadIdx.x & (SUB - 1);
  const int64_t nsub = (int64_t)gridDim.x * (SH_BLOCK / SUB);
  for (int64_t k = (int64_t)blockIdx.x * (SH_BLOCK / SUB) + (threadIdx.x / SUB); k < m1 - m0; k += nsub) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
    const int64_t e0 = rowptr[2 * k], e1 = rowptr[2 * k + 1], e2 = rowptr[2 * k + 2];
    // U entries per lane and trip, all their loads issued before the first is used (entries beyond the row are clamped to
    // its last one and weighted 0): a lane walks ~3 entries of a row and each is a chain weight/column -> gathered residual;
    // one at a time the kernel ran at 2.3 TB/s with every SIMD full (round 5)
    constexpr int U = 4;
    for (int64_t e = e0 + sl; e < e1; e += U * SUB) {
      float4 w[U];
      int32_t c[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t eu = e + u * SUB;
        const bool in = eu < e1;
        const int64_t ec = in ? eu : e1 - 1;
        w[u] = w4[ec];
        c[u] = cols[ec];
        if (!in) w[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      Triple rc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) rc[u] = *reinterpret_cast<const Triple*>(r + c[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s0 += (double)w[u].x * rc[u].a; s1 += (double)w[u].x * rc[u].b; s2 += (double)w[u].x * rc[u].c;
        // sigma x r
        t0 += (double)w[u].z * rc[u].c - (double)w[u].w * rc[u].b;
        t1 += (double)w[u].w * rc[u].a - (double)w[u].y * rc[u].c;
        t2 += (double)w[u].y * rc[u].b - (double)w[u].z * rc[u].a;
      }
    }
    for (int64_t e = e1 + sl; e < e2; e += U * SUB) {
      double w[U];
      int32_t c[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t eu = e + u * SUB;
        const bool in = eu < e2;
        const int64_t ec = in ? eu : e2 - 1;
        w[u] = in ? (double)w4[ec].x : 0.0;
        c[u] = cols[ec];
      }
      Triple rc[U];
#pragma unroll
      for (int u = 0; u < U; ++u) rc[u] = *reinterpret_cast<const Triple*>(r + c[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) { t0 += w[u] * rc[u].a; t1 += w[u] * rc[u].b; t2 += w[u] * rc[u].c; }
    }
#pragma unroll
    for (int off = SUB / 2; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64);
      t0 += __shfl_xor(t0, off, 64); t1 += __shfl_xor(t1, off, 64); t2 += __shfl_xor(t2, off, 64);
    }
    if (sl < 6) {
      const double v = sl == 0 ? s0 : (sl == 1 ? s1 : (sl == 2 ? s2 : (sl == 3 ? t0 : (sl == 4 ? t1 : t2))));
      g[6 * (m0 + k) + sl] = v;
    }
  }
}

// one lattice level, nodes [n0, n1), a thread per (node, field group):
//   down: g[p] from the node's children (chi rows), up: e[c] = B_c g_c + (transfer of the parents' e) with the node's
//   6 x 6 block B; w5 = (a, bx, by, bz, c) per entry.  dot_partials (up, finest level): per-block partial of e . g.
constexpr int LAT_H_LANES = 4;      // lanes per (node, field group) in k_lat_level_h
__global__ __launch_bounds__(256) void k_lat_level_h(int64_t n0, int64_t n1, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                     const double* __restrict__ w5, double* __restrict__ g, double* __restrict__ e, int up,
                                                     const int32_t* __restrict__ done, const double* __restrict__ blocks,
                                                     double* __restrict__ dot_partials) {
  if (done != nullptr && *done) return;
  __shared__ double lds[256 / 64];
  double dot = 0.0;
  // Round 5: four lanes share a (node, group) and split its <= 8 entries -- a lane used to walk them one after the other, each a
  // dependent index -> gather round trip, on levels too small (<= 52 k nodes) to hide it with other waves.
  const int sub = threadIdx.x & (LAT_H_LANES - 1);
  const int64_t total = (n1 - n0) * 2;
  const int64_t stride = (int64_t)gridDim.x * (blockDim.x / LAT_H_LANES);
  // (whole quads take the same trips: the shuffles below are executed by all four lanes)
  for (int64_t t = (int64_t)blockIdx.x * (blockDim.x / LAT_H_LANES) + (threadIdx.x / LAT_H_LANES); t < total; t += stride) {
    const int64_t node = n0 + (t >> 1);
    const int grp = (int)(t & 1);
    const double* src = up ? e : g;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t k = rowptr[node] + sub; k < rowptr[node + 1]; k += LAT_H_LANES) {
      const double* w = w5 + 5 * k;
      const double* sv = src + 6 * (int64_t)cols[k];
      if (up) {
        if (grp == 0) {                     // U_c = a U_p + Theta_p x b
          const V3 th = {sv[3], sv[4], sv[5]}, b = {w[1], w[2], w[3]};
          const V3 cb = cross3(th, b);
          s0 += w[0] * sv[0] + cb.x; s1 += w[0] * sv[1] + cb.y; s2 += w[0] * sv[2] + cb.z;
        } else {                            // Theta_c = c Theta_p
          s0 += w[4] * sv[3]; s1 += w[4] * sv[4]; s2 += w[4] * sv[5];
        }
      } else {
        if (grp == 0) {                     // g_U[p] += a g_U[c]
          s0 += w[0] * sv[0]; s1 += w[0] * sv[1]; s2 += w[0] * sv[2];
        } else {                            // g_Theta[p] += c g_Theta[c] + b x g_U[c]
          const V3 gu = {sv[0], sv[1], sv[2]}, b = {w[1], w[2], w[3]};
          const V3 cb = cross3(b, gu);
          s0 += w[4] * sv[3] + cb.x; s1 += w[4] * sv[4] + cb.y; s2 += w[4] * sv[5] + cb.z;
        }
      }
    }
#pragma unroll
    for (int off = LAT_H_LANES / 2; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64);
    }
    if (sub != 0) continue;
    double* out = (up ? e : g) + 6 * node + 3 * grp;
    if (!up) { out[0] = s0; out[1] = s1; out[2] = s2; continue; }
    const double* B = blocks + 36 * node + 18 * grp;
    const double* gn = g + 6 * node;
#pragma unroll
    for (int q = 0; q < 6; ++q) { s0 += B[q] * gn[q]; s1 += B[6 + q] * gn[q]; s2 += B[12 + q] * gn[q]; }
    out[0] = s0; out[1] = s1; out[2] = s2;
    dot += s0 * gn[3 * grp] + s1 * gn[3 * grp + 1] + s2 * gn[3 * grp + 2];
  }
  if (dot_partials != nullptr) {
    const double tsum = femo_block_sum<256>(dot, lds);
    if (threadIdx.x == 0) dot_partials[blockIdx.x] = tsum;
  }
}

// all levels between the coarse-solve level and the finest lattice at once (composite of the child transfers, built on
// the host in the same (A, B, C) form): one wave per node
__global__ __launch_bounds__(SH_BLOCK) void k_lat_down_composite_h(int64_t row0, int64_t n_rows, const int64_t* __restrict__ rowptr,
                                                                   const int32_t* __restrict__ cols, const double* __restrict__ w5,
                                                                   double* __restrict__ g, const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (SH_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t k = rowptr[row] + lane; k < rowptr[row + 1]; k += 64) {
    const double* w = w5 + 5 * k;
    const double* sv = g + 6 * (int64_t)cols[k];
    const V3 gu = {sv[0], sv[1], sv[2]}, b = {w[1], w[2], w[3]};
    const V3 cb = cross3(b, gu);
    s[0] += w[0] * gu.x; s[1] += w[0] * gu.y; s[2] += w[0] * gu.z;
    s[3] += w[4] * sv[3] + cb.x; s[4] += w[4] * sv[4] + cb.y; s[5] += w[4] * sv[5] + cb.z;
  }
#pragma unroll
  for (int f = 0; f < 6; ++f) s[f] = femo_wave_sum(s[f]);
  if (lane == 0) {
    double* dst = g + 6 * (row0 + row);
#pragma unroll
    for (int f = 0; f < 6; ++f) dst[f] = s[f];
  }
}

// (P_L e_L) of one point, 8 lanes per point (lane sl = corner): the three components, valid in all 8 lanes
__device__ __forceinline__ void prolong_point_h(int64_t p, int sl, int64_t n_unode, const int32_t* __restrict__ fin_idx, const float4* __restrict__ fin_w4,
                                                const double* __restrict__ t, double& s0, double& s1, double& s2) {
  const float4 w = fin_w4[p * 8 + sl];
  const int32_t idx = fin_idx[p * 8 + sl];
  if (p < n_unode) {
    // idx = 6 node: the node's six values as three 16-byte loads (48 node bytes from a 256-byte aligned base)
    const double2* tn = reinterpret_cast<const double2*>(t + idx);
    const double2 q0 = tn[0], q1 = tn[1], q2 = tn[2];
    const V3 th = {q1.y, q2.x, q2.y}, sg = {(double)w.y, (double)w.z, (double)w.w};
    const V3 cb = cross3(th, sg);
    s0 = (double)w.x * q0.x + cb.x; s1 = (double)w.x * q0.y + cb.y; s2 = (double)w.x * q1.x + cb.z;
  } else {
    const Triple tp = *reinterpret_cast<const Triple*>(t + idx);     // idx = 6 node + 3
    s0 = (double)w.x * tp.a; s1 = (double)w.x * tp.b; s2 = (double)w.x * tp.c;
  }
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off, 64);
    s1 += __shfl_xor(s1, off, 64);
    s2 += __shfl_xor(s2, off, 64);
  }
}

// z = D^-1 r + P_L e_L (8 lanes per point, one finest-level entry each, three components) and the per-block partial of
// r.z; imposed dofs: z = 0
__global__ __launch_bounds__(SH_BLOCK) void k_pc_prolong(int64_t n_pts, const int32_t* __restrict__ fin_idx, const float* __restrict__ fin_w,
                                                         const uint8_t* __restrict__ fixed, const double* __restrict__ dinv,
                                                         const double* __restrict__ r, const double* __restrict__ t, double* __restrict__ z,
                                                         double* __restrict__ partials, const int32_t* __restrict__ done,
                                                         const float* __restrict__ dinv3 = nullptr, const float4* __restrict__ fin_w4 = nullptr,
                                                         int64_t n_unode = 0) {
  if (done != nullptr && *done) return;
  __shared__ double lds[SH_BLOCK / 64];
  constexpr int SUB = 8;
  const int sl = threadIdx.x & (SUB - 1);
  const int64_t nsub = (int64_t)gridDim.x * (SH_BLOCK / SUB);
  double dot = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * (SH_BLOCK / SUB) + (threadIdx.x / SUB); p < n_pts; p += nsub) {
    double s0, s1, s2;
    if (fin_w4 != nullptr) {                                 // Hermite-type finest transfer
      prolong_point_h(p, sl, n_unode, fin_idx, fin_w4, t, s0, s1, s2);
    } else {
      const double w = (double)fin_w[p * 8 + sl];
      const Triple tp = *reinterpret_cast<const Triple*>(t + fin_idx[p * 8 + sl]);
      s0 = w * tp.a; s1 = w * tp.b; s2 = w * tp.c;
#pragma unroll
      for (int off = SUB / 2; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off, 64);
        s1 += __shfl_xor(s1, off, 64);
        s2 += __shfl_xor(s2, off, 64);
      }
    }
    if (sl < 3) {
      const int64_t row = 3 * p + sl;
      const bool rf = fixed != nullptr && fixed[row];
      const double ri = r[row];
      double sm;                                           // the smoother: point-block (3 x 3) or plain Jacobi
      if (dinv3 != nullptr) {
        const float* B = dinv3 + 9 * p + 3 * sl;
        const Triple rp = *reinterpret_cast<const Triple*>(r + 3 * p);
        sm = (double)B[0] * rp.a + (double)B[1] * rp.b + (double)B[2] * rp.c;
      } else {
        sm = dinv[row] * ri;
      }
      const double zi = rf ? 0.0 : sm + (sl == 0 ? s0 : (sl == 1 ? s1 : s2));
      z[row] = zi;
      dot += ri * zi;
    }
  }
  const double tsum = femo_block_sum<SH_BLOCK>(dot, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = tsum;
}

// The prolongation with the direction update fused in: gamma' = r . z is known before z is formed (partials of
// r . B r from k_scg_xr_pt, of (P^T r) . e from the finest k_lat_level), so beta and the stopping test are, and the pass
// writes p = z + beta p directly -- z = B r + P_L e_L is never stored, k_scg_p_z and its three vector streams are gone.
__global__ __launch_bounds__(SH_BLOCK) void k_pc_prolong_fused(int64_t n_pts, int it, int nb_rB, const double* __restrict__ part_rB, int nb_te,
                                                               const double* __restrict__ part_te, double* __restrict__ scal,
                                                               const int32_t* __restrict__ fin_idx, const float* __restrict__ fin_w,
                                                               const uint8_t* __restrict__ fixed, const double* __restrict__ dinv,
                                                               const float* __restrict__ dinv3, const double* __restrict__ r,
                                                               const double* __restrict__ t, double* __restrict__ p,
                                                               int32_t* __restrict__ flag, double* __restrict__ gamma_out,
                                                               const float4* __restrict__ fin_w4 = nullptr, int64_t n_unode = 0) {
  if (flag[0]) return;
  __shared__ double lds[SH_BLOCK / 64];
  const double g1 = femo_fold_partials<SH_BLOCK>(part_rB, nb_rB, lds) + femo_fold_partials<SH_BLOCK>(part_te, nb_te, lds);
  const double g0 = scal[0];
  const bool conv = g1 <= scal[2] || !(g1 == g1);
  const double beta = g0 != 0.0 ? g1 / g0 : 0.0;
  if (!conv) {
    constexpr int SUB = 8;
    const int sl = threadIdx.x & (SUB - 1);
    const int64_t nsub = (int64_t)gridDim.x * (SH_BLOCK / SUB);
    for (int64_t pt = (int64_t)blockIdx.x * (SH_BLOCK / SUB) + (threadIdx.x / SUB); pt < n_pts; pt += nsub) {
      double s0, s1, s2;
      if (fin_w4 != nullptr) {
        prolong_point_h(pt, sl, n_unode, fin_idx, fin_w4, t, s0, s1, s2);
      } else {
        const double w = (double)fin_w[pt * 8 + sl];
        const Triple tp = *reinterpret_cast<const Triple*>(t + fin_idx[pt * 8 + sl]);
        s0 = w * tp.a; s1 = w * tp.b; s2 = w * tp.c;
#pragma unroll
        for (int off = SUB / 2; off > 0; off >>= 1) {
          s0 += __shfl_xor(s0, off, 64);
          s1 += __shfl_xor(s1, off, 64);
          s2 += __shfl_xor(s2, off, 64);
        }
      }
      if (sl < 3) {
        const int64_t row = 3 * pt + sl;
        const bool rf = fixed != nullptr && fixed[row];
        double sm;
        if (dinv3 != nullptr) {
          const float* B = dinv3 + 9 * pt + 3 * sl;
          const Triple rp = *reinterpret_cast<const Triple*>(r + 3 * pt);
          sm = (double)B[0] * rp.a + (double)B[1] * rp.b + (double)B[2] * rp.c;
        } else {
          sm = dinv[row] * r[row];
        }
        const double zi = rf ? 0.0 : sm + (sl == 0 ? s0 : (sl == 1 ? s1 : s2));
        p[row] = zi + beta * p[row];
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gamma_out[0] = g1;
    flag[1] = it + 1;
    if (conv) { flag[2] = (g1 == g1) ? 0 : 1; __threadfence(); flag[0] = it + 1; }
  }
}

}  // namespace

// relative weight of the node-block levels in the additive sum (femo_shell_pc_weights; applied at set-up time: the inverse
// node blocks of the levels above the coarse solve are scaled once per stiffness)
static double shell_level_weight(const femo_shell* s, int) { return s->w_levels; }

extern "C" {

// Lattice preconditioner data (built on the host: fea/shell.py::ShellSpace.lattice_pc): P as ELL, `width` = 8 x levels
// entries per dof (column, weight; weight 0 pads), and P^T as CSR over the n_lat lattice unknowns.
int femo_shell_pc_create(femo_shell* s, int width, int64_t n_nodes, int n_levels, const int64_t* level_offsets,
                         const int32_t* ell_idx, const double* ell_w,
                         const int64_t* pt_rowptr, const int32_t* pt_cols, const double* pt_vals,
                         const int64_t* par_rowptr, const int32_t* par_cols, const double* par_vals,
                         const int64_t* chi_rowptr, const int32_t* chi_cols, const double* chi_vals) {
  FEMO_REQUIRE(s && level_offsets && ell_idx && ell_w && pt_rowptr && pt_cols && pt_vals && par_rowptr && par_cols && par_vals &&
               chi_rowptr && chi_cols && chi_vals, "null argument");
  FEMO_REQUIRE(n_levels > 0 && width == 8 * n_levels && n_nodes > 0 && level_offsets[n_levels] == n_nodes, "bad preconditioner shape");
  FEMO_REQUIRE(s->pc_width == 0, "the shell already has a preconditioner");
  hipStream_t st = s->ctx->stream;
  FEMO_HIP_CHECK(hipSetDevice(s->ctx->device));
  const int64_t n_lat = 6 * n_nodes;
  FEMO_TRY(to_device(&s->d_ell_idx, ell_idx, s->n_dof * width, st));
  FEMO_TRY(to_device(&s->d_ell_w, ell_w, s->n_dof * width, st));
  FEMO_TRY(to_device(&s->d_par_rowptr, par_rowptr, n_nodes + 1, st));
  FEMO_TRY(to_device(&s->d_par_cols, par_cols, par_rowptr[n_nodes], st));
  FEMO_TRY(to_device(&s->d_par_vals, par_vals, par_rowptr[n_nodes], st));
  FEMO_TRY(to_device(&s->d_chi_rowptr, chi_rowptr, n_nodes + 1, st));
  FEMO_TRY(to_device(&s->d_chi_cols, chi_cols, chi_rowptr[n_nodes], st));
  FEMO_TRY(to_device(&s->d_chi_vals, chi_vals, chi_rowptr[n_nodes], st));
  {
    // The finest level runs every iteration, in arrays of its own and per POINT (a P2 node with its three displacements,
    // a vertex with its three rotations: dofs 3 p .. 3 p + 2): the three components share the eight lattice nodes and
    // weights, so the prolongation reads 8 (index, weight) pairs per point instead of 24, and P_L^T has one row per
    // (lattice node, field group) listing points instead of six rows listing dofs.
    const int64_t n_pts = s->n_dof / 3;
    FEMO_REQUIRE(s->n_dof % 3 == 0, "dofs are not numbered 3 point + component");
    std::vector<int32_t> fi((size_t)n_pts * 8);
    std::vector<float> fw((size_t)n_pts * 8);
    for (int64_t p = 0; p < n_pts; ++p)
      for (int a = 0; a < 8; ++a) {
        const int64_t e0 = (3 * p) * width + (width - 8) + a;
        fi[(size_t)p * 8 + a] = ell_idx[e0];                      // unknown of component 0; components 1, 2 follow it
        fw[(size_t)p * 8 + a] = (float)ell_w[e0];
        for (int k = 1; k < 3; ++k) {
          const int64_t ek = (3 * p + k) * width + (width - 8) + a;
          FEMO_REQUIRE(ell_idx[ek] == ell_idx[e0] + k && ell_w[ek] == ell_w[e0], "components of a point do not share their lattice weights");
        }
      }
    FEMO_TRY(to_device(&s->d_fin_idx, fi.data(), n_pts * 8, st));
    FEMO_TRY(to_device(&s->d_fin_w, fw.data(), n_pts * 8, st));
    // rows 6 m + 0 (displacement group) and 6 m + 3 (rotation group) of P^T for the finest level's nodes m
    const int64_t m0 = level_offsets[n_levels - 1], m1 = level_offsets[n_levels];
    std::vector<int64_t> rp((size_t)(2 * (m1 - m0) + 1), 0);
    std::vector<int32_t> pc;
    std::vector<float> pv;
    for (int64_t m = m0; m < m1; ++m)
      for (int g = 0; g < 2; ++g) {
        const int64_t row = 6 * m + 3 * g;
        for (int64_t e = pt_rowptr[row]; e < pt_rowptr[row + 1]; ++e) {
          FEMO_REQUIRE(pt_cols[e] % 3 == 0, "P^T row of component 0 lists another component");
          pc.push_back(pt_cols[e]);
          pv.push_back((float)pt_vals[e]);
        }
        for (int k = 1; k < 3; ++k)
          FEMO_REQUIRE(pt_rowptr[row + k + 1] - pt_rowptr[row + k] == pt_rowptr[row + 1] - pt_rowptr[row], "P^T rows of a field group differ");
        rp[(size_t)(2 * (m - m0) + g + 1)] = (int64_t)pc.size();
      }
    FEMO_TRY(to_device(&s->d_ptp_rowptr, rp.data(), (int64_t)rp.size(), st));
    FEMO_TRY(to_device(&s->d_ptp_cols, pc.data(), (int64_t)pc.size(), st));
    FEMO_TRY(to_device(&s->d_ptp_vals, pv.data(), (int64_t)pv.size(), st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
  }
  FEMO_HIP_CHECK(hipMalloc(&s->d_coarse, n_lat * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_cblk, n_nodes * 36 * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_dinv3, (s->n_dof / 3) * 9 * sizeof(float)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_t, n_lat * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_e, n_lat * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_z, s->n_dof * sizeof(double)));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  s->level_off.assign(level_offsets, level_offsets + n_levels + 1);
  s->pc_width = width; s->pc_levels = n_levels; s->n_lat = n_lat; s->pc_nodes = n_nodes;
  return 0;
}

}  // extern "C"

// z = M^-1 r (lattice preconditioner) and the per-block partials of r.z; enqueues 2 L + 1 launches
// Pte != nullptr: the fused form -- the finest level's up kernel also emits the partials of e . g into Pte (*nb_te blocks)
// and the prolongation is left to the caller (shell_pc_prolong_fused).
// carry_x != nullptr: the first coarse product also does the solver's x += alpha p (shell_coarse_apply).
int shell_pc_apply(femo_shell* s, const uint8_t* d_fixed, double* Prz, unsigned gz, const int32_t* done, double* Pte, int* nb_te,
                   double* carry_x) {
  hipStream_t st = s->ctx->stream;
  const int L = s->pc_levels;
  const bool herm = s->hermite_on && s->cs_ready && s->blk_ready;
  auto level_up = [&](int l, const double* blocks) {
    const int64_t n0 = s->level_off[l], n1 = s->level_off[l + 1];
    const bool last = l == L - 1 && Pte != nullptr;
    if (herm) {
      const unsigned g = last ? std::min<unsigned>(sgrid((n1 - n0) * 2 * LAT_H_LANES, 256), 1024u) : sgrid((n1 - n0) * 2 * LAT_H_LANES, 256);
      if (last && nb_te) *nb_te = (int)g;
      hipLaunchKernelGGL(k_lat_level_h, dim3(g), dim3(256), 0, st, n0, n1, s->d_par_rowptr, s->d_par_cols, s->d_par_w5, s->d_t, s->d_e, 1, done, blocks,
                         last ? Pte : (double*)nullptr);
      return;
    }
    const unsigned g = last ? std::min<unsigned>(sgrid((n1 - n0) * 6, 256), 1024u) : sgrid((n1 - n0) * 6, 256);   // few partials: every block of the prolongation folds them
    if (last && nb_te) *nb_te = (int)g;
    hipLaunchKernelGGL(k_lat_level, dim3(g), dim3(256), 0, st, n0, n1, s->d_par_rowptr, s->d_par_cols, s->d_par_vals,
                       s->d_coarse, s->d_t, s->d_e, 1, done, blocks, last ? Pte : (double*)nullptr);
  };
  const int64_t m0 = s->level_off[L - 1], m1 = s->level_off[L];
  if (herm)
    hipLaunchKernelGGL(k_pc_restrict_h<32>, dim3(std::min<unsigned>(sgrid(m1 - m0, SH_BLOCK / 32), 1 << 16)), dim3(SH_BLOCK), 0, st, m0, m1,
                       s->d_hp_rowptr, s->d_hp_cols, s->d_hp_w4, s->d_r, s->d_t, done);
  else
  // 32 lanes per row (rows hold ~100 points; 8 / 16 / 32 / 64 lanes: 0.362 / 0.355 / 0.351 / 0.351 ms per iteration)
  hipLaunchKernelGGL(k_pc_restrict<32>, dim3(std::min<unsigned>(sgrid(2 * (m1 - m0), SH_BLOCK / 32), 1 << 16)), dim3(SH_BLOCK), 0, st, m0, m1,
                     s->d_ptp_rowptr, s->d_ptp_cols, s->d_ptp_vals, s->d_r, s->d_t, done);
  if (s->d_owned != nullptr && s->ctx->nranks > 1) {
    // partitioned: r is zero on the points owned elsewhere, so the sum over the ranks is P^T r; the lattice levels below
    // are replicated (same arithmetic on every rank)
    FEMO_HIP_CHECK(hipGetLastError());
    FEMO_TRY(shell_allreduce(s, s->d_t + 6 * m0, 6 * (m1 - m0), st));
  }
  if (s->cs_ready) {
    // levels above the coarse-solve level as before; on it the dense inverse replaces the diagonal levels 0 .. cs
    const int cs = s->cs_level;
    if (herm && s->d_hd_rowptr != nullptr && L - 1 > cs) {
      const int64_t rows = s->level_off[L - 1] - s->level_off[cs];
      hipLaunchKernelGGL(k_lat_down_composite_h, dim3(sgrid(rows, SH_BLOCK / 64)), dim3(SH_BLOCK), 0, st, s->level_off[cs], rows, s->d_hd_rowptr,
                         s->d_hd_cols, s->d_hd_w5, s->d_t, done);
    } else if (herm) {
      for (int l = L - 2; l >= cs; --l) {
        const int64_t n0 = s->level_off[l], n1 = s->level_off[l + 1];
        hipLaunchKernelGGL(k_lat_level_h, dim3(sgrid((n1 - n0) * 2 * LAT_H_LANES, 256)), dim3(256), 0, st, n0, n1, s->d_chi_rowptr, s->d_chi_cols, s->d_chi_w5, s->d_t, s->d_e, 0,
                           done, (const double*)nullptr, (double*)nullptr);
      }
    } else if (s->d_cd_rowptr != nullptr && L - 1 > cs) {
      const int64_t rows = s->level_off[L - 1] - s->level_off[cs];
      hipLaunchKernelGGL(k_lat_down_composite, dim3(sgrid(rows, SH_BLOCK / 64)), dim3(SH_BLOCK), 0, st, s->level_off[cs], rows, s->d_cd_rowptr,
                         s->d_cd_cols, s->d_cd_vals, s->d_t, done);
    } else {
      for (int l = L - 2; l >= cs; --l) {
        const int64_t n0 = s->level_off[l], n1 = s->level_off[l + 1];
        hipLaunchKernelGGL(k_lat_level, dim3(sgrid((n1 - n0) * 6, 256)), dim3(256), 0, st, n0, n1, s->d_chi_rowptr, s->d_chi_cols, s->d_chi_vals,
                           s->d_coarse, s->d_t, s->d_e, 0, done);
      }
    }
    shell_coarse_apply(s, done, carry_x, st);
    for (int l = cs + 1; l < L; ++l) level_up(l, s->blk_ready ? s->d_cblk : (const double*)nullptr);
  } else {
  // levels 0 .. kc (at most 256 nodes each, never the finest: with 4096 the one workgroup took 244 us, with 768 still 71) go through the fused single-workgroup kernel
    int kc = -1;
    while (kc + 1 < L - 1 && kc + 1 < 16 && s->level_off[kc + 2] - s->level_off[kc + 1] <= 256) ++kc;
    for (int l = L - 2; l > kc; --l) {
      const int64_t n0 = s->level_off[l], n1 = s->level_off[l + 1];
      hipLaunchKernelGGL(k_lat_level, dim3(sgrid((n1 - n0) * 6, 256)), dim3(256), 0, st, n0, n1, s->d_chi_rowptr, s->d_chi_cols, s->d_chi_vals,
                         s->d_coarse, s->d_t, s->d_e, 0, done);
    }
    if (kc >= 0) {
      LatLevels Lv;
      Lv.kc = kc;
      for (int l = 0; l <= kc + 1; ++l) Lv.off[l] = s->level_off[l];
      hipLaunchKernelGGL(k_lat_coarse_fused, dim3(1), dim3(1024), 0, st, Lv, s->d_chi_rowptr, s->d_chi_cols, s->d_chi_vals, s->d_par_rowptr,
                         s->d_par_cols, s->d_par_vals, s->d_coarse, s->d_t, s->d_e, done);
    }
    for (int l = kc + 1; l < L; ++l) level_up(l, (const double*)nullptr);
  }
  if (Pte != nullptr) { FEMO_HIP_CHECK(hipGetLastError()); return 0; }
  hipLaunchKernelGGL(k_pc_prolong, dim3(gz), dim3(SH_BLOCK), 0, st, s->n_dof / 3, s->d_fin_idx, s->d_fin_w, d_fixed, s->d_dinv, s->d_r, s->d_e,
                     s->d_z, Prz, done, s->dinv3_ready ? s->d_dinv3 : (const float*)nullptr, herm ? s->d_fin_w4 : (const float4*)nullptr, s->n_unode);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// the prolongation that closes a fused iteration of femo_shell_solve (after shell_pc_apply with Pte): p = z + beta p
void shell_pc_prolong_fused(femo_shell* s, const uint8_t* d_fixed, unsigned grid, int it, int nb_rB, const double* part_rB, int nb_te,
                            const double* part_te, double* gamma_out, hipStream_t st) {
  hipLaunchKernelGGL(k_pc_prolong_fused, dim3(grid), dim3(SH_BLOCK), 0, st, s->n_dof / 3, it, nb_rB, part_rB, nb_te, part_te, s->d_scal, s->d_fin_idx, s->d_fin_w,
                     d_fixed, s->d_dinv, s->dinv3_ready ? s->d_dinv3 : (const float*)nullptr, s->d_r, s->d_e, s->d_p, s->d_flag, gamma_out,
                     (s->hermite_on && s->cs_ready && s->blk_ready) ? s->d_fin_w4 : (const float4*)nullptr, s->n_unode);
}

// nodes and weights of the levels above the coarse-solve level `level`, per level and point (femo_shell_pc_coarse)
int shell_pc_compact_levels(femo_shell* s, int level, hipStream_t st) {
  const int first_slot = 8 * (level + 1);
  const int64_t n_pts = s->n_dof / 3, cnt = n_pts * ((s->pc_width - first_slot) / 8) * 8;
  if (cnt > 0) {
    FEMO_HIP_CHECK(hipMalloc(&s->d_lvl_node, cnt * sizeof(int32_t)));
    FEMO_HIP_CHECK(hipMalloc(&s->d_lvl_w, cnt * sizeof(double)));
    hipLaunchKernelGGL(k_compact_levels, dim3(sgrid(cnt, 256)), dim3(256), 0, st, n_pts, s->pc_width, first_slot, s->d_ell_idx, s->d_ell_w,
                       s->d_lvl_node, s->d_lvl_w);
    FEMO_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

extern "C" {

// Items of the node-block set-up kernel for the Hermite-type spaces (fea/shell.py::node_block_items): the points of every
// level above the coarse solve grouped by lattice cell, at most 64 per item; pcell[level][point] = packed cell coordinates.
int femo_shell_pc_block_items(femo_shell* s, int64_t n_items, const int64_t* item_ptr, const int32_t* item_lvl, const int32_t* item_pts,
                              const int32_t* pcell) {
  FEMO_REQUIRE(s && item_ptr && item_lvl && item_pts && pcell && n_items > 0, "null argument");
  FEMO_REQUIRE(s->hermite, "femo_shell_pc_block_items needs femo_shell_pc_hermite first");
  FEMO_REQUIRE(s->d_bi_ptr == nullptr, "the shell already has its node-block items");
  hipStream_t st = s->ctx->stream;
  FEMO_HIP_CHECK(hipSetDevice(s->ctx->device));
  const int64_t n_pts = s->n_dof / 3;
  const int n_above = s->pc_levels - 1 - s->cs_level;
  for (int64_t i = 0; i < n_items; ++i) {
    FEMO_REQUIRE(item_lvl[i] >= 0 && item_lvl[i] < n_above, "item level out of range");
    FEMO_REQUIRE(item_ptr[i + 1] > item_ptr[i] && item_ptr[i + 1] - item_ptr[i] <= 64, "an item holds 1 .. 64 points");
  }
  FEMO_REQUIRE(item_ptr[0] == 0 && item_ptr[n_items] == (int64_t)n_above * n_pts, "every point belongs to one item per level");
  FEMO_TRY(to_device(&s->d_bi_ptr, item_ptr, n_items + 1, st));
  FEMO_TRY(to_device(&s->d_bi_lvl, item_lvl, n_items, st));
  FEMO_TRY(to_device(&s->d_bi_pts, item_pts, item_ptr[n_items], st));
  FEMO_TRY(to_device(&s->d_bi_pcell, pcell, (int64_t)n_above * n_pts, st));
  FEMO_HIP_CHECK(hipMalloc(&s->d_fixbits, n_pts));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  s->bi_items = n_items;
  s->pc_vals_uid = 0; s->pc_vals_gen = 0;
  return 0;
}

int femo_shell_pc_weights(femo_shell* s, double w_levels, double w_coarse) {
  FEMO_REQUIRE(s != nullptr, "null argument");
  FEMO_REQUIRE(w_levels > 0.0 && w_coarse > 0.0, "the weights of the preconditioner's parts must be positive (M^-1 stays positive definite)");
  s->w_levels = w_levels; s->w_coarse = w_coarse;
  s->pc_vals_uid = 0; s->pc_vals_gen = 0;                 // next solve recomputes the preconditioner's numbers
  return 0;
}

// Hermite-type lattice spaces on the hierarchy of femo_shell_pc_create / femo_shell_pc_coarse (fea/shell.py::hermite_lattice).
int femo_shell_pc_hermite(femo_shell* s, const float* fin_w4, const int64_t* hp_rowptr, const int32_t* hp_cols, const float* hp_w4,
                          const double* par_w5, const double* chi_w5, const float* lvl_w4, const float* cs_w4,
                          const int64_t* down_rowptr, const int32_t* down_cols, const double* down_w5) {
  FEMO_REQUIRE(s && fin_w4 && hp_rowptr && hp_cols && hp_w4 && par_w5 && chi_w5 && lvl_w4 && cs_w4, "null argument");
  FEMO_REQUIRE(s->pc_width > 0 && s->cs_level >= 0, "femo_shell_pc_hermite needs femo_shell_pc_create and femo_shell_pc_coarse first");
  FEMO_REQUIRE(!s->hermite_loaded, "the shell already has its Hermite-type lattice data");
  hipStream_t st = s->ctx->stream;
  FEMO_HIP_CHECK(hipSetDevice(s->ctx->device));
  const int64_t n_pts = s->n_dof / 3;
  const int L = s->pc_levels;
  const int64_t m0 = s->level_off[L - 1], m1 = s->level_off[L];
  std::vector<int64_t> h_par((size_t)s->pc_nodes + 1), h_chi((size_t)s->pc_nodes + 1);
  FEMO_HIP_CHECK(hipMemcpy(h_par.data(), s->d_par_rowptr, (s->pc_nodes + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  FEMO_HIP_CHECK(hipMemcpy(h_chi.data(), s->d_chi_rowptr, (s->pc_nodes + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  FEMO_TRY(to_device(&s->d_fin_w4, reinterpret_cast<const float4*>(fin_w4), n_pts * 8, st));
  FEMO_TRY(to_device(&s->d_hp_rowptr, hp_rowptr, 2 * (m1 - m0) + 1, st));
  FEMO_TRY(to_device(&s->d_hp_cols, hp_cols, hp_rowptr[2 * (m1 - m0)], st));
  FEMO_TRY(to_device(&s->d_hp_w4, reinterpret_cast<const float4*>(hp_w4), hp_rowptr[2 * (m1 - m0)], st));
  FEMO_TRY(to_device(&s->d_par_w5, par_w5, 5 * h_par[(size_t)s->pc_nodes], st));
  FEMO_TRY(to_device(&s->d_chi_w5, chi_w5, 5 * h_chi[(size_t)s->pc_nodes], st));
  const int n_above = L - 1 - s->cs_level;                      // levels cs + 1 .. L - 1
  FEMO_TRY(to_device(&s->d_lvl_w4, reinterpret_cast<const float4*>(lvl_w4), (int64_t)n_above * n_pts * 8, st));
  FEMO_TRY(to_device(&s->d_cs_w4, reinterpret_cast<const float4*>(cs_w4), n_pts * 8, st));
  if (down_rowptr != nullptr && down_cols != nullptr && down_w5 != nullptr) {
    const int64_t rows = s->level_off[L - 1] - s->level_off[s->cs_level];
    FEMO_TRY(to_device(&s->d_hd_rowptr, down_rowptr, rows + 1, st));
    FEMO_TRY(to_device(&s->d_hd_cols, down_cols, down_rowptr[rows], st));
    FEMO_TRY(to_device(&s->d_hd_w5, down_w5, 5 * down_rowptr[rows], st));
  }
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  FEMO_TRY(shell_coarse_hermite_lds());
  s->hermite = true;
  s->hermite_loaded = true;
  s->pc_vals_uid = 0; s->pc_vals_gen = 0;
  return 0;
}

// State of the lattice preconditioner as the DEVICE side has it: out = {Hermite-type data uploaded, bit 0: Hermite-type spaces
// enabled (uploaded and not fallen back) | bit 1: in use for the stiffness last set up, coarse solve factorised, node blocks ready}.  After a failed factorisation of the Hermite-type
// coarse operator the library falls back to the trilinear hierarchy for good; callers that report or pin iteration counts
// read the state here instead of remembering what they asked for.
int femo_shell_pc_info(const femo_shell* s, int32_t out[4]) {
  FEMO_REQUIRE(s && out, "null argument");
  out[0] = s->hermite_loaded ? 1 : 0;
  out[1] = (s->hermite ? 1 : 0) | ((s->hermite && s->hermite_on && s->cs_ready && s->blk_ready) ? 2 : 0);
  out[2] = s->cs_ready ? 1 : 0;
  out[3] = s->blk_ready ? 1 : 0;
  return 0;
}

}  // extern "C"

// The preconditioner's numbers for the current stiffness and Dirichlet set (kept while both stay the same): dense coarse
// operator and its factors, node blocks (or Galerkin diagonals), point blocks.
// point_blocks: FEMO_SHELL_NO_POINT_BLOCKS is not set (read once per call by the caller, whose own launches depend on it).
int shell_pc_setup(femo_shell* s, const femo_vec* vals, uint64_t mh, const uint8_t* d_fixed, bool point_blocks) {
  hipStream_t st = s->ctx->stream;
  const int64_t n = s->n_dof;
  // Galerkin diagonals of the current stiffness and Dirichlet set (kept while both stay the same; mh: shell_mask_hash)
  if (s->pc_vals_uid != vals->uid || s->pc_vals_gen != vals->gen || s->pc_mask_hash != mh || vals->uid == 0) {
    const bool node_blocks = !femo_env_flag("FEMO_SHELL_NO_BLOCKS");
    FEMO_TRY(shell_pc_coarse_setup(s, vals, d_fixed, node_blocks));
    // levels the coarse solve does not replace: 6 x 6 node blocks (they see the coupling of the displacement
    // components and rotations at a node: 238 -> 203 iterations on the 128 x 128 roof, 412 -> 376 on 362 x 362), or
    // the Galerkin diagonals when there is no coarse solve
    const int first_slot = s->cs_ready ? 8 * (s->cs_level + 1) : 0;
    s->blk_ready = false;
    if (s->cs_ready && s->d_lvl_node != nullptr && node_blocks) {
      const int64_t nd0 = s->level_off[s->cs_level + 1], nd1 = s->level_off[s->pc_levels];
      FEMO_HIP_CHECK(hipMemsetAsync(s->d_cblk + 36 * nd0, 0, (nd1 - nd0) * 36 * sizeof(double), st));
      bool by_items = s->hermite_on && s->bi_items > 0 && !femo_env_flag("FEMO_SHELL_BLOCKS_BY_ROWS");
      if (by_items) {
        hipLaunchKernelGGL(k_point_fixbits, dim3(sgrid(n / 3, 256)), dim3(256), 0, st, n / 3, d_fixed, s->d_fixbits);
        hipLaunchKernelGGL(k_pc_galerkin_blocks_w, dim3((unsigned)((s->bi_items + 3) / 4)), dim3(256), 0, st, s->bi_items, n / 3, s->n_unode, s->d_bi_ptr,
                           s->d_bi_lvl, s->d_bi_pts, s->d_bi_pcell, s->d_brow, s->d_bcols, vals->d, (const uint8_t*)s->d_fixbits, s->d_lvl_node,
                           s->d_lvl_w4, s->d_cblk, s->d_cs_info);
        int32_t binfo[4] = {0, 0, 0, 0};
        FEMO_HIP_CHECK(hipMemcpyAsync(binfo, s->d_cs_info, sizeof binfo, hipMemcpyDeviceToHost, st));
        FEMO_HIP_CHECK(hipStreamSynchronize(st));
        if (binfo[1] & 2) {                                 // an element spans more than a cell of some level: the row-wise kernel has no such limit
          by_items = false;
          s->bi_items = 0;
          FEMO_HIP_CHECK(hipMemsetAsync(s->d_cblk + 36 * nd0, 0, (nd1 - nd0) * 36 * sizeof(double), st));
        }
      }
      if (by_items) {
      } else if (s->hermite_on)
        hipLaunchKernelGGL(k_pc_galerkin_blocks_h, dim3(sgrid(n / 3), 3 * ((s->pc_width - first_slot) / 8)), dim3(SH_BLOCK), 0, st, n / 3, s->n_unode,
                           s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_lvl_node, s->d_lvl_w4, s->d_cblk);
      else
        hipLaunchKernelGGL(k_pc_galerkin_blocks, dim3(sgrid(n / 3), 3 * ((s->pc_width - first_slot) / 8)), dim3(SH_BLOCK), 0, st, n / 3, s->pc_width,
                           s->n_unode, s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_lvl_node, s->d_lvl_w, s->d_cblk, first_slot);
      FEMO_HIP_CHECK(hipGetLastError());
      FEMO_TRY(shell_allreduce(s, s->d_cblk + 36 * nd0, (nd1 - nd0) * 36, st));
      for (int l = s->cs_level + 1; l < s->pc_levels; ++l) {
        const int64_t a0 = s->level_off[l], a1 = s->level_off[l + 1];
        if (a1 > a0) hipLaunchKernelGGL(k_pc_invert_blocks, dim3(sgrid(a1 - a0, 256)), dim3(256), 0, st, a0, a1, s->d_cblk, shell_level_weight(s, l));
      }
      s->blk_ready = true;
    } else {
      FEMO_HIP_CHECK(hipMemsetAsync(s->d_coarse, 0, s->n_lat * sizeof(double), st));
      hipLaunchKernelGGL(k_pc_galerkin_diag, dim3(sgrid(n * (s->pc_width - first_slot))), dim3(SH_BLOCK), 0, st, n, s->pc_width, s->d_rowptr, s->d_cols,
                         vals->d, d_fixed, s->d_ell_idx, s->d_ell_w, s->d_coarse, first_slot);
      FEMO_HIP_CHECK(hipGetLastError());
      FEMO_TRY(shell_allreduce(s, s->d_coarse, s->n_lat, st));
      hipLaunchKernelGGL(k_pc_invert, dim3(sgrid(s->n_lat)), dim3(256), 0, st, s->n_lat, s->d_coarse);
    }
    s->dinv3_ready = false;
    if (s->d_brow != nullptr && point_blocks) {
      hipLaunchKernelGGL(k_pt_block_inv, dim3(sgrid(n / 3, 256)), dim3(256), 0, st, n / 3, s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_dinv3, s->d_dinv);
      s->dinv3_ready = true;
    }
    s->pc_vals_uid = vals->uid; s->pc_vals_gen = vals->gen; s->pc_mask_hash = mh;
  }
  return 0;
}

extern "C" {

// z = M^-1 r of the lattice preconditioner for `vals` and the mask (tests compare it with oracle/shell_oracle.py::
// LatticePreconditioner.apply); entries of r on imposed dofs are ignored, z is zero there.
int femo_shell_pc_apply(femo_shell* s, const femo_vec* vals, const uint8_t* fixed_host, const femo_vec* r, femo_vec* z) {
  FEMO_REQUIRE(s && vals && r && z, "null argument");
  const int64_t n = s->n_dof;
  FEMO_REQUIRE(s->pc_width > 0, "femo_shell_pc_apply needs femo_shell_pc_create");
  FEMO_REQUIRE(vals->n >= s->nnz && r->n >= n && z->n >= n && n % 3 == 0, "vector size mismatch in shell_pc_apply");
  FEMO_REQUIRE(s->d_owned == nullptr, "femo_shell_pc_apply: one rank only");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(z);
  const uint8_t* d_fixed = nullptr;
  uint64_t mask_hash = 0;
  FEMO_TRY(shell_mask(s, fixed_host, &d_fixed, &mask_hash));
  shell_rhs_free(s, r->d, d_fixed, st);
  FEMO_TRY(shell_pc_setup(s, vals, mask_hash, d_fixed, !femo_env_flag("FEMO_SHELL_NO_POINT_BLOCKS")));
  const unsigned gz = std::min<unsigned>(sgrid(n / 3, SH_BLOCK / 8), SH_MAXPART);
  FEMO_TRY(shell_pc_apply(s, d_fixed, s->d_part + SH_MAXPART, gz, nullptr));
  FEMO_HIP_CHECK(hipMemcpyAsync(z->d, s->d_z, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"

void shell_pc_free(femo_shell* s) {
  hipFree(s->d_ell_idx); hipFree(s->d_ell_w);
  hipFree(s->d_par_rowptr); hipFree(s->d_par_cols); hipFree(s->d_par_vals); hipFree(s->d_chi_rowptr); hipFree(s->d_chi_cols); hipFree(s->d_chi_vals);
  hipFree(s->d_fin_idx); hipFree(s->d_fin_w); hipFree(s->d_ptp_rowptr); hipFree(s->d_ptp_cols); hipFree(s->d_ptp_vals);
  hipFree(s->d_coarse); hipFree(s->d_cblk); hipFree(s->d_dinv3); hipFree(s->d_t); hipFree(s->d_e); hipFree(s->d_z);
  hipFree(s->d_lvl_node); hipFree(s->d_lvl_w);                                                                    // shell_pc_compact_levels
  hipFree(s->d_bi_ptr); hipFree(s->d_bi_lvl); hipFree(s->d_bi_pts); hipFree(s->d_bi_pcell); hipFree(s->d_fixbits);   // femo_shell_pc_block_items
  hipFree(s->d_fin_w4); hipFree(s->d_hp_rowptr); hipFree(s->d_hp_cols); hipFree(s->d_hp_w4); hipFree(s->d_par_w5); hipFree(s->d_chi_w5);   // femo_shell_pc_hermite
  hipFree(s->d_lvl_w4); hipFree(s->d_cs_w4); hipFree(s->d_hd_rowptr); hipFree(s->d_hd_cols); hipFree(s->d_hd_w5);
}
