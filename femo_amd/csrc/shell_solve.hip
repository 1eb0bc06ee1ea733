// Reissner-Mindlin shell: the handle's life, the operator products (CSR, 3 x 3-block CSR, block-SELL), the CG kernels
// and the solve loop, the Dirichlet mask, and the partition over ranks with its halo (shell_internal.h has the overview).
#include "shell_internal.h"

namespace {

// ---------------------------------------------------------------- CSR operator ----
// y = A x for rows [0, n), 16 lanes per row (the element-coupling pattern has ~50 entries per row: a whole wave per
// row left three quarters of the lanes idle and a quarter of the rows in flight).  `fixed` != nullptr: the masked
// operator M A M + (I - M) (strongly imposed dofs are identity rows and columns); mask_cols = 0 skips the column test
// for callers whose x is zero on the imposed dofs anyway (the CG directions) -- a byte gather per matrix entry.
// partials != nullptr: per-block partial of x.y.
__global__ __launch_bounds__(SH_BLOCK) void k_csr_spmv(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                       const double* __restrict__ vals, const uint8_t* __restrict__ fixed, int mask_cols,
                                                       const double* __restrict__ x, double* __restrict__ y, double* __restrict__ partials,
                                                       const int32_t* __restrict__ done, double* commit_dst = nullptr,
                                                       const double* commit_src = nullptr) {
  if (done != nullptr && *done) return;
  // the CG loop publishes gamma of the iteration here (every consumer of it runs after this launch, every block of
  // the kernel that produced it has finished): saves a launch of its own
  if (commit_dst != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *commit_dst = *commit_src;
  __shared__ double lds[SH_BLOCK / 64];
  constexpr int SUB = 16;
  const int sl = threadIdx.x & (SUB - 1);
  const int64_t nsub = (int64_t)gridDim.x * (SH_BLOCK / SUB);
  double dot = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * (SH_BLOCK / SUB) + (threadIdx.x / SUB); row < n; row += nsub) {
    double s = 0.0;
    const bool rf = fixed != nullptr && fixed[row];
    if (!rf) {
      const int64_t e1 = rowptr[row + 1];
      for (int64_t e = rowptr[row] + sl; e < e1; e += SUB) {
        const int32_t cidx = cols[e];
        const double v = vals[e] * x[cidx];
        s += (mask_cols && fixed != nullptr && fixed[cidx]) ? 0.0 : v;
      }
    }
#pragma unroll
    for (int off = SUB / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (sl == 0) {
      const double xr = x[row];
      const double yi = rf ? xr : s;
      y[row] = yi;
      dot += xr * yi;
    }
  }
  if (partials != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(dot, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

// The same product over the node-block view of the pattern: the three dofs of a node have the same columns and the
// columns come in runs of three, so one column index serves nine entries (8.4 instead of 12 bytes per entry) and the
// three x values of a block are loaded once for its three rows.  The value array is the scalar CSR one, untouched:
// row 3 b + i of block row b is the run vals[9 k0 + 3 i nb ..), block k at offset 3 (k - k0).  16 lanes per block row
// (13 blocks for an edge node, ~26 for a vertex node or a rotation).  Imposed dofs: identity rows; x must be zero on
// the imposed columns (the CG directions are).
template <int SUB>
__global__ __launch_bounds__(SH_BLOCK) void k_bcsr3_spmv(int64_t nb, const int64_t* __restrict__ brow, const int32_t* __restrict__ bcols,
                                                         const double* __restrict__ vals, const uint8_t* __restrict__ fixed,
                                                         const double* __restrict__ x, double* __restrict__ y, double* __restrict__ partials,
                                                         const int32_t* __restrict__ done, double* commit_dst = nullptr,
                                                         const double* commit_src = nullptr) {
  if (done != nullptr && *done) return;
  if (commit_dst != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *commit_dst = *commit_src;
  __shared__ double lds[SH_BLOCK / 64];
  const int sl = threadIdx.x & (SUB - 1);
  const int64_t nsub = (int64_t)gridDim.x * (SH_BLOCK / SUB);
  double dot = 0.0;
  // Software pipeline over the group's block rows: the offsets of row b + 2 nsub and the first column index of row
  // b + nsub are requested before row b is computed, so a row costs one memory latency (values and x together) instead
  // of three in a chain (offsets -> column -> x).
  int64_t b = (int64_t)blockIdx.x * (SH_BLOCK / SUB) + (threadIdx.x / SUB);
  int64_t k0 = 0, k1 = 0, n0 = 0, n1 = 0;
  int32_t c = 0;
  if (b < nb) {
    k0 = brow[b]; k1 = brow[b + 1];
    if (k0 + sl < k1) c = bcols[k0 + sl];
  }
  if (b + nsub < nb) { n0 = brow[b + nsub]; n1 = brow[b + nsub + 1]; }
  for (; b < nb; b += nsub) {
    int64_t m0 = 0, m1 = 0;
    int32_t cn = 0;
    if (b + 2 * nsub < nb) { m0 = brow[b + 2 * nsub]; m1 = brow[b + 2 * nsub + 1]; }
    if (n0 + sl < n1) cn = bcols[n0 + sl];
    const int64_t len = 3 * (k1 - k0);
    const double* v0 = vals + 9 * k0;
    const double* v1 = v0 + len;
    const double* v2 = v1 + len;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t k = k0 + sl; k < k1; k += SUB) {
      if (k >= k0 + SUB) c = bcols[k];
      const int64_t o = 3 * (k - k0);
      // plain loads: a lane reads 8 bytes at a stride of 24, so a cache line serves three instructions -- with
      // nontemporal loads the product took 135 us instead of 103 (988 k dofs).  Also slower: streaming the rows in
      // storage order (lane = entry: 109-121 us), 8 or 4 lanes per block row
      const Triple r0 = *reinterpret_cast<const Triple*>(v0 + o), r1 = *reinterpret_cast<const Triple*>(v1 + o),
                   r2 = *reinterpret_cast<const Triple*>(v2 + o), xc = *reinterpret_cast<const Triple*>(x + c);
      const double a00 = r0.a, a01 = r0.b, a02 = r0.c, a10 = r1.a, a11 = r1.b, a12 = r1.c, a20 = r2.a, a21 = r2.b, a22 = r2.c;
      const double x0 = xc.a, x1 = xc.b, x2 = xc.c;
      s0 += a00 * x0 + a01 * x1 + a02 * x2;
      s1 += a10 * x0 + a11 * x1 + a12 * x2;
      s2 += a20 * x0 + a21 * x1 + a22 * x2;
    }
#pragma unroll
    for (int off = SUB / 2; off > 0; off >>= 1) {
      s0 += __shfl_xor(s0, off, 64);
      s1 += __shfl_xor(s1, off, 64);
      s2 += __shfl_xor(s2, off, 64);
    }
    if (sl < 3) {
      const int64_t row = 3 * b + sl;
      const double s = sl == 0 ? s0 : (sl == 1 ? s1 : s2);
      const bool rf = fixed != nullptr && fixed[row];
      const double xr = x[row];
      const double yi = rf ? xr : s;
      y[row] = yi;
      dot += xr * yi;
    }
    k0 = n0; k1 = n1; c = cn;
    n0 = m0; n1 = m1;
  }
  if (partials != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(dot, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

// ---- block-SELL ----
constexpr int BSW = 32;                                  // block rows per slice (16 / 32 / 64: 0.355 / 0.347 / 0.355 ms per iteration at 1.97 M dofs)
// copy of the CSR values into the slice layout: group g = bs_off[slice] + slot holds block `slot` of the slice's BSW
// block rows: cols[BSW g + lane], vals[(9 g + comp) BSW + lane]; rows with fewer blocks are padded (column = own, 0)
__global__ __launch_bounds__(256) void k_bsell_fill(int64_t nb, const int64_t* __restrict__ brow, const int32_t* __restrict__ bcols,
                                                    const double* __restrict__ vals, const int64_t* __restrict__ bs_off,
                                                    int32_t* __restrict__ cols, double* __restrict__ out) {
  const int64_t slice = blockIdx.x;
  const int lane = threadIdx.x & (BSW - 1), sub = threadIdx.x / BSW;   // 256 / BSW slots in flight per pass
  const int64_t b = slice * BSW + lane;
  const int64_t g0 = bs_off[slice], nslot = bs_off[slice + 1] - g0;
  int64_t k0 = 0, k1 = 0;
  if (b < nb) { k0 = brow[b]; k1 = brow[b + 1]; }
  const int64_t len = 3 * (k1 - k0);
  for (int64_t sl = sub; sl < nslot; sl += 256 / BSW) {
    const int64_t g = g0 + sl;
    const bool have = k0 + sl < k1;
    cols[BSW * g + lane] = have ? bcols[k0 + sl] : (int32_t)(b < nb ? 3 * b : 0);
    const double* v = vals + 9 * k0 + 3 * sl;
#pragma unroll
    for (int fa = 0; fa < 3; ++fa)
#pragma unroll
      for (int fb = 0; fb < 3; ++fb) out[(9 * g + 3 * fa + fb) * BSW + lane] = have ? v[fa * len + fb] : 0.0;
  }
}

// y = A x from the block-SELL copy: lane = block row, no cross-lane reduction; every value load of a 16-lane group is
// one contiguous 128-byte piece.  Imposed dofs: identity rows; x must be zero on the imposed columns.
__global__ __launch_bounds__(SH_BLOCK) void k_bsell_spmv(int64_t nb, int64_t n_slice, const int64_t* __restrict__ bs_off,
                                                         const int32_t* __restrict__ cols, const double* __restrict__ vals,
                                                         const uint8_t* __restrict__ fixed, const double* __restrict__ x,
                                                         double* __restrict__ y, double* __restrict__ partials, const int32_t* __restrict__ done,
                                                         double* commit_dst = nullptr, const double* commit_src = nullptr) {
  if (done != nullptr && *done) return;
  if (commit_dst != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *commit_dst = *commit_src;
  __shared__ double lds[SH_BLOCK / 64];
  const int lane = threadIdx.x & (BSW - 1);
  const int64_t nsub = (int64_t)gridDim.x * (SH_BLOCK / BSW);
  double dot = 0.0;
  for (int64_t slice = (int64_t)blockIdx.x * (SH_BLOCK / BSW) + (threadIdx.x / BSW); slice < n_slice; slice += nsub) {
    const int64_t g0 = bs_off[slice], g1 = bs_off[slice + 1];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t g = g0; g < g1; ++g) {
      const double* v = vals + (9 * g) * BSW + lane;
      // nontemporal: every line is used by exactly one instruction here (plain loads: 0.401 against 0.390 ms per iteration)
      const int32_t c = __builtin_nontemporal_load(cols + BSW * g + lane);
      const double a00 = __builtin_nontemporal_load(v), a01 = __builtin_nontemporal_load(v + 1 * BSW), a02 = __builtin_nontemporal_load(v + 2 * BSW);
      const double a10 = __builtin_nontemporal_load(v + 3 * BSW), a11 = __builtin_nontemporal_load(v + 4 * BSW), a12 = __builtin_nontemporal_load(v + 5 * BSW);
      const double a20 = __builtin_nontemporal_load(v + 6 * BSW), a21 = __builtin_nontemporal_load(v + 7 * BSW), a22 = __builtin_nontemporal_load(v + 8 * BSW);
      const Triple xc = *reinterpret_cast<const Triple*>(x + c);
      s0 += a00 * xc.a + a01 * xc.b + a02 * xc.c;
      s1 += a10 * xc.a + a11 * xc.b + a12 * xc.c;
      s2 += a20 * xc.a + a21 * xc.b + a22 * xc.c;
    }
    const int64_t b = slice * BSW + lane;
    if (b < nb) {
      const Triple xr = *reinterpret_cast<const Triple*>(x + 3 * b);
      const bool f0 = fixed != nullptr && fixed[3 * b], f1 = fixed != nullptr && fixed[3 * b + 1], f2 = fixed != nullptr && fixed[3 * b + 2];
      const double y0 = f0 ? xr.a : s0, y1 = f1 ? xr.b : s1, y2 = f2 ? xr.c : s2;
      y[3 * b] = y0; y[3 * b + 1] = y1; y[3 * b + 2] = y2;
      dot += xr.a * y0 + xr.b * y1 + xr.c * y2;
    }
  }
  if (partials != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(dot, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

__global__ void k_csr_diag_inv(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                               const double* __restrict__ vals, const uint8_t* __restrict__ fixed, double* __restrict__ dinv) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
    double d = 1.0;
    if (fixed == nullptr || !fixed[row]) {
      d = 0.0;
      for (int64_t e = rowptr[row]; e < rowptr[row + 1]; ++e)
        if (cols[e] == row) d += vals[e];
    }
    dinv[row] = d != 0.0 ? 1.0 / d : 1.0;
  }
}

// scal: [0] gamma = r.z, [1] gamma0 (tolerance reference), [2] tol^2 factor
// r = b - A x0 is prepared by the host code; z = dinv r; p = z; partial r.z
__global__ __launch_bounds__(SH_BLOCK) void k_scg_init(int64_t n, const double* __restrict__ r, const double* __restrict__ dinv,
                                                       double* __restrict__ p, double* __restrict__ partials) {
  __shared__ double lds[SH_BLOCK / 64];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SH_BLOCK) {
    const double z = dinv[i] * r[i];
    p[i] = z;
    s += r[i] * z;
  }
  const double t = femo_block_sum<SH_BLOCK>(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ __launch_bounds__(SH_BLOCK) void k_scg_gamma0(int nb, const double* __restrict__ partials, double rtol2, double atol2, double* __restrict__ scal,
                                                         int32_t* __restrict__ flag) {
  __shared__ double lds[SH_BLOCK / 64];
  const double g = femo_fold_partials<SH_BLOCK>(partials, nb, lds);
  if (threadIdx.x == 0) {
    scal[0] = g; scal[1] = g;
    scal[4] = g;                           // gamma as published by the first SpMV of the loop
    scal[2] = fmax(rtol2 * g, atol2);
    flag[0] = g <= scal[2] ? 1 : 0;
    flag[1] = 0;
  }
}

// x += alpha p; r -= alpha q; z = dinv r; partial r.z           alpha = gamma / (p.q), p.q folded here
__global__ __launch_bounds__(SH_BLOCK) void k_scg_xr(int64_t n, int nb_pq, const double* __restrict__ part_pq, const double* __restrict__ scal,
                                                     const double* __restrict__ p, const double* __restrict__ q, const double* __restrict__ dinv,
                                                     double* __restrict__ x, double* __restrict__ r, double* __restrict__ part_rz,
                                                     const int32_t* __restrict__ done) {
  if (*done) return;
  __shared__ double lds[SH_BLOCK / 64];
  const double pq = femo_fold_partials<SH_BLOCK>(part_pq, nb_pq, lds);
  const double alpha = pq != 0.0 ? scal[0] / pq : 0.0;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SH_BLOCK) {
    x[i] += alpha * p[i];
    const double ri = r[i] - alpha * q[i];
    r[i] = ri;
    s += ri * ri * dinv[i];
  }
  const double t = femo_block_sum<SH_BLOCK>(s, lds);
  if (threadIdx.x == 0) part_rz[blockIdx.x] = t;
}

// gamma' folded; beta = gamma'/gamma; p = dinv r + beta p; stopping test; one extra block-0 duty: publish gamma'
__global__ __launch_bounds__(SH_BLOCK) void k_scg_p(int64_t n, int it, int nb_rz, const double* __restrict__ part_rz, double* __restrict__ scal,
                                                    const double* __restrict__ r, const double* __restrict__ dinv, double* __restrict__ p,
                                                    int32_t* __restrict__ flag, double* __restrict__ gamma_out) {
  if (flag[0]) return;
  __shared__ double lds[SH_BLOCK / 64];
  const double g1 = femo_fold_partials<SH_BLOCK>(part_rz, nb_rz, lds);
  const double g0 = scal[0];
  const bool conv = g1 <= scal[2] || !(g1 == g1);
  const double beta = g0 != 0.0 ? g1 / g0 : 0.0;
  if (!conv) {
    for (int64_t i = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SH_BLOCK)
      p[i] = dinv[i] * r[i] + beta * p[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gamma_out[0] = g1;                   // read by the next iteration only after this kernel has finished
    flag[1] = it + 1;
    if (conv) { flag[2] = (g1 == g1) ? 0 : 1; __threadfence(); flag[0] = it + 1; }
  }
}

// r = rhs on the free dofs, 0 on the strongly imposed ones (those are set exactly after the loop)
__global__ void k_rhs_free(int64_t n, const double* __restrict__ rhs, const uint8_t* __restrict__ fixed, double* __restrict__ r) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    r[i] = (fixed != nullptr && fixed[i]) ? 0.0 : rhs[i];
}

__global__ void k_set_fixed(int64_t n, const uint8_t* __restrict__ fixed, const double* __restrict__ xfix, double* __restrict__ x) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (fixed[i]) x[i] = xfix != nullptr ? xfix[i] : 0.0;
}

// lifting: x holds the prescribed values on fixed dofs and 0 elsewhere on entry of the caller's choice; b' = b - A_fc x_c on free rows
__global__ __launch_bounds__(SH_BLOCK) void k_csr_lift(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
                                                       const double* __restrict__ vals, const uint8_t* __restrict__ fixed,
                                                       const double* __restrict__ xfix, const double* __restrict__ b, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (SH_BLOCK / 64);
  for (int64_t row = (int64_t)blockIdx.x * (SH_BLOCK / 64) + (threadIdx.x >> 6); row < n; row += nw) {
    double s = 0.0;
    if (!fixed[row]) {
      for (int64_t e = rowptr[row] + lane; e < rowptr[row + 1]; e += 64) {
        const int32_t cidx = cols[e];
        if (fixed[cidx]) s += vals[e] * xfix[cidx];
      }
    }
    s = femo_wave_sum(s);
    if (lane == 0) out[row] = fixed[row] ? xfix[row] : b[row] - s;
  }
}

__global__ void k_copy(int64_t n, const double* __restrict__ a, double* __restrict__ b) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) b[i] = a[i];
}

// lattice mode of the CG kernels: x += alpha p; r -= alpha q (no norm: r.z comes from k_pc_prolong)
__global__ __launch_bounds__(SH_BLOCK) void k_scg_xr_plain(int64_t n, int nb_pq, const double* __restrict__ part_pq, const double* __restrict__ scal,
                                                           const double* __restrict__ p, const double* __restrict__ q,
                                                           double* __restrict__ x, double* __restrict__ r, const int32_t* __restrict__ done) {
  if (*done) return;
  __shared__ double lds[SH_BLOCK / 64];
  const double pq = femo_fold_partials<SH_BLOCK>(part_pq, nb_pq, lds);
  const double alpha = pq != 0.0 ? scal[0] / pq : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SH_BLOCK) {
    x[i] += alpha * p[i];
    r[i] -= alpha * q[i];
  }
}

// p = z + beta p with z given (see k_scg_p)
__global__ __launch_bounds__(SH_BLOCK) void k_scg_p_z(int64_t n, int it, int nb_rz, const double* __restrict__ part_rz, double* __restrict__ scal,
                                                      const double* __restrict__ z, double* __restrict__ p, int32_t* __restrict__ flag,
                                                      double* __restrict__ gamma_out) {
  if (flag[0]) return;
  __shared__ double lds[SH_BLOCK / 64];
  const double g1 = femo_fold_partials<SH_BLOCK>(part_rz, nb_rz, lds);
  const double g0 = scal[0];
  const bool conv = g1 <= scal[2] || !(g1 == g1);
  const double beta = g0 != 0.0 ? g1 / g0 : 0.0;
  if (!conv) {
    for (int64_t i = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SH_BLOCK) p[i] = z[i] + beta * p[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gamma_out[0] = g1;
    flag[1] = it + 1;
    if (conv) { flag[2] = (g1 == g1) ? 0 : 1; __threadfence(); flag[0] = it + 1; }
  }
}

// x += alpha p; r -= alpha q per POINT (three dofs), and the per-block partial of r . (B r), B = the point's 3 x 3
// smoother block (or 1 / diag): the first half of r . z = r . B r + (P^T r) . e  (see k_lat_level, k_pc_prolong_fused)
__global__ __launch_bounds__(SH_BLOCK) void k_scg_xr_pt(int64_t n_pts, int nb_pq, const double* __restrict__ part_pq, const double* __restrict__ scal,
                                                        const double* __restrict__ p, const double* __restrict__ q, const double* __restrict__ dinv,
                                                        const float* __restrict__ dinv3, double* __restrict__ x, double* __restrict__ r,
                                                        double* __restrict__ part_rB, const int32_t* __restrict__ done, double* __restrict__ alpha_out = nullptr) {
  if (*done) return;
  __shared__ double lds[SH_BLOCK / 64];
  const double pq = femo_fold_partials<SH_BLOCK>(part_pq, nb_pq, lds);
  const double alpha = pq != 0.0 ? scal[0] / pq : 0.0;
  // alpha_out != nullptr: x += alpha p is carried by the preconditioner's first coarse product (ShellXCarry); this kernel
  // then streams q, r and the smoother blocks only
  const bool carry = alpha_out != nullptr;
  if (carry && blockIdx.x == 0 && threadIdx.x == 0) *alpha_out = alpha;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x; i < n_pts; i += (int64_t)gridDim.x * SH_BLOCK) {
    const Triple qq = *reinterpret_cast<const Triple*>(q + 3 * i);
    Triple rr = *reinterpret_cast<const Triple*>(r + 3 * i);
    if (!carry) {
      const Triple pp = *reinterpret_cast<const Triple*>(p + 3 * i);
      Triple xx = *reinterpret_cast<const Triple*>(x + 3 * i);
      xx.a += alpha * pp.a; xx.b += alpha * pp.b; xx.c += alpha * pp.c;
      *reinterpret_cast<Triple*>(x + 3 * i) = xx;
    }
    rr.a -= alpha * qq.a; rr.b -= alpha * qq.b; rr.c -= alpha * qq.c;
    *reinterpret_cast<Triple*>(r + 3 * i) = rr;
    if (dinv3 != nullptr) {
      const float* B = dinv3 + 9 * i;
      s += rr.a * ((double)B[0] * rr.a + (double)B[1] * rr.b + (double)B[2] * rr.c) + rr.b * ((double)B[3] * rr.a + (double)B[4] * rr.b + (double)B[5] * rr.c) +
           rr.c * ((double)B[6] * rr.a + (double)B[7] * rr.b + (double)B[8] * rr.c);
    } else {
      s += rr.a * rr.a * dinv[3 * i] + rr.b * rr.b * dinv[3 * i + 1] + rr.c * rr.c * dinv[3 * i + 2];
    }
  }
  const double t = femo_block_sum<SH_BLOCK>(s, lds);
  if (threadIdx.x == 0) part_rB[blockIdx.x] = t;
}

// ---- partitioned shells (several ranks): rows of points owned elsewhere, halo, all-reduced scalars ----------------------
// the scalar rows of block row p are the 9 (brow[p+1] - brow[p]) values from 9 brow[p] on
__global__ void k_zero_unowned_rows(int64_t n_pts, const uint8_t* __restrict__ owned, const int64_t* __restrict__ brow, double* __restrict__ vals) {
  const int lane = threadIdx.x & 63;
  for (int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < n_pts; p += (int64_t)gridDim.x * (blockDim.x >> 6)) {
    if (owned[p]) continue;
    for (int64_t k = 9 * brow[p] + lane; k < 9 * brow[p + 1]; k += 64) vals[k] = 0.0;
  }
}

__global__ void k_mask_unowned(int64_t n_pts, const uint8_t* __restrict__ owned, double* __restrict__ v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * n_pts; i += (int64_t)gridDim.x * blockDim.x)
    if (!owned[i / 3]) v[i] = 0.0;
}

__global__ void k_halo_pack(int64_t n, const int32_t* __restrict__ idx, const double* __restrict__ v, double* __restrict__ buf) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) buf[i] = v[idx[i]];
}

__global__ void k_halo_unpack(int64_t n, const int32_t* __restrict__ idx, const double* __restrict__ buf, double* __restrict__ v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[idx[i]] = buf[i];
}

// entries of the points owned by other ranks <- their owners' values (v: a state-sized device vector)
int shell_halo(femo_shell* s, double* v, hipStream_t st) {
  if (s->d_owned == nullptr || s->ctx->nranks == 1 || s->n_nbr == 0) return 0;
  const int64_t ns = s->send_ptr[(size_t)s->n_nbr], nr = s->recv_ptr[(size_t)s->n_nbr];
  if (ns > 0) hipLaunchKernelGGL(k_halo_pack, dim3(sgrid(ns, 256)), dim3(256), 0, st, ns, s->d_send_idx, v, s->d_send_buf);
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_TRY(femo_coll_neighbors(s->ctx, s->n_nbr, s->nbr.data(), s->send_ptr.data(), s->d_send_buf, s->recv_ptr.data(), s->d_recv_buf, st));
  if (nr > 0) hipLaunchKernelGGL(k_halo_unpack, dim3(sgrid(nr, 256)), dim3(256), 0, st, nr, s->d_recv_idx, s->d_recv_buf, v);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

// sum over the ranks of a device array (no-op on one rank)
int shell_allreduce(femo_shell* s, double* d, int64_t n, hipStream_t st) {
  if (s->d_owned == nullptr || s->ctx->nranks == 1) return 0;
  return femo_coll_allreduce(s->ctx, d, n, st);
}

// the rank's share of an assembled matrix: rows of the points owned elsewhere are zero
int shell_zero_unowned_rows(femo_shell* s, double* vals, hipStream_t st) {
  if (s->d_owned == nullptr) return 0;
  FEMO_REQUIRE(s->d_brow != nullptr, "a partitioned shell needs the node-block view of the pattern");
  hipLaunchKernelGGL(k_zero_unowned_rows, dim3(sgrid(s->n_bnode, 4)), dim3(256), 0, st, s->n_bnode, s->d_owned, s->d_brow, vals);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// r = rhs on the free dofs into d_r (the first step of a solve and of femo_shell_pc_apply)
void shell_rhs_free(femo_shell* s, const double* rhs, const uint8_t* d_fixed, hipStream_t st) {
  const unsigned gv = std::min<unsigned>(sgrid(s->n_dof), SH_MAXPART);
  hipLaunchKernelGGL(k_rhs_free, dim3(gv), dim3(256), 0, st, s->n_dof, rhs, d_fixed, s->d_r);
}

// 64-bit hash of the caller's Dirichlet mask, 32 bytes per step in four independent lanes (identifies the mask for the caches
// below: the device copy and the preconditioner's numbers)
static uint64_t shell_mask_hash(const uint8_t* p, int64_t n) {
  if (p == nullptr) return 1469598103934665603ull;
  uint64_t h[4] = {0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull};
  int64_t i = 0;
  for (; i + 32 <= n; i += 32) {
    uint64_t w[4];
    memcpy(w, p + i, 32);
#pragma unroll
    for (int k = 0; k < 4; ++k) { h[k] = (h[k] ^ w[k]) * 0x9FB21C651E98DF25ull; h[k] ^= h[k] >> 32; }
  }
  uint64_t t = 1469598103934665603ull ^ (uint64_t)n;
  for (; i < n; ++i) t = (t ^ p[i]) * 1099511628211ull;
  uint64_t r = t;
  for (int k = 0; k < 4; ++k) { r = (r ^ h[k]) * 0xD6E8FEB86659FD93ull; r ^= r >> 29; }
  return r != 0 ? r : 1;
}

// The mask on the device (nullptr without one) and its hash; the copy belongs to the shell and is re-uploaded only when the
// caller's array changed.
int shell_mask(femo_shell* s, const uint8_t* fixed_host, const uint8_t** d_fixed, uint64_t* hash) {
  *hash = shell_mask_hash(fixed_host, s->n_dof);
  *d_fixed = nullptr;
  if (fixed_host == nullptr) return 0;
  if (s->d_fixed_kept == nullptr) {
    FEMO_HIP_CHECK(hipMalloc(&s->d_fixed_kept, std::max<int64_t>(s->n_dof, 1)));
    s->fixed_kept_hash = 0;
  }
  if (s->fixed_kept_hash != *hash) {
    // (the stream may still run kernels of an earlier call that read the old mask: same stream, ordered)
    FEMO_HIP_CHECK(hipMemcpyAsync(s->d_fixed_kept, fixed_host, s->n_dof, hipMemcpyHostToDevice, s->ctx->stream));
    FEMO_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));        // the caller's (pageable) array may change after the call returns
    s->fixed_kept_hash = *hash;
  }
  *d_fixed = s->d_fixed_kept;
  return 0;
}

extern "C" {

int femo_shell_create(femo_ctx* ctx, int64_t n_vert, const double* x, int64_t n_cell, const int32_t* conn, int64_t n_edge,
                      const int32_t* cell_edges, const int64_t* rowptr, const int32_t* cols, const int32_t* elem_pos,
                      femo_shell** out) {
  FEMO_REQUIRE(ctx && x && conn && cell_edges && rowptr && cols && elem_pos && out, "null argument");
  FEMO_REQUIRE(n_vert > 0 && n_cell > 0 && n_edge > 0, "empty shell mesh");
  FEMO_HIP_CHECK(hipSetDevice(ctx->device));
  femo_shell* s = new femo_shell();
  s->ctx = ctx;
  s->n_vert = n_vert; s->n_cell = n_cell; s->n_edge = n_edge;
  s->n_unode = n_vert + n_edge;
  s->n_dof = 3 * s->n_unode + 3 * n_vert;
  s->nnz = rowptr[s->n_dof];
  FEMO_REQUIRE(s->nnz > 0 && s->nnz < (int64_t)1 << 31, "pattern too large for 32-bit element positions");
  hipStream_t st = ctx->stream;
  FEMO_TRY(to_device(&s->d_x, x, n_vert * 3, st));
  FEMO_TRY(to_device(&s->d_conn, conn, n_cell * 3, st));
  FEMO_TRY(to_device(&s->d_cedge, cell_edges, n_cell * 3, st));
  FEMO_TRY(to_device(&s->d_rowptr, rowptr, s->n_dof + 1, st));
  FEMO_TRY(to_device(&s->d_cols, cols, s->nnz, st));
  FEMO_TRY(to_device(&s->d_epos, elem_pos, n_cell * 729, st));
  {
    // node-block view: valid when every node's three rows have the same columns in runs of three (fea/shell.py numbers
    // the dofs 3 node + component, so the element-coupling pattern always is)
    const int64_t nbn = s->n_dof / 3;
    std::vector<int64_t> brow((size_t)nbn + 1, 0);
    std::vector<int32_t> bcols;
    bcols.reserve((size_t)(s->nnz / 9));
    bool ok = s->n_dof % 3 == 0;
    for (int64_t b = 0; ok && b < nbn; ++b) {
      const int64_t r0 = rowptr[3 * b], len = rowptr[3 * b + 1] - r0;
      ok = len % 3 == 0 && rowptr[3 * b + 2] - rowptr[3 * b + 1] == len && rowptr[3 * b + 3] - rowptr[3 * b + 2] == len &&
           r0 == 9 * brow[(size_t)b];
      for (int64_t j = 0; ok && j < len; j += 3) {
        const int32_t c = cols[r0 + j];
        ok = c % 3 == 0 && cols[r0 + j + 1] == c + 1 && cols[r0 + j + 2] == c + 2 && cols[r0 + len + j] == c &&
             cols[r0 + 2 * len + j] == c;
        bcols.push_back(c);
      }
      brow[(size_t)b + 1] = brow[(size_t)b] + len / 3;
    }
    if (ok) {
      s->n_bnode = nbn;
      FEMO_TRY(to_device(&s->d_brow, brow.data(), nbn + 1, st));
      FEMO_TRY(to_device(&s->d_bcols, bcols.data(), (int64_t)bcols.size(), st));
      // block-SELL: slots per slice = the longest of its BSW block rows
      const int64_t nsl = (nbn + BSW - 1) / BSW;
      std::vector<int64_t> off((size_t)nsl + 1, 0);
      for (int64_t sl = 0; sl < nsl; ++sl) {
        int64_t mx = 0;
        for (int64_t b = BSW * sl; b < std::min<int64_t>(BSW * sl + BSW, nbn); ++b) mx = std::max(mx, brow[(size_t)b + 1] - brow[(size_t)b]);
        off[(size_t)sl + 1] = off[(size_t)sl] + mx;
      }
      s->n_bslice = nsl; s->bsell_blocks = off[(size_t)nsl];
      FEMO_TRY(to_device(&s->d_bs_off, off.data(), nsl + 1, st));
      FEMO_HIP_CHECK(hipMalloc(&s->d_bs_cols, std::max<int64_t>(s->bsell_blocks, 1) * BSW * sizeof(int32_t)));
      FEMO_HIP_CHECK(hipMalloc(&s->d_bs_vals, std::max<int64_t>(s->bsell_blocks, 1) * 9 * BSW * sizeof(double)));
      FEMO_HIP_CHECK(hipStreamSynchronize(st));
    }
  }
  const int64_t n = s->n_dof;
  FEMO_HIP_CHECK(hipMalloc(&s->d_r, n * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_p, n * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_q, n * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_dinv, n * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_scal, 8 * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_part, 3 * SH_MAXPART * sizeof(double)));
  FEMO_HIP_CHECK(hipMalloc(&s->d_flag, 4 * sizeof(int32_t)));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  *out = s;
  return 0;
}

int femo_shell_destroy(femo_shell* s) {
  if (!s) return 0;
  hipStreamSynchronize(s->ctx->stream);
  shell_forms_free(s);
  shell_pc_free(s);
  shell_coarse_free(s);
  // this unit's own: femo_shell_create, femo_shell_set_partition, femo_shell_set_owned_cells, shell_mask
  hipFree(s->d_x); hipFree(s->d_conn); hipFree(s->d_cedge); hipFree(s->d_rowptr); hipFree(s->d_cols); hipFree(s->d_epos); hipFree(s->d_brow); hipFree(s->d_bcols);
  hipFree(s->d_bs_off); hipFree(s->d_bs_cols); hipFree(s->d_bs_vals);
  hipFree(s->d_r); hipFree(s->d_p); hipFree(s->d_q); hipFree(s->d_dinv); hipFree(s->d_scal); hipFree(s->d_part); hipFree(s->d_flag);
  hipFree(s->d_owned); hipFree(s->d_send_idx); hipFree(s->d_recv_idx); hipFree(s->d_send_buf); hipFree(s->d_recv_buf);
  hipFree(s->d_cell_owned);
  hipFree(s->d_fixed_kept);
  delete s;
  return 0;
}

int64_t femo_shell_ndof(const femo_shell* s) { return s ? s->n_dof : -1; }
int64_t femo_shell_nnz(const femo_shell* s) { return s ? s->nnz : -1; }

int femo_shell_matvec(femo_shell* s, const femo_vec* vals, const uint8_t* fixed_dev_or_null, const femo_vec* x, femo_vec* y) {
  FEMO_REQUIRE(s && vals && x && y, "null argument");
  FEMO_REQUIRE(vals->n >= s->nnz && x->n >= s->n_dof && y->n >= s->n_dof && x->d != y->d, "vector size mismatch in shell_matvec");
  femo_vec_touch(y);
  hipStream_t st = s->ctx->stream;
  if (s->d_brow != nullptr && fixed_dev_or_null == nullptr) {
    hipLaunchKernelGGL(k_bcsr3_spmv<16>, dim3(std::min<unsigned>(sgrid(s->n_bnode, SH_BLOCK / 16), SH_MAXPART)), dim3(SH_BLOCK), 0, st, s->n_bnode,
                       s->d_brow, s->d_bcols, vals->d, (const uint8_t*)nullptr, x->d, y->d, (double*)nullptr, (const int32_t*)nullptr,
                       (double*)nullptr, (const double*)nullptr);
  } else {
    hipLaunchKernelGGL(k_csr_spmv, dim3(sgrid(s->n_dof, SH_BLOCK / 16)), dim3(SH_BLOCK), 0, st, s->n_dof, s->d_rowptr, s->d_cols,
                       vals->d, fixed_dev_or_null, 1, x->d, y->d, (double*)nullptr, (const int32_t*)nullptr);
  }
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// Partition of a shell over the ranks of the context.  The handle was created on the rank's cells: all
// cells that touch a point it owns (points: P2 nodes and rotation vertices, dofs 3 p .. 3 p + 2).  owned_points flags
// them (n_dof / 3 bytes); segment k of send_dofs lists the dofs whose values rank nbr[k] needs, segment k of recv_dofs the
// dofs that receive rank nbr[k]'s values in the same order.
int femo_shell_set_partition(femo_shell* s, const uint8_t* owned_points, int n_nbr, const int32_t* nbr, const int64_t* send_ptr,
                             const int32_t* send_dofs, const int64_t* recv_ptr, const int32_t* recv_dofs) {
  FEMO_REQUIRE(s && owned_points, "null argument");
  FEMO_REQUIRE(n_nbr >= 0 && (n_nbr == 0 || (nbr && send_ptr && send_dofs && recv_ptr && recv_dofs)), "bad halo plan");
  FEMO_REQUIRE(s->d_owned == nullptr, "the shell already has a partition");
  FEMO_REQUIRE(s->d_brow != nullptr && s->n_dof % 3 == 0, "a partitioned shell needs the node-block view of the pattern");
  hipStream_t st = s->ctx->stream;
  FEMO_HIP_CHECK(hipSetDevice(s->ctx->device));
  const int64_t n_pts = s->n_dof / 3;
  for (int k = 0; k < n_nbr; ++k) {
    FEMO_REQUIRE(nbr[k] >= 0 && nbr[k] < s->ctx->nranks && nbr[k] != s->ctx->rank, "bad neighbour rank %d", nbr[k]);
    FEMO_REQUIRE(send_ptr[k + 1] >= send_ptr[k] && recv_ptr[k + 1] >= recv_ptr[k], "halo segments not ordered");
  }
  const int64_t ns = n_nbr ? send_ptr[n_nbr] : 0, nr = n_nbr ? recv_ptr[n_nbr] : 0;
  for (int64_t i = 0; i < ns; ++i) FEMO_REQUIRE(send_dofs[i] >= 0 && send_dofs[i] < s->n_dof && owned_points[send_dofs[i] / 3], "a rank sends a dof it does not own");
  for (int64_t i = 0; i < nr; ++i) FEMO_REQUIRE(recv_dofs[i] >= 0 && recv_dofs[i] < s->n_dof && !owned_points[recv_dofs[i] / 3], "a rank receives a dof it owns");
  FEMO_TRY(to_device(&s->d_owned, owned_points, n_pts, st));
  s->n_nbr = n_nbr;
  if (n_nbr > 0) {
    s->nbr.assign(nbr, nbr + n_nbr);
    s->send_ptr.assign(send_ptr, send_ptr + n_nbr + 1);
    s->recv_ptr.assign(recv_ptr, recv_ptr + n_nbr + 1);
    FEMO_TRY(to_device(&s->d_send_idx, send_dofs, ns, st));
    FEMO_TRY(to_device(&s->d_recv_idx, recv_dofs, nr, st));
    FEMO_HIP_CHECK(hipMalloc(&s->d_send_buf, std::max<int64_t>(ns, 1) * sizeof(double)));
    FEMO_HIP_CHECK(hipMalloc(&s->d_recv_buf, std::max<int64_t>(nr, 1) * sizeof(double)));
  }
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  s->pc_vals_uid = 0; s->pc_vals_gen = 0; s->bs_vals_uid = 0; s->bs_vals_gen = 0;
  return 0;
}

// The cells whose scalar outputs (mass, stress aggregate, energy, regularisation terms) this rank integrates: a uint8 per local
// cell, exactly one rank per cell of the whole mesh; the library sums the values over the ranks.  NULL clears it.
int femo_shell_set_owned_cells(femo_shell* s, const uint8_t* owned_cells) {
  FEMO_REQUIRE(s != nullptr, "null argument");
  (void)hipFree(s->d_cell_owned);
  s->d_cell_owned = nullptr;
  if (owned_cells != nullptr) FEMO_TRY(to_device(&s->d_cell_owned, owned_cells, s->n_cell, s->ctx->stream));
  FEMO_HIP_CHECK(hipStreamSynchronize(s->ctx->stream));
  return 0;
}

// x on the points owned by other ranks <- the owners' values (collective over the ranks of the partition)
int femo_shell_halo(femo_shell* s, femo_vec* x) {
  FEMO_REQUIRE(s && x, "null argument");
  FEMO_REQUIRE(x->n >= s->n_dof, "vector size mismatch in shell_halo");
  FEMO_REQUIRE(s->d_owned != nullptr, "femo_shell_halo needs femo_shell_set_partition");
  femo_vec_touch(x);
  return shell_halo(s, x->d, s->ctx->stream);
}

// x <- 0 on the points owned by other ranks: the rank's share of a vector assembled over its cells
int femo_shell_mask_unowned(femo_shell* s, femo_vec* x) {
  FEMO_REQUIRE(s && x, "null argument");
  FEMO_REQUIRE(x->n >= s->n_dof, "vector size mismatch in shell_mask_unowned");
  if (s->d_owned == nullptr) return 0;
  femo_vec_touch(x);
  hipLaunchKernelGGL(k_mask_unowned, dim3(sgrid(s->n_dof, 256)), dim3(256), 0, s->ctx->stream, s->n_dof / 3, s->d_owned, x->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// K_ff x_f = b_f - K_fc g_c with x_c = g_c on the dofs flagged in `fixed` (host array of n_dof bytes, values in xfix);
// PCG, stops on sqrt(r.M^-1 r) <= max(rtol sqrt(r0.M^-1 r0), atol); opts->pc = 0: M = D (Jacobi), 1: the lattice
// preconditioner of femo_shell_pc_create.  K symmetric: the same call serves the adjoint (fea_dolfinx.py:208-222).
int femo_shell_solve(femo_shell* s, const femo_vec* vals, const uint8_t* fixed_host, const femo_vec* xfix, const femo_vec* b,
                     femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info) {
  FEMO_REQUIRE(s && vals && b && x && opts && info, "null argument");
  const int64_t n = s->n_dof;
  FEMO_REQUIRE(vals->n >= s->nnz && b->n >= n && x->n >= n && b->d != x->d, "vector size mismatch in shell_solve");
  FEMO_REQUIRE(fixed_host == nullptr || xfix == nullptr || xfix->n >= n, "prescribed values shorter than n_dof");
  femo_ctx* ctx = s->ctx;
  hipStream_t st = ctx->stream;
  memset(info, 0, sizeof *info);
  femo_vec_touch(x);
  const uint8_t* d_fixed = nullptr;
  uint64_t mask_hash = 0;
  FEMO_TRY(shell_mask(s, fixed_host, &d_fixed, &mask_hash));
  const unsigned gv = std::min<unsigned>(sgrid(n), SH_MAXPART);
  // workgroups of the operator product (their per-block partials of p.q are folded by k_scg_xr*): 16 rows, or 16
  // node blocks of three rows, per workgroup pass
  const bool bsell = s->d_bs_vals != nullptr && getenv("FEMO_SHELL_NO_BSELL") == nullptr;
  // block-SELL: 16 slices per workgroup pass, at most 2048 workgroups (0.376 ms per iteration at 1.97 M dofs against
  // 0.390 with one pass per workgroup: fewer partial sums for the consumers to fold)
  const unsigned gs = bsell ? std::min<unsigned>(sgrid(s->n_bslice, SH_BLOCK / BSW), 2048u)
                            : std::min<unsigned>(s->d_brow != nullptr ? sgrid(s->n_bnode, SH_BLOCK / 16) : sgrid(n, SH_BLOCK / 16), SH_MAXPART);
  double *Ppq = s->d_part, *Prz = s->d_part + SH_MAXPART, *gam = s->d_scal + 4;
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev0, st));
  // right-hand side with lifting (into q); zero initial guess
  FEMO_HIP_CHECK(hipMemsetAsync(x->d, 0, n * sizeof(double), st));
  const double* rhs = b->d;
  if (d_fixed != nullptr && xfix != nullptr) {
    hipLaunchKernelGGL(k_csr_lift, dim3(gs), dim3(SH_BLOCK), 0, st, n, s->d_rowptr, s->d_cols, vals->d, d_fixed, xfix->d, b->d, s->d_q);
    rhs = s->d_q;
  }
  shell_rhs_free(s, rhs, d_fixed, st);
  // Partitioned shell (femo_shell_set_partition): the rows of K and the entries of r on points owned elsewhere are zero, so
  // every dot product below is the rank's share and P^T r, P^T K P sum over the ranks to the global objects; the producers'
  // partials are folded into one number, all-reduced, and handed to the unfused consumers as a single "partial".  The
  // direction p is refreshed on the halo before every product (x follows: it is updated with the refreshed p).
  const bool multi = s->d_owned != nullptr;
  if (multi) {
    FEMO_REQUIRE(n % 3 == 0, "a partitioned shell numbers its dofs 3 point + component");
    hipLaunchKernelGGL(k_mask_unowned, dim3(gv), dim3(256), 0, st, n / 3, s->d_owned, s->d_r);
  }
  double *one_pq = s->d_scal + 6, *one_rz = s->d_scal + 7;   // the all-reduced p.q and r.z
  const bool lattice = opts->pc == 1;
  const bool point_blocks = !femo_env_flag("FEMO_SHELL_NO_POINT_BLOCKS");   // read once: this call and the set-up must agree
  // 1 / diag: with the lattice preconditioner and its point blocks it comes out of k_pt_block_inv (below, and only when
  // the stiffness or the mask changed)
  if (!(lattice && s->d_brow != nullptr && point_blocks))
    hipLaunchKernelGGL(k_csr_diag_inv, dim3(gv), dim3(256), 0, st, n, s->d_rowptr, s->d_cols, vals->d, d_fixed, s->d_dinv);
  FEMO_REQUIRE(!lattice || s->pc_width > 0, "opts->pc = 1 needs femo_shell_pc_create");
  if (bsell && (s->bs_vals_uid != vals->uid || s->bs_vals_gen != vals->gen || vals->uid == 0)) {
    hipLaunchKernelGGL(k_bsell_fill, dim3((unsigned)s->n_bslice), dim3(256), 0, st, s->n_bnode, s->d_brow, s->d_bcols, vals->d, s->d_bs_off,
                       s->d_bs_cols, s->d_bs_vals);
    s->bs_vals_uid = vals->uid; s->bs_vals_gen = vals->gen;
  }
  const unsigned gz = std::min<unsigned>(sgrid(n / 3, SH_BLOCK / 8), SH_MAXPART);     // k_pc_prolong: 8 lanes per point
  const unsigned gx = std::min<unsigned>(sgrid(n / 3), 1024u);                        // k_scg_xr_pt: a thread per point, few partials
  double* Pte = s->d_part + 2 * SH_MAXPART;
  if (lattice) {
    FEMO_TRY(shell_pc_setup(s, vals, mask_hash, d_fixed, point_blocks));
    FEMO_TRY(shell_pc_apply(s, d_fixed, Prz, gz, nullptr));
    hipLaunchKernelGGL(k_copy, dim3(gv), dim3(256), 0, st, n, s->d_z, s->d_p);
  } else {
    hipLaunchKernelGGL(k_scg_init, dim3(gv), dim3(SH_BLOCK), 0, st, n, s->d_r, s->d_dinv, s->d_p, Prz);
  }
  // x += alpha p inside the preconditioner's first coarse product (fused loop, one rank, with the coarse solve)
  const bool carry_x = lattice && !multi && s->cs_ready;
  const int nb_rz0 = lattice ? (int)gz : (int)gv;
  if (multi) {
    FEMO_TRY(femo_launch_fold(SH_BLOCK, nb_rz0, 1, Prz, one_rz, st));
    FEMO_TRY(shell_allreduce(s, one_rz, 1, st));
    hipLaunchKernelGGL(k_scg_gamma0, dim3(1), dim3(SH_BLOCK), 0, st, 1, one_rz, opts->rtol * opts->rtol, opts->atol * opts->atol, s->d_scal, s->d_flag);
  } else {
    hipLaunchKernelGGL(k_scg_gamma0, dim3(1), dim3(SH_BLOCK), 0, st, nb_rz0, Prz, opts->rtol * opts->rtol, opts->atol * opts->atol, s->d_scal, s->d_flag);
  }
  FEMO_HIP_CHECK(hipGetLastError());
  const int max_it = opts->max_it > 0 ? opts->max_it : 100000;
  const int batch = opts->check_every > 0 ? opts->check_every : 64;
  int32_t h_flag[4] = {0, 0, 0, 0};
  double h_scal[8];
  FEMO_HIP_CHECK(hipMemcpyAsync(h_flag, s->d_flag, sizeof h_flag, hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipMemcpyAsync(h_scal, s->d_scal, sizeof h_scal, hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  info->rhs_norm = std::sqrt(h_scal[1]);
  int it = 0, since_mark = 0;
  const int n_sample = 4;
  int n_ev = 0;
  bool stalled = false;
  double best = HUGE_VAL, best_mark = HUGE_VAL;
  while (!h_flag[0] && it < max_it) {
    const int it_end = std::min(it + batch, max_it);
    for (; it < it_end; ++it) {
      // HIP events around four of the operator products (iterations 4 .. 7) for the roofline record of bench.py
      const bool sample = it >= 4 && it < 4 + n_sample;
      if (sample) FEMO_HIP_CHECK(hipEventRecord(ctx->ev_pool[2 * n_ev], st));
      // p is zero on the imposed dofs (r and the initial direction are): no column mask needed
      if (multi) FEMO_TRY(shell_halo(s, s->d_p, st));
      if (bsell)
        hipLaunchKernelGGL(k_bsell_spmv, dim3(gs), dim3(SH_BLOCK), 0, st, s->n_bnode, s->n_bslice, s->d_bs_off, s->d_bs_cols, s->d_bs_vals, d_fixed, s->d_p, s->d_q, Ppq, s->d_flag, s->d_scal, gam);
      else if (s->d_brow != nullptr)
        hipLaunchKernelGGL(k_bcsr3_spmv<16>, dim3(gs), dim3(SH_BLOCK), 0, st, s->n_bnode, s->d_brow, s->d_bcols, vals->d, d_fixed, s->d_p, s->d_q, Ppq, s->d_flag, s->d_scal, gam);
      else
        hipLaunchKernelGGL(k_csr_spmv, dim3(gs), dim3(SH_BLOCK), 0, st, n, s->d_rowptr, s->d_cols, vals->d, d_fixed, 0, s->d_p, s->d_q, Ppq, s->d_flag, s->d_scal, gam);
      if (sample) { FEMO_HIP_CHECK(hipEventRecord(ctx->ev_pool[2 * n_ev + 1], st)); ++n_ev; }
      if (multi) {
        FEMO_TRY(femo_launch_fold(SH_BLOCK, (int)gs, 1, Ppq, one_pq, st, s->d_flag));
        FEMO_TRY(shell_allreduce(s, one_pq, 1, st));
        if (lattice) {
          hipLaunchKernelGGL(k_scg_xr_plain, dim3(gv), dim3(SH_BLOCK), 0, st, n, 1, one_pq, s->d_scal, s->d_p, s->d_q, x->d, s->d_r, s->d_flag);
          FEMO_TRY(shell_pc_apply(s, d_fixed, Prz, gz, s->d_flag));
          FEMO_TRY(femo_launch_fold(SH_BLOCK, (int)gz, 1, Prz, one_rz, st, s->d_flag));
          FEMO_TRY(shell_allreduce(s, one_rz, 1, st));
          hipLaunchKernelGGL(k_scg_p_z, dim3(gv), dim3(SH_BLOCK), 0, st, n, it, 1, one_rz, s->d_scal, s->d_z, s->d_p, s->d_flag, gam);
        } else {
          hipLaunchKernelGGL(k_scg_xr, dim3(gv), dim3(SH_BLOCK), 0, st, n, 1, one_pq, s->d_scal, s->d_p, s->d_q, s->d_dinv, x->d, s->d_r, Prz, s->d_flag);
          FEMO_TRY(femo_launch_fold(SH_BLOCK, (int)gv, 1, Prz, one_rz, st, s->d_flag));
          FEMO_TRY(shell_allreduce(s, one_rz, 1, st));
          hipLaunchKernelGGL(k_scg_p, dim3(gv), dim3(SH_BLOCK), 0, st, n, it, 1, one_rz, s->d_scal, s->d_r, s->d_dinv, s->d_p, s->d_flag, gam);
        }
      } else if (lattice) {
        // One rank: the direction update is fused into the prolongation (dofs numbered 3 point + component).
        // r . z = r . B r + (P^T r) . e is known before z is: the update emits the first part, the finest lattice level
        // the second, and the prolongation writes p = z + beta p at once (9 launches and 3 vector streams fewer
        // per iteration than the unfused form above)
        int nb_te = 0;
        if (carry_x) {
          hipLaunchKernelGGL(k_scg_xr_pt, dim3(gx), dim3(SH_BLOCK), 0, st, n / 3, (int)gs, Ppq, s->d_scal, s->d_p, s->d_q, s->d_dinv,
                             s->dinv3_ready ? s->d_dinv3 : (const float*)nullptr, x->d, s->d_r, Prz, s->d_flag, s->d_scal + 5);
          FEMO_TRY(shell_pc_apply(s, d_fixed, Prz, gz, s->d_flag, Pte, &nb_te, x->d));
        } else {
          hipLaunchKernelGGL(k_scg_xr_pt, dim3(gx), dim3(SH_BLOCK), 0, st, n / 3, (int)gs, Ppq, s->d_scal, s->d_p, s->d_q, s->d_dinv,
                             s->dinv3_ready ? s->d_dinv3 : (const float*)nullptr, x->d, s->d_r, Prz, s->d_flag);
          FEMO_TRY(shell_pc_apply(s, d_fixed, Prz, gz, s->d_flag, Pte, &nb_te));
        }
        // 2048 workgroups = one resident round of 8 waves per SIMD, ten trips each: 45.0 us at 1.97 M dofs against 49.3 with 4096,
        // 56.6 with 8192, 61.5 with 1024 (every workgroup starts with two folds and three dependent scalar reads; fewer
        // partials to fold change nothing: 44.4 - 46.3 us with 256 - 1024 of each)
        const unsigned gzf = std::min<unsigned>(gz, 2048u);
        shell_pc_prolong_fused(s, d_fixed, gzf, it, (int)gx, Prz, nb_te, Pte, gam, st);
      } else {
        hipLaunchKernelGGL(k_scg_xr, dim3(gv), dim3(SH_BLOCK), 0, st, n, (int)gs, Ppq, s->d_scal, s->d_p, s->d_q, s->d_dinv, x->d, s->d_r, Prz, s->d_flag);
        hipLaunchKernelGGL(k_scg_p, dim3(gv), dim3(SH_BLOCK), 0, st, n, it, (int)gv, Prz, s->d_scal, s->d_r, s->d_dinv, s->d_p, s->d_flag, gam);
      }
    }
    FEMO_HIP_CHECK(hipGetLastError());
    FEMO_HIP_CHECK(hipMemcpyAsync(h_flag, s->d_flag, sizeof h_flag, hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipMemcpyAsync(h_scal, s->d_scal, sizeof h_scal, hipMemcpyDeviceToHost, st));
    FEMO_HIP_CHECK(hipStreamSynchronize(st));
    // Attainable accuracy: sqrt(r.M^-1 r) measures the error in the energy norm, where fp64 delivers about
    // eps sqrt(cond K) of the solution (1e-11 for a thin shell); a tolerance below that is never met and CG wanders
    // (450 s on a 2 k-dof roof with rtol 1e-12 and the coarse solve, whose norm is honest about the smooth modes).
    // Once the residual is below 1e-9 of the initial one in that norm and the best value seen has not halved in 8
    // batches, the solve ends with converged = 2.
    if (!h_flag[0]) {
      const double g = h_scal[0];
      if (g == g && g < best) {
        if (g < 0.5 * best_mark) { best_mark = g; since_mark = 0; }
        best = g;
      }
      if (++since_mark > 8 && best <= 1e-18 * h_scal[1]) { stalled = true; break; }
    }
  }
  if (d_fixed != nullptr) hipLaunchKernelGGL(k_set_fixed, dim3(gv), dim3(256), 0, st, n, d_fixed, xfix ? xfix->d : nullptr, x->d);
  if (multi) FEMO_TRY(shell_halo(s, x->d, st));          // the caller reads a consistent state on all its points
  FEMO_HIP_CHECK(hipMemcpyAsync(h_scal, s->d_scal, sizeof h_scal, hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev1, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  float ms = 0.f;
  FEMO_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  info->solve_ms = ms;
  {
    const int iters_run = h_flag[0] ? h_flag[1] : it;
    double acc = 0.0;
    int used = 0;
    for (int i = 0; i < n_ev; ++i) {
      if (4 + i >= iters_run) break;                     // a launch behind the converged iteration returned at once
      float t = 0.f;
      FEMO_HIP_CHECK(hipEventElapsedTime(&t, ctx->ev_pool[2 * i], ctx->ev_pool[2 * i + 1]));
      acc += t; ++used;
    }
    info->spmv_ms = acc;
    info->spmv_samples = used;
  }
  info->iterations = h_flag[0] ? h_flag[1] : it;
  info->converged = h_flag[0] ? (h_flag[2] ? -1 : 1) : (stalled ? 2 : 0);
  info->residual_norm = std::sqrt(std::max(h_flag[0] && h_flag[1] > 0 ? h_scal[4] : h_scal[0], 0.0));
  return 0;
}

}  // extern "C"
