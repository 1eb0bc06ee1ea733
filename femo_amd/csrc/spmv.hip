// SELL-64 SpMV for gfx950: the operator side of the Krylov solvers (solver.hip) -- the product kernels and their
// slice walk, the transposition, the ghost refresh and its overlapped forms, the scaling S, S A S.
//
// Replaces the reference's PETSc calls:
//   Mat*Vec / multTranspose  utils_dolfinx.py:256-264, 275-287   (state_model.py:176-200)
//
// SpMV layout: the diagonal is a dense vector; off-diagonals live in SELL-64
// slices with pair interleave, so lane l of a wave owns row 64*slice+l and each
// wave-instruction reads 1 KiB of values (16 B/lane) and 512 B of columns
// (8 B/lane), fully coalesced.  Consecutive lanes are consecutive rows, so for
// any bandwidth-reducing vertex order the x-gathers of one instruction fall in
// a few cache lines.  Row sums are sequential per lane: deterministic.
//
// Compacted copy of S A S (k_scale_sell<true>, k_spmv_sell<.., CP = true>): on one rank the scaling also writes a copy in
// which every regular slice keeps only the slots that are not zero in all 64 rows, packed to the front in their order; the
// products of the Krylov loops walk it (femo_launch_spmv decides).  On a structured simplicial grid that is 6 of 14 slots in
// 3-D and 4 of 6 in 2-D: the P1 stiffness is the 7- / 5-point stencil and the diagonal couplings cancel bit for bit.  A dead
// slot contributed acc += 0 * x and the live ones keep their order, so for finite x the product is the same bits.  Two edge
// cases differ: a non-finite x entry under a dead slot no longer turns the row into NaN, and a row
// whose every term is -0.0 keeps -0.0 where the full product's + 0 * x made it +0.0.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "femo_internal.h"

namespace {

// ------------------------------------------------------------------- SpMV ---
// NP pair-steps of one row, fully unrolled: all value/column loads are issued
// before the first gather, all gathers before the first FMA, so one slice costs
// two memory round trips whatever its width.  Summation order is k = 0, 1, 2, ...
// 16-B / 8-B native vectors so that the nontemporal builtin emits ONE global_load_dwordx4 / x2
// per lane (on HIP's struct double2 it splits into two 8-B loads: half the access width)
typedef double femo_v2d __attribute__((ext_vector_type(2)));
typedef int femo_v2i __attribute__((ext_vector_type(2)));

__device__ __forceinline__ double2 nt_load2(const double2* p) {
  const femo_v2d v = __builtin_nontemporal_load(reinterpret_cast<const femo_v2d*>(p));
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ int2 nt_load2(const int2* p) {
  const femo_v2i v = __builtin_nontemporal_load(reinterpret_cast<const femo_v2i*>(p));
  return make_int2(v.x, v.y);
}
// NT = false (round 5): ordinary loads for operators whose stored values fit the 256 MB Infinity Cache -- they are read again
// 28 times per solve, and the streaming hint kept them from staying there (1.03 M rows: 27.6 -> 21.0 us per product; at
// 10 M rows, 1.4 GB of values, the hint is worth 2 %: femo_launch_spmv picks by size)
template <bool NT> __device__ __forceinline__ double2 mat_load2(const double2* p) {
  if constexpr (NT) return nt_load2(p);
  else { const femo_v2d v = *reinterpret_cast<const femo_v2d*>(p); return make_double2(v.x, v.y); }
}
template <bool NT> __device__ __forceinline__ int mat_load(const int* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}

template <int NP, bool NT>
__device__ __forceinline__ double row_pairs(const double2* __restrict__ v2, const int2* __restrict__ c2,
                                            const double* __restrict__ x, double acc) {
  double2 a[NP];
  int2 j[NP];
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    if (NT) {
      a[m] = nt_load2(&v2[m * 64]);
      j[m] = nt_load2(&c2[m * 64]);
    } else {
      a[m] = v2[m * 64];
      j[m] = c2[m * 64];
    }
  }
  double xv[2 * NP];
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    xv[2 * m] = x[j[m].x];
    xv[2 * m + 1] = x[j[m].y];
  }
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    acc += a[m].x * xv[2 * m];
    acc += a[m].y * xv[2 * m + 1];
  }
  return acc;
}

template <bool NT>
__device__ __forceinline__ double row_sum(int npair, const double2* __restrict__ v2, const int2* __restrict__ c2,
                                          const double* __restrict__ x, double acc) {
  while (npair > 8) {
    acc = row_pairs<8, NT>(v2, c2, x, acc);
    v2 += 8 * 64; c2 += 8 * 64; npair -= 8;
  }
  switch (npair) {  // wave-uniform
    case 8: return row_pairs<8, NT>(v2, c2, x, acc);
    case 7: return row_pairs<7, NT>(v2, c2, x, acc);
    case 6: return row_pairs<6, NT>(v2, c2, x, acc);
    case 5: return row_pairs<5, NT>(v2, c2, x, acc);
    case 4: return row_pairs<4, NT>(v2, c2, x, acc);
    case 3: return row_pairs<3, NT>(v2, c2, x, acc);
    case 2: return row_pairs<2, NT>(v2, c2, x, acc);
    case 1: return row_pairs<1, NT>(v2, c2, x, acc);
    default: return acc;
  }
}

// Short slice: the columns as 16-bit deltas from the row, two per 4-byte word (one global_load_dword per pair and lane
// instead of a dwordx2)
template <int NP, bool NT>
__device__ __forceinline__ double row_pairs_short(const double2* __restrict__ v2, const int* __restrict__ c16,
                                                  const double* __restrict__ xrow, double acc) {
  double2 a[NP];
  int j[NP];
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    a[m] = mat_load2<NT>(&v2[m * 64]);
    j[m] = mat_load<NT>(&c16[m * 64]);
  }
  double xv[2 * NP];
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    xv[2 * m] = xrow[(int)(short)(j[m] & 0xFFFF)];
    xv[2 * m + 1] = xrow[j[m] >> 16];
  }
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    acc += a[m].x * xv[2 * m];
    acc += a[m].y * xv[2 * m + 1];
  }
  return acc;
}

template <bool NT>
__device__ __forceinline__ double row_sum_short(int npair, const double2* __restrict__ v2, const int* __restrict__ c16,
                                                const double* __restrict__ xrow, double acc) {
  while (npair > 8) {
    acc = row_pairs_short<8, NT>(v2, c16, xrow, acc);
    v2 += 8 * 64; c16 += 8 * 64; npair -= 8;
  }
  switch (npair) {  // wave-uniform
    case 8: return row_pairs_short<8, NT>(v2, c16, xrow, acc);
    case 7: return row_pairs_short<7, NT>(v2, c16, xrow, acc);
    case 6: return row_pairs_short<6, NT>(v2, c16, xrow, acc);
    case 5: return row_pairs_short<5, NT>(v2, c16, xrow, acc);
    case 4: return row_pairs_short<4, NT>(v2, c16, xrow, acc);
    case 3: return row_pairs_short<3, NT>(v2, c16, xrow, acc);
    case 2: return row_pairs_short<2, NT>(v2, c16, xrow, acc);
    case 1: return row_pairs_short<1, NT>(v2, c16, xrow, acc);
    default: return acc;
  }
}

// Regular slice: column k of lane l is row + delta[k]; x is read as 64 consecutive
// doubles per k (one coalesced 512-B load), no column indices are fetched.
template <int NP, bool NT>
__device__ __forceinline__ double row_pairs_regular(const double2* __restrict__ v2, const int32_t* __restrict__ delta,
                                                    const double* __restrict__ xrow, double acc) {
  double2 a[NP];
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    a[m] = mat_load2<NT>(&v2[m * 64]);
  }
  double xv[2 * NP];
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    xv[2 * m] = xrow[delta[2 * m]];
    xv[2 * m + 1] = xrow[delta[2 * m + 1]];
  }
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    acc += a[m].x * xv[2 * m];
    acc += a[m].y * xv[2 * m + 1];
  }
  return acc;
}

template <bool NT>
__device__ __forceinline__ double row_sum_regular(int npair, const double2* __restrict__ v2, const int32_t* __restrict__ delta,
                                                  const double* __restrict__ xrow, double acc) {
  while (npair > 8) {
    acc = row_pairs_regular<8, NT>(v2, delta, xrow, acc);
    v2 += 8 * 64; delta += 16; npair -= 8;
  }
  switch (npair) {  // wave-uniform
    case 8: return row_pairs_regular<8, NT>(v2, delta, xrow, acc);
    case 7: return row_pairs_regular<7, NT>(v2, delta, xrow, acc);
    case 6: return row_pairs_regular<6, NT>(v2, delta, xrow, acc);
    case 5: return row_pairs_regular<5, NT>(v2, delta, xrow, acc);
    case 4: return row_pairs_regular<4, NT>(v2, delta, xrow, acc);
    case 3: return row_pairs_regular<3, NT>(v2, delta, xrow, acc);
    case 2: return row_pairs_regular<2, NT>(v2, delta, xrow, acc);
    case 1: return row_pairs_regular<1, NT>(v2, delta, xrow, acc);
    default: return acc;
  }
}

// ---- boundary slices of a partitioned mesh inside the ONE launch of the merged loop (round 6) -------------------------
// With the device-initiated ghost refresh the product needs no second launch and no copy of the inbox: the slices with
// ghost columns sit at the END of every XCD's range of the slice list (flagged by the sign bit), the wave that reaches one
// first waits for the neighbours' counters (they have had the whole interior to arrive) and then gathers ghost columns
// straight from its own inbox generation.  femo_internal.h: FemoHaloDirect.
struct SpmvGhost {
  const unsigned long long* cnt; const int32_t* blocks; int n_nbr; unsigned long long epoch; int32_t* err;
  const double* ghost;          // inbox generation of this exchange, ghost k at ghost[k]
  int64_t n_own;
};
__device__ __forceinline__ void spmv_halo_wait_wave(const SpmvGhost& g, int lane) {
  if (lane < g.n_nbr) {
    const unsigned long long want = g.epoch * (unsigned long long)g.blocks[lane];
    const unsigned long long* c = g.cnt + (size_t)lane * FEMO_HALO_CNT_STRIDE;
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
      __builtin_amdgcn_s_sleep(2);
      if (wall_clock64() - t0 > 400000000ll) { atomicExch(g.err, 1); break; }
    }
  }
  // the wave reconverges here; nothing below may be issued before the counters were seen (the inbox is uncached memory:
  // no fence beyond ordering is needed, see femo_halo_signal)
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}
template <int NP, bool NT>
__device__ __forceinline__ double row_pairs_gh(const double2* __restrict__ v2, const int2* __restrict__ c2,
                                               const double* __restrict__ x, const double* __restrict__ gbase, int n_own, double acc) {
  double2 a[NP];
  int2 j[NP];
#pragma unroll
  for (int m = 0; m < NP; ++m) { a[m] = mat_load2<NT>(&v2[m * 64]); j[m] = c2[m * 64]; }
  double xv[2 * NP];
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    // (one `sc0 sc1` load either way: the ghost entries must come from the memory side, femo_halo_store; the owned entries of
    // these few slices can afford to)
    xv[2 * m] = femo_halo_load((j[m].x < n_own ? x : gbase) + j[m].x);
    xv[2 * m + 1] = femo_halo_load((j[m].y < n_own ? x : gbase) + j[m].y);
  }
#pragma unroll
  for (int m = 0; m < NP; ++m) {
    acc += a[m].x * xv[2 * m];
    acc += a[m].y * xv[2 * m + 1];
  }
  return acc;
}
template <bool NT>
__device__ __forceinline__ double row_sum_gh(int npair, const double2* __restrict__ v2, const int2* __restrict__ c2,
                                             const double* __restrict__ x, const double* __restrict__ gbase, int n_own, double acc) {
  while (npair > 4) {
    acc = row_pairs_gh<4, NT>(v2, c2, x, gbase, n_own, acc);
    v2 += 4 * 64; c2 += 4 * 64; npair -= 4;
  }
  switch (npair) {  // wave-uniform
    case 4: return row_pairs_gh<4, NT>(v2, c2, x, gbase, n_own, acc);
    case 3: return row_pairs_gh<3, NT>(v2, c2, x, gbase, n_own, acc);
    case 2: return row_pairs_gh<2, NT>(v2, c2, x, gbase, n_own, acc);
    case 1: return row_pairs_gh<1, NT>(v2, c2, x, gbase, n_own, acc);
    default: return acc;
  }
}

// DOT: 0 none; 1 partial d.Ax into partials[block] (d = dvec or x); 2 additionally partial x.x,
// 3 additionally partial Ax.Ax, into the next slot; 4 (merged BPX-PCG): x.Ax, Ax.Ax and dvec.Ax into three
// consecutive slots (p.q, q.q, r.q: everything the single all-reduce of an iteration carries besides the lattice)
// CP: `vals` is the compacted copy of S A S (femo_mat::d_valsC) with its cdelta / cpairs; a parameter of its own, so that
// every other product is the code it was
template <int DOT, bool UNIT, bool NT = true, bool GH = false, bool CP = false>
__global__ __launch_bounds__(FEMO_BLOCK) void k_spmv_sell(
    int64_t n_rows, int64_t n_slices, const int64_t* __restrict__ mptr,
    const int32_t* __restrict__ cols, const int16_t* __restrict__ cols16, const int32_t* __restrict__ sdelta, int sdelta_stride,
    const double* __restrict__ vals, const double* __restrict__ diag, const double* __restrict__ x,
    double* __restrict__ y, double* __restrict__ partials, const int32_t* __restrict__ done,
    const int32_t* __restrict__ slice_list, int64_t n_list, const double* __restrict__ dvec,
    const int32_t* __restrict__ cdelta, const int32_t* __restrict__ cpairs, SpmvGhost gh = SpmvGhost{}) {
  if (done != nullptr && *done) return;
  bool waited = false;
  __shared__ double lds[FEMO_BLOCK / 64];
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction: tell the compiler, so that slice metadata (offsets, the
  // per-slice delta table) comes through scalar loads instead of 64 identical vector loads
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware: blockIdx % 8 labels the XCD group; each group walks its own
  // contiguous eighth of the slices, its waves interleaved slice by slice, so the
  // x window the group gathers from stays in that XCD's L2.
  const int xcd = blockIdx.x & 7;
  const int64_t blk_in_xcd = blockIdx.x >> 3;
  const int64_t waves_per_xcd = (int64_t)(gridDim.x >> 3) * (FEMO_BLOCK / 64);
  // slice_list != null: walk that subset (interior or boundary slices of a partitioned mesh)
  const int64_t n_walk = slice_list ? n_list : n_slices;
  const int64_t s_lo = n_walk * xcd / 8, s_hi = n_walk * (xcd + 1) / 8;
  double dot = 0.0, dot2 = 0.0, dot3 = 0.0;
  for (int64_t si = s_lo + blk_in_xcd * (FEMO_BLOCK / 64) + wave; si < s_hi; si += waves_per_xcd) {
    const int32_t entry = slice_list ? slice_list[si] : (int32_t)si;
    const bool bnd = GH && entry < 0;                      // sign bit: the slice has ghost columns (wave-uniform)
    const int64_t slice = GH ? (int64_t)(entry & 0x7FFFFFFF) : (slice_list ? (int64_t)entry : si);
    const int64_t base = mptr[slice];
    // CP: a regular slice holds cpairs[slice] pairs of live slots at the front of its block, their deltas in cdelta; every
    // other slice is as in the full copy (scalar loads, like the offsets)
    const int npair = CP ? cpairs[slice] : (int)((mptr[slice + 1] - base) >> 7);
    const int64_t row = (slice << 6) + lane;
    if (GH && bnd && !waited) { spmv_halo_wait_wave(gh, lane); waited = true; }
    const double xr = x[row < n_rows ? row : 0];
    double acc = UNIT ? xr : diag[row] * xr;   // UNIT: symmetrically scaled operator, diagonal == 1
    const double2* __restrict__ v2 = reinterpret_cast<const double2*>(vals + base) + lane;
    const int32_t* __restrict__ dl = (CP ? cdelta : sdelta) + slice * sdelta_stride;
    if (GH && bnd) {           // 32-bit columns whatever the slice's class; ghost columns come from the inbox
      const int2* __restrict__ c2 = reinterpret_cast<const int2*>(cols + base) + lane;
      acc = row_sum_gh<NT>(npair, v2, c2, x, gh.ghost - gh.n_own, (int)gh.n_own, acc);
    } else if (dl[0] != INT32_MIN) {  // wave-uniform (scalar load)
      acc = row_sum_regular<NT>(npair, v2, dl, x + row, acc);
    } else if (dl[1] == 1) {   // 16-bit column deltas (the clamped row of a lane beyond n_rows still addresses valid entries)
      const int* __restrict__ c16 = reinterpret_cast<const int*>(cols16) + (base >> 1) + lane;
      acc = row_sum_short<NT>(npair, v2, c16, x + row, acc);
    } else {
      const int2* __restrict__ c2 = reinterpret_cast<const int2*>(cols + base) + lane;
      acc = row_sum<NT>(npair, v2, c2, x, acc);
    }
    if (row < n_rows) {
      y[row] = acc;
      if (DOT == 4) {
        dot += acc * xr;
        dot2 += acc * acc;
        dot3 += acc * dvec[row];
      } else {
        if (DOT) dot += acc * (dvec ? dvec[row] : xr);
        if (DOT == 2) dot2 += xr * xr;
        if (DOT == 3) dot2 += acc * acc;
      }
    }
  }
  if (DOT) {
    const double s = femo_block_sum<FEMO_BLOCK>(dot, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
  }
  if (DOT >= 2) {
    const double s = femo_block_sum<FEMO_BLOCK>(dot2, lds);
    if (threadIdx.x == 0) partials[FEMO_MAX_PARTIALS + blockIdx.x] = s;
  }
  if (DOT == 4) {
    const double s = femo_block_sum<FEMO_BLOCK>(dot3, lds);
    if (threadIdx.x == 0) partials[2 * FEMO_MAX_PARTIALS + blockIdx.x] = s;
  }
}

// Newton right-hand side of a LINEAR form from its assembled operator (femo_newton_rhs_linear): the product K x of
// k_spmv_sell<0, false> -- same slice walk, same three slice classes, same order of accumulation -- with the rest of the
// right-hand side in its epilogue:  y_i = (K x)_i - load_i  outside the Dirichlet set,  y_i = u_i - g_i  on it
// (bcmask == null: no set, y = K x - load).  x is u with the prescribed values imposed, so that K x carries the lifting.
// A kernel of its own, not a further flag of k_spmv_sell: the CG loop's instantiations keep their registers.
// run_if != null (Newton's flag, round 18): y already holds this very right-hand side unless *run_if is set -- the launch
// leaves as the loop kernels leave on `done`; workgroup 0 counts the launches that left (count[0]) and that ran (count[1]).
template <bool NT>
__global__ __launch_bounds__(FEMO_BLOCK) void k_spmv_sell_rhs(
    int64_t n_rows, int64_t n_slices, const int64_t* __restrict__ mptr,
    const int32_t* __restrict__ cols, const int16_t* __restrict__ cols16, const int32_t* __restrict__ sdelta, int sdelta_stride,
    const double* __restrict__ vals, const double* __restrict__ diag, const double* __restrict__ x,
    const double* __restrict__ u, const double* __restrict__ load, const uint8_t* __restrict__ bcmask,
    const double* __restrict__ bcval, double* __restrict__ y, int64_t slice0, const int32_t* __restrict__ run_if,
    int32_t* __restrict__ count) {
  if (run_if != nullptr) {
    const bool leave = *run_if == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(count + (leave ? 0 : 1), 1);
    if (leave) return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int xcd = blockIdx.x & 7;                    // (XCD-aware walk: see k_spmv_sell)
  const int64_t blk_in_xcd = blockIdx.x >> 3;
  const int64_t waves_per_xcd = (int64_t)(gridDim.x >> 3) * (FEMO_BLOCK / 64);
  // the n_slices slices from slice0 on: all of them, or a range of the streamed head (the XCD eighths are those of the range)
  const int64_t s_lo = slice0 + n_slices * xcd / 8, s_hi = slice0 + n_slices * (xcd + 1) / 8;
  for (int64_t slice = s_lo + blk_in_xcd * (FEMO_BLOCK / 64) + wave; slice < s_hi; slice += waves_per_xcd) {
    const int64_t base = mptr[slice];
    const int npair = (int)((mptr[slice + 1] - base) >> 7);
    const int64_t row = (slice << 6) + lane;
    const int64_t rc = row < n_rows ? row : 0;       // lanes beyond n_rows compute on row 0 and store nothing
    const double xr = x[rc];
    double acc = diag[row] * xr;
    const double2* __restrict__ v2 = reinterpret_cast<const double2*>(vals + base) + lane;
    const int32_t* __restrict__ dl = sdelta + slice * sdelta_stride;
    if (dl[0] != INT32_MIN) {  // wave-uniform (scalar load)
      acc = row_sum_regular<NT>(npair, v2, dl, x + row, acc);
    } else if (dl[1] == 1) {   // 16-bit column deltas
      const int* __restrict__ c16 = reinterpret_cast<const int*>(cols16) + (base >> 1) + lane;
      acc = row_sum_short<NT>(npair, v2, c16, x + row, acc);
    } else {
      const int2* __restrict__ c2 = reinterpret_cast<const int2*>(cols + base) + lane;
      acc = row_sum<NT>(npair, v2, c2, x, acc);
    }
    if (row < n_rows) {
      const bool on_set = bcmask != nullptr && bcmask[row];
      y[row] = on_set ? u[row] - bcval[row] : acc - load[row];
    }
  }
}

// y += A^T x by scatter (partitioned, structurally non-symmetric-valued operators): the transposed entry of a
// ghost column lives in a row of another rank, so the explicit transposed values cannot be formed locally.
// Row i adds a_ij x_i to y_j for all its entries, ghost columns included; the ghost tail of y then travels back
// to the owners, who add it (femo_halo_reverse_add: SURVEY.md section 8(e) "reverse halo scatter-add").  Scattered
// fp64 atomics are slow; this is the correctness path of the unsymmetric-Nitsche adjoint
// on N > 1, not a benchmark path.  y[0:n_vert] must be zero on entry.
template <bool UNIT>
__global__ __launch_bounds__(FEMO_BLOCK) void k_spmv_sell_T_scatter(int64_t n_rows, int64_t n_slices, const int64_t* __restrict__ mptr,
                                                                    const int32_t* __restrict__ cols, const int32_t* __restrict__ rowlen,
                                                                    const double* __restrict__ vals, const double* __restrict__ diag,
                                                                    const double* __restrict__ x, double* __restrict__ y,
                                                                    const int32_t* __restrict__ done) {
  if (done != nullptr && *done) return;
  const int64_t row = (int64_t)blockIdx.x * FEMO_BLOCK + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t base = mptr[row >> 6];
  const int lane = (int)(row & 63), len = rowlen[row];
  const double xi = x[row];
  unsafeAtomicAdd(&y[row], UNIT ? xi : diag[row] * xi);
  for (int k = 0; k < len; ++k) {
    const int64_t e = femo_sell_index(base, k, lane);
    unsafeAtomicAdd(&y[cols[e]], vals[e] * xi);
  }
}

// y[send_idx[i]] += buf[i]
__global__ void k_unpack_add(int64_t n, const int32_t* __restrict__ idx, const double* __restrict__ buf, double* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    unsafeAtomicAdd(&y[idx[i]], buf[i]);       // a vertex can be sent to several neighbours
}

// ------------------------------------------------------------ transposition --
__global__ void k_build_tperm(int64_t n_rows, int64_t n_slices, const int64_t* __restrict__ mptr,
                              const int32_t* __restrict__ cols, const int32_t* __restrict__ rowlen, const uint32_t* __restrict__ rowreal,
                              int32_t* __restrict__ tperm, int32_t* __restrict__ err) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_slices * 64) return;
  const int64_t slice = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t base = mptr[slice];
  const int wm = (int)((mptr[slice + 1] - base) >> 6);
  const int len = rowlen[row];
  for (int k = 0; k < wm; ++k) {
    const int64_t e = femo_sell_index(base, k, lane);
    int32_t t = (int32_t)e;  // padding and structural zeros (completed regular slices) map to themselves (value 0)
    if (k < len && (k >= 32 || ((rowreal[row] >> k) & 1u))) {
      const int64_t j = cols[e];
      if (j >= n_rows) {
        atomicExch(err, 1);  // transposed entry lives on another rank
      } else {
        const int64_t sj = j >> 6;
        const int lj = (int)(j & 63);
        const int64_t bj = mptr[sj];
        const int lenj = rowlen[j];
        int found = -1;
        for (int kk = 0; kk < lenj; ++kk) {
          const int64_t ej = femo_sell_index(bj, kk, lj);
          if (cols[ej] == row) { found = (int)ej; break; }
        }
        if (found < 0) atomicExch(err, 2);  // structurally unsymmetric pattern
        else t = found;
      }
    }
    tperm[e] = t;
  }
}

__global__ void k_gather(int64_t n, const int32_t* __restrict__ perm, const double* __restrict__ in,
                         double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = in[perm[i]];
}

// ------------------------------------------------------------------ scaling --
__global__ void k_invsqrt_diag(int64_t n, const double* __restrict__ diag, double* __restrict__ s) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    s[i] = 1.0 / sqrt(diag[i]);
}

// valsS[row][k] = s[row] * vals[row][k] * s[col]   (one wave per slice)
// PACK: the same pass also writes the compacted copy (femo_mat::d_valsC, d_cdelta, d_cpairs).  In a regular slice a slot is
// dead when the scaled value of all 64 lanes compares == 0.0 (+-0 both; NaN is live); the live slots go to the front of the
// slice's block of outC in their order, pair-interleaved as in `out` (position p at base + (p >> 1) * 128 + lane * 2 + (p & 1)),
// their deltas to cdelta; an odd count is padded with value 0.0 and delta 0 (the padding convention of the topology).  Every
// other slice is copied verbatim, its sdelta row with its flags too.  count[0..2] += live pairs, full pairs, regular slices
// (count[3]: waves that are through); hcount[0..2] receive the totals.
template <bool PACK>
__global__ __launch_bounds__(FEMO_BLOCK) void k_scale_sell(int64_t n_slices, const int64_t* __restrict__ mptr,
                                                           const int32_t* __restrict__ cols, const int32_t* __restrict__ sdelta,
                                                           int sdelta_stride, const double* __restrict__ vals,
                                                           const double* __restrict__ s, int64_t n_vert, double* __restrict__ out,
                                                           double* __restrict__ outC, int32_t* __restrict__ cdelta,
                                                           int32_t* __restrict__ cpairs, unsigned long long* __restrict__ count,
                                                           unsigned long long* __restrict__ hcount) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (FEMO_BLOCK / 64);
  unsigned long long n_live = 0, n_full = 0, n_reg = 0;       // of this wave's slices (wave-uniform)
  for (int64_t slice = (int64_t)blockIdx.x * (FEMO_BLOCK / 64) + (threadIdx.x >> 6); slice < n_slices; slice += nw) {
    const int64_t base = mptr[slice];
    const int wm = (int)((mptr[slice + 1] - base) >> 6);
    const int64_t row = (slice << 6) + lane;
    const double si = s[row < n_vert ? row : 0];
    const int32_t* dl = sdelta + slice * sdelta_stride;
    const bool regular = dl[0] != INT32_MIN;
    int32_t* cd = PACK ? cdelta + slice * sdelta_stride : nullptr;
    int p = 0;                 // live slots so far (wave-uniform)
    double2 pend;              // the pair being filled
    pend.x = 0.0; pend.y = 0.0;
    for (int k = 0; k < wm; k += 2) {
      const int64_t idx = base + (int64_t)(k >> 1) * 128 + lane * 2;
      const double2 v = *reinterpret_cast<const double2*>(vals + idx);
      int64_t c0, c1;
      if (regular) { c0 = row + dl[k]; c1 = row + dl[k + 1]; }
      else { const int2 cc = *reinterpret_cast<const int2*>(cols + idx); c0 = cc.x; c1 = cc.y; }
      double2 o;
      o.x = si * v.x * s[c0];
      o.y = si * v.y * s[c1];
      *reinterpret_cast<double2*>(out + idx) = o;
      if (PACK) {
        if (!regular) {
          *reinterpret_cast<double2*>(outC + idx) = o;
        } else {
          // a slot at a time; `live` and p are wave-uniform, so each `if` is one branch of the whole wave
          if (__ballot(!(o.x == 0.0)) != 0ull) {
            if (p & 1) { pend.y = o.x; *reinterpret_cast<double2*>(outC + base + (int64_t)(p >> 1) * 128 + lane * 2) = pend; }
            else pend.x = o.x;
            if (lane == 0) cd[p] = dl[k];
            ++p;
          }
          if (__ballot(!(o.y == 0.0)) != 0ull) {
            if (p & 1) { pend.y = o.y; *reinterpret_cast<double2*>(outC + base + (int64_t)(p >> 1) * 128 + lane * 2) = pend; }
            else pend.x = o.y;
            if (lane == 0) cd[p] = dl[k + 1];
            ++p;
          }
        }
      }
    }
    if (PACK) {
      if (regular) {
        if (p & 1) {           // odd: the last half is padding (value 0.0, delta 0: the row itself)
          pend.y = 0.0;
          *reinterpret_cast<double2*>(outC + base + (int64_t)(p >> 1) * 128 + lane * 2) = pend;
          if (lane == 0) cd[p] = 0;
          ++p;
        }
        for (int i = p + lane; i < sdelta_stride; i += 64) cd[i] = 0;
        ++n_reg;
      } else {
        for (int i = lane; i < sdelta_stride; i += 64) cd[i] = dl[i];
        p = wm;
      }
      if (lane == 0) cpairs[slice] = p >> 1;
      n_live += (unsigned long long)(p >> 1);
      n_full += (unsigned long long)(wm >> 1);
    }
  }
  if (PACK && lane == 0) {
    if (n_live) atomicAdd(count, n_live);
    if (n_full) atomicAdd(count + 1, n_full);
    if (n_reg) atomicAdd(count + 2, n_reg);
    // the wave that finishes last hands the totals to the host's copy (pinned memory: no copy is enqueued, so nothing of
    // this queues behind an upload) and leaves the device counters at zero for the next build
    __threadfence();
    if (atomicAdd(count + 3, 1ull) == (unsigned long long)gridDim.x * (FEMO_BLOCK / 64) - 1ull) {
      __threadfence();
      for (int i = 0; i < 3; ++i)
        __hip_atomic_store(hcount + i, atomicExch(count + i, 0ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      atomicExch(count + 3, 0ull);
    }
  }
}

__global__ void k_pack(int64_t n, const int32_t* __restrict__ idx, const double* __restrict__ x, double* __restrict__ buf) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) buf[i] = x[idx[i]];
}

}  // namespace

int femo_spmv_grid(const femo_mesh* m) {
  int64_t g = (m->n_slices + 3) / 4;           // one slice per wave if the mesh is small
  const int64_t cap = (int64_t)m->ctx->n_cu * 4;  // 4 x 256 threads resident per CU (~100 VGPRs)
  if (g > cap) g = cap;
  if (g > FEMO_MAX_PARTIALS) g = FEMO_MAX_PARTIALS;
  g = (g + 7) & ~int64_t(7);                   // whole XCD groups
  if (g < 8) g = 8;
  return (int)g;
}

// grid of a product over a subset of n_walk slices (same rules as femo_spmv_grid)
static int subset_grid(const femo_mesh* m, int64_t n_walk) {
  return (int)std::min<int64_t>(femo_spmv_grid(m), std::max<int64_t>(8, ((n_walk + 3) / 4 + 7) & ~int64_t(7)));
}

// streaming hint on the matrix loads only where the stored values cannot stay in the Infinity Cache between two products
static bool matrix_streams(const femo_mesh* m) {
  return (int64_t)m->sell_entries * (int64_t)sizeof(double) > FEMO_LLC_MATRIX_BYTES;
}

int femo_launch_spmv(const femo_mat* A, const double* x, double* y, const FemoSpmv& d) {
  const femo_mesh* m = A->mesh;
  FEMO_REQUIRE(d.dots == FEMO_DOTS_NONE || d.partials != nullptr, "product with dots: no partials to write them to");
  FEMO_REQUIRE(d.dots <= FEMO_DOTS_DAX || d.unit, "product with dots %d: unit-diagonal operators only", (int)d.dots);
  FEMO_REQUIRE(d.dots != FEMO_DOTS_TRIPLE || d.dvec != nullptr, "product with the merged triple: no dvec");
  FEMO_REQUIRE(!d.ghost || (d.dots == FEMO_DOTS_TRIPLE && d.unit && d.slices), "ghost-aware product: merged-loop variant only");
  const int64_t n_walk = d.slices ? d.n_slices : m->n_slices;
  if (n_walk == 0 && d.dots == FEMO_DOTS_NONE) return 0;
  const int g = d.slices ? subset_grid(m, n_walk) : femo_spmv_grid(m);
  hipStream_t st = d.stream ? d.stream : m->ctx->stream;
  // The one place that decides for the compacted copy of S A S: a product on d_valsS over all slices of a mesh without
  // ghosts, while the copy describes the values as they stand.  Slice lists, the ghost-aware walk, the transposed scatter
  // and the products on K keep the full array.
  const bool compact = d.vals == A->d_valsS && d.unit && A->scaled_valid && A->compact_valid && d.slices == nullptr && !d.ghost;
  const double* vals = compact ? A->d_valsC : d.vals;
  const int32_t* cdelta = compact ? A->d_cdelta : nullptr;
  const int32_t* cpairs = compact ? A->d_cpairs : nullptr;
  if (d.vals == A->d_valsS) ++(compact ? A->products_compact : A->products_full);
#define FEMO_SPMV_ARGS m->n_rows, m->n_slices, m->d_mptr, m->d_cols, m->d_cols16, m->d_sdelta, m->sdelta_stride, vals, A->d_diag, x, y, d.partials, d.done, d.slices, d.n_slices, d.dvec, cdelta, cpairs
  const bool nt = matrix_streams(m);
#define FEMO_SPMV_LAUNCH(DOT, UNIT)                                                                                     \
  do {                                                                                                                  \
    if (compact) {                                                                                                      \
      if (nt) hipLaunchKernelGGL((k_spmv_sell<DOT, true, true, false, true>), dim3(g), dim3(FEMO_BLOCK), 0, st, FEMO_SPMV_ARGS);   \
      else hipLaunchKernelGGL((k_spmv_sell<DOT, true, false, false, true>), dim3(g), dim3(FEMO_BLOCK), 0, st, FEMO_SPMV_ARGS);     \
    } else if (nt) hipLaunchKernelGGL((k_spmv_sell<DOT, UNIT, true>), dim3(g), dim3(FEMO_BLOCK), 0, st, FEMO_SPMV_ARGS);  \
    else hipLaunchKernelGGL((k_spmv_sell<DOT, UNIT, false>), dim3(g), dim3(FEMO_BLOCK), 0, st, FEMO_SPMV_ARGS);          \
  } while (0)
  switch (d.dots) {
    case FEMO_DOTS_NONE:
      if (d.unit) FEMO_SPMV_LAUNCH(FEMO_DOTS_NONE, true);
      else FEMO_SPMV_LAUNCH(FEMO_DOTS_NONE, false);
      break;
    case FEMO_DOTS_DAX:
      if (d.unit) FEMO_SPMV_LAUNCH(FEMO_DOTS_DAX, true);
      else FEMO_SPMV_LAUNCH(FEMO_DOTS_DAX, false);
      break;
    case FEMO_DOTS_DAX_XX: FEMO_SPMV_LAUNCH(FEMO_DOTS_DAX_XX, true); break;
    case FEMO_DOTS_DAX_AXAX: FEMO_SPMV_LAUNCH(FEMO_DOTS_DAX_AXAX, true); break;
    case FEMO_DOTS_TRIPLE:
      if (d.ghost) {                                      // the merged loop's one launch over [interior | boundary] slices
        const FemoHaloDirect* h = m->hd;
        SpmvGhost gh;
        gh.cnt = h->counters; gh.blocks = h->d_blocks; gh.n_nbr = m->n_nbr; gh.epoch = h->loop_epoch; gh.err = h->d_err;
        gh.ghost = h->inbox + (int64_t)(h->loop_epoch & 1ull) * h->n_ghost; gh.n_own = m->n_rows;
        if (nt) hipLaunchKernelGGL((k_spmv_sell<FEMO_DOTS_TRIPLE, true, true, true>), dim3(g), dim3(FEMO_BLOCK), 0, st, FEMO_SPMV_ARGS, gh);
        else hipLaunchKernelGGL((k_spmv_sell<FEMO_DOTS_TRIPLE, true, false, true>), dim3(g), dim3(FEMO_BLOCK), 0, st, FEMO_SPMV_ARGS, gh);
      } else {
        FEMO_SPMV_LAUNCH(FEMO_DOTS_TRIPLE, true);
      }
      break;
  }
#undef FEMO_SPMV_LAUNCH
#undef FEMO_SPMV_ARGS
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_halo_raw(femo_mesh* m, double* x, hipStream_t st) {
  femo_vec v;
  v.ctx = m->ctx; v.d = x; v.n = m->n_vert; v.owned = false;
  return femo_halo_exchange_on(m, &v, st);
}

// The two launches over the interior and the boundary slice lists; the caller puts what the second has to wait for
// between them
static FemoSpmv slice_part(const femo_mesh* m, const FemoSpmv& d, bool bnd) {
  FemoSpmv part = d;
  part.slices = bnd ? m->d_slices_bnd : m->d_slices_int;
  part.n_slices = bnd ? m->n_bnd : m->n_int;
  part.stream = m->ctx->stream;
  if (bnd && d.partials) part.partials = d.partials + femo_spmv_bnd_slots(d.dots) * FEMO_MAX_PARTIALS;
  return part;
}

// Ghost refresh of x overlapped with the interior rows of y = A x (nranks > 1):
//   comm stream : pack + grouped ncclSend/ncclRecv into the ghost tail of x
//   main stream : SpMV over the slices without ghost columns, then (after the halo
//                 event) over the slices that read ghosts.
// Partials (if requested) land in two places: interior at d.partials, boundary femo_spmv_bnd_slots(d.dots) slots further
// on; *g_int / *g_bnd return the block counts to fold.
static int halo_spmv_overlapped(const femo_mat* A, double* x, double* y, const FemoSpmv& d, int* g_int, int* g_bnd) {
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->stream, cs = ctx->comm_stream;
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev_main, st));
  FEMO_HIP_CHECK(hipStreamWaitEvent(cs, ctx->ev_main, 0));
  FEMO_TRY(femo_halo_raw(m, x, cs));
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev_comm, cs));
  if (g_int) *g_int = subset_grid(m, m->n_int);
  if (g_bnd) *g_bnd = subset_grid(m, m->n_bnd);
  FEMO_TRY(femo_launch_spmv(A, x, y, slice_part(m, d, false)));
  FEMO_HIP_CHECK(hipStreamWaitEvent(st, ctx->ev_comm, 0));
  return femo_launch_spmv(A, x, y, slice_part(m, d, true));
}

// The same product when the ghost refresh of x is ALREADY in flight on the communication stream (the merged BPX-PCG's
// prolongation started it, femo_pc_merged_apply): interior slices now, boundary slices behind the halo event.
static int halo_spmv_inflight(const femo_mat* A, double* x, double* y, const FemoSpmv& d, int* g_int, int* g_bnd) {
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->stream;
  if (femo_halo_direct_ready(m) && m->d_slices_all != nullptr && d.dots == FEMO_DOTS_TRIPLE && d.unit && d.partials != nullptr) {
    // round 6: ONE launch.  Interior slices first in every XCD's range, the slices with ghost columns behind them; their
    // waves wait for the neighbours' counters and read the ghosts from this rank's inbox (k_spmv_sell<.., GH = true>).
    if (ctx->emu != nullptr) FEMO_TRY(femo_emu_rendezvous(ctx, st));       // (emulated ranks meet on the host, halo_direct.hip)
    if (g_int) *g_int = femo_spmv_grid(m);
    if (g_bnd) *g_bnd = 0;
    FemoSpmv all = d;
    all.slices = m->d_slices_all; all.n_slices = m->n_slices; all.stream = st; all.ghost = true;
    return femo_launch_spmv(A, x, y, all);
  }
  if (g_int) *g_int = subset_grid(m, m->n_int);
  if (g_bnd) *g_bnd = subset_grid(m, m->n_bnd);
  FEMO_TRY(femo_launch_spmv(A, x, y, slice_part(m, d, false)));
  if (femo_halo_direct_ready(m)) {
    // device-initiated refresh (round 6): the neighbours' prolongations stored the new direction into this rank's inbox
    // while the interior slices were multiplied; one small launch of the SAME stream waits for their counters and moves
    // the generation into the ghost tail -- no second stream, no event
    FEMO_TRY(femo_halo_direct_pull(m, m->hd->loop_epoch, x + m->n_rows, st));
  } else {
    FEMO_HIP_CHECK(hipStreamWaitEvent(st, ctx->ev_comm, 0));
  }
  return femo_launch_spmv(A, x, y, slice_part(m, d, true));
}

int femo_halo_spmv(const femo_mat* A, double* x, double* y, const FemoSpmv& d, int* g_int, int* g_bnd, bool inflight) {
  femo_mesh* m = A->mesh;
  if (inflight) return halo_spmv_inflight(A, x, y, d, g_int, g_bnd);
  if (m->n_nbr > 0 && m->d_slices_int != nullptr) return halo_spmv_overlapped(A, x, y, d, g_int, g_bnd);
  if (g_int) *g_int = femo_spmv_grid(m);
  if (g_bnd) *g_bnd = 0;
  if (m->n_nbr > 0) FEMO_TRY(femo_halo_raw(m, x, m->ctx->stream));
  return femo_launch_spmv(A, x, y, d);
}

int femo_launch_spmv(const femo_mat* A, const double* vals, const double* x, double* y, double* partials) {
  return femo_launch_spmv(A, x, y, {.vals = vals, .dots = partials ? FEMO_DOTS_DAX : FEMO_DOTS_NONE, .partials = partials});
}

int femo_launch_newton_rhs_linear(const femo_mat* K, const double* x, const double* u, const double* load,
                                  const uint8_t* bcmask, const double* bcval, double* y, int64_t slice0, int64_t n_range,
                                  const int32_t* run_if, int32_t* count) {
  const femo_mesh* m = K->mesh;
  FEMO_REQUIRE(run_if == nullptr || (n_range < 0 && count != nullptr), "a range of the streamed head takes no flag");
  const int64_t n_walk = n_range >= 0 ? n_range : m->n_slices;
  if (n_walk == 0) return 0;                          // (ranges of zero rows launch nothing)
  FEMO_REQUIRE(slice0 >= 0 && slice0 + n_walk <= m->n_slices, "slice range [%lld, %lld) outside the mesh's %lld slices",
               (long long)slice0, (long long)(slice0 + n_walk), (long long)m->n_slices);
  const int64_t g = n_range >= 0 ? subset_grid(m, n_walk) : femo_spmv_grid(m);
  const bool nt = matrix_streams(m);
#define FEMO_RHS_ARGS m->n_rows, n_walk, m->d_mptr, m->d_cols, m->d_cols16, m->d_sdelta, m->sdelta_stride, K->d_vals, K->d_diag, x, u, load, bcmask, bcval, y, slice0, run_if, count
  if (nt) hipLaunchKernelGGL((k_spmv_sell_rhs<true>), dim3(g), dim3(FEMO_BLOCK), 0, m->ctx->stream, FEMO_RHS_ARGS);
  else hipLaunchKernelGGL((k_spmv_sell_rhs<false>), dim3(g), dim3(FEMO_BLOCK), 0, m->ctx->stream, FEMO_RHS_ARGS);
#undef FEMO_RHS_ARGS
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_mat_ensure_transpose(femo_mat* A) {
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  if (A->valsT_valid) return 0;
  if (m->sell_entries == 0) { A->valsT_valid = true; return 0; }
  if (!m->d_tperm) {
    FEMO_REQUIRE(m->sell_entries < (int64_t(1) << 31), "pattern too large for int32 transpose map");
    FEMO_HIP_CHECK(hipMalloc(&m->d_tperm, m->sell_entries * sizeof(int32_t)));
    FEMO_HIP_CHECK(hipMemsetAsync(ctx->d_flags + 3, 0, sizeof(int32_t), ctx->stream));
    const int64_t nr = m->n_slices * 64;
    hipLaunchKernelGGL(k_build_tperm, dim3((nr + 255) / 256), dim3(256), 0, ctx->stream, m->n_rows, m->n_slices, m->d_mptr, m->d_cols, m->d_rowlen, m->d_rowreal, m->d_tperm, ctx->d_flags + 3);
    FEMO_HIP_CHECK(hipGetLastError());
    int32_t err = 0;
    FEMO_HIP_CHECK(hipMemcpyAsync(&err, ctx->d_flags + 3, sizeof err, hipMemcpyDeviceToHost, ctx->stream));
    FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (err != 0) {
      hipFree(m->d_tperm);
      m->d_tperm = nullptr;
      femo_set_error(err == 1 ? "transposed operator needs entries owned by another rank"
                              : "sparsity pattern is not structurally symmetric");
      return 3;
    }
  }
  if (!A->d_valsT) FEMO_HIP_CHECK(hipMalloc(&A->d_valsT, m->sell_entries * sizeof(double)));
  hipLaunchKernelGGL(k_gather, dim3(2048), dim3(256), 0, ctx->stream, m->sell_entries, m->d_tperm, A->d_vals, A->d_valsT);
  FEMO_HIP_CHECK(hipGetLastError());
  A->valsT_valid = true;
  return 0;
}

// flag[slice] = 1 if any stored column of the slice is a ghost (>= n_rows)
__global__ void k_flag_ghost_slices(int64_t n_rows, int64_t n_slices, const int64_t* __restrict__ mptr,
                                    const int32_t* __restrict__ cols, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t slice = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (slice >= n_slices) return;
  const int64_t base = mptr[slice];
  const int wm = (int)((mptr[slice + 1] - base) >> 6);
  int any = 0;
  for (int k = 0; k < wm; ++k) any |= cols[femo_sell_index(base, k, lane)] >= n_rows;   // padding = own row < n_rows
  const unsigned long long b = __ballot(any);
  if (lane == 0) flag[slice] = b != 0ull;
}

int femo_mesh_classify_slices(femo_mesh* m) {
  femo_ctx* ctx = m->ctx;
  hipFree(m->d_slices_int); hipFree(m->d_slices_bnd);
  m->d_slices_int = m->d_slices_bnd = nullptr;
  m->n_int = m->n_bnd = 0;
  if (m->n_slices == 0) return 0;
  int32_t* d_flag = nullptr;
  FEMO_HIP_CHECK(hipMalloc(&d_flag, m->n_slices * sizeof(int32_t)));
  hipLaunchKernelGGL(k_flag_ghost_slices, dim3((unsigned)((m->n_slices + 3) / 4)), dim3(256), 0, ctx->stream, m->n_rows, m->n_slices, m->d_mptr, m->d_cols, d_flag);
  FEMO_HIP_CHECK(hipGetLastError());
  std::vector<int32_t> flag(m->n_slices), li, lb;
  FEMO_HIP_CHECK(hipMemcpyAsync(flag.data(), d_flag, m->n_slices * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  hipFree(d_flag);
  for (int64_t s = 0; s < m->n_slices; ++s) (flag[s] ? lb : li).push_back((int32_t)s);
  m->n_int = (int64_t)li.size(); m->n_bnd = (int64_t)lb.size();
  FEMO_HIP_CHECK(hipMalloc(&m->d_slices_int, std::max<size_t>(li.size(), 1) * sizeof(int32_t)));
  FEMO_HIP_CHECK(hipMalloc(&m->d_slices_bnd, std::max<size_t>(lb.size(), 1) * sizeof(int32_t)));
  // one list for the single-launch product of the merged loop (round 6): the kernel gives XCD k the k-th eighth of the list;
  // inside every eighth the interior slices come first, the slices with ghost columns (sign bit set) last
  hipFree(m->d_slices_all); m->d_slices_all = nullptr;
  if (!lb.empty() && femo_env_flag("FEMO_SPMV_TWO_LAUNCHES") == false) {
    std::vector<int32_t> all((size_t)m->n_slices);
    size_t w = 0;
    for (int xcd = 0; xcd < 8; ++xcd) {
      const int64_t lo = m->n_slices * xcd / 8, hi = m->n_slices * (xcd + 1) / 8;
      for (int64_t sl = lo; sl < hi; ++sl) if (!flag[(size_t)sl]) all[w++] = (int32_t)sl;
      for (int64_t sl = lo; sl < hi; ++sl) if (flag[(size_t)sl]) all[w++] = (int32_t)sl | (int32_t)0x80000000;
    }
    FEMO_HIP_CHECK(hipMalloc(&m->d_slices_all, all.size() * sizeof(int32_t)));
    FEMO_HIP_CHECK(hipMemcpyAsync(m->d_slices_all, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  if (!li.empty()) FEMO_HIP_CHECK(hipMemcpyAsync(m->d_slices_int, li.data(), li.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  if (!lb.empty()) FEMO_HIP_CHECK(hipMemcpyAsync(m->d_slices_bnd, lb.data(), lb.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return 0;
}

// ---------------------------------------------------------------- halo ------
int femo_halo_exchange_on(femo_mesh* m, femo_vec* x, hipStream_t st) {
  FEMO_REQUIRE(m && x, "null argument");
  if (m->n_nbr == 0) return 0;
  // Nobody has written x since its ghosts were refreshed: they are still the owners' values.  Skipping is SPMD-consistent
  // (every rank runs the same sequence of writes and refreshes) and it keeps host mirrors of x valid: round 5 refreshed u
  // for J, dJ/du, ... after its copy-out, each refresh a new generation, each new generation a real re-upload of the host
  // copy by the next operator call (two blocking PCIe uploads + their waits per cycle and rank, round 6).
  if (x->ghost_gen == x->gen && x->uid != 0 && x->n >= m->n_vert) return 0;
  femo_vec_touch(x);                                  // ghost entries change
  x->ghost_gen = x->gen;
  femo_ctx* ctx = m->ctx;
  FEMO_REQUIRE(ctx->comm != nullptr || ctx->emu != nullptr || ctx->model, "halo exchange before femo_comm_init");
  FEMO_REQUIRE(x->n >= m->n_vert, "vector shorter than n_vert");
  if (femo_halo_direct_ready(m)) return femo_halo_direct_exchange(m, x->d, x->d + m->n_rows, st);   // device-initiated (round 6)
  const int64_t ns = m->send_ptr[m->n_nbr];
  if (ns > 0) {
    hipLaunchKernelGGL(k_pack, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, ns, m->d_send_idx, x->d, m->d_send_buf);
    FEMO_HIP_CHECK(hipGetLastError());
  }
  return femo_coll_neighbors(ctx, m->n_nbr, m->nbr.data(), m->send_ptr.data(), m->d_send_buf, m->recv_ptr.data(),
                             x->d + m->n_rows, st);
}

extern "C" int femo_halo_exchange(femo_mesh* m, femo_vec* x) {
  FEMO_REQUIRE(m && x, "null argument");
  return femo_halo_exchange_on(m, x, m->ctx->stream);
}

// ghost tail of y -> owners, who add it to their entries (the transpose of the ghost refresh)
static int halo_reverse_add(femo_mesh* m, double* y, hipStream_t st) {
  if (m->n_nbr == 0) return 0;
  femo_ctx* ctx = m->ctx;
  FEMO_REQUIRE(ctx->comm != nullptr || ctx->emu != nullptr || ctx->model, "halo exchange before femo_comm_init");
  const int64_t ns = m->send_ptr[m->n_nbr];
  // roles swapped: what this rank receives in a forward exchange (its ghost tail) is what it sends back
  FEMO_TRY(femo_coll_neighbors(ctx, m->n_nbr, m->nbr.data(), m->recv_ptr.data(), y + m->n_rows, m->send_ptr.data(), m->d_send_buf, st));
  if (ns > 0) {
    hipLaunchKernelGGL(k_unpack_add, dim3((unsigned)std::min<int64_t>((ns + 255) / 256, 2048)), dim3(256), 0, st, ns, m->d_send_idx, m->d_send_buf, y);
    FEMO_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// y = A^T x on a partitioned mesh, A given by its own (untransposed) values
int femo_spmv_transposed_scatter(const femo_mat* A, const double* vals, bool unit, const double* x, double* y, const int32_t* done) {
  femo_mesh* m = A->mesh;
  hipStream_t st = m->ctx->stream;
  FEMO_HIP_CHECK(hipMemsetAsync(y, 0, (size_t)m->n_vert * sizeof(double), st));
  if (m->n_rows > 0) {
    const unsigned g = (unsigned)((m->n_rows + FEMO_BLOCK - 1) / FEMO_BLOCK);
    if (unit) hipLaunchKernelGGL((k_spmv_sell_T_scatter<true>), dim3(g), dim3(FEMO_BLOCK), 0, st, m->n_rows, m->n_slices, m->d_mptr, m->d_cols, m->d_rowlen, vals, A->d_diag, x, y, done);
    else hipLaunchKernelGGL((k_spmv_sell_T_scatter<false>), dim3(g), dim3(FEMO_BLOCK), 0, st, m->n_rows, m->n_slices, m->d_mptr, m->d_cols, m->d_rowlen, vals, A->d_diag, x, y, done);
    FEMO_HIP_CHECK(hipGetLastError());
  }
  return halo_reverse_add(m, y, st);
}

// ----------------------------------------------------------------- API ------
extern "C" int femo_mat_spmv(const femo_mat* A, int transpose, const femo_vec* x, femo_vec* y) {
  FEMO_REQUIRE(A && x && y, "null argument");
  femo_mesh* m = A->mesh;
  FEMO_REQUIRE(x->n >= m->n_vert && y->n >= m->n_rows, "vector size mismatch in spmv");
  FEMO_REQUIRE(x->d != y->d, "spmv cannot run in place");
  FEMO_TRY(femo_vec_await(x));             // a deferred upload of x (every reader awaits)
  femo_vec_touch(y);
  const double* vals = A->d_vals;
  if (transpose && !femo_transpose_is_local(m)) {
    FEMO_REQUIRE(y->n >= m->n_vert, "transposed product on a partitioned mesh: y needs room for the ghost contributions");
    return femo_spmv_transposed_scatter(A, A->d_vals, false, x->d, y->d, nullptr);
  }
  if (transpose) {
    FEMO_TRY(femo_mat_ensure_transpose(const_cast<femo_mat*>(A)));
    vals = A->d_valsT;
  }
  if (m->n_nbr > 0) femo_vec_touch(const_cast<femo_vec*>(x));     // its ghost entries are refreshed
  return femo_halo_spmv(A, x->d, y->d, {.vals = vals}, nullptr, nullptr);
}

// S = diag^-1/2 of the current assembly (ghost entries from their owners)
int femo_mat_ensure_s(femo_mat* A) {
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  if (A->s_valid) return 0;
  const int64_t nd = std::max<int64_t>(m->n_vert, m->n_slices * FEMO_WAVE) + 2;
  if (!A->d_s) FEMO_HIP_CHECK(hipMalloc(&A->d_s, nd * sizeof(double)));
  if (m->n_rows > 0) {
    hipLaunchKernelGGL(k_invsqrt_diag, dim3(2048), dim3(256), 0, ctx->stream, m->n_rows, A->d_diag, A->d_s);
    FEMO_HIP_CHECK(hipGetLastError());
  }
  if (m->n_nbr > 0) FEMO_TRY(femo_halo_raw(m, A->d_s, ctx->stream));   // ghost columns need the owner's scale factor
  A->s_valid = true;
  return 0;
}

// ---- the compacted copy of S A S: when it is built -------------------------------------------------------------------
// One rank on a mesh without ghosts (the N-rank products walk slice lists and keep the full array), FEMO_SPMV_COMPACT not
// "0" (read here, once per scaling -- the tests switch it -- never per launch), at least half of the mesh's slices regular
// (only regular slices are packed), and a handle whose gate has not fired.
static bool compact_wanted(const femo_mat* A) {
  const femo_mesh* m = A->mesh;
  if (A->compact_off || m->ctx->nranks > 1 || m->n_nbr > 0 || m->n_slices == 0) return false;
  const char* e = getenv("FEMO_SPMV_COMPACT");
  if (e != nullptr && e[0] == '0' && e[1] == 0) return false;
  return 2 * m->n_regular >= m->n_slices;
}

// first use: the three arrays and the counters.  A device that has no room for a second copy of the values goes on with the
// full one, and the handle does not ask again.
static bool compact_alloc(femo_mat* A) {
  const femo_mesh* m = A->mesh;
  if (A->d_valsC != nullptr) return true;
  const size_t nv = (size_t)std::max<int64_t>(m->sell_entries, 1) * sizeof(double) + 64;
  const size_t nd = (size_t)m->n_slices * (size_t)m->sdelta_stride * sizeof(int32_t);
  const bool ok = hipMalloc(&A->d_valsC, nv) == hipSuccess && hipMalloc(&A->d_cdelta, nd) == hipSuccess &&
                  hipMalloc(&A->d_cpairs, (size_t)m->n_slices * sizeof(int32_t)) == hipSuccess &&
                  hipMalloc(&A->d_ccount, 4 * sizeof(unsigned long long)) == hipSuccess &&
                  hipHostMalloc(&A->h_ccount, 3 * sizeof(unsigned long long)) == hipSuccess &&
                  hipMemsetAsync(A->d_ccount, 0, 4 * sizeof(unsigned long long), m->ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    femo_mat_compact_free(A);
    A->compact_off = true;
  }
  return ok;
}

void femo_mat_compact_free(femo_mat* A) {
  hipFree(A->d_valsC); hipFree(A->d_cdelta); hipFree(A->d_cpairs); hipFree(A->d_ccount);
  if (A->h_ccount) hipHostFree(A->h_ccount);
  A->d_valsC = nullptr; A->d_cdelta = nullptr; A->d_cpairs = nullptr; A->d_ccount = nullptr; A->h_ccount = nullptr;
  A->compact_valid = false; A->compact_pending = false;
}

// The gate.  The rule: a handle whose last build found fewer than one pair in eight dead stops building the compaction, and
// the decision is remembered for the handle (compact_off) -- below that the second write of the values per assembly, as
// large as S A S itself, costs more than the shorter products return in any leg that does not hide it under an upload.
// The build left its counters in pinned host memory; they are looked at here, where the host has just waited for the
// stream anyway (the end of a solve with A), so the gate adds no synchronisation.  Nothing is in flight on the arrays then:
// they are freed.
void femo_mat_compact_settle(femo_mat* A) {
  if (!A->compact_pending) return;
  A->compact_pending = false;
  const unsigned long long live = A->h_ccount[0], full = A->h_ccount[1];
  A->compact_live = (int64_t)live; A->compact_full = (int64_t)full; A->compact_slices = (int64_t)A->h_ccount[2];
  if ((full - live) * 8ull < full) {
    femo_mat_compact_free(A);
    A->compact_off = true;
  }
}

// ... and the scaled values S A S (or S A^T S): what the Krylov loops iterate on.  Kept apart
// from femo_mat_ensure_s because a solve that stops on its initial residual never needs them.
int femo_mat_ensure_scaled(femo_mat* A, bool transpose) {
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  if (A->scaled_valid && A->scaled_transposed == transpose) return 0;
  const double* src = A->d_vals;
  if (transpose) {
    FEMO_TRY(femo_mat_ensure_transpose(A));
    src = A->d_valsT;
  }
  FEMO_TRY(femo_mat_ensure_s(A));
  if (!A->d_valsS) FEMO_HIP_CHECK(hipMalloc(&A->d_valsS, std::max<int64_t>(m->sell_entries, 1) * sizeof(double) + 64));
  A->compact_valid = false;
  const bool pack = compact_wanted(A) && compact_alloc(A);
  if (m->n_slices > 0) {
#define FEMO_SCALE_ARGS m->n_slices, m->d_mptr, m->d_cols, m->d_sdelta, m->sdelta_stride, src, A->d_s, m->n_vert, A->d_valsS
    if (pack) {
      // the packing is redone with every S A S (nothing is kept across assemblies); the kernel leaves the counters of this
      // build in h_ccount, where the end of a solve looks at them (femo_mat_compact_settle)
      hipLaunchKernelGGL((k_scale_sell<true>), dim3(2048), dim3(FEMO_BLOCK), 0, ctx->stream, FEMO_SCALE_ARGS, A->d_valsC, A->d_cdelta, A->d_cpairs, A->d_ccount, A->h_ccount);
      A->compact_pending = true;
      A->compact_valid = true;
    } else {
      hipLaunchKernelGGL((k_scale_sell<false>), dim3(2048), dim3(FEMO_BLOCK), 0, ctx->stream, FEMO_SCALE_ARGS, (double*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
    }
#undef FEMO_SCALE_ARGS
    FEMO_HIP_CHECK(hipGetLastError());
  }
  A->scaled_valid = true;
  A->scaled_transposed = transpose;
  return 0;
}

extern "C" int femo_bench_spmv(const femo_mat* A, const femo_vec* x, femo_vec* y, int reps, double* ms_per_launch) {
  FEMO_REQUIRE(A && x && y && ms_per_launch && reps > 0, "bad argument");
  femo_ctx* ctx = A->mesh->ctx;
  FEMO_REQUIRE(x->n >= A->mesh->n_vert && y->n >= A->mesh->n_rows, "vector size mismatch");
  femo_vec_touch(y);
  // the launch the CG loop issues: scaled operator, unit diagonal, fused p.Ap partials
  FEMO_TRY(femo_mat_ensure_scaled(const_cast<femo_mat*>(A), false));
  const FemoSpmv Ap = {.vals = A->d_valsS, .unit = true, .dots = FEMO_DOTS_DAX, .partials = ctx->d_partials + 3 * FEMO_MAX_PARTIALS};
  for (int i = 0; i < 3; ++i) FEMO_TRY(femo_launch_spmv(A, x->d, y->d, Ap));
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev0, ctx->stream));
  for (int i = 0; i < reps; ++i) FEMO_TRY(femo_launch_spmv(A, x->d, y->d, Ap));
  FEMO_HIP_CHECK(hipEventRecord(ctx->ev1, ctx->stream));
  FEMO_HIP_CHECK(hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  FEMO_HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *ms_per_launch = (double)ms / reps;
  return 0;
}

// ... and the BPX weights of the operator, which depend on S and the pinned vertices only: the 85 us at C4 that stood behind
// the wait for f at the head of a cycle.  One rank, a mesh whose hierarchy a BPX solve has built (a mesh that is only ever
// solved with another preconditioner never has one); otherwise the prescale alone.
extern "C" int femo_mat_prescale(femo_mat* A) {
  FEMO_REQUIRE(A != nullptr, "null argument");
  FEMO_TRY(femo_mat_ensure_scaled(A, false));
  if (!A->bpx_ok) return 0;
  return femo_pc_weights_early(A->mesh, A->d_s, A->pc_has_mask ? A->d_pcmask : nullptr, femo_pc_weights_key(A));
}

// ---- test hooks (include/femo_hip_test.h) ------------------------------------------------------------------------------
extern "C" int femo_mat_compact_info(femo_mat* A, int64_t* out, int count) {
  FEMO_REQUIRE(A && out, "null argument");
  FEMO_HIP_CHECK(hipStreamSynchronize(A->mesh->ctx->stream));
  if (A->compact_pending) {                      // (the counters of the last build have landed; the gate is the solvers')
    A->compact_live = (int64_t)A->h_ccount[0]; A->compact_full = (int64_t)A->h_ccount[1]; A->compact_slices = (int64_t)A->h_ccount[2];
  }
  const int64_t v[6] = {(A->scaled_valid && A->compact_valid) ? 1 : 0, A->compact_slices, A->compact_live, A->compact_full,
                        A->products_compact, A->products_full};
  for (int i = 0; i < 6 && i < count; ++i) out[i] = v[i];
  return 0;
}

extern "C" int femo_mat_spmv_scaled(femo_mat* A, int dots, const femo_vec* x, femo_vec* y, double* partials, int* nblocks) {
  FEMO_REQUIRE(A && x && y, "null argument");
  FEMO_REQUIRE(dots >= FEMO_DOTS_NONE && dots <= FEMO_DOTS_DAX_AXAX, "dots %d: 0 .. 3", dots);
  FEMO_REQUIRE(dots == FEMO_DOTS_NONE || (partials && nblocks), "product with dots: no room for the partials");
  femo_mesh* m = A->mesh;
  femo_ctx* ctx = m->ctx;
  FEMO_REQUIRE(m->n_nbr == 0, "one rank only");
  FEMO_REQUIRE(x->n >= m->n_vert && y->n >= m->n_rows && x->d != y->d, "vector size mismatch");
  FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(y);
  FEMO_TRY(femo_mat_ensure_scaled(A, false));
  double* P = ctx->d_partials + 3 * FEMO_MAX_PARTIALS;
  FEMO_TRY(femo_launch_spmv(A, x->d, y->d, {.vals = A->d_valsS, .unit = true, .dots = (FemoSpmvDots)dots, .partials = dots ? P : nullptr}));
  const int g = femo_spmv_grid(m);
  for (int k = 0; k < femo_spmv_dot_slots((FemoSpmvDots)dots); ++k)
    FEMO_HIP_CHECK(hipMemcpyAsync(partials + (size_t)k * g, P + (size_t)k * FEMO_MAX_PARTIALS, (size_t)g * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (nblocks) *nblocks = g;
  return 0;
}
