// Reissner-Mindlin shell, CG2^3 x CG1^3 on flat triangular facets (BASELINE config 3;
// replaces what examples/test_shell_m3l/shell_pde.py:219-332 obtains from shell_analysis_fenicsx + dolfinx + MUMPS).
// The formulation is restated and pinned in oracle/shell_oracle.py (Scordelis-Lo, Kirchhoff plate, rigid modes);
// the kernels are checked against it entry by entry (tests/test_gpu_shell.py).
//
// This header is what the four shell units share: the handle, the view the kernels take, the few constants and host
// helpers more than one unit uses, and the host functions that cross units.  A kernel is launched only from the unit
// that defines it; each unit frees the device arrays it allocates (shell_*_free, called by femo_shell_destroy).
//   shell_forms.hip   element kernels of the forms and outputs and their entry points
//   shell_solve.hip   operator products, CG kernels and loop, partition and halo, create / destroy
//   shell.hip         lattice preconditioner: transfers and levels of both spaces, node and point blocks, set-up, apply
//                     (it stays in place under the old name: the other three units are what moved out of it)
//   shell_coarse.hip  dense coarse operator: Galerkin kernels, tiled Cholesky, triangular inverse, its two products
//
// What they do (DESIGN.md section 8 has the measurements and the versions that came before):
//   * degrees of freedom and the CSR pattern of the 27 x 27 element couplings are built on the host (Python,
//     femo_amd/fea/shell.py) and handed over as plain arrays, with the CSR position of every element entry;
//   * assembly: one thread per (cell, element column) forms the column from the facet frame and the quadrature
//     points in registers (B^T D B, nine strain rows) and adds its 27 entries with fp64 atomics;
//   * operator: the three dofs of a node share their columns, so the matrix is read as 3 x 3 blocks -- straight from
//     the CSR values (k_bcsr3_spmv) or, in the CG loop, from a block-SELL copy (k_bsell_spmv);
//   * solve: CG with device-side scalars (consumers fold the producers' per-block partials, the host polls a flag)
//     and a nested-lattice preconditioner: 3 x 3 point blocks of K as the smoother, 6 x 6 Galerkin node blocks on the
//     lattice levels, an exact dense solve (Galerkin operator formed on the device, blocked Cholesky on the fp64 matrix
//     cores) on the coarsest level kept -- 252 iterations at 1.97 M dofs where Jacobi needs ~1e5;
//   * partials and outputs: (dR/dh)^T lambda element by element from the strains of w and lambda, load and its
//     transpose, compliance, mass, elastic energy, the aggregated von Mises stress and its projection onto the vertices.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "femo_internal.h"

struct femo_shell {
  femo_ctx* ctx = nullptr;
  int64_t n_vert = 0, n_cell = 0, n_edge = 0, n_unode = 0, n_dof = 0, nnz = 0;
  double* d_x = nullptr;
  int32_t *d_conn = nullptr, *d_cedge = nullptr, *d_cols = nullptr, *d_epos = nullptr;
  int64_t* d_rowptr = nullptr;
  // node-block view of the pattern (dofs 3 b .. 3 b + 2 of a node share their columns, which come in runs of three):
  // block-row offsets and the first scalar column of every 3 x 3 block; nullptr if the pattern is not of that shape
  int64_t n_bnode = 0;
  int64_t* d_brow = nullptr;
  int32_t* d_bcols = nullptr;
  // block-SELL-16 copy of the matrix for the CG loop (k_bsell_spmv): slices of 16 consecutive block rows, per slice
  // and block slot the 16 column indices and the 9 x 16 values component by component (lane = block row)
  int64_t n_bslice = 0, bsell_blocks = 0;               // slices, 16-block groups (= sum of slots over slices)
  int64_t* d_bs_off = nullptr;                          // first 16-block group of every slice (n_bslice + 1)
  int32_t* d_bs_cols = nullptr;
  double* d_bs_vals = nullptr;
  uint64_t bs_vals_uid = 0, bs_vals_gen = 0;            // the stiffness the copy was made from
  // CG workspace
  double *d_r = nullptr, *d_p = nullptr, *d_q = nullptr, *d_dinv = nullptr, *d_scal = nullptr, *d_part = nullptr;
  int32_t* d_flag = nullptr;
  // lattice preconditioner (femo_shell_pc_create): P in ELL form (8 trilinear weights per level and dof), P^T as CSR
  int pc_width = 0, pc_levels = 0;
  int64_t n_lat = 0, pc_nodes = 0;
  std::vector<int64_t> level_off;                       // node offsets of the levels (pc_levels + 1 entries)
  int32_t *d_ell_idx = nullptr, *d_par_cols = nullptr, *d_chi_cols = nullptr;
  double *d_ell_w = nullptr, *d_par_vals = nullptr, *d_chi_vals = nullptr;
  double *d_coarse = nullptr, *d_t = nullptr, *d_e = nullptr, *d_z = nullptr;
  double* d_cblk = nullptr;                             // 6 x 6 inverse Galerkin blocks of the nodes above the coarse-solve level
  int32_t* d_lvl_node = nullptr;                        // levels above the coarse solve, per level and POINT: the eight lattice
  double* d_lvl_w = nullptr;                            // nodes and weights, contiguous ([level][point][8]; the ELL rows interleave
                                                        // all levels of a dof: 3 cache lines per access, 52 GB fetched by the
                                                        // node-block kernel at 1.97 M dofs)
  bool blk_ready = false;
  float* d_dinv3 = nullptr;                             // 3 x 3 inverse diagonal blocks of the points (finest-level smoother), single
                                                        // precision: a smoother rounded at 6e-8 is as good a smoother, products and sums stay fp64
                                                        // (round 3: 72 -> 36 bytes per point in both kernels that read it, every iteration)
  bool dinv3_ready = false;
  int32_t* d_fin_idx = nullptr;                         // the finest level's eight (unknown, weight) pairs per POINT (a P2 node's
  float* d_fin_w = nullptr;                             // three displacements / a vertex's three rotations share them); single
                                                        // precision like d_ptp_vals -- the same rounded numbers in both directions, so M^-1 stays symmetric
  int64_t* d_ptp_rowptr = nullptr;                      // P_L^T by (finest lattice node, field group): points and weights
  int32_t* d_ptp_cols = nullptr;
  float* d_ptp_vals = nullptr;
  int64_t *d_par_rowptr = nullptr, *d_chi_rowptr = nullptr;
  uint64_t pc_vals_uid = 0, pc_vals_gen = 0, pc_mask_hash = 0;     // what d_coarse was computed for
  // exact coarse solve (femo_shell_pc_coarse): on level cs_level the Galerkin operator P^T K P is formed as a dense
  // matrix, factorised (blocked Cholesky + triangular inverse, below) and A^-1 = L^-T L^-1 applied in place of the
  // diagonal levels 0 .. cs_level
  int cs_level = -1;
  int64_t cs_n = 0, cs_N = 0, cs_items = 0;            // unknowns of the level (6 x nodes), padded to 64s, items of the Galerkin kernel
  int64_t cs_max_item = 0;                             // points of the largest item
  bool cs_ready = false;                               // d_cs_A holds the factors of the inverse for the current stiffness and mask
  int64_t* d_cd_rowptr = nullptr;                      // composite restriction finest lattice -> levels cs_level .. L - 2
  int32_t* d_cd_cols = nullptr;
  double* d_cd_vals = nullptr;
  int32_t *d_cs_xyz = nullptr, *d_cs_pts = nullptr, *d_cs_nbr = nullptr, *d_cs_info = nullptr, *d_cs_pcell = nullptr;
  int64_t* d_cs_ptr = nullptr;
  double *d_cs_A = nullptr, *d_cs_tmp = nullptr;       // L^-T above / L^-1 below the diagonal (row-major, N x N); L^-1 g
  float* d_cs_Af = nullptr;                            // the same factors in single precision: what the iteration applies
  double* d_cs_dinv = nullptr;                         // inverses of the diagonal tiles of L
  double* d_cs_T = nullptr;                            // scratch of the level-wise triangular inversion (N x N)
  // Hermite-type lattice spaces (femo_shell_pc_hermite; used when the coarse solve and the node blocks are ready, else the
  // trilinear data above takes over): finest transfer weights per (point, corner), P_L^T rows per finest node (displacement
  // points, then rotation points), (a, b, c) of the node-level transfers, composed weights of the levels above the
  // coarse solve ([level][point][8], finest included) and of the coarse-solve level, composite restriction
  bool hermite = false, hermite_on = false;             // enabled (uploaded and not fallen back) / in use for the current stiffness
  bool hermite_loaded = false;                          // the device arrays exist (guards a second upload; survives a fallback)
  // Weight of the node-block levels in the additive sum (round 4).  The levels between the coarse solve and the finest
  // lattice overlap each other and the point-block smoother; summed with weight 1 they overshoot (the same reason the
  // Poisson BPX carries theta = 0.6).  Measured on the roof, iterations per solve for weights 1 / 0.5 / 0.3 / 0.25 / 0.12:
  // 362^2 (three block levels) 145 / 113 / 105 / 105 / 118, 256^2 118 / 107 / 104 / 102, 128^2 (two) 113 / 103 / 101 / 101,
  // 64^2 (one) 104 / 100 / 101 / 101; trilinear spaces at 362^2: 252 / 205 / 200.  A weight on the coarse solve (0.7, 2, 4)
  // or per-level weights change nothing beyond that.
  double w_levels = 0.3, w_coarse = 1.0;
  // items of k_pc_galerkin_blocks_w (femo_shell_pc_block_items): points grouped by (level above the coarse solve, cell)
  int64_t bi_items = 0;
  int64_t* d_bi_ptr = nullptr;
  int32_t *d_bi_lvl = nullptr, *d_bi_pts = nullptr, *d_bi_pcell = nullptr;
  uint8_t* d_fixbits = nullptr;
  // the Dirichlet mask of the last solve on the device, kept while the caller's array hashes the same (round 5: a solve used
  // to allocate, upload and free it, and to hash it byte by byte for the preconditioner's cache: 3 ms of idle device per solve)
  uint8_t* d_fixed_kept = nullptr;
  uint64_t fixed_kept_hash = 0;
  float4* d_fin_w4 = nullptr;
  int64_t* d_hp_rowptr = nullptr;
  int32_t* d_hp_cols = nullptr;
  float4* d_hp_w4 = nullptr;
  double *d_par_w5 = nullptr, *d_chi_w5 = nullptr;
  float4 *d_lvl_w4 = nullptr, *d_cs_w4 = nullptr;
  int64_t* d_hd_rowptr = nullptr;
  int32_t* d_hd_cols = nullptr;
  double* d_hd_w5 = nullptr;
  // penalty boundary terms (femo_shell_set_penalty): tagged edges, their coefficient and the CSR positions of their entries
  int64_t pen_n = 0;
  int32_t *d_pen_nodes = nullptr, *d_pen_pos = nullptr;
  double* d_pen_coef = nullptr;
  // partition (femo_shell_set_partition): this handle holds the cells that touch a point the rank
  // owns.  d_owned flags the owned points (dofs 3 p .. 3 p + 2); the rows of the others are zeroed after assembly, so
  // that K, right-hand sides and residuals are the rank's share and sums over the ranks are the global objects.  The
  // halo plan refreshes the entries of the points owned elsewhere.
  uint8_t* d_owned = nullptr;
  uint8_t* d_cell_owned = nullptr;                       // femo_shell_set_owned_cells: the cells whose scalar outputs this rank integrates
  int n_nbr = 0;
  std::vector<int32_t> nbr;
  std::vector<int64_t> send_ptr, recv_ptr;
  int32_t *d_send_idx = nullptr, *d_recv_idx = nullptr;
  double *d_send_buf = nullptr, *d_recv_buf = nullptr;
};

// plain view of the device arrays for kernels
struct femo_shell_view {
  int64_t n_vert, n_cell, n_unode;
  const double* x;
  const int32_t *conn, *cedge;
  // partitioned shells (femo_shell_set_owned_cells): 1 for the cells this rank integrates in scalar outputs (each cell of the
  // whole mesh belongs to exactly one rank; the values are summed over the ranks), nullptr on one rank.  Gradients are
  // formed over ALL local cells: every cell around a point the rank owns is local, so their entries there are complete.
  const uint8_t* cell_owned;
};
__device__ __forceinline__ double shell_value_weight(const femo_shell_view& S, int64_t c) {
  return (S.cell_owned == nullptr || c >= S.n_cell || S.cell_owned[c]) ? 1.0 : 0.0;
}

constexpr int SH_BLOCK = 256;
constexpr int SH_MAXPART = 4096;

// three consecutive doubles, 8-byte aligned: loaded as one 16-byte and one 8-byte access (global loads need no more
// than dword alignment on gfx9) -- 9 instead of 13 memory instructions per block
struct __attribute__((packed, aligned(8))) Triple { double a, b, c; };

static inline unsigned sgrid(int64_t n, int per = SH_BLOCK) {
  int64_t g = (n + per - 1) / per;
  if (g < 1) g = 1;
  return (unsigned)std::min<int64_t>(g, 1 << 20);
}

template <class T>
static int to_device(T** d, const T* h, int64_t n, hipStream_t st) {
  FEMO_HIP_CHECK(hipMalloc(d, std::max<int64_t>(n, 1) * sizeof(T)));
  if (n > 0) FEMO_HIP_CHECK(hipMemcpyAsync(*d, h, n * sizeof(T), hipMemcpyHostToDevice, st));
  return 0;
}

// ---- host functions that cross units.  The void ones only enqueue kernels of their unit on `st`: no synchronisation, no
// error check -- the caller's next FEMO_HIP_CHECK(hipGetLastError()) sees the launches, as when all this was one file.
// shell_solve.hip
int shell_allreduce(femo_shell* s, double* d, int64_t n, hipStream_t st);        // sum over the ranks of a partition (no-op on one)
int shell_zero_unowned_rows(femo_shell* s, double* vals, hipStream_t st);        // the rank's share of an assembled matrix
int shell_mask(femo_shell* s, const uint8_t* fixed_host, const uint8_t** d_fixed, uint64_t* hash);
void shell_rhs_free(femo_shell* s, const double* rhs, const uint8_t* d_fixed, hipStream_t st);   // d_r = rhs on the free dofs
// shell_forms.hip
void shell_forms_free(femo_shell* s);
// shell.hip
int shell_pc_setup(femo_shell* s, const femo_vec* vals, uint64_t mh, const uint8_t* d_fixed, bool point_blocks);
int shell_pc_apply(femo_shell* s, const uint8_t* d_fixed, double* Prz, unsigned gz, const int32_t* done, double* Pte = nullptr,
                   int* nb_te = nullptr, double* carry_x = nullptr);
void shell_pc_prolong_fused(femo_shell* s, const uint8_t* d_fixed, unsigned grid, int it, int nb_rB, const double* part_rB, int nb_te,
                            const double* part_te, double* gamma_out, hipStream_t st);
int shell_pc_compact_levels(femo_shell* s, int level, hipStream_t st);
void shell_pc_free(femo_shell* s);
// shell_coarse.hip
int shell_pc_coarse_setup(femo_shell* s, const femo_vec* vals, const uint8_t* d_fixed, bool node_blocks);
void shell_coarse_apply(femo_shell* s, const int32_t* done, double* carry_x, hipStream_t st);
int shell_coarse_hermite_lds();
void shell_coarse_free(femo_shell* s);
