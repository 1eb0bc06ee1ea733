// Shared by elasticity.hip (assembly, dR/drho, load, export, filter), elast_solve.hip (block product, PCG and the poll loop
// of every batched Krylov solve), elast_pc.hip (multilevel preconditioner), elast_stress.hip (stress aggregate), each for
// one or several load cases, elast_disp.hip (displacement aggregate), elast_block.hip (block linear algebra and the block
// iteration of the eigen solves), elast_eig.hip (mass product and the eigenfrequency pencil), elast_buckle.hip (geometric stiffness and the buckling
// pencil), elast_harm.hip (assembled mass, shifted product and MINRES of the harmonic response), elast_damp.hip (complex
// product and COCR of the damped response) and elast_transient.hip (Newmark march, its banded product and dR/drho).  The
// static and the banded SELL product of these units are prologues and epilogues around one row walk, elast_row_walk below;
// all four products choose their instantiation through elast_dispatch.  The kernels that work on cells, or on the vertex ->
// cell incidence, share their cell prologue (elast_cell, elast_cell_volume), the visit walk (for_each_visit), the
// displacement gradient, the energy density and the consistent-mass weight and row (cell_gradient, elastic_form,
// mass_weight, mass_row_add) and their launch path (elast_dispatch_d, elast_launch_cells, elast_launch_rows), all below.
// Not part of the ABI.
#pragma once

#include "femo_internal.h"

#include <functional>
#include <type_traits>

struct femo_elast_pc;   // lattice hierarchy of the multilevel preconditioner (elast_pc.hip)

struct femo_elast {
  femo_mesh* mesh = nullptr;
  int d = 0;
  double lam0 = 0.0, mu0 = 0.0;
  double* d_vals = nullptr;     // sell_entries * d^2
  double* d_diag = nullptr;     // n_rows * d^2
  double* d_dinv = nullptr;     // n_rows * d^2: inverse of the (masked) diagonal blocks
  uint8_t* d_fixed = nullptr;   // n_dof, optional
  bool has_fixed = false;
  // elastic supports (femo_elast_set_springs): one stiffness per dof; the operator is K(rho) + diag(springs) from the next
  // assembly on (k_elast_springs after k_elast_assemble; the lattice blocks take them in k_pc_springs)
  double* d_springs = nullptr;  // n_dof, optional
  bool has_springs = false;
  bool assembled = false;
  // tagged facets: vertex -> facet CSR (vertex ids of the facets, d per facet)
  int64_t n_facets = 0;
  int32_t* d_fverts = nullptr;
  int64_t* d_fptr = nullptr;    // n_vert + 1
  int32_t* d_flist = nullptr;
  // PCG work: w_cols columns of r, z, p, q, one column after the other, and w_pstride partials per column; one column from
  // femo_elast_create, grown on demand (femo_elast_work_reserve).  Per column EMS_STRIDE scalars and EMF_STRIDE flags,
  // always for FEMO_ELAST_MAX_COLS columns, like their pinned mirrors.
  int w_cols = 0;
  int64_t w_pstride = 0;
  double *w_r = nullptr, *w_z = nullptr, *w_p = nullptr, *w_q = nullptr, *w_part = nullptr, *w_s = nullptr;
  int32_t* w_flag = nullptr;
  int32_t* h_flag = nullptr;    // pinned
  double* h_s = nullptr;        // pinned; the stress aggregates come back through it as well
  // stress aggregate (femo_elast_pnorm_stress, femo_elast_pnorm_stress_multi): FEMO_ELAST_MAX_COLS slabs of partials, one per
  // column, and the folded values behind them, on first use
  double* w_smpart = nullptr;
  // displacement aggregate (femo_elast_pnorm_disp_multi, elast_disp.hip): the same layout over the blocks of the vertices
  double* w_dpart = nullptr;
  // block iteration (elast_block.hip), on first use: the right-hand sides B = Op X of w_eig_cols columns; the Gram partials
  // and their folded values, with their pinned mirror
  double* w_eig = nullptr;
  int w_eig_cols = 0;
  double* w_gram = nullptr;
  double* h_gram = nullptr;     // pinned
  // buckling (elast_buckle.hip), on first use: the cell stress C(rho) sigma_0(u) of femo_elast_geom_stress, component-major
  // (d (d+1) / 2 components of n_cell entries: the diagonal first, then 01[, 02, 12])
  double* w_gstress = nullptr;
  bool has_gstress = false;
  // harmonic response (elast_harm.hip), on first use: the scalar mass matrix on the SELL pattern (sell_entries values in the
  // slots of K, n_rows diagonal values); the three extra vectors of the MINRES loop (r1, w1, w2, w_harm_cols columns each), its
  // scalars per column and their pinned mirror.  The COCR of the damped response (elast_damp.hip) reads the same M and keeps
  // two of its vectors and its scalars in w_harm and w_ms
  double *d_mvals = nullptr, *d_mdiag = nullptr;
  bool mass_assembled = false;
  double* w_harm = nullptr;
  int w_harm_cols = 0;
  double* w_ms = nullptr;
  double* h_ms = nullptr;       // pinned
  // multilevel preconditioner (femo_elast_pc_setup); its Galerkin blocks follow (K, fixed set, springs) through pc_dirty
  // Newmark march (elast_transient.hip), on first use: the step's right-hand side, the two windows of FEMO_ELAST_MAX_COLS
  // combined columns of dR/drho (w_nm: 1 + 2 FEMO_ELAST_MAX_COLS vectors) and the inverse diagonal blocks of K + sigma M
  double* w_nm = nullptr;
  double* d_nm_dinv = nullptr;
  femo_elast_pc* pc = nullptr;
  bool pc_dirty = true;
  int method = 0;                    // of the last femo_elast_assemble ...
  uint64_t rho_uid = 0, rho_gen = 0; // ... and its density vector: looked up in the live table at the lazy build (never a
                                     // pointer: the caller may have destroyed it); uid 0 = wrapped memory, built at once
};

// the density filter (elasticity.hip builds and applies it; project.hip gathers with it)
struct femo_filter {
  femo_ctx* ctx = nullptr;
  int64_t n = 0, nnz = 0;
  int64_t* d_rowptr = nullptr;
  int32_t* d_col = nullptr;
  double* d_val = nullptr;      // W
  double* d_valT = nullptr;     // W^T on the same (symmetric) pattern
};

// Helmholtz (PDE) density filter W = V^-1 T^T A^-1 T (csrc/pde_filter.hip; include/femo_hip.h states it)
struct femo_pde_filter {
  femo_ctx* ctx = nullptr;
  femo_mesh* mesh = nullptr;
  int64_t n = 0;                // cells
  double radius = 0.0, rtol = 1e-13;   // rtol: of the solves that are not handed options of their own
  bool lumped = true, warm_start = false;
  bool have_guess = false;      // p holds the nodal field of the last forward application that converged
  femo_mat* A = nullptr;        // rt^2 L + M on the mesh pattern
  femo_vec* cv_vol = nullptr;   // n: |T_c| / (d+1), the transfer T and the transposed pipeline's way out
  femo_vec* cv_one = nullptr;   // n: 1 / (d+1), the mean and the transposed pipeline's way in
  femo_vec* b = nullptr;        // n_rows: the load
  femo_vec* p = nullptr;        // n_vert: nodal field of the forward pipeline (kept for warm_start)
  femo_vec* pT = nullptr;       // n_vert: ... of the transposed one
  femo_solve_info last = {};
};
// b = T (s x), p = A^-1 b: the two first steps of femo_pde_filter_apply.  *nodal is the solution; the caller applies the mean.
int femo_pde_filter_nodal(femo_pde_filter* f, int transpose, const femo_vec* x, const femo_solver_opts* opts,
                          femo_solve_info* info, const femo_vec** nodal);

constexpr int EB = 256;              // threads per block of the row kernels
constexpr int PCG_GRID = 512;        // blocks of the PCG reductions (one partial each)

// PCG device scalars s[]: 0 rz, 1 alpha, 2 beta, 3 tol^2, 4 rz0.  flag[]: 0 done, 1 iterations, 2 breakdown, 3 converged.
enum { S_RZ = 0, S_ALPHA = 1, S_BETA = 2, S_TOL2 = 3, S_RZ0 = 4 };
// Column l keeps its own s[] at s + l * EMS_STRIDE and its own flag[] at flag + l * EMF_STRIDE.
constexpr int EMS_STRIDE = 8, EMF_STRIDE = 4;

// columns per thread of the batched products (complex columns: half as many); one column runs the instantiation for 1
constexpr int ELAST_CHUNK = 4;

// One value per column, by value into a kernel: shifts, scales, weights.  In an unnamed namespace like the kernels that take
// it, whose symbols carry its name.
namespace {
struct ColScalars { double v[FEMO_ELAST_MAX_COLS]; };
}  // namespace

// fn(std::integral_constant<int, D>, std::bool_constant<MASKED>) for d = 2 or 3: the run-time pair as template arguments
template <typename F>
inline void elast_dispatch(int d, bool masked, F&& fn) {
  if (d == 2) {
    if (masked) fn(std::integral_constant<int, 2>(), std::true_type());
    else fn(std::integral_constant<int, 2>(), std::false_type());
  } else {
    if (masked) fn(std::integral_constant<int, 3>(), std::true_type());
    else fn(std::integral_constant<int, 3>(), std::false_type());
  }
}

// fn(std::integral_constant<int, D>) for d = 2 or 3; returns what fn returns
template <typename F>
inline auto elast_dispatch_d(int d, F&& fn) {
  return d == 2 ? fn(std::integral_constant<int, 2>()) : fn(std::integral_constant<int, 3>());
}

// blocks of EB threads for n items
inline unsigned grid_of(int64_t n, int64_t cap = 1 << 20) {
  int64_t g = (n + EB - 1) / EB;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

#if defined(__HIPCC__)
// kernel(n, args...) with one thread per item on the context's stream, ny blocks in the grid's second dimension
template <typename K, typename... A>
int elast_launch(const femo_elast* e, int64_t n, unsigned ny, K kernel, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid_of(n), ny), dim3(EB), 0, e->mesh->ctx->stream, n, args...);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}
// one thread per cell: kernel(n_cell, args...)
template <typename K, typename... A>
int elast_launch_cells(const femo_elast* e, K kernel, A... args) {
  return elast_launch(e, e->mesh->n_cell, 1u, kernel, args...);
}
// one thread per vertex row: kernel(n_rows, args...)
template <typename K, typename... A>
int elast_launch_rows(const femo_elast* e, K kernel, A... args) {
  return elast_launch(e, e->mesh->n_rows, 1u, kernel, args...);
}
#endif

// device array of n entries (at least one)
template <typename T>
int dalloc(T** p, int64_t n) {
  FEMO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), (size_t)(n > 1 ? n : 1) * sizeof(T)));
  return 0;
}

// elast_pc.hip ------------------------------------------------------------------------------------------------------
void femo_elast_pc_free(femo_elast* e);
// Rebuilds the Galerkin blocks when K or the fixed set changed since the last build (no-op otherwise).
int femo_elast_pc_ensure(femo_elast* e);
// The build itself, from the density the current K was assembled with.
int femo_elast_pc_build(femo_elast* e, const double* rho);
// The preconditioner step of the PCG loop for n_cols columns in four launches (a column dimension in every grid;
// k_pc_coarse: one workgroup per column): what k_pcg_precond does with z = M^-1 r of the multilevel form.
// update: x += alpha p, r -= alpha q first (alpha = s[S_ALPHA]; a column whose flag[0] is set is skipped).  pinit != null:
// p = z as well.  Vectors: column l at + l * n_dof; s, flag: EMS_STRIDE / EMF_STRIDE apart; part: part_stride apart.  The
// lattice work vectors grow here when n_cols exceeds what they hold.  dinv: the inverse diagonal blocks of the Jacobi term
// (e->d_dinv for K itself).
int femo_elast_pc_step(femo_elast* e, bool update, int n_cols, double* x, double* r, const double* p, const double* q,
                       double* z, double* pinit, const double* s, double* part, int64_t part_stride, const int32_t* flag,
                       const double* dinv);

// elast_solve.hip ---------------------------------------------------------------------------------------------------
// y_l = a Op x_l + b f_l for n_cols columns (+ partial dot(x_l, y_l) per block and column, part_stride apart, when part !=
// null).  masked: identity rows / columns on fixed dofs.  done != null: a column whose done[l * EMF_STRIDE] is set is skipped.
int femo_elast_spmv(femo_elast* e, bool masked, int n_cols, double a, const double* x, double b, const double* f, double* y,
                    double* part, int64_t part_stride, const int32_t* done);
// PCG work vectors for at least n_cols columns.  who: the entry point, for the error text.
int femo_elast_work_reserve(femo_elast* e, int n_cols, const char* who);
// The first guess of a Krylov loop for n_cols columns (k_pcg_start_x): x = 0 with zero_guess, and x = b on the fixed dofs.
int femo_elast_start_x(femo_elast* e, int n_cols, int zero_guess, const double* b, double* x);
// The operator of femo_elast_pcg other than K: K + sigma M (sigma >= 0, M assembled) through the shifted product, with the
// inverse diagonal blocks of K + sigma M for the Jacobi term (the lattice term of the multilevel form stays that of K).
struct femo_elast_op {
  double sigma;
  const double* dinv;
};
// The batched PCG of femo_elast_solve_multi for a caller that has checked its arguments (the eigen solve, the Newmark
// march): info: n_cols records, or null.  op == null: K.
int femo_elast_pcg(femo_elast* e, int n_cols, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info,
                   const char* who, const femo_elast_op* op = nullptr);
// What a batched Krylov solve (PCG, MINRES, COCR) hands to femo_elast_krylov_loop.  Its launches read the work vectors from
// the handle when they run: the loop reserves them before start().
struct femo_elast_krylov {
  const char* who;          // the entry point, for the error texts
  int real_cols;            // columns of work to reserve; the flags of as many columns are copied at every poll
  int n_cols;               // solver columns: column l reads the flags of real column l * flag_stride
  int flag_stride;          // 1, or 2 where a complex column owns a pair of real ones
  bool harm;                // reserves the harmonic work (w_harm, w_ms) as well
  std::function<int(int max_it)> start;              // everything up to and including the scalar kernel of iteration 0
  std::function<int(int it, int max_it)> iterate;    // the launches of iteration `it` (from 0)
  double* femo_elast::*d_scal;                       // the scalars of the columns on the device ...
  double* femo_elast::*h_scal;                       // ... their pinned mirror ...
  int scal_stride;                                   // ... and the stride between two columns
  int s_res, s_rhs;         // residual_norm and rhs_norm among a column's scalars ...
  bool squared;             // ... or their squares (possibly rounded below zero)
};
// The host side every batched Krylov solve shares: the multilevel refusal, await b / touch x, the preconditioner and work on
// demand, the defaults of check_every (multilevel 8, else 32) and max_it (100000), start(), then bursts of check_every
// iterations -- never beyond max_it -- between polls of the flags, until every column is done; the scalars' read-back and
// one femo_solve_info per column (info may be null).
int femo_elast_krylov_loop(femo_elast* e, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info,
                           const femo_elast_krylov& loop);

// elast_harm.hip ----------------------------------------------------------------------------------------------------
// scalars per column in w_ms / h_ms, always for FEMO_ELAST_MAX_COLS columns
constexpr int FEMO_ELAST_HARM_SCALARS = 16;
// The three extra vectors of the MINRES loop in w_harm (w_harm_cols columns each, one behind the other) for at least n_cols
// columns, the scalars and their pinned mirror.  The COCR of elast_damp.hip keeps two vectors and its scalars there.
int femo_elast_harm_reserve(femo_elast* e, int n_cols, const char* who);
// y_l = a (Op - shift M) x_l + b f_l on raw pointers with one shift for all columns (any sign), as femo_elast_spmv
int femo_elast_dyn_spmv(femo_elast* e, bool masked, int n_cols, double shift, double a, const double* x, double b, const double* f,
                        double* y, double* part, int64_t part_stride, const int32_t* done);

// elast_block.hip: the block linear algebra and the block iteration of the eigen solves --------------------------------
namespace elast_block {
struct BlockMatrix { double v[FEMO_ELAST_MAX_COLS][FEMO_ELAST_MAX_COLS]; };
// The Gram partials and their pinned mirror h_gram, on first use.
int gram_reserve(femo_elast* e);
// The right-hand sides w_eig of the block iteration for at least n_cols columns.
int rhs_reserve(femo_elast* e, int n_cols);
// slab s (0 or 1) <- partials of A^T B (n entries per column); folded by gram_fetch
int gram_launch(femo_elast* e, int slab, int64_t n, int n_a, const double* A, int n_b, const double* B);
// folds the first `sums0` pairs of slab 0 and `sums1` of slab 1 and waits for them in h_gram[0 ...] and
// h_gram[FEMO_ELAST_MAX_COLS^2 ...]
int gram_fetch(femo_elast* e, int64_t n, int sums0, int sums1);
// y_j = sum_i x_i Q[i][j] (+ sum_i x2_i Q2[i][j] with Q2), ascending i; y may be x (or x2)
int rotate_launch(femo_elast* e, int64_t n, int n_cols, const BlockMatrix& Q, const double* x, const BlockMatrix* Q2,
                  const double* x2, double* y);
// G_K q = theta G_M q, G_M positive definite (false when it is not): theta ascending, Q^T G_M Q = I, Q^T G_K Q = Theta
bool small_eigs(int L, const double (&GM)[FEMO_ELAST_MAX_COLS][FEMO_ELAST_MAX_COLS],
                const double (&GK)[FEMO_ELAST_MAX_COLS][FEMO_ELAST_MAX_COLS], double (&theta)[FEMO_ELAST_MAX_COLS],
                double (&Q)[FEMO_ELAST_MAX_COLS][FEMO_ELAST_MAX_COLS]);
// the entry of largest magnitude (the first of equals) of each of the n_cols columns of x becomes positive
int sign_launch(femo_elast* e, int64_t n, int n_cols, double* x);
// a femo_vec over memory it does not own
femo_vec wrap(femo_ctx* ctx, double* d, int64_t n);

// The Ritz pencil N phi = theta P phi of one block iteration: K is one side, the masked product `apply` the other.
struct Pencil {
  const char* who;          // the entry point, for the error texts
  const char* p_name;       // P in the error texts ("Y^T P Y is not positive definite")
  std::function<int(int n_cols, const double* x, double* y)> apply;   // y_l = Op_ff x_l for n_cols columns, one launch
  bool p_is_op;             // P (the positive definite side) is Op and N is K; otherwise P is K and N is Op
  bool descending;          // the modes in descending theta (ascending otherwise)
  int zero_guess;           // the inner PCG starts from zero (1) or from the previous block (0)
  int max_outer;            // outer steps at the most when the options say 0
  bool positive_only;       // a mode counts only with theta > 0, and the call fails when fewer than n_modes ever do
  bool reciprocal;          // the reported values are 1 / theta
};
// Block inverse iteration with Rayleigh-Ritz for the n_modes first modes of the pencil in a block of `block` columns of X
// (the start block on entry, the P-orthonormal modes on return), for a caller that has checked its arguments.  lambda:
// `block` values; info may be null.
int block_iteration(femo_elast* e, const Pencil& pencil, int n_modes, int block, femo_vec* X, const femo_eig_opts* opts,
                    double* lambda, femo_eig_info* info);
}  // namespace elast_block

#if defined(__HIPCC__)
// neither NaN nor infinite.  (x - x == 0 would do as well, were it not that with x = a * b the compiler contracts x - x into
// fma(a, b, -x), the rounding error of the product.)
__device__ __forceinline__ bool is_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// One SELL row of K x_i, and with MASS of M x_i (one scalar per entry in the slots of K, times I_d), for NV vectors: the walk
// under the static and the banded product (the shifted and the complex product keep copies of it, DESIGN_LOG.md R24).  The
// kernels differ before it (which columns the x_i are, which are on) and after it (how the sums combine, the right-hand
// side, the dot partials).  Both structs travel by value: behind a reference the arrays would be reached through generic
// pointers, and the kernels would not compile to what they were.
template <int NV>
struct ElastRowIn {
  const double* x[NV];      // column i; read only where on[i]
  bool on[NV];              // uniform over the block
};
template <int D, int NV, bool MASS>
struct ElastRow {
  uint8_t fo[D];            // the row's fixed bytes (0 without MASKED)
  double xo[NV][D];         // the row's own entries of x_i as stored, 0 where off
  double acc[NV][D];        // (K x_i)[row]; MASKED: fixed entries of x_i read as 0
  double accm[NV][D];       // (M x_i)[row] likewise
};
template <int D, int NV>
struct ElastRow<D, NV, false> {       // without MASS there is no mass accumulator
  uint8_t fo[D];
  double xo[NV][D];
  double acc[NV][D];
};
// The fixed bytes and the diagonal block, then per slot the block, its column index, the fixed bytes and the mass scalar
// are read ONCE for all vectors.  Every sum is seeded from the diagonal block and takes the slots in ascending order, the
// columns of a block in ascending order: one order of additions under every product, so that their bits agree.  A vector
// that is off is never read and keeps the seed of zeros.  Without MASS no mass array is touched.
template <int D, bool MASKED, int NV, bool MASS>
__device__ __forceinline__ ElastRow<D, NV, MASS> elast_row_walk(int64_t row, const int64_t* mptr, const int32_t* cols,
                                                                const int32_t* rowlen, const double* vals, const double* diag,
                                                                const uint8_t* fixed, const double* mvals, const double* mdiag,
                                                                ElastRowIn<NV> in) {
  constexpr int DD = D * D;
  ElastRow<D, NV, MASS> R;
  const int64_t slice = row >> 6;
  const int lane = (int)(row & 63);
  const int64_t mb = mptr[slice];
  const int len = rowlen[row];
#pragma unroll
  for (int r = 0; r < D; ++r) R.fo[r] = MASKED ? fixed[row * D + r] : 0;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int r = 0; r < D; ++r) R.xo[i][r] = in.on[i] ? in.x[i][row * D + r] : 0.0;
  {
    double dg[DD];
#pragma unroll
    for (int q = 0; q < DD; ++q) dg[q] = diag[row * DD + q];
    double md = 0.0;
    if constexpr (MASS) md = mdiag[row];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int r = 0; r < D; ++r) {
        double s = 0.0;
#pragma unroll
        for (int cc = 0; cc < D; ++cc) s += dg[r * D + cc] * (R.fo[cc] ? 0.0 : R.xo[i][cc]);
        R.acc[i][r] = s;
        if constexpr (MASS) R.accm[i][r] = md * (R.fo[r] ? 0.0 : R.xo[i][r]);
      }
  }
  for (int k = 0; k < len; ++k) {
    const int64_t e = femo_sell_index(mb, k, lane);
    const int64_t col = cols[e];
    double blk[DD];
#pragma unroll
    for (int q = 0; q < DD; ++q) blk[q] = vals[e * DD + q];
    double mv = 0.0;
    if constexpr (MASS) mv = mvals[e];
    uint8_t fc[D];
#pragma unroll
    for (int cc = 0; cc < D; ++cc) fc[cc] = MASKED ? fixed[col * D + cc] : 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (!in.on[i]) continue;
      double xc[D];
#pragma unroll
      for (int cc = 0; cc < D; ++cc) {
        xc[cc] = in.x[i][col * D + cc];
        if (MASKED && fc[cc]) xc[cc] = 0.0;
      }
#pragma unroll
      for (int r = 0; r < D; ++r) {
#pragma unroll
        for (int cc = 0; cc < D; ++cc) R.acc[i][r] += blk[r * D + cc] * xc[cc];
        if constexpr (MASS) R.accm[i][r] += mv * xc[r];
      }
    }
  }
  return R;
}

// gradients of the barycentric coordinates and the volume of a P1 simplex, from the vertices in `conn` order
template <int D>
__device__ __forceinline__ void simplex_grads(const double (&p)[D + 1][D], double (&g)[D + 1][D], double& vol) {
  double m[D][D];          // m[k][i] = p[k+1][i] - p[0][i]
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int i = 0; i < D; ++i) m[k][i] = p[k + 1][i] - p[0][i];
  // grad lambda_{k+1} = column k of m^-1
  if constexpr (D == 2) {
    const double det = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    const double id = 1.0 / det;
    g[1][0] = m[1][1] * id;  g[1][1] = -m[1][0] * id;
    g[2][0] = -m[0][1] * id; g[2][1] = m[0][0] * id;
    vol = 0.5 * fabs(det);
  } else {
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    const double c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    const double c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    const double id = 1.0 / det;
    // inverse (adjugate / det): inv[i][k]
    double inv[3][3];
    inv[0][0] = c00 * id;
    inv[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id;
    inv[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id;
    inv[1][0] = c01 * id;
    inv[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id;
    inv[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id;
    inv[2][0] = c02 * id;
    inv[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id;
    inv[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int i = 0; i < 3; ++i) g[k + 1][i] = inv[i][k];
    vol = fabs(det) * (1.0 / 6.0);
  }
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 1; k <= D; ++k) s += g[k][i];
    g[0][i] = -s;
  }
}

// |T| of a P1 simplex from the vertices in `conn` order (the volume of simplex_grads without the gradients)
template <int D>
__device__ __forceinline__ double simplex_volume(const double (&p)[D + 1][D]) {
  double m[D][D];
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int i = 0; i < D; ++i) m[k][i] = p[k + 1][i] - p[0][i];
  if constexpr (D == 2) {
    return 0.5 * fabs(m[0][0] * m[1][1] - m[0][1] * m[1][0]);
  } else {
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1];
    const double c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2];
    const double c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    return fabs(m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02) * (1.0 / 6.0);
  }
}

template <int D>
__device__ __forceinline__ void load_cell(const int32_t* __restrict__ conn, const double* __restrict__ x, int64_t c,
                                          int32_t (&v)[D + 1], double (&p)[D + 1][D]) {
#pragma unroll
  for (int b = 0; b <= D; ++b) {
    v[b] = conn[c * (D + 1) + b];
#pragma unroll
    for (int i = 0; i < D; ++i) p[b][i] = x[(int64_t)v[b] * D + i];
  }
}

// A P1 cell BY VALUE (DESIGN_LOG.md R24: behind a reference the arrays would be reached through generic pointers): its
// vertices in `conn` order, the gradients of the barycentric coordinates and |T| ...  Index g with constants only: a
// run-time index into a member keeps the whole record from being split into registers (R26), so a kernel that reads
// g[a] of the visit's vertex a calls load_cell and simplex_grads on arrays of its own.
template <int D>
struct ElastCell {
  int32_t v[D + 1];
  double g[D + 1][D];
  double vol;
};
template <int D>
__device__ __forceinline__ ElastCell<D> elast_cell(const int32_t* __restrict__ conn, const double* __restrict__ x, int64_t c) {
  ElastCell<D> K;
  double p[D + 1][D];
  load_cell<D>(conn, x, c, K.v, p);
  simplex_grads<D>(p, K.g, K.vol);
  return K;
}
// ... or its vertices and |T| alone
template <int D>
struct ElastCellVolume {
  int32_t v[D + 1];
  double vol;
};
template <int D>
__device__ __forceinline__ ElastCellVolume<D> elast_cell_volume(const int32_t* __restrict__ conn, const double* __restrict__ x,
                                                                int64_t c) {
  ElastCellVolume<D> K;
  double p[D + 1][D];
  load_cell<D>(conn, x, c, K.v, p);
  K.vol = simplex_volume<D>(p);
  return K;
}

// The visit walk of the vertex-row kernels: the cells around vertex `row` in ascending cell order.  Visit s < n of the walk
// is cell c as its vertex a, at index vi of visit_cell and visit_slots; the padding of a slice is not live and is skipped:
//   const ElastVisits V = elast_visits(row, vptr);
//   for (int s = 0; s < V.n; ++s) { const ElastVisit t = elast_visit(V, visit_cell, s); if (!t.live) continue; ... }
// Both structs travel by value (DESIGN_LOG.md R24, R26).
struct ElastVisits {
  int64_t vb;
  int lane, n;
};
struct ElastVisit {
  int64_t vi, c;
  int a;
  bool live;
};
__device__ __forceinline__ ElastVisits elast_visits(int64_t row, const int64_t* __restrict__ vptr) {
  const int64_t slice = row >> 6;
  ElastVisits V;
  V.lane = (int)(row & 63);
  V.vb = vptr[slice];
  V.n = (int)((vptr[slice + 1] - V.vb) >> 6);
  return V;
}
__device__ __forceinline__ ElastVisit elast_visit(ElastVisits V, const int32_t* __restrict__ visit_cell, int s) {
  ElastVisit t;
  t.vi = V.vb + (int64_t)s * 64 + V.lane;
  const int32_t ca = visit_cell[t.vi];
  t.live = ca >= 0;
  t.c = (int64_t)((uint32_t)ca >> 2);       // of a live visit: without the sign, as the compiler sees it behind `ca >= 0`
  t.a = (int)(ca & 3);
  return t;
}

// Gu[i][k] = d u_i / d x_k of the P1 field u in a cell
template <int D>
__device__ __forceinline__ void cell_gradient(const double (&g)[D + 1][D], const int32_t (&v)[D + 1],
                                              const double* __restrict__ u, double (&Gu)[D][D]) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int k = 0; k < D; ++k) Gu[i][k] = 0.0;
#pragma unroll
  for (int b = 0; b <= D; ++b)
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double ub = u[(int64_t)v[b] * D + i];
#pragma unroll
      for (int k = 0; k < D; ++k) Gu[i][k] += ub * g[b][k];
    }
}

// lam div(u) div(w) + 2 mu eps(u) : eps(w) of two gradients: the solid energy density, bilinear; the quadratic sites pass the
// same gradient twice
template <int D>
__device__ __forceinline__ double elastic_form(const double (&Gu)[D][D], const double (&Gw)[D][D], double lam, double mu) {
  double divu = 0.0, divw = 0.0, ee = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) { divu += Gu[i][i]; divw += Gw[i][i]; }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int k = 0; k < D; ++k) ee += 0.25 * (Gu[i][k] + Gu[k][i]) * (Gw[i][k] + Gw[k][i]);
  return lam * divu * divw + 2.0 * mu * ee;
}

// Solid-material stress sigma_0(u) of a P1 cell as a 3 x 3 tensor (plane strain in 2-D: sigma_zz = lam tr eps, no
// out-of-plane shear).  Its deviator does not see lam: s = 2 mu (eps - tr(eps) / 3 I), so s_zz = -2 mu tr(eps) / 3 in
// 2-D.  Returns sigma_vm = sqrt(3/2 s : s); s holds the d x d block of the deviator.
template <int D>
__device__ __forceinline__ double cell_von_mises(const double (&g)[D + 1][D], const int32_t (&v)[D + 1],
                                                 const double* __restrict__ u, double mu, double (&s)[D][D]) {
  double Gu[D][D];
  cell_gradient<D>(g, v, u, Gu);
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) tr += Gu[i][i];
  const double hyd = (2.0 / 3.0) * mu * tr;
  double ss = D == 2 ? hyd * hyd : 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double t = mu * (Gu[i][k] + Gu[k][i]) - (i == k ? hyd : 0.0);
      s[i][k] = t;
      ss += t * t;
    }
  return sqrt(1.5 * ss);
}

// SELL slot of the entry (a, b), b != a, of a visit: visit_slots packs the slots of the cell's other vertices, 8 bits each
__device__ __forceinline__ int slot_pos(uint32_t slots, int a, int b) {
  const int j = b - (b > a ? 1 : 0);
  return (int)((slots >> (8 * j)) & 0xFFu);
}

__device__ __forceinline__ double penal(int method, double r) {
  return method == FEMO_ELAST_SIMP ? r * r * r : r / (1.0 + 8.0 * (1.0 - r));
}
__device__ __forceinline__ double penal_d(int method, double r) {
  if (method == FEMO_ELAST_SIMP) return 3.0 * r * r;
  const double q = 1.0 + 8.0 * (1.0 - r);
  return 9.0 / (q * q);
}

// mass per unit of solid mass at density r: linear, or Du & Olhoff's law -- r for r >= 0.1, 6e5 r^6 - 5e6 r^7 below (value 0.1
// and slope 1 at the joint), which keeps low-density regions from carrying spurious localised modes
__device__ __forceinline__ double mass_law(int law, double r) {
  if (law == FEMO_ELAST_MASS_LINEAR || r >= 0.1) return r;
  const double r2 = r * r, r6 = r2 * r2 * r2;
  return 6e5 * r6 - 5e6 * (r6 * r);
}
__device__ __forceinline__ double mass_law_d(int law, double r) {
  if (law == FEMO_ELAST_MASS_LINEAR || r >= 0.1) return 1.0;
  const double r2 = r * r, r5 = r2 * r2 * r;
  return 36e5 * r5 - 35e6 * (r5 * r);
}

// The weight of a cell in the consistent P1 mass: m |T| / ((d+1)(d+2)), m = rho0 m(rho) or its derivative's factors
template <int D>
__device__ __forceinline__ double mass_weight(double m, double vol) {
  return m * (vol * (1.0 / ((D + 1) * (D + 2))));
}

// The P1 mass row of a visit of the cell with vertices v as its vertex va, for the n_cols first columns of x (n_dof apart):
// acc[l][i] += w (sum_b x_l[v_b, i] + x_l[v_va, i]).  MASKED: fixed entries of x read as 0.  The fixed bytes serve all columns.
template <int D, bool MASKED>
__device__ __forceinline__ void mass_row_add(const int32_t (&v)[D + 1], int va, double w, const uint8_t* __restrict__ fixed,
                                             int n_cols, int64_t n_dof, const double* __restrict__ x,
                                             double (&acc)[FEMO_ELAST_MAX_COLS][D]) {
  bool fx[D + 1][D];
#pragma unroll
  for (int b = 0; b <= D; ++b)
#pragma unroll
    for (int i = 0; i < D; ++i) fx[b][i] = MASKED && fixed[(int64_t)v[b] * D + i];
#pragma unroll
  for (int l = 0; l < FEMO_ELAST_MAX_COLS; ++l) {
    if (l >= n_cols) break;
    const double* __restrict__ xl = x + (int64_t)l * n_dof;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double sx = 0.0, own = 0.0;
#pragma unroll
      for (int b = 0; b <= D; ++b) {
        const double t = fx[b][i] ? 0.0 : xl[(int64_t)v[b] * D + i];
        sx += t;
        if (b == va) own = t;
      }
      acc[l][i] += w * (sx + own);
    }
  }
}

// block (a, b) of the element matrix without the factor C |T|; written symmetrically in (a, r) <-> (b, c)
template <int D>
__device__ __forceinline__ double kblock(const double (&g)[D + 1][D], int a, int b, int r, int c, double lam, double mu,
                                         double gab) {
  double t = lam * (g[a][r] * g[b][c]) + mu * (g[a][c] * g[b][r]);
  if (r == c) t += mu * gab;
  return t;
}

template <int D>
__device__ __forceinline__ double dotg(const double (&g)[D + 1][D], int a, int b) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) s += g[a][k] * g[b][k];
  return s;
}

// in-register inverse of a small SPD block (fixed components: identity row / column)
template <int D>
__device__ __forceinline__ void block_inverse(double (&B)[D * D], double (&Bi)[D * D]) {
  if constexpr (D == 2) {
    const double det = B[0] * B[3] - B[1] * B[2];
    const double id = 1.0 / det;
    Bi[0] = B[3] * id; Bi[1] = -B[1] * id; Bi[2] = -B[2] * id; Bi[3] = B[0] * id;
  } else {
    const double c00 = B[4] * B[8] - B[5] * B[7];
    const double c01 = B[5] * B[6] - B[3] * B[8];
    const double c02 = B[3] * B[7] - B[4] * B[6];
    const double det = B[0] * c00 + B[1] * c01 + B[2] * c02;
    const double id = 1.0 / det;
    Bi[0] = c00 * id;
    Bi[1] = (B[2] * B[7] - B[1] * B[8]) * id;
    Bi[2] = (B[1] * B[5] - B[2] * B[4]) * id;
    Bi[3] = c01 * id;
    Bi[4] = (B[0] * B[8] - B[2] * B[6]) * id;
    Bi[5] = (B[2] * B[3] - B[0] * B[5]) * id;
    Bi[6] = c02 * id;
    Bi[7] = (B[1] * B[6] - B[0] * B[7]) * id;
    Bi[8] = (B[0] * B[4] - B[1] * B[3]) * id;
  }
}

// block-Jacobi inverse of the diagonal block B of a vertex: the components flagged in fx[0 .. D) (null: none) are identity
// rows / columns of B and of the inverse, exactly.  The closed form alone gives them det * (1 / det), which is 1 only to a
// rounding where some but not all components of the vertex are fixed.
template <int D>
__device__ __forceinline__ void block_inverse_fixed(double (&B)[D * D], const uint8_t* __restrict__ fx, double (&Bi)[D * D]) {
  bool f[D];
#pragma unroll
  for (int r = 0; r < D; ++r) f[r] = fx && fx[r];
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c)
      if (f[r] || f[c]) B[r * D + c] = r == c ? 1.0 : 0.0;
  block_inverse<D>(B, Bi);
#pragma unroll
  for (int r = 0; r < D; ++r)
#pragma unroll
    for (int c = 0; c < D; ++c)
      if (f[r] || f[c]) Bi[r * D + c] = r == c ? 1.0 : 0.0;
}
#endif
