/* femo_hip.h -- C-ABI of libfemo_hip.so: MI355X (gfx950) engine for femo's
 * PDE-residual hot path (assemble residual / dR/du / dR/df, forward and
 * transposed linear solves, functional and its partials).
 *
 * The reference (RuruX/femo @ 2024_08_07) has NO FFI: its hot path is Python
 * calling dolfinx/PETSc through pybind/petsc4py.  Each entry point below
 * therefore cites the *Python call site* it replaces (paths relative to the
 * reference tree).  INTEGRATION.md shows the ctypes stub a maintainer would add
 * to femo/fea/utils_dolfinx.py to bind them.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available from femo_last_error() (thread-local).  No exception crosses
 *     the ABI.
 *   - the caller owns every host buffer; the library owns device memory behind
 *     opaque handles.  A femo_ctx owns one HIP stream; all work of the handles
 *     created from it is enqueued on that stream.  Handles are not thread-safe;
 *     distinct contexts may be used from distinct threads.
 *   - all arithmetic is fp64; indices are int32 (dolfinx/PETSc default), sizes
 *     and offsets int64.
 *   - host<->device copies are synchronous w.r.t. the host (they synchronise the
 *     context's stream); compute entry points are asynchronous unless they
 *     return a scalar to the host.  See "host memory" below for pinned blocks and
 *     the provenance rule that elides repeated uploads.
 */
#ifndef FEMO_HIP_H
#define FEMO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEMO_ABI_VERSION 10

typedef struct femo_ctx  femo_ctx;   /* device + stream + reduction workspace (+ RCCL communicator) */
typedef struct femo_vec  femo_vec;   /* fp64 device vector  (dolfinx Function.vector / PETSc Vec)     */
typedef struct femo_mesh femo_mesh;  /* P1 simplex mesh + vertex->cell incidence + sparsity pattern   */
typedef struct femo_bc   femo_bc;    /* strong Dirichlet set (fea_dolfinx.py:169-176 add_strong_bc)   */
typedef struct femo_mat  femo_mat;   /* N x N sparse matrix on the mesh pattern (PETSc Mat)           */
typedef struct femo_shell femo_shell; /* Reissner-Mindlin shell space CG2^3 x CG1^3 on a triangulated surface (below) */
typedef struct femo_elast femo_elast; /* vector CG1 linear elasticity with a DG0 density (SIMP / RAMP), below         */
typedef struct femo_filter femo_filter; /* DG0 density filter W (and W^T) built on the device, below                 */

/* closed catalogue of residual forms (UFL is not available) */
enum femo_pde_kind {
  FEMO_PDE_POISSON = 0,       /* examples/poisson_opt/run_poisson_opt.py:32-38            */
  FEMO_PDE_NL_POISSON = 1,    /* examples/nonlinear_poisson_opt/...py:88-125              */
  FEMO_PDE_MASS = 2,          /* inner(Pv, w) dx, matrix only (utils_dolfinx.py:567-572)  */
  FEMO_PDE_EB_BEAM = 3        /* examples/beam_thickness_opt/run_thickness...py:71-79: cubic Hermite
                                 Euler-Bernoulli beam; mesh vertices = DOFs (w_i, th_i), 4 per element,
                                 params = {E, width}, f = thickness per element, aux = nodal load */
};

/* closed catalogue of scalar output forms */
enum femo_functional_kind {
  FEMO_J_L2_TRACKING = 0      /* 1/2 int (u-u_d)^2 + alpha/2 int f^2 ; run_poisson_opt.py:74-76 */
};

enum femo_mesh_info_key {
  FEMO_MESH_TDIM = 0, FEMO_MESH_N_VERT = 1, FEMO_MESH_N_ROWS = 2, FEMO_MESH_N_CELL = 3,
  FEMO_MESH_NNZ = 4,            /* true nonzeros of the N x N pattern incl. diagonal   */
  FEMO_MESH_SELL_ENTRIES = 5,   /* padded off-diagonal entries stored                  */
  FEMO_MESH_MAX_ROWLEN = 6, FEMO_MESH_MAX_VALENCE = 7, FEMO_MESH_N_SLICES = 8,
  FEMO_MESH_VISIT_ENTRIES = 9,
  FEMO_MESH_REGULAR_SLICES = 10, /* slices whose column indices are row + per-slice deltas */
  FEMO_MESH_SHORT_SLICES = 11,   /* irregular slices with 16-bit column deltas (SpMV reads 2 B per entry) */
  FEMO_MESH_INFO_COUNT = 12
};

/* preconditioner of femo_solve_cg (femo_solver_opts.pc) */
enum {
  FEMO_PC_JACOBI = 0,   /* diagonal scaling only                                                    */
  FEMO_PC_BPX    = 1    /* + additive multilevel correction on an auxiliary lattice (csrc/bpx.hip);  */
                        /*   operators assembled from FEMO_PDE_POISSON / FEMO_PDE_NL_POISSON only    */
};

/* Stopping rules.  D = diag(A), M = the preconditioner (rows / columns of the Dirichlet set the matrix was
 * eliminated with are identity rows: they are solved exactly up front and take no part in any norm).
 *   FEMO_PC_JACOBI:  sqrt(r^T D^-1 r) <= max(rtol sqrt(b^T D^-1 b), atol)
 *   FEMO_PC_BPX:     sqrt(r^T M^-1 r) <= max(rtol sqrt(b^T M^-1 b), atol_pc)   or   sqrt(r^T D^-1 r) <= atol (if > 0)
 *                    r^T M^-1 r is PCG's own gamma; sqrt(gamma / gamma_0) tracks the relative energy-norm error
 *                    independently of the mesh size, which the Jacobi-norm ratio does not (its constant is cond(D^-1 A)). */
typedef struct femo_solver_opts {
  double rtol;
  double atol;          /* absolute, Jacobi norm (both preconditioners)                 */
  int32_t max_it;
  int32_t zero_guess;   /* 1: x is taken as 0 on entry (skips the initial SpMV)         */
  int32_t check_every;  /* iterations enqueued between host convergence polls (0 = 32)  */
  int32_t pc;           /* FEMO_PC_*                                                     */
  double atol_pc;       /* absolute, norm of the preconditioner (FEMO_PC_BPX only)      */
} femo_solver_opts;

typedef struct femo_solve_info {
  int32_t iterations;
  int32_t converged;    /* 1 converged, 0 hit max_it, -1 breakdown (NaN); femo_shell_solve only: 2 = stalled at the
                           attainable accuracy (below 1e-9 of the initial residual in the preconditioner's norm, no
                           progress over 8 polls)                                          */
  double  residual_norm;/* sqrt(r^T D^-1 r) at exit (recurrence residual)               */
  double  pc_residual_norm; /* sqrt(r^T M^-1 r) at exit and for the right-hand side     */
  double  pc_rhs_norm;      /* (FEMO_PC_BPX; 0 otherwise)                                */
  double  rhs_norm;     /* sqrt(b^T D^-1 b)                                             */
  double  solve_ms;     /* device time of the solve (HIP events on the ctx stream)      */
  double  spmv_ms;      /* accumulated device time of sampled SpMV launches             */
  int32_t spmv_samples; /* number of SpMV launches that were individually timed         */
  int32_t loop_allreduces;   /* all-reduce calls issued inside the iteration loop (0 on one rank): the merged BPX-PCG issues one per iteration */
} femo_solve_info;

/* ---- errors / probing ---------------------------------------------------- */
const char* femo_last_error(void);
int  femo_abi_version(void);
int  femo_device_count(int* n);

/* ---- context --------------------------------------------------------------
 * stream: a hipStream_t created by the caller (e.g. torch.cuda.Stream().cuda_stream)
 * or NULL to let the library create one.  Replaces the implicit PETSc/MPI
 * global state (utils_dolfinx.py:32 comm = MPI.COMM_WORLD).                  */
int   femo_ctx_create(int device_id, void* stream, femo_ctx** out);
int   femo_ctx_destroy(femo_ctx* ctx);
int   femo_ctx_sync(femo_ctx* ctx);
void* femo_ctx_stream(femo_ctx* ctx);

/* ---- vectors --------------------------------------------------------------
 * utils_dolfinx.py:155-167 getFuncArray / setFuncArray, :300-311 update.     */
int     femo_vec_create(femo_ctx* ctx, int64_t n, femo_vec** out);          /* zero-filled */
int     femo_vec_wrap(femo_ctx* ctx, void* device_ptr, int64_t n, femo_vec** out); /* borrow */
int     femo_vec_destroy(femo_vec* v);
int64_t femo_vec_size(const femo_vec* v);
void*   femo_vec_device_ptr(femo_vec* v);         /* mutable: counts as a write to v (provenance records and per-content
                                                     caches of v are dropped; a pending copy-out of v is waited for
                                                     on the device before the next kernel on the context's stream) */
const void* femo_vec_device_ptr_const(const femo_vec* v);   /* read-only access, no side effect */
int     femo_vec_set_host(femo_vec* v, const double* host, int64_t n);      /* setFuncArray */
int     femo_vec_get_host(const femo_vec* v, double* host, int64_t n);      /* getFuncArray */
/* host[0:n] += v[0:n]: the `d_inputs[name] += dRdf^T dR` of state_model.py:190-200 without a second
 * pass over the host array (the add runs in the host threads that drain the staging slots).       */
int     femo_vec_add_to_host(const femo_vec* v, double* host, int64_t n);
int     femo_vec_get_host_async(const femo_vec* v, double* host, int64_t n);   /* see "asynchronous results" below */
/* Deferred upload (round 4): like femo_vec_set_host, but from a whole block of femo_host_alloc the copy runs on the
 * context's copy stream and the call returns at once; the matrix half of the next assembly pass, its scaling and the
 * preconditioner weights -- none of which depend on the input -- then run under the transfer (state_model.py:94-103
 * sends the inputs before it solves).  Writers of v and the assembly entry points wait by themselves; before any
 * OTHER entry point reads v the caller says femo_vec_await_upload (engine.deferred_uploads does it on leaving the
 * scope).  Everything else (caller-owned or pageable memory, elided uploads) is femo_vec_set_host.              */
int     femo_vec_set_host_deferred(femo_vec* v, const double* host, int64_t n);
int     femo_vec_await_upload(const femo_vec* v);
int     femo_vec_fill(femo_vec* v, double value);                           /* Vec.set      */
int     femo_vec_copy(femo_vec* dst, const femo_vec* src);
int     femo_vec_axpy(femo_vec* y, double a, const femo_vec* x);            /* y += a x     */
int     femo_vec_dot(const femo_vec* x, const femo_vec* y, int64_t n, double* out);
/* out[j] = x[j][0:n] . y[j][0:n] for j < k <= 4: one pass, one reduction (all-reduced over the ranks) and ONE
 * host synchronisation for all of them -- the norms a Newton step of utils_dolfinx.py:419-449 looks at
 * (||F||, ||u||, u.Au) used to cost a stream drain each.                                                    */
int     femo_vec_dots(int k, const femo_vec* const* x, const femo_vec* const* y, int64_t n, double* out);
/* ABI 10: the same, plus out[k] = rho_0 = sum over the non-identity rows of (rb_i / sqrt(diag(A)_i))^2 -- the squared
 * Jacobi norm of the right-hand side `rb` the Krylov loops of A start from.  Newton (utils_dolfinx.py:419-449: always three
 * passes) reads it in the one host synchronisation it has after an assembly pass and takes the solver's own "nothing to
 * iterate on" decision (rho_0 <= atol^2) without launching the solve.                                                  */
int     femo_vec_dots_rhs(int k, const femo_vec* const* x, const femo_vec* const* y, int64_t n, double* out,
                          const femo_mat* A, const femo_vec* rb);
/* ... and what such a solve returns when it does not iterate from the zero guess: x_i = b_i / diag_i on the identity rows of A's
 * last assembly, 0 elsewhere (one small launch, no synchronisation).                                                    */
int     femo_mat_identity_solve(const femo_mat* A, const femo_vec* b, femo_vec* x);
/* Newton's flagged passes (one rank, linear form; utils_hip.py `_NewtonBase.solve`, FEMO_NEWTON_FLAG).  The identity solve
 * also raises a device-side flag when any entry it stores to x is not +0.0 in its bits.  femo_vec_axpy_if (y += a x with that
 * x, a < 0) and femo_newton_rhs_linear_if are the same launches as the plain entry points, handed that flag: while it is down,
 * y and the right-hand side already in place are what the launches would write, bit for bit, and the kernels leave at once.
 * The host never reads the flag.  It is handed on only while the library can show that b still holds the right-hand side of
 * this very operator content, f, u, Dirichlet set and b (generations unchanged since the launch that wrote b, except by
 * these entry points themselves); otherwise, and for partitioned meshes, rows wider than the pipelined residual takes and the
 * streamed head, the calls ARE the plain ones.                                                                            */
int     femo_mat_identity_solve_flag(const femo_mat* A, const femo_vec* b, femo_vec* x);
int     femo_vec_axpy_if(femo_vec* y, double a, const femo_vec* x);

/* ---- host memory of the array boundary (csrc/hostmem.cpp) -------------------------------------
 * The CSDL operators exchange NumPy arrays with the FE layer in every method (state_model.py:81-84,
 * 94-96, 123-124, 171-172; output_model.py:70-72, 78-80); here each exchange is a PCIe transfer.
 *   - femo_host_alloc / femo_host_free: pinned blocks (recycled, kept pinned).  Transfers from / to
 *     them are one DMA; from / to other (pageable) memory the library pipelines 8 MiB chunks through
 *     pinned staging slots with a pool of host threads.
 *   - femo_host_register / _unregister: pin a caller-owned range in place (e.g. a backend's state vector).
 *   - provenance: a pinned block filled by femo_vec_get_host, or uploaded by femo_vec_set_host,
 *     from its base address is remembered as an exact copy of that device vector.  Sending it again
 *     (to the same or another vector) moves no PCIe bytes while the source vector is unchanged.
 *     Whoever writes to such a block on the host MUST call femo_host_touch first/afterwards; the
 *     library's own host writers do.  FEMO_HOST_VERIFY=1 (environment) checks every elided upload.
 *   - femo_host_copy / femo_host_axpby: y = x, y = a x + b y on the library's host threads, for
 *     drivers that keep their variables in pinned blocks (touch the destination themselves).
 *     femo_host_axpby(a, x, 0, y) with x a block that mirrors a device vector records y as a times that
 *     vector (femo_vec_set_host from y is then a device-side scale), and queues the host pass behind a
 *     copy-out of x that is still in flight instead of waiting for it (y is then in flight itself).   */
typedef struct femo_host_stats {
  int64_t h2d_pinned, h2d_pinned_bytes;     /* one DMA from a pinned block              */
  int64_t h2d_staged, h2d_staged_bytes;     /* pageable source through the staging ring */
  int64_t h2d_skipped, h2d_skipped_bytes;   /* elided: the vector already held the data */
  int64_t h2d_as_d2d, h2d_as_d2d_bytes;     /* elided: copied from another device vector */
  int64_t d2h_pinned, d2h_pinned_bytes;
  int64_t d2h_staged, d2h_staged_bytes;     /* pageable destination, or accumulate      */
  int64_t d2h_async, d2h_async_bytes;       /* femo_vec_get_host_async                   */
  int64_t d2h_device_sum, d2h_device_sum_bytes; /* accumulate formed on the device      */
  int64_t h2d_deferred, h2d_deferred_bytes; /* of the h2d_pinned ones: femo_vec_set_host_deferred, on the copy stream */
  int64_t h2d_chunks;                       /* copies those travelled as (FEMO_H2D_CHUNK_MB; one per upload when it is 0) */
  /* the pool of pinned blocks: what a steady cycle must not do */
  int64_t pool_fresh, pool_fresh_us;        /* femo_host_alloc found no recycled block: hipHostMalloc, and the time it took */
  int64_t pool_free_deferred;               /* femo_host_free of a block with a DMA in flight: parked, recycled by a later pool
                                             * call; femo_host_free itself never waits                                      */
  int64_t pool_free_waited, pool_free_waited_us; /* releases that did wait for a DMA, and for how long: femo_host_unregister of
                                             * a caller's range with a transfer in flight (it cannot be parked)            */
} femo_host_stats;
int femo_host_alloc(int64_t bytes, void** out);
int femo_host_free(void* p);
int femo_host_trim(void);                    /* release the recycled blocks            */
int femo_host_register(void* p, int64_t bytes);   /* refused when [p, p + bytes) shares a byte with any known block    */
int femo_host_unregister(void* p);                 /* the record goes only after the runtime has let go of the range  */
int femo_host_touch(void* p);                /* the block containing p was written on the host */
int femo_host_is_pinned(const void* p, int64_t bytes);
int femo_host_threads(void);
int femo_host_fill(double* p, int64_t n, double value);   /* p[:] = value; at the base of a pinned block the library remembers
                                                            * it as that constant: sending it to a vector is a device-side fill */
int femo_host_copy(double* dst, const double* src, int64_t n);
int femo_host_axpby(int64_t n, double a, const double* x, double b, double* y);
/* Asynchronous results: femo_vec_get_host_async returns before the bytes have landed when `host` lies in a
 * pinned block (otherwise it is femo_vec_get_host).  Library entry points wait by themselves; code that reads the
 * block on its own calls femo_host_wait(p) (one block) or femo_host_sync() (all) first.                       */
int femo_host_wait(const void* p);
int femo_host_sync(void);
/* Results on demand: femo_vec_get_host_promised records the block at `host` (a whole block of femo_host_alloc) as the copy of v
 * and marks it in flight, but enqueues nothing.  The copy of femo_vec_get_host_async leaves when somebody needs the bytes
 * (femo_host_wait, femo_host_sync, any entry point that reads the block) or v is about to be written or destroyed; handed
 * back to femo_vec_set_host the block is elided like any mirror and is never read.  femo_host_forget(p): the caller will
 * never read the block under p -- a copy it was promised is dropped.  Any other `host`, a wrapped vector, less than 1 MiB, or
 * FEMO_D2H_ON_DEMAND=0 in the environment: femo_vec_get_host_async.                                                   */
int femo_vec_get_host_promised(const femo_vec* v, double* host, int64_t n);
/* The same with flags.  FEMO_PROMISE_OUTPUT: the result of an output operator (dJ/du, which goes back into the adjoint solve as
 * its right-hand side, and the explicit dJ/df, which the streamed tail overwrites from the device).  Such a promise is governed
 * by FEMO_D2H_PROMISE_OUTPUTS (default on; 0: femo_vec_get_host_async) and not by FEMO_D2H_ON_DEMAND.  femo_host_axpby(a, x, 0, y)
 * from a promised x promises y the product a x instead of sending x.                                                      */
#define FEMO_PROMISE_OUTPUT 1
int femo_vec_get_host_promised_ex(const femo_vec* v, double* host, int64_t n, int flags);
int femo_host_forget(const void* p);
int femo_host_get_stats(femo_host_stats* out);
int femo_host_reset_stats(void);

/* ---- mesh -----------------------------------------------------------------
 * x: (n_vert, tdim) row-major; conn: (n_cell, tdim+1).  n_rows <= n_vert is
 * the number of *owned* vertices (rows of every operator); vertices
 * [n_rows, n_vert) are ghosts (single-GPU: n_rows == n_vert).  Builds the
 * vertex->cell incidence and the sparsity pattern once (dolfinx create_matrix /
 * sparsity pattern [ext], utils_dolfinx.py:385).                              */
int femo_mesh_create(femo_ctx* ctx, int tdim, int64_t n_vert, int64_t n_rows,
                     const double* x, int64_t n_cell, const int32_t* conn,
                     femo_mesh** out);
int femo_mesh_destroy(femo_mesh* mesh);
int femo_mesh_info(const femo_mesh* mesh, int64_t info[FEMO_MESH_INFO_COUNT]);
/* mask[c] bit k set <=> the facet of cell c opposite its local vertex k is an exterior facet
 * (the `ds` measure of the reference's boundaryResidual, run_nonlinear_poisson_opt.py:98-117).
 * NULL clears it.                                                              */
int femo_mesh_set_boundary_facets(femo_mesh* mesh, const uint8_t* mask);
/* Partitioned meshes: bounding box (tdim doubles each) and vertex count of the WHOLE mesh, so
 * that every rank builds the same preconditioner lattice.  Call before the first BPX solve.  */
int femo_mesh_set_global(femo_mesh* mesh, const double* lo, const double* hi, int64_t n_vert_global);
/* Preconditioner lattice of the mesh (built on first use): levels and nodes of the finest one. */
int femo_mesh_pc_info(const femo_mesh* mesh, int32_t* n_levels, int64_t* finest_nodes);
/* CSR view of the pattern (rowptr: n_rows+1, col: NNZ; sorted columns).       */
int femo_mesh_pattern_csr(const femo_mesh* mesh, int64_t* rowptr, int32_t* col);

/* Host-only topology build (no GPU touched): fills the same arrays that
 * femo_mesh_create uploads.  Used by the CPU test-suite.  Buffers may be NULL
 * to query sizes via info[].                                                  */
int femo_topology_build_host(int tdim, int64_t n_vert, int64_t n_rows, int64_t n_cell,
                             const int32_t* conn, int64_t info[FEMO_MESH_INFO_COUNT],
                             int64_t* rowptr, int32_t* col);

/* Host-only plan of the BPX preconditioner lattice for `n_rows` owned vertices (no GPU touched; CPU
 * test-suite): levels and bins per axis (bins[3*l + k], coarsest level first), packed lattice
 * coordinates pk[n_rows*2] (8 B per vertex; 2-D: two words bin << 20 | 20-bit fraction, 3-D: one 64-bit word of three
 * 21-bit fields bin << 12 | 12-bit fraction), the (brick, bin) sort perm[n_rows] with
 * brick_ptr[n_bricks+1], brick_base[3*n_bricks], bin_ptr[65*n_bricks].  Array arguments may be NULL
 * (first call: sizes).                                                                           */
int femo_pc_plan_host(int dim, int64_t n_rows, const double* x, const double* lo, const double* hi,
                      int64_t n_vert_global, int32_t* n_levels, int32_t* bins, int64_t* n_bricks,
                      uint32_t* pk, int32_t* perm, int64_t* brick_ptr, int32_t* brick_base, uint32_t* bin_ptr);

/* ---- Dirichlet set (fea_dolfinx.py:169-176; dolfinx dirichletbc [ext]) ---- */
int femo_bc_create(femo_mesh* mesh, int64_t n, const int32_t* dofs, const double* vals,
                   femo_bc** out);
int femo_bc_destroy(femo_bc* bc);

/* ---- assembly -------------------------------------------------------------
 * params: up to 8 doubles of form constants (unused for POISSON; NL_POISSON: params[0] = Nitsche
 *         penalty beta (0 = none), params[1] = sgn of the nitsche_2 term: +1 symmetric (default), -1 unsymmetric).  aux: extra CG1 field of the form or NULL (NL_POISSON: the boundary data u_exact).
 *         FEMO_PDE_NL_POISSON = POISSON + int u^3 v (run_nonlinear_poisson_opt.py:88-96) and, when
 *         femo_mesh_set_boundary_facets was called, the symmetric Nitsche terms of :98-117.
 * residual: state_model.py:85 assembleVector(residual_form) -> utils:175-179; NO BCs.
 * jacobian: state_model.py:132 assembleMatrix(dR_du) (bc == NULL) and
 *           state_model.py:149 assembleSystem(dR_du, res, bcs) -> utils:189-202
 *           (bc != NULL: rows and columns of the set zeroed, diagonal 1).
 * dRdf:     state_model.py:141 assembleMatrix(derivative(res, f)); stored
 *           cell-major as (n_cell, tdim+1) values aligned with conn, i.e. the
 *           CSC of the N x n_cell matrix (column c has rows conn[c,:]).        */
int femo_assemble_residual(femo_mesh* mesh, int pde, const double* params,
                           const femo_vec* u, const femo_vec* f, const femo_vec* aux, femo_vec* r);
int femo_mat_create(femo_mesh* mesh, femo_mat** out);
int femo_mat_destroy(femo_mat* A);
int femo_assemble_jacobian(femo_mesh* mesh, int pde, const double* params,
                           const femo_vec* u, const femo_vec* f, const femo_vec* aux,
                           const femo_bc* bc, femo_mat* J);
int femo_assemble_dRdf(femo_mesh* mesh, int pde, const double* params,
                       const femo_vec* u, const femo_vec* f, femo_vec* vals);
/* The same matrix for the forms whose column c has ONE value on all its rows (Poisson-type residuals with a DG0 source:
 * dR_i/df_c = -int_c phi_i = -|T_c|/(d+1), state_model.py:136-146): cvals holds n_cell values instead of
 * (d+1) n_cell, and femo_dRdf_cell_apply is femo_dRdf_apply on that compact form (a quarter of the bytes).          */
int femo_assemble_dRdf_cell(femo_mesh* mesh, int pde, const double* params, femo_vec* cvals);
int femo_dRdf_cell_apply(femo_mesh* mesh, const femo_vec* cvals, int transpose,
                         const femo_vec* x, femo_vec* y, int accumulate);
/* host[0:n] += (dR/df)^T x, n = n_cell: femo_dRdf_cell_apply(transpose) into the scratch vector y followed by
 * femo_vec_add_to_host(y, host, n) -- and where that sum would be formed on the device (host is a whole pinned block that is
 * the exact copy of a live vector, one rank), product, sum and copy-out run range by range of FEMO_D2H_CHUNK_MB MiB
 * (default 64, fractions allowed, 0: the two steps above) with the copies on the copy stream under the next range's
 * kernel.  The same bits either way.  y holds the product or is left untouched.                                       */
int femo_dRdf_cell_apply_T_add_to_host(femo_mesh* mesh, const femo_vec* cvals, const femo_vec* x, femo_vec* y,
                                       double* host, int64_t n);
/* One pass over the mesh for any subset of: J_nobc (state_model.py:132), A_bc
 * (state_model.py:149) and the Newton right-hand side  rhs = F + K[:,bc](g-u),
 * rhs[bc] = u-g  (dolfinx NonlinearProblem.F/J [ext], utils_dolfinx.py:431).
 * Unused outputs are NULL.  Results are identical to the separate calls.       */
int femo_assemble_system(femo_mesh* mesh, int pde, const double* params,
                         const femo_vec* u, const femo_vec* f, const femo_vec* aux,
                         const femo_bc* bc, femo_mat* J_nobc, femo_mat* A_bc, femo_vec* rhs);
/* b[bc] = u[bc] - g  (dolfinx set_bc(b, bcs, x, -1.0) [ext]).                    */
int femo_bc_apply_rhs(const femo_bc* bc, const femo_vec* u, femo_vec* b);
/* Newton right-hand side with Dirichlet lifting, dolfinx NonlinearProblem.F
 * [ext] as driven by utils_dolfinx.py:431:  b = F + K[:,bc](g-u); b[bc] = u-g. */
int femo_newton_rhs(const femo_mat* K_nobc, const femo_vec* F, const femo_vec* u,
                    const femo_bc* bc, femo_vec* b);
/* The same right-hand side for a LINEAR form (linear Poisson), from its assembled operator instead of a pass over
 * the mesh:  b = K u' - L  outside the set (u' = u with g on the set, L = the load vector of f),  b[bc] = u - g;
 * bc == NULL: the plain residual K u - L.  One product with K (no BCs), the rest in its epilogue.                  */
int femo_newton_rhs_linear(const femo_mat* K_nobc, const femo_vec* f, const femo_vec* u,
                           const femo_bc* bc, femo_vec* b);
/* ... behind femo_mat_identity_solve_flag and femo_vec_axpy_if (see there) */
int femo_newton_rhs_linear_if(const femo_mat* K_nobc, const femo_vec* f, const femo_vec* u,
                              const femo_bc* bc, femo_vec* b);

/* ---- operator application (state_model.py:161-200) -------------------------
 * mat_spmv:   utils_dolfinx.py:256-264 (A*x) / :275-287 (A^T*R).
 * dRdf_apply: transpose=1: y (n_cell) = dRdf^T x (n_vert); transpose=0:
 *             y (n_rows) = dRdf x (n_cell).  accumulate=1 adds into y.         */
int femo_mat_spmv(const femo_mat* A, int transpose, const femo_vec* x, femo_vec* y);
int femo_dRdf_apply(femo_mesh* mesh, const femo_vec* vals, int transpose,
                    const femo_vec* x, femo_vec* y, int accumulate);
int femo_mat_export_csr(const femo_mat* A, int64_t* rowptr, int32_t* col, double* val);
int femo_mat_diagonal(const femo_mat* A, femo_vec* d);

/* S = diag(A)^-1/2 and the scaled copy S A S the Krylov loops iterate on, formed NOW instead of at the start of the first
 * solve with A (collective on a partitioned mesh: the ghost entries of S come from their owners).  For callers that have
 * idle time before the solve -- the operator layer assembles and scales the adjoint system of a linear form while the
 * input of the forward solve is still on its way to the device (state_model.py:117-158 reordered, same work).           */
int femo_mat_prescale(femo_mat* A);
/* On one rank, for a matrix of a form BPX takes and a mesh whose lattice hierarchy an earlier BPX solve has built, the
 * preconditioner's per-vertex weights of this operator are formed here too (they depend on S and the pinned vertices only);
 * the solves that find them in place do not form them again.  FEMO_NEWTON_FLAG=0: the weights at every solve.          */

/* ---- linear solve (fea_dolfinx.py:192-222; utils_dolfinx.py:476-512) --------
 * Jacobi-preconditioned CG on A (transpose=0) or A^T (transpose=1).  The
 * reference factorises with MUMPS; CG+Jacobi is the BASELINE.json design.
 * A must be symmetric positive definite (Poisson with Dirichlet elimination).  */
int femo_solve_cg(const femo_mat* A, int transpose, const femo_vec* b, femo_vec* x,
                  const femo_solver_opts* opts, femo_solve_info* info);

/* z = M^-1 r with the BPX preconditioner femo_solve_cg uses for A (pc = FEMO_PC_BPX), in unscaled
 * variables: M^-1 = D^-1 + 0.6 sum_l P_l C_l P_l^T (csrc/bpx.hip; restated in oracle/bpx_oracle.py).
 * For callers that drive their own Krylov loop, and for the parity tests.                         */
int femo_mat_pc_apply(const femo_mat* A, const femo_vec* r, femo_vec* z);

/* BiCGSTAB on A or A^T for non-symmetric operators (e.g. unsymmetric Nitsche terms), Jacobi
 * preconditioning by symmetric diagonal scaling; stops on ||S r||_2 <= max(rtol ||S b||_2, atol),
 * S = diag(A)^-1/2.  Same options / info as femo_solve_cg.                                      */
int femo_solve_bicgstab(const femo_mat* A, int transpose, const femo_vec* b, femo_vec* x,
                        const femo_solver_opts* opts, femo_solve_info* info);

/* ---- scalar output and its partials (output_model.py:69-87) ---------------- */
int femo_functional_value(femo_mesh* mesh, int kind, const double* params,
                          const femo_vec* u, const femo_vec* f, const femo_vec* u_d,
                          double* value);
int femo_functional_grad_u(femo_mesh* mesh, int kind, const double* params,
                           const femo_vec* u, const femo_vec* f, const femo_vec* u_d,
                           femo_vec* g);
int femo_functional_grad_f(femo_mesh* mesh, int kind, const double* params,
                           const femo_vec* u, const femo_vec* f, const femo_vec* u_d,
                           femo_vec* g);

/* ---- DG0 field expressions for projected outputs (fea_dolfinx.py:148-161) --------
 * kind 0: out_c = |grad in| (in: CG1, n_vert);  kind 1: out_c = in_c ** params[0] (in: DG0). */
int femo_cell_expression(femo_mesh* mesh, int kind, const double* params,
                         const femo_vec* in, femo_vec* out);
/* y_i = x_i / d_i  (Vec.pointwiseDivide, utils_dolfinx.py:566)                       */
int femo_vec_pointwise_divide(femo_vec* y, const femo_vec* x, const femo_vec* d, int64_t n);

/* ---- measurement helper ------------------------------------------------------
 * Launches `reps` SpMVs of A on x bracketed by HIP events on the ctx stream and
 * returns the mean device milliseconds per launch (bench.py roofline leg).     */
int femo_bench_spmv(const femo_mat* A, const femo_vec* x, femo_vec* y, int reps,
                    double* ms_per_launch);

/* ---- multi-GPU (new design; the reference is single-rank) ----
 * One process per GPU.  unique id = ncclUniqueId (128 bytes) created on rank 0
 * and broadcast by the host (torch.distributed).  After comm_init every dot
 * product inside femo_solve_cg / femo_vec_dot / femo_functional_value is
 * all-reduced over xGMI; femo_mesh_set_halo installs the ghost exchange plan:
 * for neighbour k, send_idx[send_ptr[k]:send_ptr[k+1]] are owned local indices
 * whose values go to rank nbr[k]; values received from nbr[k] land in local
 * ghost slots [n_rows + recv_ptr[k], n_rows + recv_ptr[k+1]).                  */
int femo_comm_unique_id(char id[128]);
int femo_comm_init(femo_ctx* ctx, const char id[128], int rank, int nranks);
int femo_comm_rank(const femo_ctx* ctx, int* rank, int* nranks);
int femo_mesh_set_halo(femo_mesh* mesh, int n_nbr, const int32_t* nbr,
                       const int64_t* send_ptr, const int32_t* send_idx,
                       const int64_t* recv_ptr);
int femo_halo_exchange(femo_mesh* mesh, femo_vec* x);
int femo_allreduce_sum(femo_ctx* ctx, double* host_inout, int n);

/* ---- device-initiated ghost refresh (ABI 9; new design -- the reference's ghost updates are implicit PETSc scatters,
 * utils_dolfinx.py:167,200 [ext]; SURVEY.md section 5 "distributed comm backend": IPC-mapped peer buffers over xGMI) ----
 * Instead of ncclSend/ncclRecv, a rank's producer kernels store the values a neighbour needs straight into that
 * neighbour's INBOX (uncached device memory the neighbour exported) and bump a counter there; consumers wait on their own
 * counters.  Two kernels of the compute stream per refresh -- none where the producer is the kernel that computes the
 * values anyway (the merged BPX-PCG's prolongation).  Set-up, collective over the ranks that share `mesh`'s halo plan
 * (femo_amd/dist does it through the control plane):
 *   1. every rank: femo_mesh_halo_direct_export -> 64-byte hipIpcMemHandle (other processes) / device address (same
 *      process), workgroups per producer launch;
 *   2. ranks exchange {handle, address, workgroups, their neighbour list and recv_ptr};
 *   3. every rank: femo_mesh_halo_direct_connect, per neighbour k of its plan: the neighbour's handle / address
 *      (mode 0 = handles of other processes, 1 = addresses in this process), remote_offset[k] = the neighbour's recv_ptr
 *      entry for THIS rank, remote_n_ghost[k] = its ghost count, remote_slot[k] = this rank's index in ITS neighbour
 *      list, remote_blocks[k] = its workgroups per producer launch;
 *   4. every rank: femo_mesh_halo_direct_selftest (one exchange of a known pattern through the solver's device code);
 *   5. the ranks reduce the results; femo_mesh_halo_direct_enable(mesh, all passed) -- all or none.
 * Without an enabled plan femo_halo_exchange and the solvers use ncclSend/ncclRecv as before.                        */
int femo_mesh_halo_direct_export(femo_mesh* mesh, char ipc_handle[64], uint64_t* address, int32_t* n_blocks);
int femo_mesh_halo_direct_connect(femo_mesh* mesh, int mode, const char* handles, const uint64_t* addresses,
                                  const int64_t* remote_offset, const int64_t* remote_n_ghost,
                                  const int32_t* remote_slot, const int32_t* remote_blocks);
int femo_mesh_halo_direct_selftest(femo_mesh* mesh, int* ok);
int femo_mesh_halo_direct_enable(femo_mesh* mesh, int on);
/* out = {enabled, exchanges issued, consumer time-outs seen, workgroups per producer launch} */
int femo_mesh_halo_direct_info(femo_mesh* mesh, int64_t out[4]);

/* Blocking waits of the host on the device (hipStreamSynchronize / hipEventSynchronize / hipDeviceSynchronize) the library
 * has executed in this process since the last reset -- each costs an idle device for one host round trip.  bench.py
 * divides by the cycle count (`host_syncs_per_step`).  (The reference synchronises implicitly in every PETSc / dolfinx
 * call: it has no asynchronous path, utils_dolfinx.py:155-212.)                                                      */
int femo_host_sync_stats(int64_t* count, int reset);

/* Collectives issued on this context since the last reset: out = {all-reduce calls, doubles all-reduced, neighbour
 * exchanges, doubles sent}.  What `bench.py`'s scaling record and the tests divide by the CG iteration count (the
 * reference's only collective is the ghost update of utils_dolfinx.py:32,236).                                    */
int femo_comm_stats(femo_ctx* ctx, int64_t out[4], int reset);

/* ---- Reissner-Mindlin shell (examples/test_shell_m3l/shell_pde.py:219-332) ----------
 * State w = (u_mid in CG2^3, theta in CG1^3) on flat triangular facets: 3 dofs per P2 node (vertices [0, n_vert), then
 * edge midpoints), then 3 per vertex; thickness h and surface load f are CG1 fields at the vertices (shell_pde.py:
 * 228-231).  Formulation: oracle/shell_oracle.py (membrane + bending + shear + drilling energies, ElasticModel of the
 * un-vendored shell_analysis_fenicsx restated from its published source, pinned by the Scordelis-Lo roof).
 * The host side (femo_amd/fea/shell.py) numbers the edges and builds the CSR pattern of the element couplings:
 *   cell_edges[c][k] = edge of local edge k = (0,1), (1,2), (2,0);   rowptr / cols: pattern over the n_dof dofs;
 *   elem_pos[c][27 i + j] = CSR position of the coupling of local dofs i, j (local order: 6 displacement nodes x 3
 *   components, then 3 rotation nodes x 3).
 * Matrices are plain value arrays (femo_vec of nnz entries) on that pattern.                                        */
int femo_shell_create(femo_ctx* ctx, int64_t n_vert, const double* x, int64_t n_cell, const int32_t* conn, int64_t n_edge,
                      const int32_t* cell_edges, const int64_t* rowptr, const int32_t* cols, const int32_t* elem_pos,
                      femo_shell** out);
int femo_shell_destroy(femo_shell* s);
int64_t femo_shell_ndof(const femo_shell* s);
int64_t femo_shell_nnz(const femo_shell* s);
/* K(h): stiffness of the elastic energy (pdeRes / elasticEnergy, shell_pde.py:246-253); dR/dw of the linear residual */
int femo_shell_assemble(femo_shell* s, double E, double nu, const femo_vec* h, femo_vec* vals);
/* y = K x; fixed_dev != NULL (device array of n_dof bytes): the operator with strongly imposed dofs as identity rows/columns */
int femo_shell_matvec(femo_shell* s, const femo_vec* vals, const uint8_t* fixed_dev_or_null, const femo_vec* x, femo_vec* y);
/* F (+)= sign * int f . v (weakFormResidual's load term) and its transpose: out (+)= sign * (dF/df)^T lambda */
int femo_shell_load(femo_shell* s, const femo_vec* f, double sign, int accumulate, femo_vec* F);
int femo_shell_load_T(femo_shell* s, const femo_vec* lam, double sign, int accumulate, femo_vec* out);
/* out_b (+)= v^T (dK/dh_b) w -- (dR/dh)^T lambda for R = K(h) w - F with v = lambda; *energy = 1/2 v^T K w (shell_pde.py:299-302) */
int femo_shell_dform_dh(femo_shell* s, double E, double nu, const femo_vec* h, const femo_vec* v, const femo_vec* w,
                        int accumulate, femo_vec* out, double* energy);
/* y (+)= (dK/dh [dh]) w: the FORWARD product with the thickness partial of the elastic residual (the fwd branch of
 * compute_jacvec_product, state_model.py:176-188); the exact transpose of femo_shell_dform_dh: <v, y> = <dh, out>.         */
int femo_shell_dform_dh_fwd(femo_shell* s, double E, double nu, const femo_vec* h, const femo_vec* dh, const femo_vec* w,
                            int accumulate, femo_vec* y);
/* 1/2 int u_mid . u_mid (shell_pde.py:287-288) and its gradient; int rho h (shell_pde.py:293-294) and its gradient */
int femo_shell_compliance(femo_shell* s, const femo_vec* w, double* value, int accumulate, femo_vec* grad);
int femo_shell_mass(femo_shell* s, double rho, const femo_vec* h, double* value, int accumulate, femo_vec* grad);
/* The compliance over a tagged subset of cells -- the `dxx` measure the shell drivers pass (shell_pde.py:66,284-285:
 * dx_2(10)): cell_weight is a DG0 indicator (n_cell doubles; NULL: the whole surface).                                 */
int femo_shell_compliance_dx(femo_shell* s, const femo_vec* w, const femo_vec* cell_weight, double* value, int accumulate, femo_vec* grad);
/* Thickness regularisation of `compliance` (shell_pde.py:262-282, ShellPDE.regularization): kind 1 'H1', 2 'L2H1',
 * 3 'L2' (alpha1 = 1e3, alpha2 = 1, h_mesh = CellDiameter); value and/or grad (+)= d/dh.  femo_shell_hpower: int coef h^p dx
 * with the degree-4 rule -- the thickness term of pnorm_stress(regularization=True), shell_pde.py:307-309.              */
int femo_shell_regularization(femo_shell* s, int kind, const femo_vec* h, double* value, int accumulate, femo_vec* grad);
int femo_shell_hpower(femo_shell* s, double coef, double p, const femo_vec* h, double* value, int accumulate, femo_vec* grad);
/* Penalty form of the boundary conditions, `pdeRes(..., penalty=True, dss, dSS, g)` (shell_pde.py:34,59-61,246-253 ->
 * ElasticModel.weakFormResidual of the un-vendored shell_analysis_fenicsx; restated in oracle/shell_oracle.py::
 * penalty_matrix in the idiom of the tree's other penalty terms, run_poisson_opt.py:60, motor_pde.py:177-178):
 *     R_pen(dw) = sum over tagged edges of coef_e int_e (w - g) . dw,    coef_e = beta (1/h_E('+') + 1/h_E('-')),
 * all six fields of w, exterior (ds) and interior (dS) facets alike.  The host passes per tagged edge its three
 * displacement nodes (end vertices, midpoint node), coef_e |e| and the CSR positions of its 3 x (9 + 4) entries
 * (component-major; 9 displacement pairs row-major over (v0, v1, mid), then 4 rotation pairs over (v0, v1)).
 * femo_shell_penalty_add: vals += K_pen (after femo_shell_assemble);  femo_shell_penalty_apply: y (+)= K_pen (x - g).   */
int femo_shell_set_penalty(femo_shell* s, int64_t n_edges, const int32_t* edge_nodes, const double* coef, const int32_t* pos);
int femo_shell_penalty_add(femo_shell* s, femo_vec* vals);
int femo_shell_penalty_apply(femo_shell* s, const femo_vec* x, const femo_vec* g, int accumulate, femo_vec* y);
/* Inertial residual, `kinetic_residual(rho, h)` (shell_pde.py:255-256 -> ElasticModel.inertialResidual [absent package];
 * its use with accelerations: run_aeroelasticity_dynamic.py:93): y (+)= M(h) acc with
 * M = int rho h N_a N_b (displacements) + int rho h^3/12 phi_a phi_b (rotations), consistent, degree-4 rule;
 * femo_shell_inertia_dh: out_b (+)= lam^T (dM/dh_b) acc, its thickness partial transposed.                             */
int femo_shell_inertia_apply(femo_shell* s, double rho, const femo_vec* h, const femo_vec* acc, int accumulate, femo_vec* y);
int femo_shell_inertia_dh(femo_shell* s, double rho, const femo_vec* h, const femo_vec* lam, const femo_vec* acc, int accumulate, femo_vec* out);
/* y (+)= (dM/dh [dh]) acc: the same for the inertial residual.                                                           */
int femo_shell_inertia_dh_fwd(femo_shell* s, double rho, const femo_vec* h, const femo_vec* dh, const femo_vec* acc, int accumulate, femo_vec* y);
/* L2 projection of the von Mises stress onto CG1 (shell_pde.py:315-332; the field output of the shell drivers,
 * shell_dynamic_pde.py:82-83,129): rhs_i = int sigma_vm phi_i, lumped_i = row sum of the P1 mass matrix (may be NULL);
 * femo_shell_p1_mass: y = M x with that mass matrix (the host side runs Jacobi-CG with it, utils_dolfinx.py:549-583). */
int femo_shell_vm_rhs(femo_shell* s, double E, double nu, const femo_vec* h, const femo_vec* w, double surface, femo_vec* rhs,
                      femo_vec* lumped);
int femo_shell_p1_mass(femo_shell* s, const femo_vec* x, femo_vec* y);
/* J = 1 / alpha int (m sigma_vm)^rho dx: the aggregated von Mises stress of the shell drivers (shell_pde.py:297-313,
 * `pnorm_stress`; sigma(z) = C (eps + z kappa) at z = surface * h / 2, surface = +1 top, 0 mid, -1 bottom as in
 * shell_pde.py:315-328).  value and/or partials: grad_w (+)= dJ/dw (n_dof), grad_h (+)= dJ/dh (n_vert).             */
int femo_shell_pnorm_stress(femo_shell* s, double E, double nu, const femo_vec* h, const femo_vec* w, double m, double rho, double alpha,
                            double surface, double* value, int accumulate, femo_vec* grad_w, femo_vec* grad_h);
/* Lattice preconditioner for femo_shell_solve (opts->pc = 1): M^-1 = D^-1 + sum_l P_l C_l P_l^T, P_l = trilinear
 * interpolation from nested lattices over the bounding cube (2, 4, ... cells per axis) to the dof nodes, per component,
 * C_l = 1 / diag(P_l^T K P_l) (recomputed on the device when K or the Dirichlet set change).  The host passes
 *   ell_idx / ell_w   P of every level: 8 (lattice unknown, weight) pairs per level and dof (width = 8 n_levels);
 *                     lattice unknown = 6 * node + field, nodes numbered level by level (level_offsets, n_levels + 1)
 *   pt_*              the finest level's P^T as CSR over all 6 n_nodes unknowns
 *   par_* / chi_*     node-level transfers between consecutive lattices: parents (<= 8) and children (<= 27) of a node. */
int femo_shell_pc_create(femo_shell* s, int width, int64_t n_nodes, int n_levels, const int64_t* level_offsets,
                         const int32_t* ell_idx, const double* ell_w,
                         const int64_t* pt_rowptr, const int32_t* pt_cols, const double* pt_vals,
                         const int64_t* par_rowptr, const int32_t* par_cols, const double* par_vals,
                         const int64_t* chi_rowptr, const int32_t* chi_cols, const double* chi_vals);
/* Exact coarse solve for the lattice preconditioner (optional, after femo_shell_pc_create): on lattice level `level`
 * (not the finest; 6 x nodes <= 8192 unknowns) the Galerkin operator P^T K P is formed as a dense matrix on the device,
 * factorised by the library's own blocked Cholesky + triangular inverse on the fp64 matrix cores (shell_coarse.hip) whenever
 * the stiffness or the Dirichlet set change, and A^-1 = L^-T L^-1 applied in place
 * of the diagonal levels 0 .. level: M^-1 = D^-1 + sum_{l > level} P_l C_l P_l^T + P_c (P_c^T K P_c)^-1 P_c^T.  What
 * the reference's direct solver (MUMPS, utils_dolfinx.py:476-512) does for the whole matrix is done here for the
 * ~3000 unknowns that carry the smooth, nearly inextensional modes a diagonal cannot see.
 *   node_xyz   int32[3 x nodes]: lattice coordinates of the level's nodes (level-local numbering)
 *   item_*     work items of the Galerkin kernel: points (first dof / 3) of one coarse cell and one field group, any
 *              number each, 256 by default (item_ptr n_items + 1, item_pts), and the level-local numbers of the 4 x 4 x 4 nodes around
 *              the cell (item_nbr 64 per item, x fastest, -1 where the surface does not touch the lattice)
 *   down_*     optional (NULL: level by level): composite restriction from the finest lattice's nodes to the nodes of
 *              levels `level` .. n_levels - 2 as CSR (rows in node order, columns = node numbers on the finest lattice):
 *              one launch per iteration in place of n_levels - 1 - level                                             */
int femo_shell_pc_coarse(femo_shell* s, int level, const int32_t* node_xyz, int64_t n_items, const int64_t* item_ptr,
                         const int32_t* item_pts, const int32_t* item_nbr, const int64_t* down_rowptr, const int32_t* down_cols,
                         const double* down_vals);
/* For tests: the dense coarse operator (inverse = 0) or the factors of its inverse (1: L^-T above, L^-1 below the
 * diagonal) for `vals` and the mask, row-major n x n into `out` (host; NULL: only *n_out).                           */
/* Hermite-type lattice spaces on the hierarchy of femo_shell_pc_create / femo_shell_pc_coarse (round 4): the nodal rotations
 * of a lattice act as the slopes of its displacement interpolation, u = sum_n [alpha_n U_n + Theta_n x sigma_n], so coarse
 * lattices reproduce bending modes instead of locking on them (the solve that stands where the reference factorises with
 * MUMPS, shell_pde.py:246-253, needs about half the iterations).  fin_w4: (alpha, sigma) per (point, corner) of the finest
 * lattice ((w, 0, 0, 0) for rotation points); hp_*: P_L^T by finest node -- row 2 k lists the displacement points of node k
 * (first dof, w4), row 2 k + 1 its rotation points; par_w5 / chi_w5: (a, b, c) per entry of the parent / child CSR;
 * lvl_w4: composed weights of the levels above the coarse solve, [level][point][8][4]; cs_w4: of the coarse-solve level;
 * down_*: composite restriction finest lattice -> levels cs .. L - 2 in (A, B, C) form (optional).  On a partitioned shell: the
 * rows of the rank's local points on the global lattice (the Galerkin sums are all-reduced like the trilinear ones).       */
int femo_shell_pc_hermite(femo_shell* s, const float* fin_w4, const int64_t* hp_rowptr, const int32_t* hp_cols, const float* hp_w4,
                          const double* par_w5, const double* chi_w5, const float* lvl_w4, const float* cs_w4,
                          const int64_t* down_rowptr, const int32_t* down_cols, const double* down_w5);
/* What the device side runs with: out = {Hermite-type data uploaded, bit 0: Hermite-type spaces enabled (not fallen back) |
 * bit 1: in use for the last stiffness set up, coarse solve factorised, node blocks ready}.  The library falls back to the trilinear hierarchy (once, with a warning
 * on stderr) when the Hermite-type coarse operator cannot be factorised; reports and pinned iteration counts read this.  */
int femo_shell_pc_info(const femo_shell* s, int32_t out[4]);
/* Items of the node-block set-up for the Hermite-type spaces (optional; without it the blocks are formed row by row, 10.5
 * instead of ~2 ms at 1.97 M dofs): for every level above the coarse solve (item_lvl = level - cs_level - 1) the points grouped by
 * the lattice cell that contains them, at most 64 per item (item_ptr into item_pts; every point once per level);
 * pcell[level][point] = the cell's coordinates packed as x | y << 10 | z << 20.                                        */
int femo_shell_pc_block_items(femo_shell* s, int64_t n_items, const int64_t* item_ptr, const int32_t* item_lvl, const int32_t* item_pts,
                              const int32_t* pcell);
/* Weights of the additive parts of the lattice preconditioner: w_levels multiplies the node-block corrections of the levels
 * between the coarse solve and the finest lattice (default 0.3: the overlapping levels overshoot when summed with weight 1,
 * like the Poisson BPX's theta; 145 -> 105 iterations on the 1.97 M-dof roof), w_coarse the exact coarse solve (default 1).
 * Both must be positive.  Takes effect at the next set-up (the next solve).                                               */
int femo_shell_pc_weights(femo_shell* s, double w_levels, double w_coarse);
/* z = M^-1 r of the lattice preconditioner for the stiffness `vals` and the mask (set up if needed): what the parity tests
 * compare with the oracle's operator.  One rank.                                                                      */
int femo_shell_pc_apply(femo_shell* s, const femo_vec* vals, const uint8_t* fixed_host, const femo_vec* r, femo_vec* z);
int femo_shell_pc_coarse_matrix(femo_shell* s, const femo_vec* vals, const uint8_t* fixed_host, int inverse, double* out,
                                int64_t* n_out);
/* K x = b with x = xfix on the dofs flagged in fixed_host (n_dof bytes; NULL: none; xfix NULL: zero values).
 * PCG, sqrt(r.M^-1 r) <= max(rtol sqrt(r0.M^-1 r0), atol), opts->pc: 0 Jacobi, 1 lattice; K is symmetric, so the
 * adjoint solve (fea_dolfinx.py:208-222) is the same call.  The reference uses MUMPS (utils_dolfinx.py:476-512).
 * info->converged: 1 tolerance met, 2 stalled at the attainable accuracy (residual below 1e-9 of the initial one in the
 * preconditioner's norm and no progress over 8 batches of check_every iterations), 0 max_it, -1 breakdown (NaN).      */
int femo_shell_solve(femo_shell* s, const femo_vec* vals, const uint8_t* fixed_host, const femo_vec* xfix, const femo_vec* b,
                     femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info);
/* The shell on the N ranks of a context (femo_comm_init; the reference is single-rank, SURVEY.md section 0.3 -- the
 * partitioning of section 8(e) applied to the shell).  Each rank creates its handle on the cells that touch a point it
 * owns (a point: a P2 node with its three displacements or a vertex with its three rotations, dofs 3 p .. 3 p + 2),
 * builds the lattice arrays of femo_shell_pc_create / _pc_coarse on the GLOBAL lattice (same nodes on every rank, the
 * rows of its own points), then declares the partition:
 *   owned_points  uint8[n_dof / 3]: 1 for the points this rank owns
 *   nbr           the ranks it exchanges with; segment k of send_dofs (send_ptr) lists the owned dofs rank nbr[k] holds
 *                 copies of, segment k of recv_dofs (recv_ptr) the local dofs of the points rank nbr[k] owns, in the order
 *                 that rank sends them.
 * From then on femo_shell_assemble / _penalty_add leave the rows of points owned elsewhere zero (the rank's share of K:
 * owned rows are complete because every cell around an owned point is local), femo_shell_solve masks the right-hand
 * side the same way, refreshes the search direction on the halo before every product, all-reduces its two scalars, the
 * restricted residual on the finest lattice and -- per stiffness -- the Galerkin blocks and the dense coarse operator,
 * and returns x consistent on all local points.  Values of outputs are all-reduced: integrate over owned cells only
 * (femo_shell_compliance_dx with the ownership indicator as cell weight).
 * femo_shell_halo: x on the points owned elsewhere <- the owners' values.  femo_shell_mask_unowned: x <- 0 there.        */
int femo_shell_set_partition(femo_shell* s, const uint8_t* owned_points, int n_nbr, const int32_t* nbr, const int64_t* send_ptr,
                             const int32_t* send_dofs, const int64_t* recv_ptr, const int32_t* recv_dofs);
/* Partitioned shells: the local cells whose SCALAR outputs (mass, volume, p-norm stress, elastic energy, regularisation and
 * h-power terms; shell_pde.py:262-313) this rank integrates -- one rank per cell of the whole mesh, the values are summed
 * over the ranks.  Gradients are integrated over all local cells (complete on the points the rank owns).                */
int femo_shell_set_owned_cells(femo_shell* s, const uint8_t* owned_cells);
int femo_shell_halo(femo_shell* s, femo_vec* x);
int femo_shell_mask_unowned(femo_shell* s, femo_vec* x);

/* ---- SIMP topology optimisation (examples/beam_topo_opt/run_topo_opt_cantilever_beam.py) ------------------------------
 * Linear elasticity on the P1 simplices of a femo_mesh: state u in VectorFunctionSpace(mesh, ("CG", 1)), blocked dofs
 * dof = d * vertex + component (d = tdim), one DG0 density rho_e per cell.
 *   R(u; rho) = sum_e C(rho_e) int_e sigma_0(u) : eps(v) dx - int_ds t . v ds            (pdeRes, :85-101)
 *   C = rho^3 (FEMO_ELAST_SIMP) or rho / (1 + 8 (1 - rho)) (FEMO_ELAST_RAMP); sigma_0 = lambda_0 tr(eps) I + 2 mu_0 eps
 * K(rho) is stored as one d x d fp64 block per entry of the mesh's scalar SELL pattern (the column index is shared with the
 * scalar operators), assembled vertex by vertex without atomics, so K is deterministic and symmetric entry for entry.
 * Single GPU only: a mesh with a halo plan is refused.                                                                   */
enum { FEMO_ELAST_SIMP = 0, FEMO_ELAST_RAMP = 1 };
enum { FEMO_ELAST_INFO_DIM = 0, FEMO_ELAST_INFO_NDOF = 1, FEMO_ELAST_INFO_NNZ = 2, FEMO_ELAST_INFO_SELL = 3,
       FEMO_ELAST_INFO_SPMV_BYTES = 4, FEMO_ELAST_INFO_COUNT = 5 };
/* FEA(mesh) + VectorFunctionSpace(mesh, ("CG", 1)) with E, nu of pdeRes (:85-93)                                        */
int femo_elast_create(femo_mesh* mesh, double E, double nu, femo_elast** out);
int femo_elast_destroy(femo_elast* e);
/* [dim, n_dof, nnz of the scalar pattern, SELL entries, bytes one block SpMV moves: nnz (4 + 8 d^2) + n_vert 16 d + rowptr] */
int femo_elast_info(const femo_elast* e, int64_t info[FEMO_ELAST_INFO_COUNT]);
/* Strong Dirichlet dofs (fea.add_strong_bc, :152-156): mask[n_dof] = 1 on fixed dofs; NULL clears.  Used by the masked
 * products (identity rows and columns) and by the block-Jacobi inverse of the next femo_elast_assemble.                  */
int femo_elast_set_fixed(femo_elast* e, const uint8_t* mask);
/* Elastic supports (a workpiece or port spring, a Winkler foundation, a structure held by springs alone): k[n_dof] >= 0, one
 * stiffness per dof, host memory; NULL or all zeros clears them.  A NaN, an infinity or a negative entry is refused and
 * leaves the handle as it was.  From the next femo_elast_assemble on the handle's operator is K_s(rho) = K(rho) + diag(k):
 * products, residual, export, block-Jacobi, the shifted and banded operators of the dynamic paths, the eigen and buckling
 * pencils and the lattice blocks of the multilevel preconditioner (P_l^T diag(k) P_l) all follow.  The call invalidates the
 * assembled operator: products and solves are refused until the next femo_elast_assemble.  A spring on a fixed dof is
 * legal: the masked operator keeps its identity row and column there, the unmasked one (and the lifting F - K_s g) carries
 * it.  The springs do not depend on rho: dR/drho is unchanged.                                                           */
int femo_elast_set_springs(femo_elast* e, const double* k /* [n_dof] or NULL */);
/* Tagged boundary facets of ds_(100) (locate_entities_boundary + meshtags, :44-52): d vertex ids per facet.             */
int femo_elast_set_facets(femo_elast* e, int64_t n_facets, const int32_t* facet_verts);
/* K(rho) (dolfinx assemble_matrix of derivative(pdeRes, u), fea_dolfinx.py / state_model.py:117-158) and the inverted
 * diagonal blocks of the preconditioner (rows / columns of fixed dofs replaced by the identity).                         */
int femo_elast_assemble(femo_elast* e, int method, const femo_vec* rho);
/* y = a K x + b f  (masked = 0) or  y = a A x + b f  with A = K with identity rows / columns on the fixed dofs (masked = 1,
 * the A of state_model.py:149).  f may be NULL (b ignored).  a = 1, b = -1 gives the residual R = K u - F of
 * assembleVector(pdeRes) in the same launch (state_model.py:75-85).                                                     */
int femo_elast_apply(femo_elast* e, int masked, double a, const femo_vec* x, double b, const femo_vec* f, femo_vec* y);
/* F = int_ds t . v ds for a constant traction t[d] (Constant(mesh, (0, -1/4)), :73): t |f| / d per facet vertex.       */
int femo_elast_load(femo_elast* e, const double* t, femo_vec* F);
/* dR/drho (assemble_matrix of derivative(pdeRes, rho)), column e = C'(rho_e) K0_e u_e, matrix free:
 *   transpose = 1:  y[n_cell] (+)= C'(rho_e) x_e^T K0_e u_e       (state_model.py:190-200, rev mode)
 *   transpose = 0:  y[n_dof]  (+)= sum_e C'(rho_e) x_e K0_e u_e   (state_model.py:176-188, fwd mode; vertex walk)     */
int femo_elast_drho(femo_elast* e, int method, int transpose, const femo_vec* rho, const femo_vec* u, const femo_vec* x,
                    femo_vec* y, int accumulate);
/* Aggregated von Mises stress of the SOLID material (a stress constraint beside the volume constraint):
 *   J = 1/alpha sum_e |T_e| (m rho_e^q sigma_vm,e)^p,   sigma_vm = sqrt(3/2 s : s),  s = dev sigma_0(u) as a 3 x 3 tensor
 * (plane strain in 2-D: sigma_zz = lambda_0 tr eps), lambda_0, mu_0 from femo_elast_create.  rho_e^q sigma_vm is the
 * qp-relaxed cell stress (q = 0: the solid stress).  Any of the outputs may be NULL:
 *   value             J, folded on the device in a fixed order (the call waits for it)
 *   grad_u[n_dof]     (+)= dJ/du, vertex walk without float atomics: the same bits every call
 *   grad_rho[n_cell]  (+)= dJ/drho_e = p q / rho_e J_e
 * accumulate = 1 adds onto both gradients.  A cell with sigma_vm = 0 contributes 0 to all three.  Needs m > 0, p >= 1,
 * q >= 0, alpha > 0; rho_e > 0 is the caller's contract when q > 0.                                                     */
int femo_elast_pnorm_stress(femo_elast* e, const femo_vec* rho, const femo_vec* u, double m, double p, double q, double alpha,
                            double* value, femo_vec* grad_u, femo_vec* grad_rho, int accumulate);
/* out_cells[n_cell] = rho_e^q sigma_vm,e, the cell field of the aggregate above; rho may be NULL when q == 0.  The value is
 * written as it is: a non-finite state gives a non-finite stress in the cells it touches.  Both entry points are the
 * one-column case (m, w = 1, scale = 1) of the _multi forms below and run one-column instantiations of the same kernels
 * (csrc/elast_stress.hip); femo_elast_apply and femo_elast_drho likewise share one body each with their _multi forms.    */
int femo_elast_von_mises(femo_elast* e, const femo_vec* rho, const femo_vec* u, double q, femo_vec* out_cells);
/* A x = b by device-resident PCG with the block-Jacobi preconditioner (solveKSP_mumps, utils_dolfinx.py:476-493); K is
 * symmetric, so the adjoint solve is the same call.  Fixed dofs: x = b there.  Stops on sqrt(r^T M^-1 r) <=
 * max(rtol sqrt(r0^T M^-1 r0), atol); convergence is polled every check_every iterations (0 = 32, or 8 with the
 * multilevel preconditioner).  opts->pc: FEMO_ELAST_PC_MULTILEVEL selects the preconditioner below (an error unless
 * femo_elast_pc_setup was called); every other value is block-Jacobi (M = the diagonal blocks), as before the field was read. */
enum { FEMO_ELAST_PC_JACOBI = 0, FEMO_ELAST_PC_MULTILEVEL = 1 };
int femo_elast_solve(femo_elast* e, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info);
/* Several load cases at once (csrc/elast_solve.hip).  n_cols columns, 1 <= n_cols <= FEMO_ELAST_MAX_COLS, lie one after
 * the other in ONE femo_vec of length n_cols * n_dof: column l starts at l * n_dof and keeps the blocked layout
 * d * vertex + component.  All columns share K(rho), the fixed set and the preconditioner.                               */
enum { FEMO_ELAST_MAX_COLS = 8 };
/* y_l = a Op x_l + b f_l for every column in one launch (Op = K or the masked A, as femo_elast_apply; f may be NULL).
 * A thread keeps the accumulators of up to 4 columns and reads each d x d block, column index and fixed byte
 * once for them; more columns take further passes inside the same launch.                                               */
int femo_elast_apply_multi(femo_elast* e, int masked, int n_cols, double a, const femo_vec* x, double b, const femo_vec* f,
                           femo_vec* y);
/* femo_elast_solve for n_cols right-hand sides in one PCG loop: every launch of an iteration carries all columns, so an
 * iteration costs the launches of a single-column one (5 with block-Jacobi, 8 with the multilevel preconditioner).  Each
 * column has its own scalars and its own stopping test sqrt(r_l^T M^-1 r_l) <= max(rtol sqrt(r0_l^T M^-1 r0_l), atol); a
 * column that converged, broke down (NaN) or met the test at iteration 0 (a zero right-hand side) is frozen: its x is not
 * touched again while the others go on.  The host polls all columns every check_every iterations and stops when every
 * column is finished or max_it is reached.  info[l]: iterations, converged, residual and rhs norm of column l; solve_ms
 * is the device time of the whole batched solve, in every info[l].  Within a column the sums run in the order of
 * femo_elast_solve: no float atomics, the same bits every call.                                                         */
int femo_elast_solve_multi(femo_elast* e, int n_cols, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts,
                           femo_solve_info* info /* [n_cols] */);
/* femo_elast_drho with n_cols states u_l (u: n_cols * n_dof):
 *   transpose = 1:  y[n_cell] (+)= sum_l C'(rho_e) x_{l,e}^T K0_e u_{l,e}      (x: n_cols * n_dof)
 *   transpose = 0:  y_l[n_dof] (+)= sum_e C'(rho_e) x_e K0_e u_{l,e}           (x: n_cell, y: n_cols * n_dof)             */
int femo_elast_drho_multi(femo_elast* e, int method, int transpose, int n_cols, const femo_vec* rho, const femo_vec* u,
                          const femo_vec* x, femo_vec* y, int accumulate);
/* femo_elast_pnorm_stress for n_cols states u_l in one pass (csrc/elast_stress.hip): one aggregate per load case,
 *   J_l = 1/alpha sum_e |T_e| (m_l rho_e^q sigma_vm,e(u_l))^p,     J = sum_l w_l J_l
 * with one scale m_l > 0 per load case, weights w_l >= 0 (NULL = 1), and p, q, alpha shared.  The cell geometry and rho^q
 * are computed once per cell (and once per cell visit of the vertex walk) for all columns.  Any output may be NULL:
 *   values[n_cols]          the UNWEIGHTED J_l, folded on the device in a fixed order (one copy, one wait per call)
 *   grad_u[n_cols * n_dof]  column l (+)= w_l dJ_l/du_l; without accumulate a column with w_l = 0 is written as zeros
 *   grad_rho[n_cell]        (+)= sum_l w_l p q / rho_e J_{l,e}, summed in ascending l
 * The zero-stress guard holds per (cell, column): a column with u_l = 0 gives exact zeros.  No float atomics: the same bits
 * every call.                                                                                                             */
int femo_elast_pnorm_stress_multi(femo_elast* e, int n_cols, const femo_vec* rho, const femo_vec* u,
                                  const double* m /* [n_cols] */, const double* w /* [n_cols] or NULL */, double p, double q,
                                  double alpha, double* values /* [n_cols] or NULL */, femo_vec* grad_u, femo_vec* grad_rho,
                                  int accumulate);
/* Aggregated nodal displacement of n_cols states u_l in one pass (csrc/elast_disp.hip): "no vertex of this region moves more
 * than delta" as one smooth output,
 *   J_l = 1/alpha sum_v a_v (m_l |u_{l,v}|)^p,     J = sum_l w_l J_l,     |u_v| = the Euclidean norm of the d components
 * with nodal weights a[n_vert] >= 0 (a device vector: 1 on a vertex list, the lumped facet or cell measure of a region), one
 * scale m_l > 0 per load case, weights w_l >= 0 (NULL = 1), p >= 1, and alpha = sum_v a_v when alpha <= 0 is passed.  Either
 * output may be NULL:
 *   values[n_cols]          the UNWEIGHTED J_l, folded on the device in a fixed order (the call waits for them)
 *   grad_u[n_cols * n_dof]  column l (+)= w_l dJ_l/du_l, dJ_l/du_{l,v,i} = p/alpha a_v m_l^p |u_v|^(p-2) u_{v,i}; without
 *                           accumulate a column with w_l = 0 is written as zeros
 * A vertex with |u_v| == 0 contributes exact zeros (never a NaN); a vertex with a_v == 0 is skipped without reading u.  A
 * non-finite entry of u shows in J_l of its column and in the d gradient entries of its vertex, nowhere else.  No float
 * atomics: the same bits every call, and column l does not depend on n_cols.                                              */
int femo_elast_pnorm_disp_multi(femo_elast* e, int n_cols, const femo_vec* u, const femo_vec* a /* [n_vert] */,
                                const double* m /* [n_cols] */, const double* w /* [n_cols] or NULL */, double p, double alpha,
                                double* values /* [n_cols] or NULL */, femo_vec* grad_u, int accumulate);
/* out_cells[n_cell] = max_l scale_l rho_e^q sigma_vm,e(u_l), the envelope over the load cases (column = -1), or
 * scale_column rho_e^q sigma_vm,e(u_column) (0 <= column < n_cols).  scale > 0 per load case, NULL = 1; rho may be NULL
 * when q == 0.  With n_cols > 1 a NaN stress reads as 0 in the maximum; one column is written as it is.                */
int femo_elast_von_mises_multi(femo_elast* e, int n_cols, const femo_vec* rho, const femo_vec* u,
                               const double* scale /* [n_cols] or NULL */, double q, int column, femo_vec* out_cells);
/* Body loads: self-weight and inertial load cases (csrc/elast_body.hip).  A body force b_l in R^d (mass density times
 * acceleration) is constant per load case; the mass is linear in the density, so the load is F_l(rho) = T_l + (G_B rho)_l
 * with the linear operator G_B of B = (b_0 ... b_{n_cols-1}), b: n_cols * 3 doubles, unused components 0:
 *   transpose = 0:  y[l n_dof + d v + i] = [accumulate ? y : (base ? base : 0)] + a b_l[i] sum_{c around v} x_c |T_c| / (d+1)
 *                   (x: n_cell, y and base: n_cols * n_dof; base may be NULL).  zero_fixed = 1 writes 0 on the dofs of the
 *                   fixed set of every column instead (needs femo_elast_set_fixed): with base = the traction columns that is
 *                   the right-hand side for homogeneous supports in the same launch.
 *   transpose = 1:  y[c] = (accumulate ? y[c] : 0) + a |T_c| / (d+1) sum_l b_l . sum_{v in c} x_l[v]
 *                   (x: n_cols * n_dof, y: n_cell; base NULL and zero_fixed 0), summed in ascending l.
 * dR/drho of R_l = K(rho) u_l - F_l(rho) is femo_elast_drho_multi - G_B, and d/drho of sum_l w_l F_l(rho) . u_l is G_{wB}^T u.
 * One launch for all columns either way; the vertex sum and the cell volume are formed once for all of them.  No float
 * atomics: the same bits every call, and column l does not depend on n_cols.                                             */
int femo_elast_body_apply(femo_elast* e, int n_cols, const double* b /* [n_cols * 3] */, int transpose, double a,
                          const femo_vec* x, const femo_vec* base /* or NULL */, int zero_fixed, femo_vec* y, int accumulate);
/* Thermal expansion load (csrc/elast_thermal.hip).  sigma = C(rho) (sigma_0(u) - beta_0 theta I) on the 3 x 3 tensor, with
 * beta_0 = (3 lambda_0 + 2 mu_0) alpha from the handle's lambda_0, mu_0 (the same constant in plane strain and in 3-D) and
 * theta = T - t_ref, T the P1 field `temp` (n_vert nodal values) or, with temp = NULL, the uniform value t_uniform.  The load
 * of load case l is s_l H(C(rho); theta) with
 *   H(w; theta)[d v + i] = sum_{c around v} w_c beta_0 thetabar_c |T_c| d_i phi_v^c,   thetabar_c = the mean of theta over c
 * (exact for P1 theta: div v is constant per cell).  C and C' are those of `method`; column l at l * n_dof; s: n_cols scales.
 *   FEMO_ELAST_THERMAL_N:       y_l = [accumulate ? y_l : (base ? base_l : 0)] + a s_l H(w; theta), w = C(rho) with x = NULL
 *                               and w_c = C'(rho_c) x_c with the cell vector x (dR/drho forward; dR/dT forward is the call
 *                               with temp = dT and t_ref = 0).  y and base: n_cols * n_dof.  zero_fixed = 1 writes 0 on the dofs
 *                               of the fixed set of every column instead (needs femo_elast_set_fixed).
 *   FEMO_ELAST_THERMAL_T_RHO:   y[c] = (accumulate ? y[c] : 0) + a C'(rho_c) beta_0 thetabar_c |T_c| sum_l s_l div(x_l)_c
 *   FEMO_ELAST_THERMAL_T_TEMP:  y[v] = (accumulate ? y[v] : 0) + a sum_{c around v} C(rho_c) beta_0 |T_c| / (d+1) sum_l s_l div(x_l)_c
 *                               (x: n_cols * n_dof; y: n_cell resp. n_vert; base NULL and zero_fixed 0; div(x)_c = sum_a
 *                               grad phi_a . x[a]; summed in ascending l; temp and t_uniform are not read by T_TEMP).
 * They are the transposes of w -> N and of theta -> N.  One launch for all columns; no float atomics: the same bits every
 * call, and column l does not depend on n_cols.  A non-finite density or temperature reaches y.  One rank only.           */
enum { FEMO_ELAST_THERMAL_N = 0, FEMO_ELAST_THERMAL_T_RHO = 1, FEMO_ELAST_THERMAL_T_TEMP = 2 };
int femo_elast_thermal_apply(femo_elast* e, int method, int product, int n_cols, const double* s /* [n_cols] */, double alpha,
                             const femo_vec* rho, const femo_vec* temp /* or NULL */, double t_uniform, double t_ref, double a,
                             const femo_vec* x /* or NULL (N) */, const femo_vec* base /* or NULL */, int zero_fixed,
                             femo_vec* y, int accumulate);
/* Lowest eigenfrequencies (csrc/elast_eig.hip): K(rho) phi = lambda M(rho) phi on the free dofs, with the consistent P1 mass
 *   M(rho) = density sum_e m(rho_e) M0_e,   M0_e[(a,i),(b,j)] = delta_ij |T_e| (1 + delta_ab) / ((d+1)(d+2)),
 *   m = rho (FEMO_ELAST_MASS_LINEAR) or rho for rho >= 0.1 and 6e5 rho^6 - 5e6 rho^7 below (FEMO_ELAST_MASS_DU_OLHOFF, C^1 at
 *   0.1: the usual cure for spurious localised modes in low-density regions).
 * Columns as above (column l at l * n_dof, 1 <= n_cols <= FEMO_ELAST_MAX_COLS).  No float atomics anywhere: the same bits
 * every call; a column of the mass product and an entry of a Gram matrix do not depend on how many columns go with them. */
enum { FEMO_ELAST_MASS_LINEAR = 0, FEMO_ELAST_MASS_DU_OLHOFF = 1 };
/* y_l = a M(rho) x_l, matrix free (vertex walk).  masked = 1: M_ff -- fixed entries of x read as 0, y exactly 0 on the fixed
 * dofs (needs femo_elast_set_fixed).                                                                                      */
int femo_elast_mass_apply_multi(femo_elast* e, int mass_law, double density, int masked, int n_cols, double a,
                                const femo_vec* rho, const femo_vec* x, femo_vec* y);
/* G[i * n_b + j] = a_i . b_j over n_dof entries for all n_a x n_b pairs in one pass, folded on the device in a fixed order
 * (the call waits for it).                                                                                                */
int femo_elast_block_gram(femo_elast* e, int n_a, const femo_vec* a, int n_b, const femo_vec* b, double* G /* [n_a * n_b] */);
/* y_j = sum_i x_i Q[i * n_cols + j], summed in ascending i; y may be x.                                                 */
int femo_elast_block_rotate(femo_elast* e, int n_cols, const double* Q /* [n_cols * n_cols] */, const femo_vec* x, femo_vec* y);
/* y[n_cell] (+)= sum_k c_k [ C'(rho_e) phi_k,e^T K0_e phi_k,e - lambda_k density m'(rho_e) phi_k,e^T M0_e phi_k,e ]: with
 * M-orthonormal modes the bracket is d lambda_k / d rho_e.  One launch for all n_modes columns of phi, ascending k.       */
int femo_elast_eig_drho(femo_elast* e, int method, int mass_law, double density, int n_modes, const femo_vec* rho,
                        const femo_vec* phi, const double* lambda /* [n_modes] */, const double* c /* [n_modes] */, femo_vec* y,
                        int accumulate);
typedef struct femo_eig_opts {
  double rtol;          /* every mode k < n_modes: |K phi_k - lambda_k M phi_k|_2 <= rtol lambda_k |M phi_k|_2               */
  double pcg_rtol;      /* the inner solves, relative to their first residual as in femo_elast_solve                         */
  int32_t max_outer;    /* 0 = 200                                                                                           */
  int32_t pcg_max_it;   /* 0 = the default of femo_elast_solve                                                               */
  int32_t pc;           /* FEMO_ELAST_PC_JACOBI | FEMO_ELAST_PC_MULTILEVEL                                                   */
  int32_t reserved;
} femo_eig_opts;
typedef struct femo_eig_info {
  int32_t outer_iterations;
  int32_t pcg_iterations;                  /* iterations of the batched loop, summed over the outer steps                    */
  int32_t converged;                       /* 1: every tested mode met rtol                                                  */
  int32_t reserved;
  double residual[FEMO_ELAST_MAX_COLS];    /* |K phi_k - lambda_k M phi_k| / (lambda_k |M phi_k|), guard columns included     */
  double solve_ms;                         /* device time of the inner solves                                                */
} femo_eig_info;
/* The n_modes lowest eigenpairs by block inverse iteration with Rayleigh-Ritz on the assembled K of the handle and its fixed
 * set (an error without one: K is singular on a free-free structure; a shift is out of scope).  X: block columns, the start
 * block on entry (any block of full rank; fixed entries are ignored), the modes on return -- ascending lambda, X^T M X = I,
 * exact zeros on the fixed dofs, the entry of largest magnitude of each column positive.  The block - n_modes last columns
 * are guard vectors: they speed up the others and are not tested.  An outer step is B = M_ff X, one batched PCG K Y = B
 * from the previous block, the two Gram matrices Y^T M Y and Y^T K Y, their block x block eigenproblem on the host (Cholesky
 * and cyclic Jacobi) and X = Y Q.  lambda[block].  An inner solve that does not converge is an error; an outer iteration
 * that runs out of steps returns with info->converged = 0.                                                                 */
int femo_elast_eigs(femo_elast* e, int mass_law, double density, const femo_vec* rho, int n_modes, int block, femo_vec* X,
                    const femo_eig_opts* opts, double* lambda, femo_eig_info* info);
/* Linearised buckling (csrc/elast_buckle.hip): (K(rho) + lambda K_G(u, rho)) phi = 0 on the free dofs for the state u of ONE
 * load case, with the geometric stiffness of the cell stress sigma_e = C(rho_e) sigma_0(u_e) (the stiffness law itself: no
 * separate stress interpolation; sigma_0 = lam0 tr(eps) I + 2 mu0 eps, its d x d in-plane block):
 *   K_G,e[(a,i),(b,j)] = delta_ij |T_e| g_a . sigma_e g_b,   g_a the barycentric gradients.
 * The critical load factor is the smallest positive lambda.  Columns as above; no float atomics anywhere: the same bits every
 * call, and a column of the product does not depend on how many columns go with it.
 *
 * femo_elast_geom_stress fills the cell stress buffer of the handle (d (d+1) / 2 components of n_cell entries, component-major:
 * the diagonal first, then 01[, 02, 12]; allocated on first use), so that the product touches neither u nor rho;
 * femo_elast_geom_stress_get copies it into out (tests, output).                                                           */
int femo_elast_geom_stress(femo_elast* e, int method, const femo_vec* rho, const femo_vec* u);
int femo_elast_geom_stress_get(femo_elast* e, femo_vec* out /* d (d+1) / 2 * n_cell */);
/* y_l = a K_G x_l with the stress of the last femo_elast_geom_stress, matrix free (vertex walk), one launch for all columns.
 * masked = 1: (K_G)_ff -- fixed entries of x read as 0, y exactly 0 on the fixed dofs (needs femo_elast_set_fixed).         */
int femo_elast_geom_apply_multi(femo_elast* e, int masked, int n_cols, double a, const femo_vec* x, femo_vec* y);
/* out[(v,j)] = sum_{e around v} C(rho_e) |T_e| (Sigma_H g_v)_j,  Sigma_H = lam0 tr(H) I + 2 mu0 H,
 * H = sum_k w_k (grad phi_k)^T (grad phi_k): with K-orthonormal modes and w_k = lambda_k^2 this is d lambda_k / d u, non-zero on
 * clamped dofs.  One launch for all n_modes columns of phi, ascending k.                                                   */
int femo_elast_buckle_du(femo_elast* e, int method, int n_modes, const femo_vec* rho, const femo_vec* phi,
                         const double* w /* [n_modes] */, femo_vec* out);
/* y[n_cell] (+)= C'(rho_e) |T_e| sum_k [ w1_k (lam0 (div phi_k)^2 + 2 mu0 eps(phi_k) : eps(phi_k)) + w2_k sigma_0(u_e) : H_e(phi_k) ]:
 * with K-orthonormal modes, w1_k = lambda_k and w2_k = lambda_k^2 this is d lambda_k / d rho_e at fixed u.                   */
int femo_elast_buckle_drho(femo_elast* e, int method, int n_modes, const femo_vec* rho, const femo_vec* u, const femo_vec* phi,
                           const double* w1 /* [n_modes] */, const double* w2 /* [n_modes] */, femo_vec* y, int accumulate);
/* The n_modes smallest positive load factors on the assembled K of the handle and its fixed set, solved as
 * (-K_G) phi = mu K phi, mu = 1 / lambda, for the largest positive mu: femo_elast_eigs with the roles changed.  The call fills
 * the stress buffer itself.  X: block columns, the start block on entry, the modes on return -- descending mu, X^T K X = I,
 * exact zeros on the fixed dofs, the entry of largest magnitude of each column positive.  An outer step is B = (-K_G)_ff X, one
 * batched PCG K Y = B from a zero first guess (so that its stopping level is relative to |B|), the Gram matrices Y^T K Y and
 * Y^T (-K_G) Y, their block x block eigenproblem on the host and X = Y Q.  It stops when |(-K_G) x_k - mu_k K x_k| <= rtol mu_k
 * |K x_k| (info->residual) and mu_k > 0 for every k < n_modes.  opts: max_outer 0 = 400.  lambda[block] = 1 / mu: ascending over
 * the positive ones; a guard column may carry a negative value.
 * The block converges to the modes of largest |mu| of EITHER sign; negative mu is buckling under the reversed load.  When one
 * of the n_modes largest Ritz values is still not positive at the last outer step, the block is too small for this load and
 * the call fails: raise block.  (With n_modes positive ones that merely miss rtol it returns with info->converged = 0.)  Shifted or sign-selective iterations are out of scope, as are several load cases, a stress
 * interpolation of its own against low-density pseudo-modes, and nonlinear pre-buckling.                                    */
int femo_elast_buckle(femo_elast* e, int method, const femo_vec* rho, const femo_vec* u, int n_modes, int block, femo_vec* X,
                      const femo_eig_opts* opts, double* lambda, femo_eig_info* info);
/* Harmonic response (csrc/elast_harm.hip): (K(rho) - omega_l^2 M(rho)) u_l = F_l, undamped, in real arithmetic, with the mass
 * matrix of femo_elast_mass_apply_multi.  Columns as above; column l carries its own shift sigma_l = omega_l^2 >= 0
 * (shifts[n_cols]).  No float atomics anywhere: the same bits every call, and a column does not depend on n_cols.
 *
 * femo_elast_mass_assemble stores M as a scalar matrix on the mesh's SELL pattern (one double per pattern entry in the slots
 * of K and one per row; M = that times I_d), allocated on first use and freed with the handle.  Symmetric bit for bit.      */
int femo_elast_mass_assemble(femo_elast* e, int mass_law, double density, const femo_vec* rho);
/* y_l = a (K - sigma_l M) x_l + b f_l (f may be NULL) with the assembled K and M in ONE pass over the pattern.  masked = 1:
 * identity rows / columns on the fixed dofs, exactly as the masked femo_elast_apply_multi.  sigma_l = 0 gives the bits of
 * femo_elast_apply_multi.                                                                                                 */
int femo_elast_dyn_apply_multi(femo_elast* e, int masked, int n_cols, const double* shifts /* [n_cols] */, double a,
                               const femo_vec* x, double b, const femo_vec* f /* or NULL */, femo_vec* y);
/* (K - sigma_l M) x_l = b_l with the fixed set of the handle (x = b on the fixed dofs) by ONE batched preconditioned MINRES
 * (Paige & Saunders): the matrix is indefinite above the first resonance, where the PCG of femo_elast_solve_multi breaks
 * down.  opts as for femo_elast_solve_multi; opts->pc selects block-Jacobi or the multilevel preconditioner, both of the
 * UNSHIFTED masked K (symmetric positive definite).  It stops on phibar_l <= max(rtol beta1_l, atol), beta1 = sqrt(r0 . M^-1 r0)
 * -- the norm of the PCG's test; phibar is the recurrence's estimate of sqrt(r . M^-1 r), which parts from the true residual
 * near eps cond.  info[n_cols]: converged 1 (also for a zero right-hand side, at iteration 0, and for an invariant subspace),
 * 0 (max_it reached) or -1 (a non-finite value); residual_norm = phibar, rhs_norm = beta1.  A finished column is frozen
 * while the others go on.  Damping: femo_elast_cdyn_solve_multi below.  Shifted or deflated preconditioners are out of
 * scope.                                                                                                                  */
int femo_elast_dyn_solve_multi(femo_elast* e, int n_cols, const double* shifts /* [n_cols] */, const femo_vec* b, femo_vec* x,
                               const femo_solver_opts* opts, femo_solve_info* info /* [n_cols] or NULL */);
/* The mass part of dR/drho for R_l = (K - sigma_l M) u_l - F_l, called with scales s_l = -sigma_l and accumulate = 1 on top of
 * femo_elast_drho_multi:
 *   transpose = 1:  y[c] (+)= sum_l s_l density m'(rho_c) x_{l,c}^T M0_c u_{l,c}            (x: n_cols * n_dof, y: n_cell)
 *   transpose = 0:  y_l (+)= s_l sum_{c around v} density m'(rho_c) x_c M0_c u_{l,c}        (x: n_cell, y: n_cols * n_dof)
 * exact transposes of one another; one launch for all columns either way.                                                 */
int femo_elast_mass_drho_multi(femo_elast* e, int mass_law, double density, int transpose, int n_cols,
                               const double* scales /* [n_cols] */, const femo_vec* rho, const femo_vec* u, const femo_vec* x,
                               femo_vec* y, int accumulate);
/* Damped harmonic response (csrc/elast_damp.hip): Z_l u_l = F_l in complex arithmetic with the complex SYMMETRIC
 *   Z_l = (K - sigma_l M) + i (cK_l K + cM_l M),   sigma_l = omega_l^2 >= 0, cK_l >= 0, cM_l >= 0
 * (a structural loss factor eta and Rayleigh damping alpha M + beta K give cK = eta + omega beta, cM = omega alpha), K and M
 * as for femo_elast_dyn_apply_multi.  Complex column l is the pair of real columns 2 l (Re) and 2 l + 1 (Im) of the layout
 * above: 1 <= n_cols <= FEMO_ELAST_MAX_COLS / 2, vectors of 2 n_cols n_dof entries; shifts, ck, cm: n_cols values each.
 * conj = 1 takes conj(Z_l), the transpose of the real operator on the 2 n_cols columns (adjoint solves).  No float atomics.
 *
 * y_l = a Z_l x_l + b f_l (f may be NULL) in ONE pass over the pattern: an entry of K and M is read once for both parts of
 * the complex columns of a chunk.  masked = 1: identity rows / columns on the fixed dofs of both parts.  With ck = cm = 0
 * each part has the bits of femo_elast_dyn_apply_multi on that real column.                                               */
int femo_elast_cdyn_apply_multi(femo_elast* e, int masked, int conj, int n_cols, const double* shifts /* [n_cols] */,
                                const double* ck /* [n_cols] */, const double* cm /* [n_cols] */, double a, const femo_vec* x,
                                double b, const femo_vec* f /* or NULL */, femo_vec* y);
/* Z_l x_l = b_l with the fixed set of the handle (x = b on the fixed dofs of both parts) by ONE batched preconditioned COCR
 * (Sogabe & Zhang 2007: conjugate residuals in the unconjugated form x^T y), with the real preconditioners of
 * femo_elast_dyn_solve_multi applied to both parts: one product and one preconditioner application per iteration.  With
 * damping it converges at and next to a resonance, where the undamped MINRES does not.  It stops on sqrt(Re(r^H M^-1 r)) <=
 * max(rtol beta1, atol), beta1 that of the first residual.  info[n_cols]: converged 1 (also for a zero right-hand side), 0
 * (max_it reached) or -1 (a non-finite value, or a zero denominator of alpha or beta); residual_norm and rhs_norm as for the
 * MINRES.  A finished column is frozen while the others go on, and a column has the same bits whatever n_cols is.  Out of
 * scope: frequency-band integrals, shifted preconditioners, viscous dampers at points.                                  */
int femo_elast_cdyn_solve_multi(femo_elast* e, int conj, int n_cols, const double* shifts /* [n_cols] */,
                                const double* ck /* [n_cols] */, const double* cm /* [n_cols] */, const femo_vec* b, femo_vec* x,
                                const femo_solver_opts* opts, femo_solve_info* info /* [n_cols] or NULL */);
/* Transient response (csrc/elast_transient.hip): Newmark(beta, gamma) with Rayleigh damping C = c_m M + c_k K, as its two-step
 * recurrence in the displacements, from rest (u_0 = u_-1 = 0, g_-1 = 0), for n = 0 ... N - 1:
 *   A1 u_{n+1} + A0 u_n + A- u_{n-1} = dt^2 (beta g_{n+1} + b0 g_n + b- g_{n-1}) F,    A_j = m_j M + k_j K,
 *   m1 =  1 + gamma dt c_m,          k1 = gamma dt c_k + beta dt^2,
 *   m0 = -2 + (1 - 2 gamma) dt c_m,  k0 = (1 - 2 gamma) dt c_k + b0 dt^2,    b0 = 1/2 + gamma - 2 beta,
 *   m- =  1 - (1 - gamma) dt c_m,    k- = -(1 - gamma) dt c_k + b- dt^2,     b- = 1/2 - gamma + beta,
 * with K of femo_elast_assemble and M of femo_elast_mass_assemble.  A history holds N columns of n_dof entries, column t =
 * u_{t+1} at t * n_dof (any N: no column limit).  It solves L U = B with L block lower-banded and block-Toeplitz with
 * symmetric blocks, so L^T is the same recurrence from the last column to the first.  With a fixed set (homogeneous
 * supports) A1 has identity rows / columns on the fixed dofs and A0, A- zero ones: L is the identity there.  Needs dt > 0,
 * beta > 0, gamma >= 1/2, c_m >= 0, c_k >= 0.  No float atomics: the same inputs give the same bits.                      */
typedef struct femo_newmark_params {
  double dt, beta, gamma, c_m, c_k;
} femo_newmark_params;
/* y = cr rhs - (m0 M + k0 K) u_n - (mm M + km K) u_{n-1} in ONE pass over the pattern (u: 2 n_dof entries, u_n then u_{n-1};
 * rhs may be NULL): the right-hand side of a step.  masked = 1: fixed entries of u read as 0 and a fixed row gives crf rhs.   */
int femo_elast_newmark_rhs(femo_elast* e, int masked, double cr, double crf, double m0, double k0, double mm, double km,
                           const femo_vec* rhs /* or NULL */, const femo_vec* u, femo_vec* y);
/* All n_steps steps in one call on the context's stream: L U = B (reverse = 0) or L^T U = B (reverse = 1), B either the
 * history rhs (n_steps columns) or, forward only, dt^2 (beta g_{t+1} + b0 g_t + b- g_{t-1}) F from one load pattern F and the
 * n_steps + 1 samples g of its signal (F is read as 0 on the fixed dofs).  Each step is one fused right-hand-side launch and
 * one PCG on K + (m1 / k1) M -- the loop of femo_elast_solve, opts as there, the Jacobi term from the diagonal blocks of
 * K + (m1 / k1) M -- from the first guess 2 u_prev - u_prev2 (extrapolate = 1) or zero.  The host waits only where the PCG polls
 * its flag; nothing is allocated after the first step.  info[n_steps] (or NULL): the record of every step taken, indexed by
 * column; zeroed on entry, so a step that was not taken reads as zeros.  A step that does not converge stops the march: *stopped_at = its column (-1: all steps converged), the columns of
 * the later steps are not written.                                                                                           */
int femo_elast_newmark_march(femo_elast* e, const femo_newmark_params* p, int n_steps, int reverse,
                             const femo_vec* rhs /* or NULL */, const femo_vec* F /* or NULL */, const double* g /* or NULL */,
                             femo_vec* U, const femo_solver_opts* opts, int extrapolate, femo_solve_info* info /* or NULL */,
                             int32_t* stopped_at);
/* Y = L X (transpose = 0) or L^T X for a history, FEMO_ELAST_MAX_COLS columns per launch.  masked as above.                  */
int femo_elast_newmark_apply(femo_elast* e, const femo_newmark_params* p, int n_steps, int transpose, int masked,
                             const femo_vec* X, femo_vec* Y);
/* dR/drho of R = L U - B at fixed B, for the columns first ... first + count - 1 of the history U of n_steps columns:
 * column t is C'(rho) K0 uK_t + density m'(rho) M0 uM_t with uK_t = k1 u_{t+1} + k0 u_t + k- u_{t-1}, uM_t likewise with m_j.
 *   transpose = 1:  y[n_cell] (+)= sum_t (dR_t/drho)^T x_t      (x: n_steps columns)
 *   transpose = 0:  y_t (+)= dR_t/drho x                        (x: n_cell, y: n_steps columns)
 * through femo_elast_drho_multi and femo_elast_mass_drho_multi in windows of FEMO_ELAST_MAX_COLS columns from `first`, in
 * ascending order: the whole history gives the bits of its windows accumulated one after the other.  Unmasked.            */
int femo_elast_newmark_drho(femo_elast* e, const femo_newmark_params* p, int method, int mass_law, double density, int transpose,
                            int n_steps, int first, int count, const femo_vec* rho, const femo_vec* U, const femo_vec* x,
                            femo_vec* y, int accumulate);
/* out[t] = f . U_t for every column, in windows through the Gram kernel (the call waits for them).                          */
int femo_elast_newmark_dots(femo_elast* e, int n_steps, const femo_vec* f, const femo_vec* U, double* out /* [n_steps] */);
/* Y_t = a[t] f for every column.                                                                                            */
int femo_elast_newmark_outer(femo_elast* e, int n_steps, const double* a /* [n_steps] */, const femo_vec* f, femo_vec* Y);
/* Additive multilevel preconditioner on nested auxiliary lattices over the mesh's bounding box (csrc/elast_pc.hip):
 *   M^-1 = D_blk^-1 + sum_l P_l C_l P_l^T,   C_l = blockdiag_d(P_l^T A P_l)^-1
 * A = K(rho) with identity rows / columns on the fixed dofs, P_l = multilinear interpolation from lattice l to the vertices
 * (the same weights for all d components, zero rows on fixed dofs).  The coarsest lattice has one bin along the shortest
 * axis of the box; every finer one halves the spacing; there are 1 + round(log2(shortest extent / (spacing_factor * mean
 * edge length))) of them (spacing_factor 0 = the default, 2).  The plan is built once per mesh; the d x d blocks are rebuilt
 * inside femo_elast_solve / femo_elast_pc_apply / femo_elast_pc_export_level whenever femo_elast_assemble,
 * femo_elast_set_fixed or femo_elast_set_springs ran since the last build (with springs the blocks are those of
 * K + diag(k): P_l^T diag(k) P_l is added level by level).  The rebuild reads the density vector of the last femo_elast_assemble,
 * which must still exist and be unchanged (an error otherwise: assemble again); a wrapped vector (femo_vec_wrap) cannot be
 * recognised later, so its blocks are built inside femo_elast_assemble when the plan exists.  femo_elast_pc_setup refuses a
 * mesh whose second-finest lattice exceeds 2^18 nodes: the lattices below the finest are swept by one workgroup.        */
enum { FEMO_ELAST_PC_INFO_LEVELS = 0,      /* number of lattices                                                      */
       FEMO_ELAST_PC_INFO_BYTES = 1,       /* device bytes of the lattices: blocks, their inverses, work vectors      */
       FEMO_ELAST_PC_INFO_BUILDS = 2,      /* block builds so far                                                     */
       FEMO_ELAST_PC_INFO_BUILD_US = 3,    /* device time of the last block build, microseconds                       */
       FEMO_ELAST_PC_INFO_NODES = 4,       /* [4 + l]: nodes of lattice l, coarsest first (FEMO_ELAST_PC_MAX_LEVELS)   */
       FEMO_ELAST_PC_MAX_LEVELS = 12, FEMO_ELAST_PC_INFO_COUNT = 16 };
int femo_elast_pc_setup(femo_elast* e, double spacing_factor);
int femo_elast_pc_info(const femo_elast* e, int64_t info[FEMO_ELAST_PC_INFO_COUNT]);
/* blocks[nodes(level) * d * d]: the Galerkin blocks blockdiag_d(P_l^T A P_l) BEFORE inversion, row-major per node
 * (node index: x fastest); zero where no free dof touches the node.  Rebuilds the blocks first if they are out of date. */
int femo_elast_pc_export_level(femo_elast* e, int level, double* blocks);
/* z = M^-1 r outside the solver (tests); on fixed dofs z = r, as the block-Jacobi inverse maps them.                    */
int femo_elast_pc_apply(femo_elast* e, const femo_vec* r, femo_vec* z);
/* K as block CSR on the scalar pattern of femo_mesh_pattern_csr: val[nnz * d * d], block (row comp, col comp) row-major. */
int femo_elast_export_csr(const femo_elast* e, int64_t* rowptr, int32_t* col, double* val);
/* reps block SpMV launches (unmasked) timed with device events: mean ms per launch.                                      */
int femo_elast_bench_spmv(femo_elast* e, const femo_vec* x, femo_vec* y, int reps, double* ms);
/* GeneralFilterOperation (pre_processor/general_filter_model.py): W_ij = (r - d_ij) / sum_k (r - d_ik) over the points j
 * with d_ij <= r, r = beta h_avg, from n points in dim dimensions (the DG0 dof coordinates).  Built on the device: uniform
 * hash grid of cell size >= r, count / scan / fill, rows sorted by column; W^T is kept as its own CSR.  A coordinate
 * that is NaN or +-inf is an error ("filter: coordinates must be finite"), found on the host before any device work.    */
int femo_filter_create(femo_ctx* ctx, int dim, int64_t n, const double* coords, double radius, femo_filter** out);
int femo_filter_destroy(femo_filter* f);
int femo_filter_nnz(const femo_filter* f, int64_t* nnz);
/* y = W x (transpose = 0, compute: weight_mtx.dot) or y = W^T x (transpose = 1, the rev product)                      */
int femo_filter_apply(femo_filter* f, int transpose, const femo_vec* x, femo_vec* y);
/* the rows / cols / val that declare_derivatives('density', 'density_unfiltered', ...) is given (CSR of W or W^T)     */
int femo_filter_export_csr(const femo_filter* f, int transpose, int64_t* rowptr, int32_t* col, double* val);

/* ---- Helmholtz (PDE) density filter (csrc/pde_filter.hip) ----------------------------------------------------------------
 * The filter of Lazarov & Sigmund (2011), (-rt^2 Laplace + 1) xt = x with natural boundary conditions and rt = r / (2 sqrt 3),
 * r the radius of the neighbour filter above whose length scale it matches.  For a DG0 field x on a mesh of d-simplices
 *   xt = W x,   W = V^-1 T^T A^-1 T,   A = rt^2 L + M,
 *   L_vw = sum_c |T_c| grad phi_v . grad phi_w,   T[v,c] = |T_c| / (d+1),   V = diag |T_c|,
 *   M lumped:     M_vv = sum_{c around v} |T_c| / (d+1)                       (the default)
 *   M consistent: |T_c| (1 + delta_ab) / ((d+1)(d+2)) per cell,
 * so xt_c is the mean of the nodal solution over the vertices of c.  W^T = V W V^-1: the same pipeline with 1 / |T_c| on the way
 * in and |T_c| on the way out; there is no second operator and no second solve path.  The memory is that of one scalar
 * operator on the mesh pattern, whatever r is; an application is one Jacobi-preconditioned CG solve, whose iteration count
 * grows with r / h and not with the mesh.
 * A 1 = T 1 for both mass choices, hence W 1 = 1 and v^T W x = v^T x (v = the cell volumes) up to the solve's tolerance.
 * Why lumped is the default: the consistent mass has positive off-diagonal entries, and A^-1 then undershoots -- the indicator of
 * one cell of a 24 x 12 rectangle goes to -1.2e-2 at r = h and -7.9e-4 at r = 2 h, which SIMP turns into negative stiffness.
 * With the lumped mass the off-diagonal entries of A are those of rt^2 L: non-positive on a mesh without obtuse cells, A is
 * then an M-matrix and W x >= 0 for x >= 0.  On obtuse cells positivity is not guaranteed with either mass.
 * create: d = 2, 3; refused: a partitioned mesh (one rank, as the rest of the SIMP track), a radius that is not finite or <= 0.
 * apply: y = W x (transpose = 0) or W^T x.  opts NULL: the handle's rtol (1e-13) from the zero guess, so that apply is a pure
 *   function of its input; opts->zero_guess is ignored and opts->pc must be FEMO_PC_JACOBI.  info may be NULL.  Refused (and the next call works):
 *   vectors shorter than n_cell, x overlapping y, an input with a NaN or an infinity (found as the load's non-finite norm; y may
 *   have been written).  A solve that does not converge is an error that names the iteration count.
 * set(rtol, warm_start): the tolerance of the solves that get no options of their own (finite, > 0), and, with warm_start = 1,
 *   the nodal field of the last converged forward application is the first guess of the next forward one
 *   (results then depend on the history within the tolerance).  The transpose never warm-starts.
 * export_csr: A in the layout of femo_mat_export_csr (pattern: femo_mesh_pattern_csr).  bytes: device bytes the handle holds.
 * No float atomics: A is symmetric bit for bit and has the same bits on every build; an application has the same bits every time. */
typedef struct femo_pde_filter femo_pde_filter;
int femo_pde_filter_create(femo_mesh* mesh, double radius, int lumped, femo_pde_filter** out);
int femo_pde_filter_destroy(femo_pde_filter* f);
int femo_pde_filter_apply(femo_pde_filter* f, int transpose, const femo_vec* x, femo_vec* y, const femo_solver_opts* opts,
                          femo_solve_info* info);
int femo_pde_filter_set(femo_pde_filter* f, double rtol, int warm_start);
int femo_pde_filter_export_csr(const femo_pde_filter* f, int64_t* rowptr, int32_t* col, double* val);
int femo_pde_filter_bytes(const femo_pde_filter* f, int64_t* bytes);

/* ---- Heat conduction with a penalised conductivity (csrc/conduction.hip) ------------------------------------------------
 * The second physics of the SIMP track, the heat-sink problem: on a mesh of P1 triangles or tetrahedra on one rank,
 *   K_theta(rho) = sum_c k(rho_c) |T_c| grad phi_a . grad phi_b,   k(rho) = k_min + (k_0 - k_min) C(rho),
 * C = rho^3 (FEMO_ELAST_SIMP) or rho / (1 + 8 (1 - rho)) (FEMO_ELAST_RAMP), 0 <= k_min < k_0, in femo_mat on the mesh pattern.
 * assemble: K_theta of the DG0 density rho and, with a Dirichlet set bc, the eliminated matrix beside it in the same launch
 *   (zero rows and columns and a unit diagonal on the set; it keeps its identity rows, which femo_solve_cg solves up front).
 *   No float atomics: both are symmetric bit for bit and have the same bits on every build.
 * apply: y = K_theta x, or with eliminated = 1 the eliminated matrix.
 * lift: the right-hand side for Dirichlet values g (NULL: zero): b = g on the set, b = q - K_theta g elsewhere; g holds the
 *   values on the set and zeros elsewhere; work: n_rows scratch entries (needed with g).
 * solve: femo_solve_cg with the eliminated matrix (the plain one without a set); opts NULL: Jacobi, rtol 1e-13 from the zero
 *   guess.  opts->pc selects the preconditioner and with it the stopping rule, as femo_solver_opts defines them:
 *     FEMO_PC_JACOBI (default)  sqrt(r^T D^-1 r) <= max(rtol sqrt(b^T D^-1 b), atol)
 *     FEMO_PC_BPX               sqrt(r^T M^-1 r) <= max(rtol sqrt(b^T M^-1 b), atol_pc)   or   sqrt(r^T D^-1 r) <= atol (if > 0)
 *   FEMO_PC_BPX is the auxiliary-lattice preconditioner of csrc/bpx.hip with level weights taken from this operator,
 *     M^-1 = D^-1 + sum_l P_l C_l P_l^T,   C_l[I] = keep_l[I] 0.6 / G_l[I],   G_l[I] = (Pt_l^T A Pt_l)_II
 *   (Pt_l: multilinear interpolation from lattice l to the free vertices, A the matrix that is solved; tests/cond_pc_ref.py).
 *   G is formed on the device by the first such solve after an assembly and shared by the later ones; it reads the density
 *   handed to femo_cond_assemble again, which must still be alive and unchanged then.  The sums of G are fp64 atomics: a BPX
 *   solve repeats to rounding, not bit for bit; the Jacobi path is untouched by all of this.  A non-finite density or
 *   right-hand side is found as the non-finite Jacobi norm of the right-hand side, or as the breakdown of the first iteration,
 *   and refused with either preconditioner (x may have been written; the next call works).  Whether the solve converged is
 *   in info.
 * pc_apply: z = M^-1 r with the FEMO_PC_BPX operator above in unscaled variables, as femo_mat_pc_apply (tests).
 * pc_info: out[0] lattice levels, out[1] builds of G so far, out[2 + l] nodes of level l (coarsest first), count entries at most.
 * pc_export_level: the count of pc_info's out[2 + level] weights C_level of the current assembly, to host memory.
 * drho: the density products of R = K_theta(rho) T - Q at the temperature T, k' = (k_0 - k_min) C',
 *   transpose = 0:  y[v] = (accumulate ? y[v] : 0) + a sum_{c around v} k'(rho_c) x_c |T_c| grad phi_v . grad T_c   (x: n_cell)
 *   transpose = 1:  y[c] = (accumulate ? y[c] : 0) + a k'(rho_c) |T_c| grad x_c . grad T_c                         (x: n_vert)
 *   exact transposes in exact arithmetic; one writer per entry, the cells around a vertex in ascending order.
 * export_csr: either matrix in the layout of femo_mat_export_csr.                                                        */
typedef struct femo_cond femo_cond;
int femo_cond_create(femo_mesh* mesh, femo_cond** out);
int femo_cond_destroy(femo_cond* c);
int femo_cond_assemble(femo_cond* c, int method, double k0, double k_min, const femo_vec* rho, const femo_bc* bc /* or NULL */);
int femo_cond_apply(femo_cond* c, int eliminated, const femo_vec* x, femo_vec* y);
int femo_cond_lift(femo_cond* c, const femo_vec* q, const femo_vec* g /* or NULL */, femo_vec* work /* or NULL */, femo_vec* b);
int femo_cond_solve(femo_cond* c, const femo_vec* b, femo_vec* x, const femo_solver_opts* opts, femo_solve_info* info);
int femo_cond_pc_apply(femo_cond* c, const femo_vec* r, femo_vec* z);
int femo_cond_pc_info(femo_cond* c, int64_t* out, int count);
int femo_cond_pc_export_level(femo_cond* c, int level, double* coef);
int femo_cond_drho(femo_cond* c, int method, double k0, double k_min, int transpose, double a, const femo_vec* rho,
                   const femo_vec* T, const femo_vec* x, femo_vec* y, int accumulate);
int femo_cond_export_csr(const femo_cond* c, int eliminated, int64_t* rowptr, int32_t* col, double* val);

/* ---- Method of Moving Asymptotes (csrc/mma.hip) -------------------------------------------------------------------------
 * What the reference's drivers hand to modopt (run_topo_opt_cantilever_beam.py: modopt.CSDLProblem + SLSQP / SNOPT), as a
 * device-resident update: minimise f_0(x) subject to f_i(x) <= 0, i = 1..m, xmin <= x <= xmax (Svanberg 1987; Svanberg 2007,
 * "MMA and GCMMA -- two methods for nonlinear optimization", his defaults).  n variables, 0 <= m <= FEMO_MMA_MAX_M general
 * constraints, finite bounds with xmax > xmin everywhere, fp64.  Per design step k = 1, 2, ...
 *   asymptotes   k <= 2: L = x - 0.5 range, U = x + 0.5 range, range = xmax - xmin;  k >= 3: z = (x - x1)(x1 - x2) with the two
 *                previous iterates, gamma = 1.2 / 0.7 / 1 for z > 0 / < 0 / = 0, L = x - gamma (x1 - L_old),
 *                U = x + gamma (U_old - x1), then L into [x - 10 range, x - 0.01 range], U into [x + 0.01 range, x + 10 range];
 *   move limits  alpha = max(xmin, L + 0.1 (x - L), x - move range), beta = min(xmax, U - 0.1 (U - x), x + move range);
 *   p_ij = (U - x)^2 (1.001 g+ + 0.001 g- + rho), q_ij = (x - L)^2 (0.001 g+ + 1.001 g- + rho), g+- = max(+-df_i/dx_j, 0),
 *                rho = 1e-5 / range;  b_i = sum_j (p_ij / (U - x) + q_ij / (x - L)) - f_i;
 *   subproblem   min sum_j p_0j / (U_j - x_j) + q_0j / (x_j - L_j) + sum_i (c_i y_i + d_i y_i^2 / 2)
 *                s.t. sum_j p_ij / (U_j - x_j) + q_ij / (x_j - L_j) - y_i <= b_i, alpha <= x <= beta, y >= 0
 *                (Svanberg's z and a_i are dropped: a_i = 0 makes z = 0 at the optimum);
 *   solver       his primal-dual interior-point Newton iteration on (x, y, lambda, xi, eta, mu, s): barrier 10^0 ... 10^-K,
 *                K = ceil(-log10(sub_tol)) counted by an integer; per barrier Newton steps until the max-norm of the residual
 *                is <= 0.9 barrier (at most 200); step 1 / max(1, 1.01 max(-delta / variable)) over the positive unknowns and
 *                both bound distances of x, halved until the residual's 2-norm does not exceed the previous one (at most 50
 *                times).  m = 0: x_j = clamp((sqrt(p_0) L + sqrt(q_0) U) / (sqrt(p_0) + sqrt(q_0)), alpha, beta), no iteration.
 * Per variable the handle keeps x1, x2, L, U, alpha, beta, xi, eta and p, q for i = 0..m; the Newton direction of x, xi, eta is
 * recomputed in registers from the m values of delta lambda.  The m x m Newton system is folded from per-block partial sums
 * in a fixed order and solved on the host inside the call (small_solve.h); three blocking copies of at most 64 doubles per
 * Newton step.  No float atomics: the same inputs give the same bits.  One rank.  Out of scope: GCMMA's inner conservative
 * loop, equality constraints, m > FEMO_MMA_MAX_M.  xmax = xmin is refused: passive cells enter through the projection
 * below, which fixes their density and zeroes their Jacobian rows.                                                        */
#define FEMO_MMA_MAX_M 8
typedef struct femo_mma femo_mma;
typedef struct femo_mma_params {
  double move;                   /* move limit as a fraction of the range, > 0 (Svanberg: 0.5)                 */
  double sub_tol;                /* the last barrier value is the first 10^-K <= sub_tol; in (0, 1] (1e-7)      */
  double c[FEMO_MMA_MAX_M];      /* c_i >= 0 (1000: presumes an objective of order one)                        */
  double d[FEMO_MMA_MAX_M];      /* d_i > 0 (1)                                                                */
} femo_mma_params;
typedef struct femo_mma_info {
  int32_t converged;             /* 1; 0 when a cap was hit (200 Newton steps in a stage, 50 halvings) or the iteration
                                    left the finite numbers -- x then holds the last iterate                    */
  int32_t step;                  /* k of this update, from 1                                                    */
  int32_t stages;                /* barrier values gone through (0 for m = 0)                                   */
  int32_t newton_steps;          /* in all stages                                                               */
  int32_t halvings;              /* step halvings in all                                                        */
  int32_t blocking_copies;       /* times the host waited for folded sums                                       */
  double residual_max;           /* max-norm of the perturbed KKT rows at the last barrier value                */
  double max_dx;                 /* max_j |x^{k+1} - x^k|                                                        */
  double max_dx_rel;             /* max_j |x^{k+1} - x^k| / range_j                                              */
  double update_ms;              /* host time of the call                                                       */
  double lam[FEMO_MMA_MAX_M];    /* multipliers of the general constraints                                      */
  double y[FEMO_MMA_MAX_M];
} femo_mma_info;
/* xmin, xmax: n entries each, copied.  params NULL: the defaults above.  Refused: a bound that is not finite, xmax <= xmin
 * anywhere, m outside 0..FEMO_MMA_MAX_M, move <= 0, sub_tol outside (0, 1], c_i < 0, d_i <= 0.                             */
int femo_mma_create(femo_ctx* ctx, int64_t n, int m, const femo_vec* xmin, const femo_vec* xmax, const femo_mma_params* params,
                    femo_mma** out);
/* One design step: x <- x^{k+1} in place.  df0: n entries; f: m values on the host; df: m stacked columns of n entries
 * (NULL for m = 0).  Refused before anything changes: a value or gradient entry that is not finite, x outside its bounds.  */
int femo_mma_update(femo_mma* h, femo_vec* x, double f0, const femo_vec* df0, const double* f, const femo_vec* df,
                    femo_mma_info* info);
/* Forget the history: the next update is step 1 again.                                                                   */
int femo_mma_reset(femo_mma* h);
int femo_mma_destroy(femo_mma* h);

/* ---- Heaviside projection of the filtered density (csrc/project.hip) ------------------------------------------------------
 * The third field of the three-field formulation (Wang, Lazarov, Sigmund 2011): xt = W x (the filter above), and on the
 * active cells
 *   rho_i = H(xt_i) = (tanh(beta eta) + tanh(beta (xt_i - eta))) / D,   D = tanh(beta eta) + tanh(beta (1 - eta)),
 *   H_x   = beta (1 - tanh^2(beta (xt - eta))) / D,
 *   H_eta = (N_eta D - N D_eta) / D^2,  N = tanh(beta eta) + tanh(beta (xt - eta)),
 *           N_eta = beta (tanh^2(beta (xt - eta)) - tanh^2(beta eta)),  D_eta = beta (tanh^2(beta (1 - eta)) - tanh^2(beta eta)).
 * beta = 0 is the identity (rho = xt, a copy; H_x = 1, H_eta = 0).  Passive cells: rho_i = 1 on `solid`, rho_i = void_value on
 * `void`; their Jacobian rows are zero in both products and they take no part in any sum below.
 * FEMO_PROJECT_FIXED: eta as set.  FEMO_PROJECT_VOLUME (Xu, Cai, Cheng 2010): eta is the root of
 *   g(eta) = sum_active v_i H(xt_i; beta, eta) - sum_active v_i xt_i,
 * found by 53 bisection steps on [0, 1] (mid = (lo + hi) / 2; g(mid) > 0: lo = mid, else hi = mid; eta = (lo + hi) / 2), all on
 * the device: per step one reduction launch (wave shuffle -> LDS -> one partial per block into the handle's own buffer) and one
 * fold in the order of femo_fold_partials that also moves lo / hi in the handle's device record {lo, hi, eta, target, S_a, S_v,
 * vol_out}; one blocking copy of that record at the end.  The Jacobian then has a rank-one term,
 *   (J^T a)_j = a_j H_x,j + (S_a / S_v) v_j (1 - H_x,j),   (J d)_i = H_x,i d_i + H_eta,i sum_j v_j (1 - H_x,j) d_j / S_v,
 *   S_a = sum_active a_i H_eta,i,  S_v = sum_active v_i H_eta,i,
 * dropped when S_v == 0 exactly (every active cell saturated, or beta = 0; info->flat = 1).  No float atomics: the same inputs
 * give the same bits.  fp64, one rank, the context's stream.                                                              */
#define FEMO_PROJECT_FIXED 0
#define FEMO_PROJECT_VOLUME 1
typedef struct femo_project femo_project;
typedef struct femo_project_info {
  double eta;                    /* the threshold used (volume mode: the root)                                   */
  double vol_in;                 /* sum_active v_i xt_i                                                          */
  double vol_out;                /* sum_active v_i rho_i                                                         */
  double s_v;                    /* S_v at eta (volume mode; 0 in fixed mode)                                    */
  double ms;                     /* host time of the call, its one blocking copy included                        */
  int32_t flat;                  /* volume mode: S_v == 0, the rank-one term is dropped                          */
  int32_t mode;
  int32_t launches;              /* kernels of the call                                                          */
  int32_t reserved;
} femo_project_info;
/* v: n cell volumes on the host, copied (NULL: ones).  solid / void_: n_solid / n_void cell indices on the host.  Refused
 * before any launch: beta < 0 or not finite, eta outside [0, 1], an unknown mode, an index outside 0..n-1, a cell in both
 * sets, void_value outside (0, 1], an entry of v that is not positive and finite, volume mode without an active cell.      */
int femo_project_create(femo_ctx* ctx, int64_t n, const double* v, int64_t n_solid, const int64_t* solid, int64_t n_void,
                        const int64_t* void_, double void_value, double beta, double eta, int mode, femo_project** out);
int femo_project_destroy(femo_project* p);
int femo_project_set(femo_project* p, double beta, double eta, int mode);
/* rho = P(xt).  info may be NULL in fixed mode (then nothing is copied back).  Refused: vectors shorter than n, xt
 * overlapping rho.                                                                                                      */
int femo_project_forward(femo_project* p, const femo_vec* xt, femo_vec* rho, femo_project_info* info);
/* xt = W x and rho = P(xt).  Fixed mode: one gather launch (the row loop of femo_filter_apply, then H in registers).  Volume
 * mode: the gather also leaves the partials of sum v xt; the bisection; one element-wise launch for rho.  Refused as above,
 * and x overlapping xt or rho.                                                                                           */
int femo_filter_project(femo_filter* f, femo_project* p, const femo_vec* x, femo_vec* xt, femo_vec* rho, femo_project_info* info);
/* The same with the Helmholtz filter: load, solve (the handle's defaults), then ONE launch that forms the cell means and, in
 * fixed mode, applies H in registers, so that xt and rho leave one launch; volume mode: the mean launch also leaves the partials
 * of sum v xt, then the bisection and the element-wise launch as above.  Refusals of both entry points apply.              */
int femo_pde_filter_project(femo_pde_filter* f, femo_project* p, const femo_vec* x, femo_vec* xt, femo_vec* rho,
                            femo_project_info* info);
/* out = J^T a and out = J d at xt, with the threshold of the last forward call (volume mode).  out may be a / d itself.    */
int femo_project_reverse(femo_project* p, const femo_vec* xt, const femo_vec* a, femo_vec* out);
int femo_project_tangent(femo_project* p, const femo_vec* xt, const femo_vec* d, femo_vec* out);
/* M_nd = 4 sum v rho (1 - rho) / sum v over all cells                                                                    */
int femo_project_grayness(femo_project* p, const femo_vec* rho, double* mnd);

#ifdef __cplusplus
}
#endif
#endif /* FEMO_HIP_H */
