/* femo_hip_test.h -- entry points of libfemo_hip.so that exist for the test suite and the scaling model only.
 * They are exported by the same library but are NOT part of the product ABI (include/femo_hip.h): no
 * production caller needs them, and a reference-side binding never touches them.          */
#ifndef FEMO_HIP_TEST_H
#define FEMO_HIP_TEST_H

#include "femo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct femo_emu_group femo_emu_group;  /* in-process rank emulation */

/* ---- rank emulation on ONE GPU (tests) -----------------------------------------------------------
 * RCCL cannot place two ranks on one device.  With a femo_emu_group, `nranks` contexts on the same GPU,
 * each driven by its own host thread, behave as the ranks of a job: every collective of the library
 * (halo exchange, all-reduced scalars, all-reduced lattice accumulators) is staged through host memory
 * and a barrier instead of RCCL, so the multi-rank code paths run for real on a one-GPU box.  A rank
 * that never reaches a collective makes the others fail after 60 s instead of hanging.             */
int femo_emu_group_create(int nranks, femo_emu_group** out);
int femo_emu_group_destroy(femo_emu_group* group);
int femo_comm_emulate(femo_ctx* ctx, femo_emu_group* group, int rank);

/* ---- "model" communicator (bench.py's scaling_model) ------------------------------------------------
 * Makes ONE context run the N-rank code paths of the library alone on its GPU: ctx behaves as rank `rank` of
 * `nranks` (partitioned-mesh branches of the solvers, the pack kernel of the merged BPX-PCG loop, the split
 * interior / boundary SpMV with its halo pack), while every collective completes at once without moving a byte
 * -- an all-reduce leaves the rank's own contribution in place, a neighbour exchange fills the ghost entries with
 * zeros (one memset on the stream).  The collectives are still counted (femo_comm_stats).  What this measures:
 * everything a rank of an N-GPU job does per iteration except the time on the wire.  The numbers it computes
 * are those of the rank's block solved on its own (zero ghost values), not of the global problem.           */
int femo_comm_model(femo_ctx* ctx, int rank, int nranks);

/* ---- merged BPX-PCG: which loop ran, and on how many kept directions (tests) -----------------------------
 * out[0] = 1 if BPX-PCG solves on this mesh take the merged loop (builds the lattice hierarchy if need be; honours
 *          the environment switches that select the classic loop), else 0;
 * out[1] = ring slots the last merged solve on this mesh's context used (0: x += alpha p every iteration);
 * out[2] = flush launches that solve enqueued (ring full, batch polls, max_it);
 * out[3] = merged solves on this context that asked for a ring and got fewer slots than asked for, or none.
 * Entries beyond `count` are not written.                                                                   */
int femo_mesh_pcg_info(femo_mesh* mesh, int64_t* out, int count);

/* ---- streamed head: what the load vector of the Poisson forms did on this mesh (tests) --------------------
 * Under a deferred upload of f that travels in chunks (FEMO_H2D_CHUNK_MB) the first Newton right-hand side of a cycle
 * forms the load vector and K u' - L range by range, on the row blocks (256 rows) whose cells have landed.
 * out[0] = row blocks of the mesh;
 * out[1] = row blocks the last streamed head walked BEFORE the range of its last chunk;
 * out[2] = streamed heads on this mesh so far;
 * out[3] = load vectors formed on this mesh so far, streamed or in one launch (a cached one is not formed again).
 * Entries beyond `count` are not written.  A library that exports this entry point also fills the h2d_chunks
 * field at the end of femo_host_stats.                                                                      */
int femo_mesh_head_info(femo_mesh* mesh, int64_t* out, int count);

/* ---- streamed tail: what femo_dRdf_cell_apply_T_add_to_host did on this mesh (tests) ----------------------------
 * out[0] = calls that streamed product, sum and copy-out range by range;
 * out[1] = ranges of those calls in all;
 * out[2] = calls that took the product followed by femo_vec_add_to_host.
 * Entries beyond `count` are not written.                                                                   */
int femo_mesh_tail_info(femo_mesh* mesh, int64_t* out, int count);

/* ---- the ranges of the streamed head and tail (host only, no GPU touched; csrc/range_plan.h) -------------------------------
 * The plan both streamed transfers cut their n entries by: bounds[2 k], bounds[2 k + 1] = begin and end of range k, written
 * while 2 k + 1 < room; returns the number of ranges.  taper 0: pieces of `chunk` entries; 1: the chunked upload's plan (pieces
 * shrink by `factor` down to `floor` at the end); 2: the streamed tail's (they grow by `factor` from `floor`, on to `cap`).
 * The library calls it with FEMO_H2D_CHUNK_MB / FEMO_D2H_CHUNK_MB, FEMO_RANGE_FLOOR_MB, FEMO_RANGE_FACTOR and
 * FEMO_D2H_MAX_CHUNK_MB in entries.                                                                            */
int femo_range_plan_host(int64_t n, int64_t chunk, int taper, int64_t floor, int64_t factor, int64_t cap, int64_t* bounds,
                         int64_t room);

/* ---- Newton's flagged passes: what the launches that were handed the flag did (tests) -----------------------
 * Synchronises the context's stream, then
 * out[0] / out[1] = flagged launches of the axpy that left early / that ran (a device counter, bumped by workgroup 0);
 * out[2] / out[3] = the same for the product of femo_newton_rhs_linear_if;
 * out[4] = launches that were handed the flag at all (host side; the rest ran as the plain entry points);
 * out[5] = the flag as the last identity solve left it;
 * out[6] = BPX solves on this context that found the preconditioner's weights in place (femo_mat_prescale).
 * Counters run from the creation of the context.  Entries beyond `count` are not written.                    */
int femo_ctx_newton_flag_info(femo_ctx* ctx, int64_t* out, int count);

/* ---- compacted copy of S A S: what the scaling built and which copy the products read (tests) ------------------
 * The scaling S A S of a matrix also writes a copy in which every regular slice keeps only the slots that are not zero
 * in all 64 rows (one rank, FEMO_SPMV_COMPACT not 0, at least half of the slices regular); the products of the Krylov
 * loops read it while it is valid.  Synchronises the context's stream, then
 * out[0] = 1 if the copy describes the scaled values as they stand, else 0;
 * out[1] = regular slices the last build packed;
 * out[2] / out[3] = pairs the product walks in the copy / in the full array, over all slices, of the last build;
 * out[4] / out[5] = products on S A S launched on the copy / on the full array, from the creation of the matrix.
 * A handle whose build finds fewer than one pair in eight dead stops building the copy at the end of the first solve
 * that follows (out[0] = 0 from then on; out[1..3] keep the figures of that build).  Entries beyond `count` are not
 * written.                                                                                                   */
int femo_mat_compact_info(femo_mat* A, int64_t* out, int count);

/* y = (S A S) x: the launch the Krylov loops issue (scaling the matrix first if need be), with the fused partial sums
 * of variant `dots` (0 none, 1 x.Ax, 2 x.Ax | x.x, 3 x.Ax | Ax.Ax) copied to `partials` (host; *nblocks per sum, one
 * sum after the other; room for 2 x 2048).  One rank.                                                        */
int femo_mat_spmv_scaled(femo_mat* A, int dots, const femo_vec* x, femo_vec* y, double* partials, int* nblocks);

/* Chosen values in a matrix: `val` in the order of femo_mat_export_csr (nnz entries, the diagonal among them).
 * Counts as an assembly into A: everything derived from the old values is invalid.                           */
int femo_mat_import_csr(femo_mat* A, const double* val);

/* ---- MMA: what the last update built, and one subproblem from given arrays (tests) ------------------------------------------
 * femo_mma_get copies to the host what the last femo_mma_update (or femo_mma_solve_subproblem) left in the handle:
 * what = 0 L, 1 U, 2 alpha, 3 beta (n doubles each), 4 p_i, 5 q_i (n doubles, i = 0..m), 6 b (m doubles), 7 the sums
 * b_i + f_i (m doubles), 8 xi, 9 eta (n doubles each).                                                                    */
int femo_mma_get(femo_mma* h, int what, int i, double* out);
/* Solves the subproblem given by host arrays (p, q: m + 1 rows of n; b: m values) with the handle's c, d and sub_tol.  x, xi,
 * eta: n doubles each; small: 4 m doubles, y | lambda | mu | s.  The handle's history is left alone, its L ... q are
 * overwritten.                                                                                                           */
int femo_mma_solve_subproblem(femo_mma* h, const double* L, const double* U, const double* alpha, const double* beta,
                              const double* p, const double* q, const double* b, double* x, double* xi, double* eta,
                              double* small, femo_mma_info* info);

#ifdef __cplusplus
}
#endif
#endif
