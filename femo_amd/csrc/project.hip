// Heaviside projection of the filtered density, passive cells and the volume-preserving threshold: the third field of the
// SIMP track's design chain (include/femo_hip.h, "Heaviside projection", states the formulation; tests/projection_ref.py
// restates it in NumPy).
//
// Layout.  Everything per cell runs in element-wise kernels with grid-stride loops, 256 threads (4 wave64); every sum goes
// wave shuffle -> LDS -> one partial per block into the handle's own buffer (three slots) and is folded by k_p_fold in the
// fixed order of femo_fold_partials into the handle's device record.  The grid depends on n alone, so a call gives the same
// bits from run to run; no float atomics.  The record is written by thread 0 of the fold's one block with ordinary stores.
//
// Fixed threshold: tanh(beta eta) and D are formed once on the host and travel as kernel arguments, so a cell costs one tanh.
// femo_filter_project is then one launch: the row loop of k_f_apply (elasticity.hip), then p_cell on the sum in registers.
// femo_pde_filter_project: load and solve of the Helmholtz filter (pde_filter.hip), then k_p_mean in the gather's place: the
// cell means of the nodal field, and p_cell on each in registers.
// Volume-preserving threshold: k_p_gsum / k_p_fold<STEP> 53 times -- no host round trip -- then k_p_forward, which reads the
// root from the record, and one blocking copy of the record.  Bytes per launch: DESIGN.md section 10, "Projection".
//
// Reverse and tangent products in volume mode: k_p_jsum (S_a or the tangent's sum, and S_v), a fold, k_p_jac.  W^T is applied
// by femo_filter_apply afterwards: fusing tanh into that gather would evaluate it once per non-zero.
#include <chrono>
#include <cmath>

#include "elast_internal.h"

struct femo_project {
  femo_ctx* ctx = nullptr;
  int64_t n = 0, n_active = 0;
  double beta = 0.0, eta = 0.5, void_value = 1e-4;
  int mode = FEMO_PROJECT_FIXED;
  bool have_eta = false;        // volume mode: the record's eta is that of a forward call since the last set
  int nb = 1;
  double* d_v = nullptr;        // n cell volumes
  int8_t* d_flag = nullptr;     // 0 active, 1 solid, -1 void
  double* d_part = nullptr;     // P_SLOTS slots of nb partials
  double* d_rec = nullptr;      // P_REC doubles, see below
  double* h_rec = nullptr;      // pinned mirror
};

namespace {

constexpr int P_BLOCK = 256;
constexpr int P_WAVES = P_BLOCK / FEMO_WAVE;
constexpr int P_SLOTS = 3;
constexpr int P_BISECT = 53;
// the device record
enum { R_LO = 0, R_HI = 1, R_ETA = 2, R_TARGET = 3, R_SA = 4, R_SV = 5, R_VOUT = 6, R_G0 = 7, R_G1 = 8, P_REC = 16 };
enum { FOLD_PLAIN = 0, FOLD_INIT = 1, FOLD_STEP = 2 };

struct PCoef {
  double beta, eta, tbe, t1e, D;     // tbe = tanh(beta eta), t1e = tanh(beta (1 - eta)), D = tbe + t1e
};

__host__ __device__ __forceinline__ PCoef p_coef(double beta, double eta) {
  PCoef c;
  c.beta = beta; c.eta = eta;
  c.tbe = tanh(beta * eta);
  c.t1e = tanh(beta * (1.0 - eta));
  c.D = c.tbe + c.t1e;
  return c;
}

// H, H_x and H_eta of one active cell, operation by operation as the restatement has them: without contraction, so that
// H_eta is exactly zero on a saturated cell (xt = 0: N = N_eta = 0; xt = 1: N = D and N_eta = D_eta bit for bit).
__device__ __forceinline__ void p_cell(const PCoef& c, double x, double& H, double& Hx, double& Heta) {
#pragma clang fp contract(off)
  if (c.beta == 0.0) { H = x; Hx = 1.0; Heta = 0.0; return; }
  const double t = tanh(c.beta * (x - c.eta));
  const double N = c.tbe + t;
  H = N / c.D;
  Hx = c.beta * (1.0 - t * t) / c.D;
  const double tb2 = c.tbe * c.tbe;
  const double Ne = c.beta * (t * t - tb2), De = c.beta * (c.t1e * c.t1e - tb2);
  Heta = (Ne * c.D - N * De) / (c.D * c.D);
}

// NS sums of the block into part[j * nb + blockIdx.x]: one barrier, fixed order
template <int NS>
__device__ __forceinline__ void p_block_reduce(const double* s, double* lds /* P_WAVES * NS */, double* __restrict__ part, int nb) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const double t = femo_wave_sum(s[j]);
    if (lane == 0) lds[w * NS + j] = t;
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < NS) {
    double t = lds[j];
    for (int k = 1; k < P_WAVES; ++k) t += lds[k * NS + j];
    part[(int64_t)j * nb + blockIdx.x] = t;
  }
}

// One block: slot j of the partials into rec[dst[j]], j < nslot.  FOLD_INIT: slot 0 is the target, the bracket is [0, 1].
// FOLD_STEP: slot 0 is sum v H at mid = rec[R_ETA]; the bracket moves and rec[R_ETA] becomes the next midpoint.
struct PFoldDst { int dst[P_SLOTS]; };
__global__ __launch_bounds__(P_BLOCK) void k_p_fold(int nb, int nslot, PFoldDst D, int op, const double* __restrict__ part,
                                                    double* __restrict__ rec) {
  __shared__ double lds[P_WAVES];
  for (int j = 0; j < nslot; ++j) {
    const double t = femo_fold_partials<P_BLOCK>(part + (int64_t)j * nb, nb, lds);
    if (threadIdx.x != 0) continue;
    if (op == FOLD_INIT && j == 0) {
      rec[R_TARGET] = t; rec[R_LO] = 0.0; rec[R_HI] = 1.0; rec[R_ETA] = 0.5;
    } else if (op == FOLD_STEP && j == 0) {
      double lo = rec[R_LO], hi = rec[R_HI];
      const double mid = rec[R_ETA];
      if (t - rec[R_TARGET] > 0.0) lo = mid; else hi = mid;
      rec[R_LO] = lo; rec[R_HI] = hi; rec[R_ETA] = 0.5 * (lo + hi);
    } else {
      rec[D.dst[j]] = t;
    }
  }
}

// sums: [0] sum_active v xt
__global__ __launch_bounds__(P_BLOCK) void k_p_volin(int64_t n, const double* __restrict__ xt, const double* __restrict__ v,
                                                     const int8_t* __restrict__ fl, double* __restrict__ part, int nb) {
  __shared__ double lds[P_WAVES];
  double s[1] = {0.0};
  for (int64_t j = (int64_t)blockIdx.x * P_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * P_BLOCK)
    if (fl[j] == 0) s[0] += v[j] * xt[j];
  p_block_reduce<1>(s, lds, part, nb);
}

// one bisection step's sum: [0] sum_active v H(xt; beta, mid), mid from the record
__global__ __launch_bounds__(P_BLOCK) void k_p_gsum(int64_t n, double beta, const double* __restrict__ xt, const double* __restrict__ v,
                                                    const int8_t* __restrict__ fl, const double* __restrict__ rec,
                                                    double* __restrict__ part, int nb) {
  __shared__ double lds[P_WAVES];
  const PCoef c = p_coef(beta, rec[R_ETA]);
  double s[1] = {0.0};
  for (int64_t j = (int64_t)blockIdx.x * P_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * P_BLOCK) {
    if (fl[j] != 0) continue;
    double H, Hx, He;
    p_cell(c, xt[j], H, Hx, He);
    s[0] += v[j] * H;
  }
  p_block_reduce<1>(s, lds, part, nb);
}

// rho of one cell and its contributions to the sums [0] v xt, [1] v rho, [2] v H_eta (active cells)
__device__ __forceinline__ double p_rho(const PCoef& c, int8_t flag, double x, double vj, double void_value, double* s) {
  if (flag > 0) return 1.0;
  if (flag < 0) return void_value;
  double H, Hx, He;
  p_cell(c, x, H, Hx, He);
  s[0] += vj * x; s[1] += vj * H; s[2] += vj * He;
  return H;
}

// rho = P(xt).  VOLUME: the threshold is the record's.
template <bool VOLUME>
__global__ __launch_bounds__(P_BLOCK) void k_p_forward(int64_t n, PCoef c, double void_value, const double* __restrict__ xt,
                                                       const double* __restrict__ v, const int8_t* __restrict__ fl,
                                                       const double* __restrict__ rec, double* __restrict__ rho,
                                                       double* __restrict__ part, int nb) {
  __shared__ double lds[P_WAVES * 3];
  if (VOLUME) c = p_coef(c.beta, rec[R_ETA]);
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t j = (int64_t)blockIdx.x * P_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * P_BLOCK)
    rho[j] = p_rho(c, fl[j], xt[j], v[j], void_value, s);
  p_block_reduce<3>(s, lds, part, nb);
}

// xt = W x by the row loop of k_f_apply (same order, same contraction), then -- PROJECT -- rho = P(xt) from the register
template <bool PROJECT>
__global__ __launch_bounds__(P_BLOCK) void k_p_gather(int64_t n, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      const double* __restrict__ val, const double* __restrict__ x, PCoef c,
                                                      double void_value, const double* __restrict__ v, const int8_t* __restrict__ fl,
                                                      double* __restrict__ xt, double* __restrict__ rho, double* __restrict__ part, int nb) {
  __shared__ double lds[P_WAVES * 3];
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * P_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * P_BLOCK) {
    double a = 0.0;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) a += val[e] * x[col[e]];
    xt[i] = a;
    if (PROJECT) rho[i] = p_rho(c, fl[i], a, v[i], void_value, s);
    else if (fl[i] == 0) s[0] += v[i] * a;
  }
  p_block_reduce<3>(s, lds, part, nb);
}

// xt = the mean of the nodal field p over the vertices of the cell, scaled by cv (the last step of femo_pde_filter_apply: the sum
// in `conn` order, then one product, as k_dRdf_cell_apply_T has it), then -- PROJECT -- rho = P(xt) from the register
template <int D, bool PROJECT>
__global__ __launch_bounds__(P_BLOCK) void k_p_mean(int64_t n, const int32_t* __restrict__ conn, const double* __restrict__ cv,
                                                    const double* __restrict__ p, PCoef c, double void_value,
                                                    const double* __restrict__ v, const int8_t* __restrict__ fl,
                                                    double* __restrict__ xt, double* __restrict__ rho, double* __restrict__ part, int nb) {
  __shared__ double lds[P_WAVES * 3];
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * P_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * P_BLOCK) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k <= D; ++k) a += p[conn[i * (D + 1) + k]];
    a *= cv[i];
    xt[i] = a;
    if (PROJECT) rho[i] = p_rho(c, fl[i], a, v[i], void_value, s);
    else if (fl[i] == 0) s[0] += v[i] * a;
  }
  p_block_reduce<3>(s, lds, part, nb);
}

// sums of the rank-one term: [0] S_a = sum_active a H_eta (TANGENT: sum_active v (1 - H_x) a), [1] S_v = sum_active v H_eta
template <bool TANGENT>
__global__ __launch_bounds__(P_BLOCK) void k_p_jsum(int64_t n, double beta, const double* __restrict__ xt, const double* __restrict__ v,
                                                    const int8_t* __restrict__ fl, const double* __restrict__ a,
                                                    const double* __restrict__ rec, double* __restrict__ part, int nb) {
  __shared__ double lds[P_WAVES * 2];
  const PCoef c = p_coef(beta, rec[R_ETA]);
  double s[2] = {0.0, 0.0};
  for (int64_t j = (int64_t)blockIdx.x * P_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * P_BLOCK) {
    if (fl[j] != 0) continue;
    double H, Hx, He;
    p_cell(c, xt[j], H, Hx, He);
    const double vj = v[j];
    s[0] += TANGENT ? vj * (1.0 - Hx) * a[j] : a[j] * He;
    s[1] += vj * He;
  }
  p_block_reduce<2>(s, lds, part, nb);
}

// out = J^T a (or J a, TANGENT); VOLUME: with the rank-one term from the record unless S_v == 0.  out may be a.
template <bool VOLUME, bool TANGENT>
__global__ __launch_bounds__(P_BLOCK) void k_p_jac(int64_t n, PCoef c, const double* __restrict__ xt, const double* __restrict__ v,
                                                   const int8_t* __restrict__ fl, const double* a, const double* __restrict__ rec,
                                                   double* out) {
  double ratio = 0.0;
  bool rank_one = false;
  if (VOLUME) {
    c = p_coef(c.beta, rec[R_ETA]);
    const double sv = rec[R_SV];
    rank_one = sv != 0.0;
    if (rank_one) ratio = rec[R_SA] / sv;
  }
  for (int64_t j = (int64_t)blockIdx.x * P_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * P_BLOCK) {
    double r = 0.0;
    if (fl[j] == 0) {
      double H, Hx, He;
      p_cell(c, xt[j], H, Hx, He);
      r = a[j] * Hx;
      if (VOLUME && rank_one) r += TANGENT ? He * ratio : ratio * v[j] * (1.0 - Hx);
    }
    out[j] = r;
  }
}

// sums over all cells: [0] v rho (1 - rho), [1] v
__global__ __launch_bounds__(P_BLOCK) void k_p_gray(int64_t n, const double* __restrict__ rho, const double* __restrict__ v,
                                                    double* __restrict__ part, int nb) {
  __shared__ double lds[P_WAVES * 2];
  double s[2] = {0.0, 0.0};
  for (int64_t j = (int64_t)blockIdx.x * P_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * P_BLOCK) {
    const double r = rho[j], vj = v[j];
    s[0] += vj * r * (1.0 - r);
    s[1] += vj;
  }
  p_block_reduce<2>(s, lds, part, nb);
}

int p_grid(const femo_ctx* ctx, int64_t n) {
  int64_t g = (n + P_BLOCK - 1) / P_BLOCK;
  const int64_t cap = (int64_t)ctx->n_cu * 4;
  if (g > cap) g = cap;
  if (g > FEMO_MAX_PARTIALS) g = FEMO_MAX_PARTIALS;
  return (int)(g < 1 ? 1 : g);
}

int p_check_params(double beta, double eta, int mode) {
  FEMO_REQUIRE(std::isfinite(beta) && beta >= 0.0, "project: beta = %g, must be finite and >= 0", beta);
  FEMO_REQUIRE(eta >= 0.0 && eta <= 1.0, "project: eta = %g, must lie in [0, 1]", eta);
  FEMO_REQUIRE(mode == FEMO_PROJECT_FIXED || mode == FEMO_PROJECT_VOLUME, "project: unknown mode %d", mode);
  return 0;
}

bool p_overlap(const femo_vec* a, const femo_vec* b, int64_t n) {
  return a == b || (a->d < b->d + n && b->d < a->d + n);
}

int p_fold(femo_project* p, int nslot, int d0, int d1, int d2, int op) {
  PFoldDst D{{d0, d1, d2}};
  hipLaunchKernelGGL(k_p_fold, dim3(1), dim3(P_BLOCK), 0, p->ctx->stream, p->nb, nslot, D, op, p->d_part, p->d_rec);
  return 0;
}

// the record to the host: the call's one blocking copy
int p_fetch(femo_project* p) {
  hipStream_t st = p->ctx->stream;
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_HIP_CHECK(hipMemcpyAsync(p->h_rec, p->d_rec, P_REC * sizeof(double), hipMemcpyDeviceToHost, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

// The 53 steps on xt, the target's partials being in slot 0; leaves the root in rec[R_ETA].  Returns the launches.
int p_bisect(femo_project* p, const double* xt) {
  hipStream_t st = p->ctx->stream;
  p_fold(p, 1, R_TARGET, 0, 0, FOLD_INIT);
  for (int k = 0; k < P_BISECT; ++k) {
    hipLaunchKernelGGL(k_p_gsum, dim3(p->nb), dim3(P_BLOCK), 0, st, p->n, p->beta, xt, p->d_v, p->d_flag, p->d_rec, p->d_part, p->nb);
    p_fold(p, 1, 0, 0, 0, FOLD_STEP);
  }
  return 1 + 2 * P_BISECT;
}

// what follows xt (and, in fixed mode with rho_done, rho) being in place; vol_in's partials are in slot 0
int p_finish(femo_project* p, const double* xt, double* rho, bool rho_done, int launches, femo_project_info* info,
             std::chrono::steady_clock::time_point t0) {
  hipStream_t st = p->ctx->stream;
  const bool volume = p->mode == FEMO_PROJECT_VOLUME;
  if (volume) {
    launches += p_bisect(p, xt);
    hipLaunchKernelGGL(k_p_forward<true>, dim3(p->nb), dim3(P_BLOCK), 0, st, p->n, p_coef(p->beta, 0.5), p->void_value, xt, p->d_v,
                       p->d_flag, p->d_rec, rho, p->d_part, p->nb);
    ++launches;
    p->have_eta = true;
  } else if (!rho_done) {
    hipLaunchKernelGGL(k_p_forward<false>, dim3(p->nb), dim3(P_BLOCK), 0, st, p->n, p_coef(p->beta, p->eta), p->void_value, xt, p->d_v,
                       p->d_flag, p->d_rec, rho, p->d_part, p->nb);
    ++launches;
  }
  FEMO_HIP_CHECK(hipGetLastError());
  if (!info) return 0;
  // volume mode: slot 0 of the last launch repeats the target
  p_fold(p, 3, R_TARGET, R_VOUT, R_SV, FOLD_PLAIN);
  ++launches;
  FEMO_TRY(p_fetch(p));
  *info = femo_project_info{};
  info->mode = p->mode;
  info->eta = volume ? p->h_rec[R_ETA] : p->eta;
  info->vol_in = p->h_rec[R_TARGET];
  info->vol_out = p->h_rec[R_VOUT];
  info->s_v = volume ? p->h_rec[R_SV] : 0.0;
  info->flat = volume && p->h_rec[R_SV] == 0.0;
  info->launches = launches;
  info->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

int p_jac(femo_project* p, const femo_vec* xt, const femo_vec* a, femo_vec* out, bool tangent) {
  FEMO_REQUIRE(p && xt && a && out, "null argument");
  const int64_t n = p->n;
  FEMO_REQUIRE(xt->n >= n && a->n >= n && out->n >= n, "project: a vector is shorter than n = %lld", (long long)n);
  FEMO_REQUIRE(!p_overlap(xt, out, n), "project: the output overlaps xt");
  FEMO_REQUIRE(a == out || !p_overlap(a, out, n), "project: the output overlaps its input without being it");
  const bool volume = p->mode == FEMO_PROJECT_VOLUME;
  FEMO_REQUIRE(!volume || p->have_eta, "project: volume mode needs a forward call before a Jacobian product");
  FEMO_TRY(femo_vec_await(xt));
  FEMO_TRY(femo_vec_await(a));
  femo_vec_touch(out);
  hipStream_t st = p->ctx->stream;
  const dim3 g(p->nb), b(P_BLOCK);
  if (volume) {
    const PCoef c = p_coef(p->beta, 0.5);
    if (tangent) hipLaunchKernelGGL(k_p_jsum<true>, g, b, 0, st, n, p->beta, xt->d, p->d_v, p->d_flag, a->d, p->d_rec, p->d_part, p->nb);
    else hipLaunchKernelGGL(k_p_jsum<false>, g, b, 0, st, n, p->beta, xt->d, p->d_v, p->d_flag, a->d, p->d_rec, p->d_part, p->nb);
    p_fold(p, 2, R_SA, R_SV, 0, FOLD_PLAIN);
    if (tangent) hipLaunchKernelGGL((k_p_jac<true, true>), g, b, 0, st, n, c, xt->d, p->d_v, p->d_flag, a->d, p->d_rec, out->d);
    else hipLaunchKernelGGL((k_p_jac<true, false>), g, b, 0, st, n, c, xt->d, p->d_v, p->d_flag, a->d, p->d_rec, out->d);
  } else {
    // without the rank-one term J is diagonal: the two products are one kernel
    hipLaunchKernelGGL((k_p_jac<false, false>), g, b, 0, st, n, p_coef(p->beta, p->eta), xt->d, p->d_v, p->d_flag, a->d, p->d_rec, out->d);
  }
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int femo_project_destroy(femo_project* p) {
  if (!p) return 0;
  hipFree(p->d_v); hipFree(p->d_flag); hipFree(p->d_part); hipFree(p->d_rec);
  if (p->h_rec) hipHostFree(p->h_rec);
  delete p;
  return 0;
}

extern "C" int femo_project_create(femo_ctx* ctx, int64_t n, const double* v, int64_t n_solid, const int64_t* solid, int64_t n_void,
                                   const int64_t* void_, double void_value, double beta, double eta, int mode, femo_project** out) {
  FEMO_REQUIRE(ctx && out, "null argument");
  *out = nullptr;
  FEMO_REQUIRE(ctx->nranks == 1, "project: one rank only (partitioned meshes are out of scope)");
  FEMO_REQUIRE(n >= 1, "project: n = %lld, need at least one cell", (long long)n);
  FEMO_REQUIRE(n_solid >= 0 && n_void >= 0 && (n_solid == 0 || solid) && (n_void == 0 || void_), "project: bad passive sets");
  FEMO_REQUIRE(void_value > 0.0 && void_value <= 1.0, "project: void_value = %g, must lie in (0, 1]", void_value);
  FEMO_TRY(p_check_params(beta, eta, mode));
  std::vector<int8_t> flag((size_t)n, 0);
  for (int64_t k = 0; k < n_solid; ++k) {
    FEMO_REQUIRE(solid[k] >= 0 && solid[k] < n, "project: solid cell %lld outside 0..%lld", (long long)solid[k], (long long)n - 1);
    flag[(size_t)solid[k]] = 1;
  }
  for (int64_t k = 0; k < n_void; ++k) {
    FEMO_REQUIRE(void_[k] >= 0 && void_[k] < n, "project: void cell %lld outside 0..%lld", (long long)void_[k], (long long)n - 1);
    FEMO_REQUIRE(flag[(size_t)void_[k]] != 1, "project: cell %lld is both solid and void", (long long)void_[k]);
    flag[(size_t)void_[k]] = -1;
  }
  int64_t n_active = 0;
  for (int64_t j = 0; j < n; ++j) n_active += flag[(size_t)j] == 0;
  FEMO_REQUIRE(mode != FEMO_PROJECT_VOLUME || n_active > 0, "project: the volume-preserving threshold needs an active cell");
  std::vector<double> ones;
  if (v) {
    for (int64_t j = 0; j < n; ++j)
      FEMO_REQUIRE(std::isfinite(v[j]) && v[j] > 0.0, "project: volume %g of cell %lld, must be positive and finite", v[j], (long long)j);
  } else {
    ones.assign((size_t)n, 1.0);
    v = ones.data();
  }
  femo_project* p = new femo_project;
  p->ctx = ctx; p->n = n; p->n_active = n_active; p->beta = beta; p->eta = eta; p->mode = mode; p->void_value = void_value;
  p->nb = p_grid(ctx, n);
  auto fail = [&](int rc) { femo_project_destroy(p); return rc; };
  if (hipMalloc(&p->d_v, (size_t)n * sizeof(double)) != hipSuccess || hipMalloc(&p->d_flag, (size_t)n) != hipSuccess ||
      hipMalloc(&p->d_part, (size_t)P_SLOTS * p->nb * sizeof(double)) != hipSuccess ||
      hipMalloc(&p->d_rec, P_REC * sizeof(double)) != hipSuccess ||
      hipHostMalloc(&p->h_rec, P_REC * sizeof(double), hipHostMallocDefault) != hipSuccess) {
    femo_set_error("project: out of memory for %lld cells", (long long)n);
    return fail(1);
  }
  hipStream_t st = ctx->stream;
  if (hipMemcpyAsync(p->d_v, v, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(p->d_flag, flag.data(), (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(p->d_rec, 0, P_REC * sizeof(double), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    femo_set_error("project: copying the volumes and flags failed");
    return fail(1);
  }
  *out = p;
  return 0;
}

extern "C" int femo_project_set(femo_project* p, double beta, double eta, int mode) {
  FEMO_REQUIRE(p, "null argument");
  FEMO_TRY(p_check_params(beta, eta, mode));
  FEMO_REQUIRE(mode != FEMO_PROJECT_VOLUME || p->n_active > 0, "project: the volume-preserving threshold needs an active cell");
  p->beta = beta; p->eta = eta; p->mode = mode;
  p->have_eta = false;
  return 0;
}

extern "C" int femo_project_forward(femo_project* p, const femo_vec* xt, femo_vec* rho, femo_project_info* info) {
  FEMO_REQUIRE(p && xt && rho, "null argument");
  const int64_t n = p->n;
  FEMO_REQUIRE(xt->n >= n && rho->n >= n, "project: a vector is shorter than n = %lld", (long long)n);
  FEMO_REQUIRE(!p_overlap(xt, rho, n), "project: xt overlaps rho");
  FEMO_REQUIRE(info || p->mode == FEMO_PROJECT_FIXED, "project: volume mode needs an info record");
  const auto t0 = std::chrono::steady_clock::now();
  FEMO_TRY(femo_vec_await(xt));
  femo_vec_touch(rho);
  int launches = 0;
  if (p->mode == FEMO_PROJECT_VOLUME) {
    hipLaunchKernelGGL(k_p_volin, dim3(p->nb), dim3(P_BLOCK), 0, p->ctx->stream, n, xt->d, p->d_v, p->d_flag, p->d_part, p->nb);
    ++launches;
  }
  return p_finish(p, xt->d, rho->d, false, launches, info, t0);
}

extern "C" int femo_filter_project(femo_filter* f, femo_project* p, const femo_vec* x, femo_vec* xt, femo_vec* rho, femo_project_info* info) {
  FEMO_REQUIRE(f && p && x && xt && rho, "null argument");
  const int64_t n = p->n;
  FEMO_REQUIRE(f->n == n && f->ctx == p->ctx, "project: the filter has %lld points, the projection %lld cells", (long long)f->n, (long long)n);
  FEMO_REQUIRE(x->n >= n && xt->n >= n && rho->n >= n, "project: a vector is shorter than n = %lld", (long long)n);
  FEMO_REQUIRE(!p_overlap(xt, rho, n) && !p_overlap(x, xt, n) && !p_overlap(x, rho, n), "project: x, xt and rho must not overlap");
  FEMO_REQUIRE(info || p->mode == FEMO_PROJECT_FIXED, "project: volume mode needs an info record");
  const auto t0 = std::chrono::steady_clock::now();
  FEMO_TRY(femo_vec_await(x));
  femo_vec_touch(xt);
  femo_vec_touch(rho);
  hipStream_t st = p->ctx->stream;
  const bool fixed = p->mode == FEMO_PROJECT_FIXED;
  if (fixed)
    hipLaunchKernelGGL(k_p_gather<true>, dim3(p->nb), dim3(P_BLOCK), 0, st, n, f->d_rowptr, f->d_col, f->d_val, x->d, p_coef(p->beta, p->eta),
                       p->void_value, p->d_v, p->d_flag, xt->d, rho->d, p->d_part, p->nb);
  else
    hipLaunchKernelGGL(k_p_gather<false>, dim3(p->nb), dim3(P_BLOCK), 0, st, n, f->d_rowptr, f->d_col, f->d_val, x->d, p_coef(p->beta, 0.5),
                       p->void_value, p->d_v, p->d_flag, xt->d, rho->d, p->d_part, p->nb);
  return p_finish(p, xt->d, rho->d, fixed, 1, info, t0);
}

extern "C" int femo_pde_filter_project(femo_pde_filter* f, femo_project* p, const femo_vec* x, femo_vec* xt, femo_vec* rho,
                                       femo_project_info* info) {
  FEMO_REQUIRE(f && p && x && xt && rho, "null argument");
  const int64_t n = p->n;
  FEMO_REQUIRE(f->n == n && f->ctx == p->ctx, "project: the filter has %lld cells, the projection %lld", (long long)f->n, (long long)n);
  FEMO_REQUIRE(x->n >= n && xt->n >= n && rho->n >= n, "project: a vector is shorter than n = %lld", (long long)n);
  FEMO_REQUIRE(!p_overlap(xt, rho, n) && !p_overlap(x, xt, n) && !p_overlap(x, rho, n), "project: x, xt and rho must not overlap");
  FEMO_REQUIRE(info || p->mode == FEMO_PROJECT_FIXED, "project: volume mode needs an info record");
  const auto t0 = std::chrono::steady_clock::now();
  const femo_vec* nodal = nullptr;
  FEMO_TRY(femo_pde_filter_nodal(f, 0, x, nullptr, nullptr, &nodal));
  femo_vec_touch(xt);
  femo_vec_touch(rho);
  const femo_mesh* m = f->mesh;
  hipStream_t st = p->ctx->stream;
  const bool fixed = p->mode == FEMO_PROJECT_FIXED;
  const PCoef c = p_coef(p->beta, fixed ? p->eta : 0.5);
  const dim3 g(p->nb), b(P_BLOCK);
#define P_MEAN(DIM, PROJECT)                                                                                                     \
  hipLaunchKernelGGL((k_p_mean<DIM, PROJECT>), g, b, 0, st, n, m->d_conn, f->cv_one->d, nodal->d, c, p->void_value, p->d_v, p->d_flag, \
                     xt->d, rho->d, p->d_part, p->nb)
  if (m->tdim == 2) { if (fixed) P_MEAN(2, true); else P_MEAN(2, false); }
  else { if (fixed) P_MEAN(3, true); else P_MEAN(3, false); }
#undef P_MEAN
  return p_finish(p, xt->d, rho->d, fixed, 1, info, t0);
}

extern "C" int femo_project_reverse(femo_project* p, const femo_vec* xt, const femo_vec* a, femo_vec* out) {
  return p_jac(p, xt, a, out, false);
}

extern "C" int femo_project_tangent(femo_project* p, const femo_vec* xt, const femo_vec* d, femo_vec* out) {
  return p_jac(p, xt, d, out, true);
}

extern "C" int femo_project_grayness(femo_project* p, const femo_vec* rho, double* mnd) {
  FEMO_REQUIRE(p && rho && mnd, "null argument");
  FEMO_REQUIRE(rho->n >= p->n, "project: rho is shorter than n = %lld", (long long)p->n);
  FEMO_TRY(femo_vec_await(rho));
  hipLaunchKernelGGL(k_p_gray, dim3(p->nb), dim3(P_BLOCK), 0, p->ctx->stream, p->n, rho->d, p->d_v, p->d_part, p->nb);
  p_fold(p, 2, R_G0, R_G1, 0, FOLD_PLAIN);
  FEMO_TRY(p_fetch(p));
  *mnd = 4.0 * p->h_rec[R_G0] / p->h_rec[R_G1];
  return 0;
}
