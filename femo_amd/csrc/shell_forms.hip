// Reissner-Mindlin shell: the element kernels of the forms and outputs -- assembly, thickness partials of the bilinear
// form, load and its transpose, compliance, aggregated von Mises stress and its projection, mass, penalty boundary
// terms, inertia, regularisation -- and the entry points that launch them (shell_internal.h has the overview).
#include "shell_internal.h"

namespace {

// quadrature rules of oracle/shell_oracle.py: Dunavant degree 4 (in-plane terms), degree 2 (shear)
__constant__ double c_lam6[6][3] = {
    {0.108103018168070, 0.445948490915965, 0.445948490915965}, {0.445948490915965, 0.108103018168070, 0.445948490915965},
    {0.445948490915965, 0.445948490915965, 0.108103018168070}, {0.816847572980459, 0.091576213509771, 0.091576213509771},
    {0.091576213509771, 0.816847572980459, 0.091576213509771}, {0.091576213509771, 0.091576213509771, 0.816847572980459}};
__constant__ double c_w6[6] = {0.223381589678011, 0.223381589678011, 0.223381589678011,
                               0.109951743655322, 0.109951743655322, 0.109951743655322};
__constant__ double c_lam3[3][3] = {{2.0 / 3, 1.0 / 6, 1.0 / 6}, {1.0 / 6, 2.0 / 3, 1.0 / 6}, {1.0 / 6, 1.0 / 6, 2.0 / 3}};

struct Facet {
  double e1[3], e2[3], e3[3], area;
  double gl[3][2];            // tangent gradients of the barycentric coordinates
};

__device__ __forceinline__ void facet_frame(const double* __restrict__ x, const int32_t* __restrict__ conn, int64_t c, Facet& F) {
  double p[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k) p[a][k] = x[(int64_t)conn[c * 3 + a] * 3 + k];
  double t1[3], t2[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { t1[k] = p[1][k] - p[0][k]; t2[k] = p[2][k] - p[0][k]; }
  n[0] = t1[1] * t2[2] - t1[2] * t2[1]; n[1] = t1[2] * t2[0] - t1[0] * t2[2]; n[2] = t1[0] * t2[1] - t1[1] * t2[0];
  const double dbl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  const double l1 = sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) { F.e3[k] = n[k] / dbl; F.e1[k] = t1[k] / l1; }
  F.e2[0] = F.e3[1] * F.e1[2] - F.e3[2] * F.e1[1];
  F.e2[1] = F.e3[2] * F.e1[0] - F.e3[0] * F.e1[2];
  F.e2[2] = F.e3[0] * F.e1[1] - F.e3[1] * F.e1[0];
  F.area = 0.5 * dbl;
  // tangent coordinates of the vertices: (0,0), (a,0), (b,c)
  const double a = t1[0] * F.e1[0] + t1[1] * F.e1[1] + t1[2] * F.e1[2];
  const double b = t2[0] * F.e1[0] + t2[1] * F.e1[1] + t2[2] * F.e1[2];
  const double cc = t2[0] * F.e2[0] + t2[1] * F.e2[1] + t2[2] * F.e2[2];
  const double X[3] = {0.0, a, b}, Y[3] = {0.0, 0.0, cc};
  const double det = 2.0 * F.area;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    F.gl[i][0] = (Y[j] - Y[k]) / det;
    F.gl[i][1] = (X[k] - X[j]) / det;
  }
}

// tangent gradient of P2 shape function a at barycentric point lam (vertices 0..2, then edges (0,1), (1,2), (2,0))
__device__ __forceinline__ void p2_grad(const Facet& F, const double* lam, int a, double& g1, double& g2) {
  if (a < 3) {
    const double d = 4.0 * lam[a] - 1.0;
    g1 = d * F.gl[a][0]; g2 = d * F.gl[a][1];
  } else {
    const int i = a - 3, j = (a - 2) % 3;
    g1 = 4.0 * (lam[j] * F.gl[i][0] + lam[i] * F.gl[j][0]);
    g2 = 4.0 * (lam[j] * F.gl[i][1] + lam[i] * F.gl[j][1]);
  }
}

__device__ __forceinline__ double p2_value(const double* lam, int a) {
  if (a < 3) return lam[a] * (2.0 * lam[a] - 1.0);
  const int i = a - 3, j = (a - 2) % 3;
  return 4.0 * lam[i] * lam[j];
}

// Column `col` (0..26) of the strain operator at one point: rows 0-2 membrane (Voigt, engineering shear), 3-5 bending,
// 6-7 transverse shear, 8 drilling (oracle/shell_oracle.py::_strain_operators)
__device__ __forceinline__ void strain_column(const Facet& F, const double* lam, int col, double (&b)[9]) {
#pragma unroll
  for (int r = 0; r < 9; ++r) b[r] = 0.0;
  if (col < 18) {
    const int a = col / 3, k = col % 3;
    double g1, g2;
    p2_grad(F, lam, a, g1, g2);
    b[0] = F.e1[k] * g1;
    b[1] = F.e2[k] * g2;
    b[2] = F.e1[k] * g2 + F.e2[k] * g1;
    b[6] = F.e3[k] * g1;
    b[7] = F.e3[k] * g2;
    b[8] = 0.5 * (F.e1[k] * g2 - F.e2[k] * g1);
  } else {
    const int v = (col - 18) / 3, k = (col - 18) % 3;
    const double g1 = F.gl[v][0], g2 = F.gl[v][1], M = lam[v];
    b[3] = -F.e2[k] * g1;
    b[4] = F.e1[k] * g2;
    b[5] = -F.e2[k] * g2 + F.e1[k] * g1;
    b[6] = F.e2[k] * M;
    b[7] = -F.e1[k] * M;
    b[8] = F.e3[k] * M;
  }
}

__device__ __forceinline__ int64_t shell_gdof(const femo_shell_view& S, int64_t c, int i) {
  if (i < 18) {
    const int a = i / 3, k = i % 3;
    const int64_t node = a < 3 ? (int64_t)S.conn[c * 3 + a] : S.n_vert + S.cedge[c * 3 + a - 3];
    return 3 * node + k;
  }
  const int v = (i - 18) / 3, k = (i - 18) % 3;
  return 3 * S.n_unode + 3 * (int64_t)S.conn[c * 3 + v] + k;
}

struct Material { double c11, c12, c33, mu_s, E; };     // plane stress, shear modulus x 5/6, Young's modulus

__device__ __forceinline__ Material material(double E, double nu) {
  Material m;
  const double f = E / (1.0 - nu * nu);
  m.c11 = f; m.c12 = f * nu; m.c33 = f * 0.5 * (1.0 - nu);
  m.mu_s = (5.0 / 6.0) * E / (2.0 * (1.0 + nu));
  m.E = E;
  return m;
}

// K_e[:, col] for every (cell, col): B^T D B over the two rules, added to the CSR values with atomics
__global__ __launch_bounds__(SH_BLOCK) void k_shell_assemble(femo_shell_view S, double E, double nu, const double* __restrict__ h,
                                                             const int32_t* __restrict__ epos, double* __restrict__ vals) {
  const int64_t t = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  const int64_t c = t / 27;
  const int col = (int)(t % 27);
  if (c >= S.n_cell) return;
  Facet F;
  facet_frame(S.x, S.conn, c, F);
  const Material m = material(E, nu);
  const double hv[3] = {h[S.conn[c * 3]], h[S.conn[c * 3 + 1]], h[S.conn[c * 3 + 2]]};
  double acc[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) acc[i] = 0.0;
  for (int q = 0; q < 6; ++q) {
    const double* lam = c_lam6[q];
    const double hq = hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2];
    const double w = c_w6[q] * F.area;
    const double dm = w * hq, db = w * hq * hq * hq * (1.0 / 12.0), dd = w * m.E * hq * hq * hq;
    double bj[9];
    strain_column(F, lam, col, bj);
    // D B[:, col]: membrane, bending, drilling
    const double s0 = dm * (m.c11 * bj[0] + m.c12 * bj[1]), s1 = dm * (m.c12 * bj[0] + m.c11 * bj[1]), s2 = dm * m.c33 * bj[2];
    const double s3 = db * (m.c11 * bj[3] + m.c12 * bj[4]), s4 = db * (m.c12 * bj[3] + m.c11 * bj[4]), s5 = db * m.c33 * bj[5];
    const double s8 = dd * bj[8];
    for (int i = 0; i < 27; ++i) {
      double bi[9];
      strain_column(F, lam, i, bi);
      acc[i] += bi[0] * s0 + bi[1] * s1 + bi[2] * s2 + bi[3] * s3 + bi[4] * s4 + bi[5] * s5 + bi[8] * s8;
    }
  }
  for (int q = 0; q < 3; ++q) {
    const double* lam = c_lam3[q];
    const double hq = hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2];
    const double ds = (1.0 / 3.0) * F.area * m.mu_s * hq;
    double bj[9];
    strain_column(F, lam, col, bj);
    const double s6 = ds * bj[6], s7 = ds * bj[7];
    for (int i = 0; i < 27; ++i) {
      double bi[9];
      strain_column(F, lam, i, bi);
      acc[i] += bi[6] * s6 + bi[7] * s7;
    }
  }
  const int32_t* ep = epos + c * 729;
  for (int i = 0; i < 27; ++i) atomicAdd(&vals[ep[i * 27 + col]], acc[i]);
}

// strains B w_e (9 rows) of an element vector at one point
__device__ __forceinline__ void element_strain(const Facet& F, const double* lam, const double (&we)[27], double (&s)[9]) {
#pragma unroll
  for (int r = 0; r < 9; ++r) s[r] = 0.0;
  for (int i = 0; i < 27; ++i) {
    double bi[9];
    strain_column(F, lam, i, bi);
#pragma unroll
    for (int r = 0; r < 9; ++r) s[r] += bi[r] * we[i];
  }
}

// out[b] += sum_e v_e^T (dK_e/dh_b) w_e  (one thread per cell): the thickness derivative of the bilinear form.
// v == w gives 2 dEnergy/dh.  energy != nullptr: per-block partials of 1/2 v^T K w as well.
__global__ __launch_bounds__(SH_BLOCK) void k_shell_dform_dh(femo_shell_view S, double E, double nu, const double* __restrict__ h,
                                                             const double* __restrict__ v, const double* __restrict__ w,
                                                             double* __restrict__ out, double* __restrict__ energy) {
  __shared__ double lds[SH_BLOCK / 64];
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  double en = 0.0;
  if (c < S.n_cell) {
    Facet F;
    facet_frame(S.x, S.conn, c, F);
    const Material m = material(E, nu);
    const double hv[3] = {h[S.conn[c * 3]], h[S.conn[c * 3 + 1]], h[S.conn[c * 3 + 2]]};
    double ve[27], we[27];
    for (int i = 0; i < 27; ++i) {
      const int64_t g = shell_gdof(S, c, i);
      ve[i] = v[g]; we[i] = w[g];
    }
    double g[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < 6; ++q) {
      const double* lam = c_lam6[q];
      const double hq = hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2];
      const double wq = c_w6[q] * F.area;
      double sv[9], sw[9];
      element_strain(F, lam, ve, sv);
      element_strain(F, lam, we, sw);
      const double mem = sv[0] * (m.c11 * sw[0] + m.c12 * sw[1]) + sv[1] * (m.c12 * sw[0] + m.c11 * sw[1]) + sv[2] * m.c33 * sw[2];
      const double ben = sv[3] * (m.c11 * sw[3] + m.c12 * sw[4]) + sv[4] * (m.c12 * sw[3] + m.c11 * sw[4]) + sv[5] * m.c33 * sw[5];
      const double dri = m.E * sv[8] * sw[8];
      en += wq * (hq * mem + hq * hq * hq * (ben * (1.0 / 12.0) + dri));
      const double d = wq * (mem + hq * hq * (0.25 * ben + 3.0 * dri));        // d/dh of h, h^3/12, h^3
#pragma unroll
      for (int b = 0; b < 3; ++b) g[b] += d * lam[b];
    }
    for (int q = 0; q < 3; ++q) {
      const double* lam = c_lam3[q];
      const double hq = hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2];
      const double wq = (1.0 / 3.0) * F.area;
      double sv[9], sw[9];
      element_strain(F, lam, ve, sv);
      element_strain(F, lam, we, sw);
      const double sh = m.mu_s * (sv[6] * sw[6] + sv[7] * sw[7]);
      en += wq * hq * sh;
#pragma unroll
      for (int b = 0; b < 3; ++b) g[b] += wq * sh * lam[b];
    }
    if (out != nullptr) {
#pragma unroll
      for (int b = 0; b < 3; ++b) atomicAdd(&out[S.conn[c * 3 + b]], g[b]);
    }
  }
  if (energy != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(0.5 * en * shell_value_weight(S, c), lds);
    if (threadIdx.x == 0) energy[blockIdx.x] = t;
  }
}

// y += (dK/dh [dh]) w: the FORWARD product with the thickness partial of the elastic residual (state_model.py:176-188, fwd
// mode: d_residuals += dR/dh . d_h).  Element by element from the strains of w: sigma' = (d/dh of the section weights in the
// direction dh) D B w_e at every quadrature point, y_e = sum_q B^T sigma'.  One thread per cell, 27 atomics (the reverse
// product k_shell_dform_dh is its exact transpose: <v, y> = <dh, out> -- tests/test_gpu_shell_round3.py).
__global__ __launch_bounds__(SH_BLOCK) void k_shell_dform_dh_fwd(femo_shell_view S, double E, double nu, const double* __restrict__ h,
                                                                 const double* __restrict__ dh, const double* __restrict__ w,
                                                                 double* __restrict__ y) {
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  if (c >= S.n_cell) return;
  Facet F;
  facet_frame(S.x, S.conn, c, F);
  const Material m = material(E, nu);
  const double hv[3] = {h[S.conn[c * 3]], h[S.conn[c * 3 + 1]], h[S.conn[c * 3 + 2]]};
  const double dv[3] = {dh[S.conn[c * 3]], dh[S.conn[c * 3 + 1]], dh[S.conn[c * 3 + 2]]};
  double we[27], acc[27];
  for (int i = 0; i < 27; ++i) { we[i] = w[shell_gdof(S, c, i)]; acc[i] = 0.0; }
  for (int q = 0; q < 6; ++q) {
    const double* lam = c_lam6[q];
    const double hq = hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2];
    const double dq = dv[0] * lam[0] + dv[1] * lam[1] + dv[2] * lam[2];
    const double wq = c_w6[q] * F.area;
    const double dm = wq * dq, db = wq * 0.25 * hq * hq * dq, dd = wq * 3.0 * m.E * hq * hq * dq;   // d/dh of h, h^3/12, E h^3
    double sw[9];
    element_strain(F, lam, we, sw);
    const double s0 = dm * (m.c11 * sw[0] + m.c12 * sw[1]), s1 = dm * (m.c12 * sw[0] + m.c11 * sw[1]), s2 = dm * m.c33 * sw[2];
    const double s3 = db * (m.c11 * sw[3] + m.c12 * sw[4]), s4 = db * (m.c12 * sw[3] + m.c11 * sw[4]), s5 = db * m.c33 * sw[5];
    const double s8 = dd * sw[8];
    for (int i = 0; i < 27; ++i) {
      double bi[9];
      strain_column(F, lam, i, bi);
      acc[i] += bi[0] * s0 + bi[1] * s1 + bi[2] * s2 + bi[3] * s3 + bi[4] * s4 + bi[5] * s5 + bi[8] * s8;
    }
  }
  for (int q = 0; q < 3; ++q) {
    const double* lam = c_lam3[q];
    const double dq = dv[0] * lam[0] + dv[1] * lam[1] + dv[2] * lam[2];
    const double ds = (1.0 / 3.0) * F.area * m.mu_s * dq;
    double sw[9];
    element_strain(F, lam, we, sw);
    const double s6 = ds * sw[6], s7 = ds * sw[7];
    for (int i = 0; i < 27; ++i) {
      double bi[9];
      strain_column(F, lam, i, bi);
      acc[i] += bi[6] * s6 + bi[7] * s7;
    }
  }
  for (int i = 0; i < 27; ++i) atomicAdd(&y[shell_gdof(S, c, i)], acc[i]);
}

// F += int f . v  (f: CG1 vector field at the vertices, force per unit area), sign * that
__global__ __launch_bounds__(SH_BLOCK) void k_shell_load(femo_shell_view S, const double* __restrict__ f, double sign, double* __restrict__ Fv) {
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  if (c >= S.n_cell) return;
  Facet F;
  facet_frame(S.x, S.conn, c, F);
  double fv[3][3];
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int k = 0; k < 3; ++k) fv[b][k] = f[(int64_t)S.conn[c * 3 + b] * 3 + k];
  double acc[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) acc[i] = 0.0;
  for (int q = 0; q < 6; ++q) {
    const double* lam = c_lam6[q];
    const double wq = c_w6[q] * F.area;
    double fq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) fq[k] = lam[0] * fv[0][k] + lam[1] * fv[1][k] + lam[2] * fv[2][k];
    for (int a = 0; a < 6; ++a) {
      const double N = p2_value(lam, a) * wq;
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[a * 3 + k] += N * fq[k];
    }
  }
  for (int i = 0; i < 18; ++i) atomicAdd(&Fv[shell_gdof(S, c, i)], sign * acc[i]);
}

// out[vertex b, k] += sign * int phi_b (lambda_u)_k : transpose of the load map applied to a state-sized vector
__global__ __launch_bounds__(SH_BLOCK) void k_shell_load_T(femo_shell_view S, const double* __restrict__ lam_state, double sign, double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  if (c >= S.n_cell) return;
  Facet F;
  facet_frame(S.x, S.conn, c, F);
  double le[18];
  for (int i = 0; i < 18; ++i) le[i] = lam_state[shell_gdof(S, c, i)];
  double acc[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int q = 0; q < 6; ++q) {
    const double* lam = c_lam6[q];
    const double wq = c_w6[q] * F.area;
    double uq[3] = {0, 0, 0};
    for (int a = 0; a < 6; ++a) {
      const double N = p2_value(lam, a);
#pragma unroll
      for (int k = 0; k < 3; ++k) uq[k] += N * le[a * 3 + k];
    }
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[b][k] += wq * lam[b] * uq[k];
  }
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&out[(int64_t)S.conn[c * 3 + b] * 3 + k], sign * acc[b][k]);
}

// compliance 1/2 int u.u (partials per block) and, if grad != nullptr, its gradient M_u w added to grad
// cellw (optional, one weight per cell): the `dxx` measure of shell_pde.py:66,284 -- dx_2(10), a tagged subset of cells --
// as a DG0 indicator; cells of weight 0 are skipped
__global__ __launch_bounds__(SH_BLOCK) void k_shell_compliance(femo_shell_view S, const double* __restrict__ w, const double* __restrict__ cellw,
                                                               double* __restrict__ partials, double* __restrict__ grad) {
  __shared__ double lds[SH_BLOCK / 64];
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  double J = 0.0;
  const double chi = (c < S.n_cell && cellw != nullptr) ? cellw[c] : 1.0;
  if (c < S.n_cell && chi != 0.0) {
    Facet F;
    facet_frame(S.x, S.conn, c, F);
    F.area *= chi;
    double ue[18], ge[18];
    for (int i = 0; i < 18; ++i) { ue[i] = w[shell_gdof(S, c, i)]; ge[i] = 0.0; }
    for (int q = 0; q < 6; ++q) {
      const double* lam = c_lam6[q];
      const double wq = c_w6[q] * F.area;
      double uq[3] = {0, 0, 0};
      for (int a = 0; a < 6; ++a) {
        const double N = p2_value(lam, a);
#pragma unroll
        for (int k = 0; k < 3; ++k) uq[k] += N * ue[a * 3 + k];
      }
      J += 0.5 * wq * (uq[0] * uq[0] + uq[1] * uq[1] + uq[2] * uq[2]);
      for (int a = 0; a < 6; ++a) {
        const double N = p2_value(lam, a) * wq;
#pragma unroll
        for (int k = 0; k < 3; ++k) ge[a * 3 + k] += N * uq[k];
      }
    }
    if (grad != nullptr)
      for (int i = 0; i < 18; ++i) atomicAdd(&grad[shell_gdof(S, c, i)], ge[i]);
  }
  if (partials != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(J, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

// int rho h (partials) and its gradient rho |T| / 3 per vertex
// J = 1 / alpha int (m sigma_vm)^rho dx, sigma_vm the von Mises stress of the in-plane stress C (eps + z kappa) at
// z = surface * h / 2 (oracle/shell_oracle.py::pnorm_stress; shell_pde.py:297-313), degree-4 rule; partials: per-block
// sums of the value, grad_w += dJ/dw (n_dof), grad_h += dJ/dh (n_vert).  One thread per cell.
__global__ __launch_bounds__(SH_BLOCK) void k_shell_pnorm_stress(femo_shell_view S, double E, double nu, const double* __restrict__ h,
                                                                 const double* __restrict__ w, double mscale, double rho, double inv_alpha,
                                                                 double surface, double* __restrict__ partials, double* __restrict__ grad_w,
                                                                 double* __restrict__ grad_h) {
  __shared__ double lds[SH_BLOCK / 64];
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  double val = 0.0;
  if (c < S.n_cell) {
    Facet F;
    facet_frame(S.x, S.conn, c, F);
    const Material mt = material(E, nu);
    const double hv[3] = {h[S.conn[c * 3]], h[S.conn[c * 3 + 1]], h[S.conn[c * 3 + 2]]};
    double we[27], gw[27];
    for (int i = 0; i < 27; ++i) { we[i] = w[shell_gdof(S, c, i)]; gw[i] = 0.0; }
    double gh[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < 6; ++q) {
      const double* lam = c_lam6[q];
      const double z = 0.5 * surface * (hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2]);
      const double wq = c_w6[q] * F.area;
      double sw[9];
      element_strain(F, lam, we, sw);
      const double e0 = sw[0] + z * sw[3], e1 = sw[1] + z * sw[4], e2 = sw[2] + z * sw[5];
      const double s0 = mt.c11 * e0 + mt.c12 * e1, s1 = mt.c12 * e0 + mt.c11 * e1, s2 = mt.c33 * e2;
      const double vm = sqrt(s0 * s0 - s0 * s1 + s1 * s1 + 3.0 * s2 * s2);
      if (vm == 0.0) continue;                 // exactly zero only: a non-finite stress shows in the value and both gradients
      const double pw = pow(mscale * vm, rho - 1.0);
      val += wq * pw * mscale * vm * inv_alpha;
      if (grad_w == nullptr && grad_h == nullptr) continue;
      const double fac = wq * rho * mscale * pw * inv_alpha / (2.0 * vm);             // dJ/dvm / (2 vm)
      const double d0 = fac * (2.0 * s0 - s1), d1 = fac * (2.0 * s1 - s0), d2 = fac * 6.0 * s2;   // dJ / d sigma
      const double t0 = mt.c11 * d0 + mt.c12 * d1, t1 = mt.c12 * d0 + mt.c11 * d1, t2 = mt.c33 * d2;   // dJ / d (eps + z kappa)
      const double dk = 0.5 * surface * (t0 * sw[3] + t1 * sw[4] + t2 * sw[5]);
#pragma unroll
      for (int b = 0; b < 3; ++b) gh[b] += dk * lam[b];
      if (grad_w != nullptr) {
        for (int col = 0; col < 27; ++col) {
          double bc[9];
          strain_column(F, lam, col, bc);
          gw[col] += t0 * (bc[0] + z * bc[3]) + t1 * (bc[1] + z * bc[4]) + t2 * (bc[2] + z * bc[5]);
        }
      }
    }
    if (grad_w != nullptr)
      for (int i = 0; i < 27; ++i)
        if (gw[i] != 0.0) atomicAdd(&grad_w[shell_gdof(S, c, i)], gw[i]);
    if (grad_h != nullptr) {
#pragma unroll
      for (int b = 0; b < 3; ++b) atomicAdd(&grad_h[S.conn[c * 3 + b]], gh[b]);
    }
  }
  if (partials != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(val * shell_value_weight(S, c), lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

// right-hand side of the L2 projection of the von Mises stress onto CG1 (shell_pde.py:330-332): b_i += int sigma_vm phi_i,
// and the row sums of the P1 mass matrix, lumped_i += |T| / 3.  One thread per cell.
__global__ __launch_bounds__(SH_BLOCK) void k_shell_vm_rhs(femo_shell_view S, double E, double nu, const double* __restrict__ h,
                                                           const double* __restrict__ w, double surface, double* __restrict__ rhs,
                                                           double* __restrict__ lumped) {
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  if (c >= S.n_cell) return;
  Facet F;
  facet_frame(S.x, S.conn, c, F);
  const Material mt = material(E, nu);
  const double hv[3] = {h[S.conn[c * 3]], h[S.conn[c * 3 + 1]], h[S.conn[c * 3 + 2]]};
  double we[27];
  for (int i = 0; i < 27; ++i) we[i] = w[shell_gdof(S, c, i)];
  double b[3] = {0.0, 0.0, 0.0};
  for (int q = 0; q < 6; ++q) {
    const double* lam = c_lam6[q];
    const double z = 0.5 * surface * (hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2]);
    double sw[9];
    element_strain(F, lam, we, sw);
    const double e0 = sw[0] + z * sw[3], e1 = sw[1] + z * sw[4], e2 = sw[2] + z * sw[5];
    const double s0 = mt.c11 * e0 + mt.c12 * e1, s1 = mt.c12 * e0 + mt.c11 * e1, s2 = mt.c33 * e2;
    const double vm = sqrt(s0 * s0 - s0 * s1 + s1 * s1 + 3.0 * s2 * s2);
#pragma unroll
    for (int a = 0; a < 3; ++a) b[a] += c_w6[q] * F.area * vm * lam[a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicAdd(&rhs[S.conn[c * 3 + a]], b[a]);
    if (lumped != nullptr) atomicAdd(&lumped[S.conn[c * 3 + a]], F.area * (1.0 / 3.0));
  }
}

// y += M x with the P1 mass matrix of the surface, element by element: M_e = |T| / 12 (1 + delta)
__global__ __launch_bounds__(SH_BLOCK) void k_shell_p1_mass(femo_shell_view S, const double* __restrict__ x, double* __restrict__ y) {
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  if (c >= S.n_cell) return;
  Facet F;
  facet_frame(S.x, S.conn, c, F);
  const int32_t v0 = S.conn[c * 3], v1 = S.conn[c * 3 + 1], v2 = S.conn[c * 3 + 2];
  const double x0 = x[v0], x1 = x[v1], x2 = x[v2], sum = x0 + x1 + x2, k = F.area * (1.0 / 12.0);
  atomicAdd(&y[v0], k * (sum + x0));
  atomicAdd(&y[v1], k * (sum + x1));
  atomicAdd(&y[v2], k * (sum + x2));
}

__global__ __launch_bounds__(SH_BLOCK) void k_shell_mass(femo_shell_view S, double rho, const double* __restrict__ h, double* __restrict__ partials,
                                                         double* __restrict__ grad) {
  __shared__ double lds[SH_BLOCK / 64];
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  double M = 0.0;
  if (c < S.n_cell) {
    Facet F;
    facet_frame(S.x, S.conn, c, F);
    const double a3 = rho * F.area * (1.0 / 3.0);
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      M += a3 * h[S.conn[c * 3 + b]];
      if (grad != nullptr) atomicAdd(&grad[S.conn[c * 3 + b]], a3);
    }
  }
  if (partials != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(M * shell_value_weight(S, c), lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

// ------------------------------------------------- penalty boundary terms, inertia, regularisation (round 3) ----
// Edge mass matrices on [0, 1] x length: P2 (end vertices, midpoint) and P1
__constant__ double c_m2[3][3] = {{4.0 / 30, -1.0 / 30, 2.0 / 30}, {-1.0 / 30, 4.0 / 30, 2.0 / 30}, {2.0 / 30, 2.0 / 30, 16.0 / 30}};
__constant__ double c_m1[2][2] = {{2.0 / 6, 1.0 / 6}, {1.0 / 6, 2.0 / 6}};

// vals += K_pen: per tagged edge and component 9 + 4 entries at the CSR positions the host looked up (pos: 39 per edge,
// component-major: 9 displacement pairs row-major over (v0, v1, mid), then 4 rotation pairs over (v0, v1)); coef =
// beta (sum over adjacent cells of 1 / h_E) |edge|  (oracle/shell_oracle.py::penalty_matrix)
__global__ void k_shell_penalty_add(int64_t n_e, const int32_t* __restrict__ pos, const double* __restrict__ coef, double* __restrict__ vals) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_e * 39) return;
  const int64_t e = t / 39;
  const int r = (int)(t % 39) % 13;
  const double m = r < 9 ? c_m2[r / 3][r % 3] : c_m1[(r - 9) / 2][(r - 9) % 2];
  atomicAdd(&vals[pos[t]], coef[e] * m);
}

// y += K_pen (x - g)   (g == nullptr: homogeneous data)
__global__ void k_shell_penalty_apply(int64_t n_e, const int32_t* __restrict__ nodes, const double* __restrict__ coef, int64_t n_unode,
                                      const double* __restrict__ x, const double* __restrict__ g, double* __restrict__ y) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_e) return;
  const int64_t un[3] = {nodes[3 * e], nodes[3 * e + 1], nodes[3 * e + 2]};
  const double cf = coef[e];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { const int64_t dof = 3 * un[i] + k; d[i] = x[dof] - (g ? g[dof] : 0.0); }
#pragma unroll
    for (int i = 0; i < 3; ++i) atomicAdd(&y[3 * un[i] + k], cf * (c_m2[i][0] * d[0] + c_m2[i][1] * d[1] + c_m2[i][2] * d[2]));
    double t2[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { const int64_t dof = 3 * n_unode + 3 * un[i] + k; t2[i] = x[dof] - (g ? g[dof] : 0.0); }
#pragma unroll
    for (int i = 0; i < 2; ++i) atomicAdd(&y[3 * n_unode + 3 * un[i] + k], cf * (c_m1[i][0] * t2[0] + c_m1[i][1] * t2[1]));
  }
}

// Inertial residual (shell_pde.py:255-256 kinetic_residual -> inertialResidual [ext]):
//   y += M(h) a,  M = int rho h  N_a N_b (displacements, P2) + int rho h^3 / 12  phi_a phi_b (rotations, P1), degree-4 rule;
//   out_h[b] += lam^T (dM/dh_b) a   when lam != nullptr (y is not written then).  One thread per cell.
//   dh != nullptr (with lam == nullptr): y += (dM/dh [dh]) a, the forward product -- the section weights h and h^3/12 replaced
//   by their derivatives in the direction dh.
__global__ __launch_bounds__(SH_BLOCK) void k_shell_inertia(femo_shell_view S, double rho, const double* __restrict__ h, const double* __restrict__ a,
                                                            const double* __restrict__ lam_state, double* __restrict__ y, double* __restrict__ out_h,
                                                            const double* __restrict__ dh = nullptr) {
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  if (c >= S.n_cell) return;
  Facet F;
  facet_frame(S.x, S.conn, c, F);
  const double hv[3] = {h[S.conn[c * 3]], h[S.conn[c * 3 + 1]], h[S.conn[c * 3 + 2]]};
  double ae[27], le[27], acc[27];
  for (int i = 0; i < 27; ++i) {
    const int64_t gd = shell_gdof(S, c, i);
    ae[i] = a[gd];
    le[i] = lam_state ? lam_state[gd] : 0.0;
    acc[i] = 0.0;
  }
  double gh[3] = {0.0, 0.0, 0.0};
  for (int q = 0; q < 6; ++q) {
    const double* lam = c_lam6[q];
    const double hq = hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2];
    const double wq = c_w6[q] * F.area * rho;
    double uq[3] = {0, 0, 0}, tq[3] = {0, 0, 0}, lu[3] = {0, 0, 0}, lt[3] = {0, 0, 0};
    for (int n = 0; n < 6; ++n) {
      const double N = p2_value(lam, n);
#pragma unroll
      for (int k = 0; k < 3; ++k) { uq[k] += N * ae[3 * n + k]; lu[k] += N * le[3 * n + k]; }
    }
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int k = 0; k < 3; ++k) { tq[k] += lam[b] * ae[18 + 3 * b + k]; lt[k] += lam[b] * le[18 + 3 * b + k]; }
    if (lam_state == nullptr) {
      double cu = wq * hq, ct = wq * hq * hq * hq * (1.0 / 12.0);
      if (dh != nullptr) {
        const double dq = dh[S.conn[c * 3]] * lam[0] + dh[S.conn[c * 3 + 1]] * lam[1] + dh[S.conn[c * 3 + 2]] * lam[2];
        cu = wq * dq; ct = wq * 0.25 * hq * hq * dq;
      }
      for (int n = 0; n < 6; ++n) {
        const double N = p2_value(lam, n) * cu;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[3 * n + k] += N * uq[k];
      }
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[18 + 3 * b + k] += ct * lam[b] * tq[k];
    } else {
      const double d = wq * ((lu[0] * uq[0] + lu[1] * uq[1] + lu[2] * uq[2]) + 0.25 * hq * hq * (lt[0] * tq[0] + lt[1] * tq[1] + lt[2] * tq[2]));
#pragma unroll
      for (int b = 0; b < 3; ++b) gh[b] += d * lam[b];
    }
  }
  if (lam_state == nullptr) {
    for (int i = 0; i < 27; ++i) atomicAdd(&y[shell_gdof(S, c, i)], acc[i]);
  } else {
#pragma unroll
    for (int b = 0; b < 3; ++b) atomicAdd(&out_h[S.conn[c * 3 + b]], gh[b]);
  }
}

// `ShellPDE.regularization(h, type)` (shell_pde.py:262-282), alpha1 = 1e3, alpha2 = 1, CG1 thickness on flat facets:
//   kind 1 'H1':  1/2 alpha1 int |grad h|^2     kind 2 'L2H1': 1/2 alpha1 int h^2 + 1/2 alpha2 int h_mesh^2 |grad h|^2
//   kind 3 'L2':  1/2 alpha1 int h^2            h_mesh = CellDiameter = the largest vertex distance of the cell [ext]
// partials: per-block sums of the value; grad += d/dh.  One thread per cell.
__global__ __launch_bounds__(SH_BLOCK) void k_shell_regularization(femo_shell_view S, int kind, const double* __restrict__ h,
                                                                   double* __restrict__ partials, double* __restrict__ grad) {
  __shared__ double lds[SH_BLOCK / 64];
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  double val = 0.0;
  if (c < S.n_cell) {
    Facet F;
    facet_frame(S.x, S.conn, c, F);
    const double a1 = 1e3, a2 = 1.0;
    const double hv[3] = {h[S.conn[c * 3]], h[S.conn[c * 3 + 1]], h[S.conn[c * 3 + 2]]};
    double g[3] = {0.0, 0.0, 0.0};
    if (kind == 2 || kind == 3) {
      const double k12 = F.area * (1.0 / 12.0), sum = hv[0] + hv[1] + hv[2];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const double Mh = k12 * (sum + hv[b]);
        val += 0.5 * a1 * hv[b] * Mh;
        g[b] += a1 * Mh;
      }
    }
    if (kind == 1 || kind == 2) {
      double coef = a1 * F.area;
      if (kind == 2) {
        double d2 = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int j = (i + 1) % 3;
          double l2 = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double dx = S.x[(int64_t)S.conn[c * 3 + i] * 3 + k] - S.x[(int64_t)S.conn[c * 3 + j] * 3 + k];
            l2 += dx * dx;
          }
          d2 = fmax(d2, l2);
        }
        coef = a2 * d2 * F.area;
      }
      const double g1 = F.gl[0][0] * hv[0] + F.gl[1][0] * hv[1] + F.gl[2][0] * hv[2];
      const double g2 = F.gl[0][1] * hv[0] + F.gl[1][1] * hv[1] + F.gl[2][1] * hv[2];
      val += 0.5 * coef * (g1 * g1 + g2 * g2);
#pragma unroll
      for (int b = 0; b < 3; ++b) g[b] += coef * (F.gl[b][0] * g1 + F.gl[b][1] * g2);
    }
    if (grad != nullptr) {
#pragma unroll
      for (int b = 0; b < 3; ++b) atomicAdd(&grad[S.conn[c * 3 + b]], g[b]);
    }
  }
  if (partials != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(val * shell_value_weight(S, c), lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

// int coef h^p dx with the degree-4 rule (the thickness term of pnorm_stress(regularization=True), shell_pde.py:307-309:
// 0.5 * 1e3 * h**rho * dx) and its gradient.  One thread per cell.
__global__ __launch_bounds__(SH_BLOCK) void k_shell_hpower(femo_shell_view S, double coef, double p, const double* __restrict__ h,
                                                           double* __restrict__ partials, double* __restrict__ grad) {
  __shared__ double lds[SH_BLOCK / 64];
  const int64_t c = (int64_t)blockIdx.x * SH_BLOCK + threadIdx.x;
  double val = 0.0;
  if (c < S.n_cell) {
    Facet F;
    facet_frame(S.x, S.conn, c, F);
    const double hv[3] = {h[S.conn[c * 3]], h[S.conn[c * 3 + 1]], h[S.conn[c * 3 + 2]]};
    double g[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < 6; ++q) {
      const double* lam = c_lam6[q];
      const double hq = hv[0] * lam[0] + hv[1] * lam[1] + hv[2] * lam[2];
      const double wq = c_w6[q] * F.area * coef;
      const double pm1 = pow(hq, p - 1.0);
      val += wq * pm1 * hq;
#pragma unroll
      for (int b = 0; b < 3; ++b) g[b] += wq * p * pm1 * lam[b];
    }
    if (grad != nullptr) {
#pragma unroll
      for (int b = 0; b < 3; ++b) atomicAdd(&grad[S.conn[c * 3 + b]], g[b]);
    }
  }
  if (partials != nullptr) {
    const double t = femo_block_sum<SH_BLOCK>(val * shell_value_weight(S, c), lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
  }
}

femo_shell_view view(const femo_shell* s) {
  femo_shell_view v;
  v.n_vert = s->n_vert; v.n_cell = s->n_cell; v.n_unode = s->n_unode;
  v.x = s->d_x; v.conn = s->d_conn; v.cedge = s->d_cedge;
  v.cell_owned = s->d_cell_owned;
  return v;
}

int reduce_partials(femo_ctx* ctx, const double* d_part, int nb, double* host) {
  std::vector<double> h((size_t)nb);
  FEMO_HIP_CHECK(hipMemcpyAsync(h.data(), d_part, nb * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  double s = 0.0;
  for (double v : h) s += v;
  if (ctx->nranks > 1) {
    // a shell on several ranks is partitioned: the caller integrates over the cells it owns (cell weights) and the
    // value is the sum over the ranks
    FEMO_HIP_CHECK(hipMemcpyAsync(ctx->d_scal, &s, sizeof s, hipMemcpyHostToDevice, ctx->stream));
    FEMO_TRY(femo_coll_allreduce(ctx, ctx->d_scal, 1, ctx->stream));
    FEMO_HIP_CHECK(hipMemcpyAsync(&s, ctx->d_scal, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
    FEMO_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  *host = s;
  return 0;
}

}  // namespace

extern "C" {

int femo_shell_assemble(femo_shell* s, double E, double nu, const femo_vec* h, femo_vec* vals) {
  FEMO_REQUIRE(s && h && vals, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && vals->n >= s->nnz, "vector size mismatch in shell_assemble");
  FEMO_REQUIRE(E > 0.0 && nu > -1.0 && nu < 0.5, "bad material");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(vals);
  FEMO_HIP_CHECK(hipMemsetAsync(vals->d, 0, s->nnz * sizeof(double), st));
  hipLaunchKernelGGL(k_shell_assemble, dim3(sgrid(s->n_cell * 27)), dim3(SH_BLOCK), 0, st, view(s), E, nu, h->d, s->d_epos, vals->d);
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_TRY(shell_zero_unowned_rows(s, vals->d, st));       // partitioned: the rank's share of K (its points' rows are complete)
  return 0;
}

int femo_shell_load(femo_shell* s, const femo_vec* f, double sign, int accumulate, femo_vec* F) {
  FEMO_REQUIRE(s && f && F, "null argument");
  FEMO_REQUIRE(f->n >= 3 * s->n_vert && F->n >= s->n_dof, "vector size mismatch in shell_load");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(F);
  if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(F->d, 0, s->n_dof * sizeof(double), st));
  hipLaunchKernelGGL(k_shell_load, dim3(sgrid(s->n_cell)), dim3(SH_BLOCK), 0, st, view(s), f->d, sign, F->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_shell_load_T(femo_shell* s, const femo_vec* lam, double sign, int accumulate, femo_vec* out) {
  FEMO_REQUIRE(s && lam && out, "null argument");
  FEMO_REQUIRE(lam->n >= s->n_dof && out->n >= 3 * s->n_vert, "vector size mismatch in shell_load_T");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(out);
  if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(out->d, 0, 3 * s->n_vert * sizeof(double), st));
  hipLaunchKernelGGL(k_shell_load_T, dim3(sgrid(s->n_cell)), dim3(SH_BLOCK), 0, st, view(s), lam->d, sign, out->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// out_b (+)= sign * v^T (dK/dh_b) w;  energy (optional) = 1/2 v^T K(h) w
int femo_shell_dform_dh(femo_shell* s, double E, double nu, const femo_vec* h, const femo_vec* v, const femo_vec* w,
                        int accumulate, femo_vec* out, double* energy) {
  FEMO_REQUIRE(s && h && v && w, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && v->n >= s->n_dof && w->n >= s->n_dof, "vector size mismatch in shell_dform_dh");
  FEMO_REQUIRE(out == nullptr || out->n >= s->n_vert, "output shorter than n_vert");
  hipStream_t st = s->ctx->stream;
  const unsigned g = sgrid(s->n_cell);
  FEMO_REQUIRE(energy == nullptr || g <= 3 * SH_MAXPART, "mesh too large for the energy reduction buffer");
  if (out) {
    femo_vec_touch(out);
    if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(out->d, 0, s->n_vert * sizeof(double), st));
  }
  hipLaunchKernelGGL(k_shell_dform_dh, dim3(g), dim3(SH_BLOCK), 0, st, view(s), E, nu, h->d, v->d, w->d, out ? out->d : nullptr,
                     energy ? s->d_part : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  if (energy) FEMO_TRY(reduce_partials(s->ctx, s->d_part, (int)g, energy));
  return 0;
}

// y (+)= (dK/dh [dh]) w: forward product with the thickness partial of the elastic residual
int femo_shell_dform_dh_fwd(femo_shell* s, double E, double nu, const femo_vec* h, const femo_vec* dh, const femo_vec* w, int accumulate, femo_vec* y) {
  FEMO_REQUIRE(s && h && dh && w && y, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && dh->n >= s->n_vert && w->n >= s->n_dof && y->n >= s->n_dof && w->d != y->d, "vector size mismatch in shell_dform_dh_fwd");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(y);
  if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(y->d, 0, s->n_dof * sizeof(double), st));
  hipLaunchKernelGGL(k_shell_dform_dh_fwd, dim3(sgrid(s->n_cell)), dim3(SH_BLOCK), 0, st, view(s), E, nu, h->d, dh->d, w->d, y->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_shell_compliance(femo_shell* s, const femo_vec* w, double* value, int accumulate, femo_vec* grad) {
  return femo_shell_compliance_dx(s, w, nullptr, value, accumulate, grad);
}

int femo_shell_compliance_dx(femo_shell* s, const femo_vec* w, const femo_vec* cell_weight, double* value, int accumulate, femo_vec* grad) {
  FEMO_REQUIRE(s && w, "null argument");
  FEMO_REQUIRE(w->n >= s->n_dof && (grad == nullptr || grad->n >= s->n_dof), "vector size mismatch in shell_compliance");
  FEMO_REQUIRE(cell_weight == nullptr || cell_weight->n >= s->n_cell, "cell weights shorter than n_cell");
  hipStream_t st = s->ctx->stream;
  const unsigned g = sgrid(s->n_cell);
  FEMO_REQUIRE(value == nullptr || g <= 3 * SH_MAXPART, "mesh too large for the reduction buffer");
  if (grad) {
    femo_vec_touch(grad);
    if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(grad->d, 0, s->n_dof * sizeof(double), st));
  }
  hipLaunchKernelGGL(k_shell_compliance, dim3(g), dim3(SH_BLOCK), 0, st, view(s), w->d, cell_weight ? cell_weight->d : (const double*)nullptr,
                     value ? s->d_part : nullptr, grad ? grad->d : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  if (value) FEMO_TRY(reduce_partials(s->ctx, s->d_part, (int)g, value));
  return 0;
}

int femo_shell_pnorm_stress(femo_shell* s, double E, double nu, const femo_vec* h, const femo_vec* w, double m, double rho, double alpha,
                            double surface, double* value, int accumulate, femo_vec* grad_w, femo_vec* grad_h) {
  FEMO_REQUIRE(s && h && w, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && w->n >= s->n_dof && (grad_w == nullptr || grad_w->n >= s->n_dof) &&
               (grad_h == nullptr || grad_h->n >= s->n_vert), "vector size mismatch in shell_pnorm_stress");
  FEMO_REQUIRE(E > 0.0 && nu > -1.0 && nu < 0.5 && m > 0.0 && rho >= 1.0 && alpha > 0.0, "bad parameters of the stress aggregate");
  hipStream_t st = s->ctx->stream;
  const unsigned g = sgrid(s->n_cell);
  FEMO_REQUIRE(value == nullptr || g <= 3 * SH_MAXPART, "mesh too large for the reduction buffer");
  if (grad_w) {
    femo_vec_touch(grad_w);
    if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(grad_w->d, 0, s->n_dof * sizeof(double), st));
  }
  if (grad_h) {
    femo_vec_touch(grad_h);
    if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(grad_h->d, 0, s->n_vert * sizeof(double), st));
  }
  hipLaunchKernelGGL(k_shell_pnorm_stress, dim3(g), dim3(SH_BLOCK), 0, st, view(s), E, nu, h->d, w->d, m, rho, 1.0 / alpha, surface,
                     value ? s->d_part : nullptr, grad_w ? grad_w->d : nullptr, grad_h ? grad_h->d : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  if (value) FEMO_TRY(reduce_partials(s->ctx, s->d_part, (int)g, value));
  return 0;
}

int femo_shell_vm_rhs(femo_shell* s, double E, double nu, const femo_vec* h, const femo_vec* w, double surface, femo_vec* rhs,
                      femo_vec* lumped) {
  FEMO_REQUIRE(s && h && w && rhs, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && w->n >= s->n_dof && rhs->n >= s->n_vert && (lumped == nullptr || lumped->n >= s->n_vert),
               "vector size mismatch in shell_vm_rhs");
  FEMO_REQUIRE(E > 0.0 && nu > -1.0 && nu < 0.5, "bad material");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(rhs);
  FEMO_HIP_CHECK(hipMemsetAsync(rhs->d, 0, s->n_vert * sizeof(double), st));
  if (lumped) {
    femo_vec_touch(lumped);
    FEMO_HIP_CHECK(hipMemsetAsync(lumped->d, 0, s->n_vert * sizeof(double), st));
  }
  hipLaunchKernelGGL(k_shell_vm_rhs, dim3(sgrid(s->n_cell)), dim3(SH_BLOCK), 0, st, view(s), E, nu, h->d, w->d, surface, rhs->d,
                     lumped ? lumped->d : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_shell_p1_mass(femo_shell* s, const femo_vec* x, femo_vec* y) {
  FEMO_REQUIRE(s && x && y, "null argument");
  FEMO_REQUIRE(x->n >= s->n_vert && y->n >= s->n_vert && x->d != y->d, "vector size mismatch in shell_p1_mass");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(y);
  FEMO_HIP_CHECK(hipMemsetAsync(y->d, 0, s->n_vert * sizeof(double), st));
  hipLaunchKernelGGL(k_shell_p1_mass, dim3(sgrid(s->n_cell)), dim3(SH_BLOCK), 0, st, view(s), x->d, y->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

int femo_shell_mass(femo_shell* s, double rho, const femo_vec* h, double* value, int accumulate, femo_vec* grad) {
  FEMO_REQUIRE(s && h, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && (grad == nullptr || grad->n >= s->n_vert), "vector size mismatch in shell_mass");
  hipStream_t st = s->ctx->stream;
  const unsigned g = sgrid(s->n_cell);
  FEMO_REQUIRE(value == nullptr || g <= 3 * SH_MAXPART, "mesh too large for the reduction buffer");
  if (grad) {
    femo_vec_touch(grad);
    if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(grad->d, 0, s->n_vert * sizeof(double), st));
  }
  hipLaunchKernelGGL(k_shell_mass, dim3(g), dim3(SH_BLOCK), 0, st, view(s), rho, h->d, value ? s->d_part : nullptr, grad ? grad->d : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  if (value) FEMO_TRY(reduce_partials(s->ctx, s->d_part, (int)g, value));
  return 0;
}

// ---- penalty boundary terms: K_pen = sum over tagged edges of coef_e x (edge mass matrices), all six fields ----
int femo_shell_set_penalty(femo_shell* s, int64_t n_edges, const int32_t* edge_nodes, const double* coef, const int32_t* pos) {
  FEMO_REQUIRE(s != nullptr && n_edges >= 0, "bad argument");
  FEMO_REQUIRE(n_edges == 0 || (edge_nodes && coef && pos), "null argument");
  hipStream_t st = s->ctx->stream;
  FEMO_HIP_CHECK(hipSetDevice(s->ctx->device));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  hipFree(s->d_pen_nodes); hipFree(s->d_pen_pos); hipFree(s->d_pen_coef);
  s->d_pen_nodes = s->d_pen_pos = nullptr; s->d_pen_coef = nullptr; s->pen_n = 0;
  if (n_edges == 0) return 0;
  for (int64_t e = 0; e < n_edges; ++e) {
    FEMO_REQUIRE(edge_nodes[3 * e] >= 0 && edge_nodes[3 * e] < s->n_vert && edge_nodes[3 * e + 1] >= 0 && edge_nodes[3 * e + 1] < s->n_vert &&
                 edge_nodes[3 * e + 2] >= s->n_vert && edge_nodes[3 * e + 2] < s->n_unode, "penalty edge %lld: bad node numbers", (long long)e);
    for (int k = 0; k < 39; ++k) FEMO_REQUIRE(pos[39 * e + k] >= 0 && pos[39 * e + k] < s->nnz, "penalty edge %lld: position outside the pattern", (long long)e);
  }
  FEMO_TRY(to_device(&s->d_pen_nodes, edge_nodes, 3 * n_edges, st));
  FEMO_TRY(to_device(&s->d_pen_pos, pos, 39 * n_edges, st));
  FEMO_TRY(to_device(&s->d_pen_coef, coef, n_edges, st));
  FEMO_HIP_CHECK(hipStreamSynchronize(st));
  s->pen_n = n_edges;
  return 0;
}

int femo_shell_penalty_add(femo_shell* s, femo_vec* vals) {
  FEMO_REQUIRE(s && vals, "null argument");
  FEMO_REQUIRE(vals->n >= s->nnz, "vector size mismatch in shell_penalty_add");
  if (s->pen_n == 0) return 0;
  femo_vec_touch(vals);
  hipLaunchKernelGGL(k_shell_penalty_add, dim3(sgrid(s->pen_n * 39, 256)), dim3(256), 0, s->ctx->stream, s->pen_n, s->d_pen_pos, s->d_pen_coef, vals->d);
  FEMO_HIP_CHECK(hipGetLastError());
  FEMO_TRY(shell_zero_unowned_rows(s, vals->d, s->ctx->stream));
  return 0;
}

int femo_shell_penalty_apply(femo_shell* s, const femo_vec* x, const femo_vec* g, int accumulate, femo_vec* y) {
  FEMO_REQUIRE(s && x && y, "null argument");
  FEMO_REQUIRE(x->n >= s->n_dof && y->n >= s->n_dof && (g == nullptr || g->n >= s->n_dof) && x->d != y->d, "vector size mismatch in shell_penalty_apply");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(y);
  if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(y->d, 0, s->n_dof * sizeof(double), st));
  if (s->pen_n == 0) return 0;
  hipLaunchKernelGGL(k_shell_penalty_apply, dim3(sgrid(s->pen_n, 256)), dim3(256), 0, st, s->pen_n, s->d_pen_nodes, s->d_pen_coef, s->n_unode, x->d,
                     g ? g->d : (const double*)nullptr, y->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// y (+)= M(h) acc: the inertial residual for the accelerations `acc` in state layout
int femo_shell_inertia_apply(femo_shell* s, double rho, const femo_vec* h, const femo_vec* acc, int accumulate, femo_vec* y) {
  FEMO_REQUIRE(s && h && acc && y, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && acc->n >= s->n_dof && y->n >= s->n_dof && acc->d != y->d, "vector size mismatch in shell_inertia_apply");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(y);
  if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(y->d, 0, s->n_dof * sizeof(double), st));
  hipLaunchKernelGGL(k_shell_inertia, dim3(sgrid(s->n_cell)), dim3(SH_BLOCK), 0, st, view(s), rho, h->d, acc->d, (const double*)nullptr, y->d, (double*)nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// out_b (+)= lam^T (dM/dh_b) acc: the thickness partial of the inertial residual, transposed
int femo_shell_inertia_dh(femo_shell* s, double rho, const femo_vec* h, const femo_vec* lam, const femo_vec* acc, int accumulate, femo_vec* out) {
  FEMO_REQUIRE(s && h && lam && acc && out, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && lam->n >= s->n_dof && acc->n >= s->n_dof && out->n >= s->n_vert, "vector size mismatch in shell_inertia_dh");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(out);
  if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(out->d, 0, s->n_vert * sizeof(double), st));
  hipLaunchKernelGGL(k_shell_inertia, dim3(sgrid(s->n_cell)), dim3(SH_BLOCK), 0, st, view(s), rho, h->d, acc->d, lam->d, (double*)nullptr, out->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// y (+)= (dM/dh [dh]) acc: the thickness partial of the inertial residual, forward mode
int femo_shell_inertia_dh_fwd(femo_shell* s, double rho, const femo_vec* h, const femo_vec* dh, const femo_vec* acc, int accumulate, femo_vec* y) {
  FEMO_REQUIRE(s && h && dh && acc && y, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && dh->n >= s->n_vert && acc->n >= s->n_dof && y->n >= s->n_dof && acc->d != y->d, "vector size mismatch in shell_inertia_dh_fwd");
  hipStream_t st = s->ctx->stream;
  femo_vec_touch(y);
  if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(y->d, 0, s->n_dof * sizeof(double), st));
  hipLaunchKernelGGL(k_shell_inertia, dim3(sgrid(s->n_cell)), dim3(SH_BLOCK), 0, st, view(s), rho, h->d, acc->d, (const double*)nullptr, y->d, (double*)nullptr, dh->d);
  FEMO_HIP_CHECK(hipGetLastError());
  return 0;
}

// kind 1 'H1', 2 'L2H1', 3 'L2' (shell_pde.py:262-282); value and / or gradient w.r.t. the thickness
int femo_shell_regularization(femo_shell* s, int kind, const femo_vec* h, double* value, int accumulate, femo_vec* grad) {
  FEMO_REQUIRE(s && h, "null argument");
  FEMO_REQUIRE(kind >= 1 && kind <= 3, "unknown regularisation kind %d", kind);
  FEMO_REQUIRE(h->n >= s->n_vert && (grad == nullptr || grad->n >= s->n_vert), "vector size mismatch in shell_regularization");
  hipStream_t st = s->ctx->stream;
  const unsigned g = sgrid(s->n_cell);
  FEMO_REQUIRE(value == nullptr || g <= 3 * SH_MAXPART, "mesh too large for the reduction buffer");
  if (grad) {
    femo_vec_touch(grad);
    if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(grad->d, 0, s->n_vert * sizeof(double), st));
  }
  hipLaunchKernelGGL(k_shell_regularization, dim3(g), dim3(SH_BLOCK), 0, st, view(s), kind, h->d, value ? s->d_part : nullptr, grad ? grad->d : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  if (value) FEMO_TRY(reduce_partials(s->ctx, s->d_part, (int)g, value));
  return 0;
}

// int coef h^p dx and its thickness gradient
int femo_shell_hpower(femo_shell* s, double coef, double p, const femo_vec* h, double* value, int accumulate, femo_vec* grad) {
  FEMO_REQUIRE(s && h, "null argument");
  FEMO_REQUIRE(h->n >= s->n_vert && (grad == nullptr || grad->n >= s->n_vert), "vector size mismatch in shell_hpower");
  hipStream_t st = s->ctx->stream;
  const unsigned g = sgrid(s->n_cell);
  FEMO_REQUIRE(value == nullptr || g <= 3 * SH_MAXPART, "mesh too large for the reduction buffer");
  if (grad) {
    femo_vec_touch(grad);
    if (!accumulate) FEMO_HIP_CHECK(hipMemsetAsync(grad->d, 0, s->n_vert * sizeof(double), st));
  }
  hipLaunchKernelGGL(k_shell_hpower, dim3(g), dim3(SH_BLOCK), 0, st, view(s), coef, p, h->d, value ? s->d_part : nullptr, grad ? grad->d : nullptr);
  FEMO_HIP_CHECK(hipGetLastError());
  if (value) FEMO_TRY(reduce_partials(s->ctx, s->d_part, (int)g, value));
  return 0;
}

}  // extern "C"

void shell_forms_free(femo_shell* s) {
  hipFree(s->d_pen_nodes); hipFree(s->d_pen_pos); hipFree(s->d_pen_coef);
}
