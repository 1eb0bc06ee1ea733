// Dense solve of the MMA subproblem's dual Newton system (mma.hip): at most FEMO_SMALL_MAX unknowns, Gaussian elimination
// with partial pivoting on the host.  Plain C++ with no dependency on the library, so that it can be compiled into a
// stand-alone program (tests/native/small_solve_main.cpp).
#pragma once

#include <cmath>

constexpr int FEMO_SMALL_MAX = 9;

// Solves A x = b in place: A is n x n row-major with row stride lda and is destroyed, b becomes x.
// Returns 0, or 1 when a pivot is zero or not finite (A singular to working precision, or bad input); b is then undefined.
inline int femo_small_solve(int n, double* A, int lda, double* b) {
  if (n < 0 || n > FEMO_SMALL_MAX || lda < n) return 1;
  for (int k = 0; k < n; ++k) {
    int piv = k;
    double big = std::fabs(A[k * lda + k]);
    for (int i = k + 1; i < n; ++i) {
      const double v = std::fabs(A[i * lda + k]);
      if (v > big) { big = v; piv = i; }
    }
    if (!(big > 0.0) || !std::isfinite(big)) return 1;
    if (piv != k) {
      for (int j = k; j < n; ++j) { const double t = A[k * lda + j]; A[k * lda + j] = A[piv * lda + j]; A[piv * lda + j] = t; }
      const double t = b[k]; b[k] = b[piv]; b[piv] = t;
    }
    const double inv = 1.0 / A[k * lda + k];
    for (int i = k + 1; i < n; ++i) {
      const double l = A[i * lda + k] * inv;
      if (l == 0.0) continue;
      for (int j = k + 1; j < n; ++j) A[i * lda + j] -= l * A[k * lda + j];
      b[i] -= l * b[k];
    }
  }
  for (int k = n - 1; k >= 0; --k) {
    double s = b[k];
    for (int j = k + 1; j < n; ++j) s -= A[k * lda + j] * b[j];
    b[k] = s / A[k * lda + k];
    if (!std::isfinite(b[k])) return 1;
  }
  return 0;
}
