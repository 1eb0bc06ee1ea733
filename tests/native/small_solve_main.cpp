// Stand-alone driver of femo_amd/csrc/small_solve.h (the dense solve of the MMA subproblem's Newton system).  Reads systems
// from standard input -- a count, then per system n, the n x n matrix row by row and the right-hand side -- solves each in a
// buffer of stride FEMO_SMALL_MAX, as mma.hip does, and prints "rc x_0 ... x_{n-1}" per system with 17 significant digits.
// Built with -fsanitize=address,undefined and run by tests/test_small_solve_native.py, which compares with numpy.linalg.solve.
#include <cstdio>
#include <vector>

#include "small_solve.h"

int main() {
  int count = 0;
  if (std::scanf("%d", &count) != 1 || count < 0) return 2;
  for (int c = 0; c < count; ++c) {
    int n = 0;
    if (std::scanf("%d", &n) != 1) return 2;
    if (n < 0 || n > FEMO_SMALL_MAX) {           // refused sizes: nothing follows on the input
      std::vector<double> none(1, 0.0);
      std::printf("%d\n", femo_small_solve(n, none.data(), n, none.data()));
      continue;
    }
    std::vector<double> A((size_t)FEMO_SMALL_MAX * FEMO_SMALL_MAX, 0.0), b((size_t)FEMO_SMALL_MAX, 0.0);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        if (std::scanf("%lf", &A[(size_t)i * FEMO_SMALL_MAX + j]) != 1) return 2;
    for (int i = 0; i < n; ++i)
      if (std::scanf("%lf", &b[(size_t)i]) != 1) return 2;
    const int rc = femo_small_solve(n, A.data(), FEMO_SMALL_MAX, b.data());
    std::printf("%d", rc);
    for (int i = 0; i < n; ++i) std::printf(" %.17g", rc == 0 ? b[(size_t)i] : 0.0);
    std::printf("\n");
  }
  std::printf("small_solve: done\n");
  return 0;
}
