// Stand-alone check of the host half of the density filter's build plan (femo_amd/csrc/filter_grid.h): the bounding box,
// the cell-size loop and the cell counts.  Built with -fsanitize=address,undefined and run by
// tests/test_filter_grid_native.py; exits 0 when every case holds.
//
// For every finite input: the plan ends, ncell <= 4 n + 1024, h >= r, every direction has at least one cell, the cell of
// every point needs no clamping (0 <= floor((p - lo) / h) < n[k]) and equals what the kernels' formula gives, and two points
// within r of each other lie in cells that differ by at most one in every direction -- the property the 3^d walk of the
// row kernel rests on.  Non-finite input is refused; the loop as it stood before this header (restated below with a cap on
// its iterations) does not end on it.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "filter_grid.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static uint64_t rng_state = 11;
static double uniform() {                      // [0, 1), 53 bits
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0);
}

static std::vector<double> cloud(int dim, int64_t n, double scale, const double* shift = nullptr) {
  std::vector<double> x((size_t)(n * dim));
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < dim; ++k) x[(size_t)(i * dim + k)] = uniform() * scale + (shift ? shift[k] : 0.0);
  return x;
}

// The plan loop as it was inside femo_filter_create before the finite check, stopped after `cap` growth steps.
// Returns true if it ended by itself.
static bool old_loop_ends(int dim, int64_t n, const double* coords, double radius, int cap) {
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int k = 0; k < dim; ++k) { lo[k] = coords[k]; hi[k] = coords[k]; }
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < dim; ++k) { lo[k] = std::min(lo[k], coords[i * dim + k]); hi[k] = std::max(hi[k], coords[i * dim + k]); }
  double h = radius;
  for (int it = 0; it < cap; ++it) {
    double cells = 1.0;
    for (int k = 0; k < dim; ++k) cells *= std::floor((hi[k] - lo[k]) / h) + 1.0;
    if (cells <= 4.0 * (double)n + 1024.0) return true;
    h *= 1.25;
  }
  return false;
}

// every property of a finite input; returns the plan for case-specific checks
static FilterGrid check_plan(const char* name, int dim, const std::vector<double>& x, double r, int64_t* ncell_out = nullptr) {
  const int64_t n = (int64_t)x.size() / dim;
  FilterGrid G{};
  int64_t ncell = -1;
  const int rc = filter_grid_plan(dim, n, x.data(), r, &G, &ncell);
  const int before = failures;
  CHECK(rc == FILTER_GRID_OK);
  CHECK(old_loop_ends(dim, n, x.data(), r, 100000));       // finite input never needed the check
  CHECK(G.h >= r);
  CHECK(ncell >= 1 && ncell <= 4 * n + 1024);
  CHECK(G.n[0] * G.n[1] * G.n[2] == ncell);
  for (int k = 0; k < 3; ++k) CHECK(G.n[k] >= 1);
  for (int k = dim; k < 3; ++k) CHECK(G.n[k] == 1);
  std::vector<int64_t> cell((size_t)(n * dim));
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < dim; ++k) {
      const double p = x[(size_t)(i * dim + k)];
      const double q = std::floor((p - G.lo[k]) / G.h);
      CHECK(q >= 0.0 && q < (double)G.n[k]);               // inside the box nothing is clamped
      const int64_t c = filter_grid_index(G, k, p);
      CHECK(c >= 0 && c < G.n[k]);
      CHECK((double)c == std::min(std::max(q, 0.0), (double)(G.n[k] - 1)));
      cell[(size_t)(i * dim + k)] = c;
    }
  int64_t far = 0;
  for (int64_t i = 0; i < n; ++i)
    for (int64_t j = i + 1; j < n; ++j) {
      double s = 0.0;                                      // the kernels' distance (dist_sym)
      for (int k = 0; k < dim; ++k) { const double t = x[(size_t)(i * dim + k)] - x[(size_t)(j * dim + k)]; s += t * t; }
      if (std::sqrt(s) > r) continue;
      for (int k = 0; k < dim; ++k)
        if (std::llabs((long long)(cell[(size_t)(i * dim + k)] - cell[(size_t)(j * dim + k)])) > 1) ++far;
    }
  CHECK(far == 0);
  if (failures != before) std::printf("  in case %s (n = %lld, h = %g, ncell = %lld)\n", name, (long long)n, G.h, (long long)ncell);
  if (ncell_out) *ncell_out = ncell;
  return G;
}

static void check_refused(const char* name, int dim, const std::vector<double>& x, double r, bool old_spins) {
  const int64_t n = (int64_t)x.size() / dim;
  FilterGrid G{};
  int64_t ncell = -1;
  const int before = failures;
  CHECK(filter_grid_plan(dim, n, x.data(), r, &G, &ncell) == FILTER_GRID_NONFINITE);
  // what the loop did without the check: 100000 growth steps take h from any double past DBL_MAX, so a loop that has not
  // ended by then never ends
  CHECK(old_loop_ends(dim, n, x.data(), r, 100000) == !old_spins);
  if (failures != before) std::printf("  in case %s\n", name);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

  // ---- non-finite input ----
  {
    std::vector<double> x = cloud(2, 50, 1.0);
    std::vector<double> a = x; a[0] = nan;
    check_refused("NaN first", 2, a, 0.1, true);
    a = x; a[1] = nan;
    check_refused("NaN first point, second direction", 2, a, 0.1, true);
    a = x; a[51] = nan;                                    // std::min / std::max skip it: the old loop ended, and the
    check_refused("NaN inside", 2, a, 0.1, false);         // device then gave that point an empty row
    a = x; a[37] = inf;
    check_refused("+inf", 2, a, 0.1, true);
    a = x; a[64] = -inf;
    check_refused("-inf", 2, a, 0.1, true);
    std::vector<double> y = cloud(3, 40, 1.0);
    y[3 * 39 + 2] = nan;
    check_refused("NaN last, 3-D", 3, y, 0.2, false);
    y[3 * 39 + 2] = inf;
    check_refused("+inf last, 3-D", 3, y, 0.2, true);
    std::vector<double> one = {nan, 0.0};
    check_refused("n = 1, NaN", 2, one, 1.0, true);
    std::vector<double> wide = {-1.5e308, 0.0, 1.5e308, 1.0};   // finite points, but hi - lo is not
    check_refused("extent overflows", 2, wide, 1.0, true);
  }

  // ---- degenerate geometry ----
  {
    int64_t nc = 0;
    std::vector<double> one2 = {0.3, -0.7}, one3 = {1e6, -2e6, 3.0};
    FilterGrid G = check_plan("n = 1 (2-D)", 2, one2, 0.5, &nc);
    CHECK(nc == 1 && G.h == 0.5);
    check_plan("n = 1 (3-D)", 3, one3, 1e-3, &nc);
    CHECK(nc == 1);
    std::vector<double> same(3 * 7);
    for (int i = 0; i < 7; ++i) { same[3 * i] = 0.25; same[3 * i + 1] = -4.0; same[3 * i + 2] = 1e6; }
    check_plan("zero extent in all directions", 3, same, 0.1, &nc);
    CHECK(nc == 1);
    std::vector<double> col = cloud(2, 500, 1.0);
    for (int i = 0; i < 500; ++i) col[2 * i + 1] = 0.375;
    G = check_plan("collinear", 2, col, 0.01, &nc);
    CHECK(G.n[1] == 1 && G.n[0] > 1);
    std::vector<double> pl = cloud(3, 500, 1.0);
    for (int i = 0; i < 500; ++i) pl[3 * i + 2] = -0.625;
    G = check_plan("coplanar", 3, pl, 0.05, &nc);
    CHECK(G.n[2] == 1 && G.n[0] > 1 && G.n[1] > 1);
  }

  // ---- extreme radii on a unit box ----
  {
    int64_t nc = 0;
    std::vector<double> x = cloud(2, 100, 1.0);
    x[0] = 0.0; x[1] = 0.0; x[2] = 1.0; x[3] = 1.0;
    FilterGrid G = check_plan("r = 1e-300", 2, x, 1e-300, &nc);
    CHECK(G.h > 1e-300 && nc > 1);                         // some three thousand growth steps, and it ends
    G = check_plan("r = 1e300", 2, x, 1e300, &nc);
    CHECK(nc == 1 && G.h == 1e300);
    std::vector<double> y = cloud(3, 100, 1.0);
    check_plan("r = 1e-300 (3-D)", 3, y, 1e-300, &nc);
    check_plan("r = 1e300 (3-D)", 3, y, 1e300, &nc);
    CHECK(nc == 1);
  }

  // ---- the shapes of tests/test_gpu_filter_edges.py, at their sizes ----
  {
    int64_t nc = 0;
    FilterGrid G = check_plan("cells2d", 2, cloud(2, 2000, 1.0), 0.02, &nc);
    CHECK(G.h == 0.02 && nc > 2048);                       // no growth; more than two scan chunks of cells
    G = check_plan("cells3d", 3, cloud(3, 1500, 1.0), 0.08, &nc);
    CHECK(G.h == 0.08 && nc > 1024);
    std::vector<double> cap = cloud(2, 300, 1.0);
    for (int i = 0; i < 20; ++i) { cap.push_back(cap[(size_t)(2 * i)] + 3e-4); cap.push_back(cap[(size_t)(2 * i + 1)]); }
    G = check_plan("capped", 2, cap, 1e-3, &nc);
    CHECK(G.h > 1e-3);                                     // the growth loop ran
    G = check_plan("onecell", 3, cloud(3, 300, 1.0), 2.0, &nc);
    CHECK(nc == 1);
    const double shift[2] = {1e6, -2e6};
    G = check_plan("shifted", 2, cloud(2, 600, 3.0, shift), 0.3, &nc);
    CHECK(G.lo[0] >= 1e6 && G.lo[1] >= -2e6 && G.lo[1] < -2e6 + 3.0);
    const int64_t sizes[] = {1, 2, 255, 256, 257, 1023, 1024, 1025};
    for (int64_t n : sizes) {
      std::vector<double> x = cloud(2, n, 1.0);
      if (n == 2) { x[2] = x[0]; x[3] = x[1]; }            // the same point twice
      check_plan("sizes", 2, x, std::sqrt(10.0 / (3.14159265358979 * (double)n)), &nc);
    }
    std::vector<double> lat;
    for (int i = 0; i < 12; ++i)
      for (int j = 0; j < 9; ++j) { lat.push_back(i * 0.1); lat.push_back(j * 0.1); }
    G = check_plan("lattice", 2, lat, 0.2, &nc);
    CHECK(G.h == 0.2);
  }

  if (failures) return 1;
  std::printf("filter_grid: ok\n");
  return 0;
}
