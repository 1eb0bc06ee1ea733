// Host half of the density filter's build plan (femo_filter_create, elasticity.hip): the bounding box of the points, the
// cell size of the uniform grid and the cell counts.  Plain C++, no HIP: elasticity.hip includes it, and
// tests/native/filter_grid_main.cpp checks it alone under the host sanitizers.
//
// The grid has cubic cells of size h >= r, so the 3^d cells around a point's own cell hold every neighbour within r, and
// at most 4 n + 1024 cells: h starts at r and grows by a quarter until the count fits (scattered points with a tiny
// radius would otherwise ask for an unbounded grid).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

struct FilterGrid {
  double lo[3];
  double h;
  int64_t n[3];
};

enum { FILTER_GRID_OK = 0, FILTER_GRID_NONFINITE = 1 };

// Fills G and ncell for n > 0 points of dimension dim (2 or 3) and a finite radius > 0.  FILTER_GRID_NONFINITE if a
// coordinate is NaN or +-inf, or if the box is so large that its extent is not a finite double: std::min / std::max skip
// a NaN (or keep one met first), and with a non-finite extent the cell count below is never small enough -- the loop would
// not end.
inline int filter_grid_plan(int dim, int64_t n, const double* coords, double radius, FilterGrid* G, int64_t* ncell) {
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int k = 0; k < dim; ++k) { lo[k] = coords[k]; hi[k] = coords[k]; }
  bool finite = true;
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < dim; ++k) {
      const double c = coords[i * dim + k];
      finite = finite && std::isfinite(c);
      lo[k] = std::min(lo[k], c);
      hi[k] = std::max(hi[k], c);
    }
  for (int k = 0; k < dim; ++k) finite = finite && std::isfinite(hi[k] - lo[k]);
  if (!finite) return FILTER_GRID_NONFINITE;
  double h = radius;
  for (;;) {
    double cells = 1.0;
    for (int k = 0; k < dim; ++k) cells *= std::floor((hi[k] - lo[k]) / h) + 1.0;
    if (cells <= 4.0 * (double)n + 1024.0) break;
    h *= 1.25;
  }
  G->h = h;
  int64_t nc = 1;
  for (int k = 0; k < 3; ++k) {
    G->lo[k] = lo[k];
    G->n[k] = k < dim ? (int64_t)std::floor((hi[k] - lo[k]) / h) + 1 : 1;
    nc *= G->n[k];
  }
  *ncell = nc;
  return FILTER_GRID_OK;
}

// Cell index of coordinate p in direction k: the formula of the kernels' grid_cell (elasticity.hip), stated once more for
// the host so that the stand-alone check can compare the two.
inline int64_t filter_grid_index(const FilterGrid& G, int k, double p) {
  int64_t q = (int64_t)std::floor((p - G.lo[k]) / G.h);
  return q < 0 ? 0 : (q >= G.n[k] ? G.n[k] - 1 : q);
}
