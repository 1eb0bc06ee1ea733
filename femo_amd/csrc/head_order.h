// Row blocks ordered by the last cell they need: the host half of the streamed head (assemble.hip).  Plain C++ with no
// HIP in it, so that a stand-alone program can run it under a sanitizer (tests/native/head_order_main.cpp).
#ifndef FEMO_HEAD_ORDER_H
#define FEMO_HEAD_ORDER_H

#include <algorithm>
#include <cstdint>
#include <vector>

// ready[b] = max over b' <= b of block_maxcell[b'], where block_maxcell[b] is the largest cell id row block b visits
// (-1: it visits none).  Nondecreasing by construction, whatever the numbering.
inline void femo_head_running_max(const int32_t* block_maxcell, int64_t n_blocks, std::vector<int64_t>& ready) {
  ready.assign((size_t)std::max<int64_t>(n_blocks, 0), -1);
  int64_t run = -1;
  for (int64_t b = 0; b < n_blocks; ++b) {
    run = std::max<int64_t>(run, block_maxcell[b]);
    ready[(size_t)b] = run;
  }
}

// B(e) = #{b : ready[b] < e}: once cells [0, e) are known, row blocks [0, B(e)) -- always a prefix -- have all their cells.
// A lexicographic or Morton numbering lets B grow with e; a random one keeps it near 0 until e reaches the last cell.
inline int64_t femo_head_blocks_ready(const std::vector<int64_t>& ready, int64_t e) {
  return (int64_t)(std::lower_bound(ready.begin(), ready.end(), e) - ready.begin());
}

#endif
