// Stand-alone check of the host half of the streamed head (femo_amd/csrc/head_order.h): the running maximum of the row
// blocks' last cells and B(e), the number of row blocks complete once cells [0, e) are known.  Built with
// -fsanitize=address,undefined and run by tests/test_head_order_native.py; exits 0 when every case holds.
#include <cstdio>
#include <cstdlib>

#include "head_order.h"

static int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// B(e) by its definition, for comparison
static int64_t brute(const std::vector<int32_t>& mc, int64_t e) {
  int64_t n = 0, run = -1;
  for (size_t b = 0; b < mc.size(); ++b) {
    run = std::max<int64_t>(run, mc[b]);
    if (run < e) ++n;
  }
  return n;
}

int main() {
  std::vector<int64_t> ready;
  {  // empty mesh: no row blocks, whatever e
    femo_head_running_max(nullptr, 0, ready);
    CHECK(ready.empty());
    CHECK(femo_head_blocks_ready(ready, 0) == 0);
    CHECK(femo_head_blocks_ready(ready, 1000) == 0);
    CHECK(femo_head_blocks_ready(ready, -5) == 0);
  }
  {  // a single block that needs cells up to 41
    const int32_t mc[1] = {41};
    femo_head_running_max(mc, 1, ready);
    CHECK(ready.size() == 1 && ready[0] == 41);
    CHECK(femo_head_blocks_ready(ready, 0) == 0);
    CHECK(femo_head_blocks_ready(ready, 41) == 0);      // cell 41 itself is not among [0, 41)
    CHECK(femo_head_blocks_ready(ready, 42) == 1);
    CHECK(femo_head_blocks_ready(ready, INT64_MAX) == 1);
  }
  {  // a block without visits is ready at once; behind a block that is not, it waits with it (prefix property)
    const int32_t mc[3] = {-1, 7, -1};
    femo_head_running_max(mc, 3, ready);
    CHECK(ready[0] == -1 && ready[1] == 7 && ready[2] == 7);
    CHECK(femo_head_blocks_ready(ready, 0) == 1);
    CHECK(femo_head_blocks_ready(ready, 7) == 1);
    CHECK(femo_head_blocks_ready(ready, 8) == 3);
  }
  {  // non-monotone order: the running maximum makes the ready set a prefix
    const std::vector<int32_t> mc = {5, 3, 9, 2, 9, 30, 11, 29, 31, 0};
    femo_head_running_max(mc.data(), (int64_t)mc.size(), ready);
    for (size_t b = 1; b < ready.size(); ++b) CHECK(ready[b - 1] <= ready[b]);
    const int64_t ends[] = {-1, 0, 1, 3, 5, 6, 9, 10, 29, 30, 31, 32, 33, 1 << 20};   // at and beyond both ends
    int64_t prev = 0;
    for (int64_t e : ends) {
      const int64_t B = femo_head_blocks_ready(ready, e);
      CHECK(B == brute(mc, e));
      CHECK(B >= prev && B <= (int64_t)mc.size());
      for (int64_t b = 0; b < B; ++b) CHECK(mc[(size_t)b] < e);   // every ready block has all its cells
      prev = B;
    }
    CHECK(femo_head_blocks_ready(ready, 31) == 8);
    CHECK(femo_head_blocks_ready(ready, 32) == 10);
  }
  {  // a random numbering: the first block already needs (nearly) the last cell, nothing is ready before the end
    std::vector<int32_t> mc(64);
    uint32_t s = 12345u;
    for (auto& v : mc) { s = s * 1664525u + 1013904223u; v = 900 + (int32_t)(s >> 24) % 100; }
    mc[0] = 999;
    femo_head_running_max(mc.data(), 64, ready);
    CHECK(femo_head_blocks_ready(ready, 999) == 0);
    CHECK(femo_head_blocks_ready(ready, 1000) == 64);
  }
  if (failures) return 1;
  std::printf("head_order: ok\n");
  return 0;
}
