// The range plan of the streamed head and tail (femo_amd/csrc/range_plan.h) in a program of its own: every combination of
// size, chunk and taper the Python test walks, plus sizes near 2^31 and 2^40 entries and INT64_MAX (one range: beyond what 1024 chunks cover) and factors that overflow if multiplied
// carelessly.  Built with -fsanitize=address,undefined and run by tests/test_range_plan_host.py; exits 0 when every plan holds.
#include <cstdio>
#include <cstdlib>

#include "range_plan.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void check_plan(int64_t n, int64_t chunk, int taper, int64_t floor, int64_t factor, int64_t cap) {
  const auto p = femo_range_plan(n, chunk, taper, floor, factor, cap);
  const char* fmt = "n %lld chunk %lld taper %d floor %lld factor %lld cap %lld";
#define ARGS (long long)n, (long long)chunk, taper, (long long)floor, (long long)factor, (long long)cap
  if (n <= 0) { CHECK(p.empty(), fmt, ARGS); return; }
  CHECK(!p.empty() && (int)p.size() <= FEMO_MAX_RANGES, fmt, ARGS);
  if (p.empty()) return;
  if (chunk <= 0) CHECK(p.size() == 1, fmt, ARGS);
  int64_t pos = 0;
  for (size_t k = 0; k < p.size(); ++k) {
    CHECK(p[k].first == pos && p[k].second > pos, fmt, ARGS);
    pos = p[k].second;
    if (k + 1 < p.size()) CHECK(pos % FEMO_RANGE_ALIGN == 0, fmt, ARGS);
  }
  CHECK(pos == n, fmt, ARGS);
  const int64_t fl = std::max<int64_t>(floor / 256 * 256, 512);
  const bool tapered = n <= (int64_t(1) << 61) && chunk > 0 && taper != FEMO_TAPER_NONE && factor >= 2 && n > std::max<int64_t>(chunk / 256 * 256, 256) && fl < chunk / 256 * 256;
  if (tapered && (int)p.size() < FEMO_MAX_RANGES / 2) {  // (a doubled chunk may have switched the taper off)
    if (taper == FEMO_TAPER_HEAD) CHECK(p.back().second - p.back().first <= fl, fmt, ARGS);
    if (taper == FEMO_TAPER_TAIL) CHECK(p.front().second - p.front().first <= fl, fmt, ARGS);
  }
#undef ARGS
}

int main() {
  const int64_t mib = 131072;
  const int64_t sizes[] = {0, 1, 255, 256, 257, 511, 512, 513, mib - 1, mib, mib + 1, 1053696, 1053695, 59627250,
                           (int64_t(1) << 31) - 1, (int64_t(1) << 31) + 257, (int64_t(1) << 40) + 3, INT64_MAX};
  const int64_t chunks[] = {0, 1, 256, 257, 4096, mib, 8 * mib, 64 * mib, int64_t(1) << 45, INT64_MAX};
  const int64_t floors[] = {0, 1, 256, 512, 1000, mib / 8, mib, 8 * mib, INT64_MAX / 2, INT64_MAX};
  const int64_t factors[] = {0, 1, 2, 3, 4, 1000, INT64_MAX};
  const int64_t caps[] = {0, mib, 128 * mib, INT64_MAX};
  long plans = 0;
  for (int64_t n : sizes)
    for (int64_t c : chunks)
      for (int taper = -1; taper <= 3; ++taper)
        for (int64_t fl : floors)
          for (int64_t fa : factors)
            for (int64_t cap : caps) { check_plan(n, c, taper, fl, fa, cap); ++plans; }
  check_plan(-5, mib, FEMO_TAPER_HEAD, 512, 2, 0);
  if (failures) { std::printf("range_plan: %d failure(s)\n", failures); return 1; }
  std::printf("range_plan: ok (%ld plans)\n", plans);
  return 0;
}
