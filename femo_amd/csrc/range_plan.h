// Ranges of a streamed transfer: the pieces of the chunked upload of f (hostmem.cpp, femo_vec_set_host_deferred) and the
// ranges of the streamed tail (femo_dRdf_cell_apply_T_add_to_host).  Host code only, no HIP: the library, the test entry
// point femo_range_plan_host and the stand-alone sanitizer program (tests/native/range_plan_main.cpp) include this one function.
//
// What runs behind an upload waits for its last piece, and a download's first byte for its first range: the kernels of a
// range that another piece follows run under that piece, only those of the LAST range stand behind the upload's last byte,
// and the first byte of a download leaves when the FIRST range's kernel is done.  So the upload's pieces shrink towards its
// end and the download's grow from its start, by `factor` per piece, down to / up from `floor` entries; elsewhere they have
// `chunk` entries (the download's grow on to `cap`: every copy costs the engine a gap).
#ifndef FEMO_RANGE_PLAN_H
#define FEMO_RANGE_PLAN_H

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

enum { FEMO_TAPER_NONE = 0, FEMO_TAPER_HEAD = 1, FEMO_TAPER_TAIL = 2 };
constexpr int FEMO_MAX_RANGES = 1024;
constexpr int64_t FEMO_RANGE_ALIGN = 256;

// (begin, end) of the ranges of [0, n), in order.  Every end but the last is a multiple of 256 entries; at most 1024 ranges
// (chunk is doubled until that holds).  n <= 0: no range.  chunk <= 0: one range.
//   FEMO_TAPER_NONE  pieces of `chunk` entries, the last one what remains.
//   FEMO_TAPER_TAIL  floor, factor * floor, factor^2 * floor, ... up to max(cap, chunk) and so on; what remains is the last
//                    piece, or part of it when it is at most half of a piece.
//   FEMO_TAPER_HEAD  the mirror image with cap = chunk: what remains comes first, the last piece is at most `floor`.
// floor >= chunk, factor < 2 and n <= chunk (one copy, as for any transfer of at most one chunk) leave FEMO_TAPER_NONE's plan.
inline std::vector<std::pair<int64_t, int64_t>> femo_range_plan(int64_t n, int64_t chunk, int taper, int64_t floor, int64_t factor,
                                                                int64_t cap) {
  std::vector<std::pair<int64_t, int64_t>> out;
  if (n <= 0) return out;
  if (chunk <= 0) { out.emplace_back(0, n); return out; }
  const int64_t big = INT64_MAX / 4096;                  // (sizes are multiplied by a factor of at most 1024)
  auto align = [&](int64_t v) { return std::max(FEMO_RANGE_ALIGN, std::min(v, big) / FEMO_RANGE_ALIGN * FEMO_RANGE_ALIGN); };
  chunk = std::max(align(chunk), align(n / FEMO_MAX_RANGES + (n % FEMO_MAX_RANGES != 0) + FEMO_RANGE_ALIGN - 1));
  factor = std::min<int64_t>(factor, 1024);
  if (taper != FEMO_TAPER_HEAD && taper != FEMO_TAPER_TAIL) taper = FEMO_TAPER_NONE;
  if (floor < 2 * FEMO_RANGE_ALIGN) floor = 2 * FEMO_RANGE_ALIGN;        // (room for the odd entries of the head's last piece)
  floor = align(floor);
  if (floor >= chunk || factor < 2 || n <= chunk) taper = FEMO_TAPER_NONE;
  // A plan of more than 1024 ranges doubles the chunk.  64 doublings reach every chunk `align` lets through; an array that
  // 1024 such chunks cannot cover (beyond 2^61 entries) is one range.
  for (int attempt = 0; attempt < 64; ++attempt, chunk = align(chunk * 2)) {
    std::vector<int64_t> len;                            // ascending: the tail's order
    if (taper == FEMO_TAPER_NONE) {
      for (int64_t rem = n; rem > 0; rem -= len.back()) len.push_back(std::min(chunk, rem));
    } else {
      const int64_t top = taper == FEMO_TAPER_TAIL ? std::max(align(cap), chunk) : chunk;
      // the head's last piece carries the entries beyond the last multiple of 256 and still is at most `floor`
      const int64_t odd = n % FEMO_RANGE_ALIGN;
      int64_t size = floor, rem = n;
      int64_t want = taper == FEMO_TAPER_HEAD && odd != 0 ? floor - FEMO_RANGE_ALIGN + odd : floor;
      while (rem > 0) {
        const int64_t take = (!len.empty() && rem <= want + want / 2) ? rem : std::min(want, rem);
        len.push_back(take);
        rem -= take;
        size = std::min(top, align(std::min(size, big) * factor));
        want = size;
      }
    }
    if ((int64_t)len.size() > FEMO_MAX_RANGES) continue;
    if (taper == FEMO_TAPER_HEAD) std::reverse(len.begin(), len.end());
    int64_t pos = 0;
    for (int64_t l : len) { out.emplace_back(pos, pos + l); pos += l; }
    return out;
  }
  out.emplace_back(0, n);
  return out;
}

#endif
