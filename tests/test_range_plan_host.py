"""The plan of the streamed ranges (femo_amd/csrc/range_plan.h) through femo_range_plan_host of the test header -- what the
chunked upload of f and the streamed tail cut their arrays by -- and the same function in a stand-alone C++ program built
with -fsanitize=address,undefined and run as a child process.  Host code only: nothing here touches a GPU.

Properties, for every size, chunk and taper setting below: the ranges tile [0, n) once and in order; every end but the last
is a multiple of 256; there are at most 1024; chunk = 0 gives one range; without a taper (mode 0, a floor of at least the
chunk, a factor below 2, an array of at most one chunk) the plan is the equal pieces the library cut before; with one, the
upload's last range and the download's first are at most the floor, the sizes inside the taper are monotone, and no range
is longer than the chunk (upload) or one and a half times the cap (download)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, HEAD, TAIL = 0, 1, 2
MIB = 131072                          # entries of 8 bytes
SIZES = (0, 1, 255, 256, 257, MIB - 1, MIB, MIB + 1, 1053696, 1053695)
# (chunk, floor, factor, cap): every taper setting the library can be given -- its defaults in entries (64 MiB, 8 MiB, 4,
# 128 MiB), the settings of the GPU tests (1 MiB chunks tapering to 1/8 MiB), a floor at and above the chunk, factors that
# switch the taper off, a cap below the chunk
SETTINGS = [(MIB, MIB // 8, 2, MIB), (MIB, MIB // 8, 2, 4 * MIB), (MIB, MIB // 8, 4, 2 * MIB), (MIB, MIB // 16, 3, MIB),
            (64 * MIB, 8 * MIB, 4, 128 * MIB), (MIB, MIB, 2, MIB), (MIB, 8 * MIB, 4, 128 * MIB), (MIB, MIB // 8, 1, MIB),
            (MIB, MIB // 8, 0, MIB), (MIB, 0, 2, 0), (256, 256, 2, 256), (1, 1, 2, 1), (0, MIB // 8, 2, MIB)]


def plan(n, chunk, taper, floor, factor, cap):
    from femo_amd import _lib
    lib = _lib.load()
    count = lib.femo_range_plan_host(n, chunk, taper, floor, factor, cap, None, 0)
    buf = (C.c_int64 * (2 * max(count, 1)))()
    assert lib.femo_range_plan_host(n, chunk, taper, floor, factor, cap, buf, 2 * count) == count
    return [(int(buf[2 * k]), int(buf[2 * k + 1])) for k in range(count)]


def equal_pieces(n, chunk):
    if n <= 0:
        return []
    if chunk <= 0:
        return [(0, n)]
    chunk = max(chunk // 256 * 256, 256, ((n + 1023) // 1024 + 255) // 256 * 256)
    return [(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)]


@pytest.mark.parametrize("taper", [NONE, HEAD, TAIL])
@pytest.mark.parametrize("setting", SETTINGS)
def test_plan_properties(taper, setting):
    chunk, floor, factor, cap = setting
    for n in SIZES:
        p = plan(n, chunk, taper, floor, factor, cap)
        what = f"n {n} chunk {chunk} taper {taper} floor {floor} factor {factor} cap {cap}: {p[:4]} ... {p[-3:]}"
        if n == 0:
            assert p == [], what
            continue
        assert 1 <= len(p) <= 1024, what
        assert p[0][0] == 0 and p[-1][1] == n and all(a[1] == b[0] for a, b in zip(p, p[1:])), what
        assert all(b > a for a, b in p) and all(b % 256 == 0 for _, b in p[:-1]), what
        if chunk == 0:
            assert len(p) == 1, what
            continue
        # the chunk in effect: a multiple of 256, and large enough for 1024 equal pieces to cover the array
        c, fl = max(chunk // 256 * 256, 256, ((n + 1023) // 1024 + 255) // 256 * 256), max(floor // 256 * 256, 512)
        if taper == NONE or fl >= c or factor < 2 or n <= c:
            assert p == equal_pieces(n, chunk), what
            continue
        size = [b - a for a, b in p]
        if taper == HEAD:
            assert size[-1] <= fl and max(size) <= c + c // 2, what
            inner = size[1:]                              # what remains comes first; behind it the sizes only fall
            assert all(x >= y for x, y in zip(inner, inner[1:])), what
            # (the last piece is the floor less up to 255 entries: it carries the entries beyond the last multiple of 256)
            assert all(x == c or x <= max(y, fl) * factor for x, y in zip(inner, inner[1:])), what
        else:
            top = max(cap // 256 * 256, c)
            assert size[0] <= fl and max(size) <= top + top // 2, what
            inner = size[:-1]                             # what remains comes last; before it the sizes only rise
            assert all(x <= y for x, y in zip(inner, inner[1:])), what
            assert all(y == top or y <= x * factor for x, y in zip(inner, inner[1:])), what


def test_the_named_plans():
    """One chunk and one entry either side of it, and the n = 56 cube's cells in 1 MiB chunks: the counts the GPU tests see."""
    assert plan(MIB, MIB, HEAD, MIB // 8, 2, 0) == [(0, MIB)] and plan(MIB - 1, MIB, TAIL, MIB // 8, 2, MIB) == [(0, MIB - 1)]
    head = plan(MIB + 1, MIB, HEAD, MIB // 8, 2, 0)
    assert head[-1] == (MIB + 1 - (MIB // 8 - 255), MIB + 1) and head[-1][1] - head[-1][0] <= MIB // 8
    tail = plan(MIB + 1, MIB, TAIL, MIB // 8, 2, MIB)
    assert tail[0] == (0, MIB // 8) and tail[-1][1] == MIB + 1
    n = 1053696
    assert len(plan(n, MIB, NONE, 0, 0, 0)) == 9 and len(plan(n, MIB, HEAD, 8 * MIB, 4, 0)) == 9      # the library's default floor
    head, tail = plan(n, MIB, HEAD, MIB // 8, 2, 0), plan(n, MIB, TAIL, MIB // 8, 2, 2 * MIB)
    assert [b - a for a, b in head][-4:] == [MIB, MIB // 2, MIB // 4, MIB // 8]
    assert [b - a for a, b in tail][:5] == [MIB // 8, MIB // 4, MIB // 2, MIB, 2 * MIB]
    assert len(head) > 9 > len(tail)
    # the headline's 59,627,250 cells with the defaults: eight pieces up as before, five ranges down
    n = 59627250
    assert [round((b - a) / MIB) for a, b in plan(n, 64 * MIB, HEAD, 8 * MIB, 4, 0)] == [95, 64, 64, 64, 64, 64, 32, 8]
    assert [round((b - a) / MIB) for a, b in plan(n, 64 * MIB, TAIL, 8 * MIB, 4, 128 * MIB)] == [8, 32, 128, 128, 159]


def _compiler():
    """A compiler and the flags that link the sanitizer runtimes statically (the program then needs nothing preloaded)."""
    for c, static in (("/opt/rocm/lib/llvm/bin/clang++", []), ("clang++", []),
                      ("g++", ["-static-libasan", "-static-libubsan"]), ("c++", ["-static-libasan", "-static-libubsan"])):
        if shutil.which(c):
            return [shutil.which(c)] + static
    raise RuntimeError("no C++ compiler found")


def test_range_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "range_plan_main")
    cmd = _compiler() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "femo_amd", "csrc"),
                         os.path.join(ROOT, "tests", "native", "range_plan_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "range_plan: ok" in run.stdout
