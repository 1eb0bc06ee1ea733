"""The dense solve of the MMA subproblem's Newton system (femo_amd/csrc/small_solve.h: Gaussian elimination with partial
pivoting, at most 9 unknowns) in a stand-alone C++ program of its own, built with -fsanitize=address,undefined and run as a
child process, against numpy.linalg.solve: random systems, nearly singular ones, systems that need the row exchange, exactly
singular ones (refused) and sizes out of range (refused).  Host code only -- nothing here touches a GPU or loads into the
interpreter."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(float).eps


def _compiler():
    """A compiler and the flags that link the sanitizer runtimes statically (the program then needs nothing preloaded)."""
    for c, static in (("/opt/rocm/lib/llvm/bin/clang++", []), ("clang++", []),
                      ("g++", ["-static-libasan", "-static-libubsan"]), ("c++", ["-static-libasan", "-static-libubsan"])):
        if shutil.which(c):
            return [shutil.which(c)] + static
    raise RuntimeError("no C++ compiler found")


def _systems():
    rng = np.random.default_rng(42)
    out = []
    for n in range(1, 10):
        for _ in range(4):                                  # random, well conditioned
            out.append((rng.standard_normal((n, n)) + n * np.eye(n), rng.standard_normal(n)))
        # nearly singular: singular values from 1 down to 1e-10
        u, _ = np.linalg.qr(rng.standard_normal((n, n)))
        v, _ = np.linalg.qr(rng.standard_normal((n, n)))
        out.append((u @ np.diag(np.logspace(0, -10, n)) @ v.T, rng.standard_normal(n)))
        # a zero in the first pivot position: only the row exchange gets past it
        A = rng.standard_normal((n, n)) + n * np.eye(n)
        if n > 1:
            A[0, 0] = 0.0
        out.append((A, rng.standard_normal(n)))
        # the shape the Newton system has: diagonal + G D G^T with a wide spread of D
        G = rng.standard_normal((n, 50))
        out.append((np.diag(rng.uniform(1e-8, 1.0, n)) + (G * np.logspace(-6, 3, 50)) @ G.T, rng.standard_normal(n)))
    return out


def test_small_solve_under_sanitizers(tmp_path):
    exe = str(tmp_path / "small_solve_main")
    cmd = _compiler() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "femo_amd", "csrc"),
                         os.path.join(ROOT, "tests", "native", "small_solve_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    good = _systems()
    singular = [(np.zeros((1, 1)), np.ones(1)), (np.ones((3, 3)), np.ones(3)),
                (np.array([[1.0, 2.0], [2.0, 4.0]]), np.ones(2)), (np.array([[np.nan]]), np.ones(1))]
    lines = [str(len(good) + len(singular) + 3)]
    for A, b in good + singular:
        lines.append(f"{A.shape[0]} " + " ".join(repr(float(v)) for v in A.ravel()) + " " + " ".join(repr(float(v)) for v in b))
    lines += ["0", "10", "-1"]                               # an empty system is fine; sizes out of range are refused
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = run.stdout.strip().split("\n")
    assert rows[-1] == "small_solve: done" and len(rows) == len(good) + len(singular) + 4
    for (A, b), row in zip(good, rows):
        f = row.split()
        assert f[0] == "0", (A, row)
        x = np.array([float(v) for v in f[1:]])
        ref = np.linalg.solve(A, b)
        # backward stable: the error is bounded by the condition number times a modest multiple of eps
        bound = 64 * A.shape[0] * EPS * np.linalg.cond(A) * np.abs(ref).max()
        assert np.abs(x - ref).max() <= bound, (A.shape[0], np.abs(x - ref).max(), bound)
        assert np.abs(A @ x - b).max() <= 64 * A.shape[0] * EPS * (np.abs(A).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max())
    for row in rows[len(good):len(good) + len(singular)]:
        assert row.split()[0] == "1", row
    assert rows[-4].split()[0] == "0" and rows[-3] == "1" and rows[-2] == "1"
