"""Host half of the streamed head (femo_amd/csrc/head_order.h: running maximum of the row blocks' last cells, and the
number of row blocks complete after a chunk of f) in a stand-alone C++ program of its own, built with
-fsanitize=address,undefined and run as a child process: an empty mesh, a single block, a non-monotone order, chunk ends at
and beyond both ends.  Host code only -- nothing here touches a GPU or loads into the interpreter."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    """A compiler and the flags that link the sanitizer runtimes statically (the program then needs nothing preloaded)."""
    for c, static in (("/opt/rocm/lib/llvm/bin/clang++", []), ("clang++", []),
                      ("g++", ["-static-libasan", "-static-libubsan"]), ("c++", ["-static-libasan", "-static-libubsan"])):
        if shutil.which(c):
            return [shutil.which(c)] + static
    raise RuntimeError("no C++ compiler found")


def test_head_order_under_sanitizers(tmp_path):
    exe = str(tmp_path / "head_order_main")
    cmd = _compiler() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "femo_amd", "csrc"),
                         os.path.join(ROOT, "tests", "native", "head_order_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "head_order: ok" in run.stdout
