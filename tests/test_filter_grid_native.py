"""Host half of the density filter's build plan (femo_amd/csrc/filter_grid.h: bounding box, cell-size loop, cell counts) in a
stand-alone C++ program of its own, built with -fsanitize=address,undefined and run as a child process: non-finite
coordinates (refused; the loop as it stood before does not end on them), a single point, zero extent, extreme radii, and
the shapes of tests/test_gpu_filter_edges.py.  Host code only -- nothing here touches a GPU or loads into the interpreter."""
import os
import subprocess

from test_head_order_native import ROOT, _compiler


def test_filter_grid_under_sanitizers(tmp_path):
    exe = str(tmp_path / "filter_grid_main")
    cmd = _compiler() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "femo_amd", "csrc"),
                         os.path.join(ROOT, "tests", "native", "filter_grid_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "filter_grid: ok" in run.stdout
