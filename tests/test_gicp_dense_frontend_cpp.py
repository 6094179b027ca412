"""GeneralizedICP::Compute(pF1, pF2, guess) of the C++ mirror
(include/odo_frontend.hpp, standing in for Odometry/generalizedicp.cpp:41-53):
the program tests/cpp/gicp_dense_mirror.cpp, compiled here against the header
and the library, against Odometry.gicp_dense on the same two frames."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, load_pkg, sequence

INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "gicp_dense_mirror.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]


def test_mirror_compiles_with_warnings_as_errors():
    subprocess.run(["g++", *FLAGS, "-fsyntax-only", "-I", INC, SRC], check=True)


@pytest.mark.gpu
def test_mirror_equals_the_binding(tmp_path):
    bgr, dep, _ = sequence(2, seed=0x5EED0034)
    bgr, dep = np.ascontiguousarray(bgr), np.ascontiguousarray(dep)
    frames = tmp_path / "f.bin"
    with open(frames, "wb") as f:
        f.write(bgr.tobytes())
        f.write(dep.tobytes())
    exe = tmp_path / "gicp_dense_mirror"
    subprocess.run(["g++", "-O1", *FLAGS, "-o", str(exe), SRC, "-I", INC, "-L", PKG_DIR, "-lodo_hip",
                    f"-Wl,-rpath,{PKG_DIR}"], check=True)
    r = subprocess.run([str(exe), str(frames), "640", "480", "0.03", "3", "0.05"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0] == ["empty", "0"] and lines[1][0] == "gicp" and len(lines[1]) == 18
    pkg = load_pkg()
    odo = pkg.Odometry(pkg.default_config(640, 480, 2))  # the mirror's own context: default calibration
    try:
        info = odo.dense_clouds_host(bgr, dep, 0.03)
        assert info["n_points"].min() > 1000
        T, conv, it, nc = odo.gicp_dense([(0, 1)], None, 3, 0.05)[0]
        assert int(lines[1][1]) == conv == 1 and nc > 1000
        assert [int(v, 16) for v in lines[1][2:]] == [int(v) for v in T.reshape(-1).view(np.uint32)]
    finally:
        odo.close()
