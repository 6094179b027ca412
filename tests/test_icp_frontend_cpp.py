"""IcpPointToPlane of the C++ mirror (include/odo_frontend.hpp, standing in for
Odometry/icp/icpPointToPlane.h): the program tests/cpp/icp_mirror.cpp, compiled
here against the header and the library, against Odometry.icp_plane_batch on
the same clouds, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import icp_ref as I
from conftest import PKG_DIR, ROOT, load_pkg

INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "icp_mirror.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]


def test_mirror_compiles_with_warnings_as_errors():
    subprocess.run(["g++", *FLAGS, "-fsyntax-only", "-I", INC, SRC], check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n_t", [300, 4])
def test_mirror_equals_the_binding(tmp_path, n_t):
    T, M, _ = I.loop_cases()["corner300_test_program"]
    T = T[:n_t]
    clouds = tmp_path / "c.bin"
    with open(clouds, "wb") as f:
        f.write(np.int32([len(T), len(M)]).tobytes())
        f.write(T.tobytes())
        f.write(M.tobytes())
    exe = tmp_path / "icp_mirror"
    subprocess.run(["g++", "-O1", *FLAGS, "-o", str(exe), SRC, "-I", INC, "-L", PKG_DIR, "-lodo_hip",
                    f"-Wl,-rpath,{PKG_DIR}"], check=True)
    r = subprocess.run([str(exe), str(clouds), "15", "12", "1e-8", "0.01"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0] == ["dim", "1"] and lines[1][0] == "fit" and len(lines[1]) == 18
    pkg = load_pkg()
    odo = pkg.Odometry(pkg.default_config(640, 480, 1))
    try:
        rec = odo.icp_plane_batch([(T, M, None)], pkg.icp_params(num_neighbors=15, max_iterations=12, min_delta=1e-8,
                                                                 indist=0.01))[0]
    finally:
        odo.close()
    P = rec["T"].reshape(4, 4)
    want = [int(v) for v in np.r_[P[:3, :3].reshape(-1), P[:3, 3]].astype(np.float32).view(np.uint32)]
    assert [int(v, 16) for v in lines[1][1:13]] == want
    assert int(lines[1][13], 16) == int(np.float64(rec["residual"]).view(np.uint64))
    assert int(lines[1][14]) == rec["n_active"] and int(lines[1][16]) == rec["iterations"] and int(lines[1][17]) == rec["status"]
    assert int(lines[1][15], 16) == int(np.float64(rec["n_active"] / len(T)).view(np.uint64))
    if n_t == 4:
        assert rec["status"] == I.SHORT_TEMPLATE and np.array_equal(P, np.eye(4)) and rec["residual"] == 0.0
    else:
        assert rec["status"] == I.OK and rec["iterations"] >= 3 and rec["n_active"] > 250
