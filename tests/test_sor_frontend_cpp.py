"""Frame::StatisticalOutlierRemovalFilterCloud and GeneralizedICP::mScore of the
C++ mirror (include/odo_frontend.hpp, standing in for Core/frame.cpp:228-238 and
Odometry/generalizedicp.cpp:82-87): the program tests/cpp/sor_mirror.cpp,
compiled here against the header and the library, against the Python binding's
dense_clouds_host + dense_sor + gicp_dense + gicp_dense_fitness on the same two
frames."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, load_pkg, sequence
from test_cloud_frontend_cpp import checksum

INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "sor_mirror.cpp")
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
    exe = tmp_path / "sor_mirror"
    subprocess.run(["g++", "-O1", *FLAGS, "-o", str(exe), SRC, "-I", INC, "-L", PKG_DIR, "-lodo_hip",
                    f"-Wl,-rpath,{PKG_DIR}"], check=True)
    r = subprocess.run([str(exe), str(frames), "640", "480", "0.03", "50", "1.0", "3", "0.05"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[0] for ln in lines] == ["voxel", "sor", "voxel", "sor", "gicp", "short"]
    pkg = load_pkg()
    odo = pkg.Odometry(pkg.default_config(640, 480, 2))  # the mirror's own context: default calibration
    try:
        odo.dense_clouds_host(bgr, dep, 0.03)
        for i in range(2):
            pts = odo.get_dense_cloud(i)
            assert (int(lines[2 * i][1]), int(lines[2 * i][2], 16)) == (len(pts), checksum(pts))
        info = odo.dense_sor(50, 1.0)
        for i in range(2):
            pts = odo.get_dense_cloud(i)
            assert (int(lines[2 * i + 1][1]), int(lines[2 * i + 1][2], 16)) == (len(pts), checksum(pts))
            assert 1000 < int(info[i]["n_out"]) == len(pts) < int(info[i]["n_in"]) == int(lines[2 * i][1])
        T, conv, it, nc = odo.gicp_dense([(0, 1)], None, 3, 0.05)[0]
        assert int(lines[4][1]) == conv == 1 and nc > 1000
        score = float(odo.gicp_dense_fitness([(0, 1)], [T])[0])
        print(f"mScore {lines[4][2]} = {float.fromhex(lines[4][2]):.6g}, C ABI {score:.6g}")
        assert float.fromhex(lines[4][2]) == score and 0 < score < 1e-3
        assert lines[5][1] == "0" and float.fromhex(lines[5][2]) == 1e6
    finally:
        odo.close()
