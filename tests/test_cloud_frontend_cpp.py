"""Frame::CreateCloud / Frame::VoxelGridFilterCloud of the C++ mirror
(include/odo_frontend.hpp, standing in for Core/frame.h:48-49 and :80): the
program tests/cpp/cloud_mirror.cpp, compiled here against the header and the
library, against Odometry.dense_clouds_host on the same frame."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, load_pkg, sequence

INC = os.path.join(ROOT, "include")
SRC = os.path.join(ROOT, "tests", "cpp", "cloud_mirror.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter"]


def checksum(pts):
    """cloud_mirror.cpp's: the sum of word[i] * (2 i + 1) modulo 2^64."""
    w = np.frombuffer(pts.tobytes(), np.uint32).astype(np.uint64)
    return int((w * (2 * np.arange(len(w), dtype=np.uint64) + 1)).sum(dtype=np.uint64))


def test_mirror_compiles_with_warnings_as_errors(tmp_path):
    """The header with the cloud members, alone and under the program, -Wall -Wextra -Werror."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "odo_frontend.hpp"\nint main() { odo_hip::Frame* f = nullptr; '
                   'return f ? (int)f->mpCloud.size() : (int)sizeof(odo_cloud_point) - 16; }\n')
    for s in (str(src), SRC):
        subprocess.run(["g++", *FLAGS, "-fsyntax-only", "-I", INC, s], check=True)


@pytest.mark.gpu
def test_mirror_equals_the_binding(tmp_path):
    bgr, dep, _ = sequence(1, seed=0x5EED0033)
    bgr, dep = np.ascontiguousarray(bgr), np.ascontiguousarray(dep)
    frames = tmp_path / "f.bin"
    with open(frames, "wb") as f:
        f.write(bgr.tobytes())
        f.write(dep.tobytes())
    exe = tmp_path / "cloud_mirror"
    subprocess.run(["g++", "-O1", *FLAGS, "-o", str(exe), SRC, "-I", INC, "-L", PKG_DIR, "-lodo_hip",
                    f"-Wl,-rpath,{PKG_DIR}"], check=True)
    r = subprocess.run([str(exe), str(frames), "640", "480", "0.03"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[0] for ln in lines] == ["create", "create", "filter"] and lines[0] == lines[1]
    pkg = load_pkg()
    odo = pkg.Odometry(pkg.default_config(640, 480, 2))  # the mirror's own context: default calibration
    try:
        for leaf, ln in ((0.0, lines[0]), (0.03, lines[2])):
            info = odo.dense_clouds_host(bgr, dep, leaf)
            pts = odo.get_dense_cloud(0)
            assert int(ln[1]) == info[0]["n_points"] == len(pts) > 0
            assert int(ln[2], 16) == checksum(pts)
        assert int(lines[2][1]) < int(lines[0][1])
    finally:
        odo.close()
