"""odo_gicp_grid_fitness (k_gicp.hip: k_gicp_fit_*) against tests/sor_ref.py's
restatement of getFitnessScore: the nearest squared distance of every
transformed source point bit for bit, the score within the bound of a sum in
another fixed order. Source points far outside the target's bounds on every
axis and direction exercise the stop rule from a clamped cell (sor_ref's
docstring); forced cells give bit-equal results. odo_gicp_dense_fitness is held
against this entry point in tests/test_sor_gpu.py::test_dense_sor.
"""
import numpy as np
import pytest

import sor_ref as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CASES = S.fitness_cases()
CELLS = (0.0, 0.02, 0.3, 1000.0)


@pytest.fixture(scope="module")
def odo():
    pkg = load_pkg()
    o = pkg.Odometry(pkg.default_config(640, 480, 1))
    yield o
    o.close()


def check(score, nn, ref, ns, what):
    rs, rn = ref
    print(f"{what}: score {score:.17g}, reference {rs:.17g}, bound {S.fitness_bound(rs, ns):.3g}")
    assert nn.tobytes() == rn.tobytes(), what
    if rs == S.DBL_MAX:
        assert score == S.DBL_MAX, what
    else:
        assert abs(score - rs) <= S.fitness_bound(rs, ns), what


@pytest.mark.parametrize("name", list(CASES))
def test_case(odo, name):
    src, tgt, T = CASES[name]
    ref = S.fitness(src, tgt, T)
    first = None
    for cell in CELLS:
        score, nn = odo.gicp_grid_fitness([(src, tgt, T)], cell)
        check(float(score[0]), nn[0], ref, len(src), (name, cell))
        got = (score.tobytes(), nn[0].tobytes())
        first = first or got
        assert got == first, (name, cell)
    if name == "coincident":
        assert score[0] == 0.0
    if name.startswith("empty"):
        assert score[0] == S.DBL_MAX


def test_batch_equals_single_calls(odo):
    names = list(CASES)
    batch = [CASES[n] for n in names]
    score, nn = odo.gicp_grid_fitness(batch)
    assert len(score) == len(batch)
    for i, n in enumerate(names):
        one, onn = odo.gicp_grid_fitness([batch[i]])
        assert one[0] == score[i] and onn[0].tobytes() == nn[i].tobytes(), n
    assert len(odo.gicp_grid_fitness([])[0]) == 0


def test_argument_errors_write_nothing(odo):
    lib, h = odo.lib, odo.h
    src, tgt, _ = CASES["scene"]
    src, tgt = np.ascontiguousarray(src), np.ascontiguousarray(tgt)
    I4 = np.eye(4, dtype=np.float32)
    score, nn = np.full(1, 7.0), np.full(300, 7.0, np.float32)
    ok = dict(src=src, so=[0, 300], tgt=tgt, to=[0, 300], T=I4, n=1, cell=0.0, score=score)

    def call(**kw):
        a = {**ok, **kw}
        so, to = np.asarray(a["so"], np.int32), np.asarray(a["to"], np.int32)
        p = lambda x: None if x is None else x.ctypes.data
        return lib.odo_gicp_grid_fitness(h, p(a["src"]), so.ctypes.data, p(a["tgt"]), to.ctypes.data, p(a["T"]), a["n"],
                                         a["cell"], p(a["score"]), nn.ctypes.data)

    nan_T = I4.copy()
    nan_T[0, 3] = np.nan
    nan_s = src.copy()
    nan_s[5, 1] = np.inf
    for kw in (dict(src=None), dict(tgt=None), dict(T=None), dict(score=None), dict(so=[1, 300]), dict(to=[0, 300, 200], so=[0, 300, 300], n=2),
               dict(cell=-1.0), dict(cell=float("nan")), dict(T=nan_T), dict(src=nan_s), dict(n=-1)):
        assert call(**kw) == S.ERR_ARG, kw
    assert call(cell=1e-4) == S.ERR_CAPACITY
    assert score[0] == 7.0 and np.all(nn == 7.0)
    assert call(n=0) == 0 and score[0] == 7.0
    assert call() == 0 and nn.tobytes() == S.fitness(src, tgt)[1].tobytes()
