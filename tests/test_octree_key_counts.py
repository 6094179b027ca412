"""CPU: images whose level 0 has an exact, chosen number of FAST keys.

k_octree keeps a workgroup's keys in registers while a (frame, level) has at
most RESIDENT_CAP of them and falls back to HBM scratch beyond, so its tests
(test_octree_resident_gpu.py) need key counts on both sides of that edge and of
the 256-thread stride. An isolated single-pixel dot on a flat background is one
FAST corner; dots on a 4-pixel grid stay isolated, so the first K grid
positions give exactly K keys at level 0. That is asserted here with
fast_level_ref.
"""
import numpy as np
import pytest

import extract_ref as R

RESIDENT_CAP = 2048  # k_octree: OT_THREADS * OT_KB keys stay in registers
W, H = 320, 240
BACKGROUND = 40
POSITIONS = [(y, x) for y in range(20, 220, 4) for x in range(20, 300, 4)]
KS = (0, 1, 2, 255, 256, 257, RESIDENT_CAP - 1, RESIDENT_CAP, RESIDENT_CAP + 1)


def dots(k, values=None):
    """The first k grid positions set to 255, or to values[i]."""
    img = np.full((H, W), BACKGROUND, np.uint8)
    for i, (y, x) in enumerate(POSITIONS[:k]):
        img[y, x] = 255 if values is None else values[i]
    return img


def dots_random(k):
    """Dot values drawn from [120, 256): many distinct responses, so the
    octree's retention is not decided by ties alone."""
    return dots(k, np.random.default_rng(7).integers(120, 256, size=k))


def test_enough_positions():
    assert len(POSITIONS) > RESIDENT_CAP + 1


@pytest.mark.parametrize("k", KS)
def test_equal_dots_give_k_keys(k):
    x, y, r, _ = R.fast_level_ref(dots(k))
    assert len(x) == k
    assert len(set(r.tolist())) <= 1  # ties everywhere: the first candidate of a node wins


def test_random_dots_give_k_keys_and_many_responses():
    k = RESIDENT_CAP + 1
    x, y, r, _ = R.fast_level_ref(dots_random(k))
    assert len(x) == k
    assert len(set(r.tolist())) > 100
