"""The fewest waves a product plan gives a block of the forward tile kernel (action_fwd.h
tile_min_waves), the bound by which the product's mu-free fused kernel leaves out the
one-wave block's code -- the angle maths behind the prologue barrier -- and holds the angle
waves' indices as constants.  A plan below the bound would run a kernel that has no code for
it, so the bound must agree with plan_tile (action.hip) over every shape.  Host-only entries
(lv_action_fwd_plan of the product, lv_ab_fwd_min_waves of the A/B library): no GPU call, so
this runs on CPU."""
import json
import os
import subprocess
import sys

import pytest

from lie_vae import _lib
from test_plan import NS

F32, BF16 = _lib.LV_DTYPE_F32, _lib.LV_DTYPE_BF16
CHANNELS = (1, 3, 10, 16, 64)  # test_plan.py's sweep

_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from lie_vae import _lib
print(json.dumps([_lib.fwd_min_waves(L) for L in range(21)]))
"""


@pytest.fixture(scope="module")
def bound():
    """lv_ab_fwd_min_waves for l_max = 0..20 (the A/B library, in a child process: this
    process holds the product library)."""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lie-vae_amd")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LV_")}
    env["LIEVAE_HIP_LIB"] = os.path.join(pkg, "lie_vae", "liblievae_hip_ab.so")
    r = subprocess.run([sys.executable, "-c", _SCRIPT, pkg], env=env, check=True, capture_output=True,
                       text=True, timeout=120)
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bound_values(bound):
    """ceil(total chain cost / 560), the large-batch target, within [1, min(8, L + 1)]: one
    wave up to l_max = 5 (total 476), two at 6 and 7, three at 8 and 9, four at 10 (1,987),
    eight from 14; the angle maths behind the barrier is held exactly where it is one."""
    assert [b["min_waves"] for b in bound] == [1] * 6 + [2, 2, 3, 3, 4, 5, 6, 7] + [8] * 7
    for L, b in enumerate(bound):
        assert b["late_angles"] == (1 if b["min_waves"] == 1 else 0), L
        assert b["min_waves"] == min(b["few"], b["mid"], b["large"]) == b["large"], (L, b)
        assert 1 <= b["min_waves"] <= min(8, L + 1), (L, b)
    assert (bound[10]["few"], bound[10]["mid"], bound[10]["large"]) == (7, 8, 4)


@pytest.mark.parametrize("L", list(range(0, 21)))
def test_no_product_plan_is_below_the_bound(bound, L):
    b = bound[L]
    M = (L + 1) ** 2
    fewest = None
    for C in CHANNELS:
        for n in NS:
            for fused, fstride, dt in ((1, 0, F32), (1, 0, BF16), (0, 0, F32), (0, 0, BF16), (0, M * C, F32)):
                p = _lib.plan("fwd", fused, fstride, dt, n, L, C)
                if not p["tile"]:
                    continue
                assert p["segments"] >= b["min_waves"], (C, n, fused, dt, p["segments"], b)
                if C == 10 and fused:
                    fewest = p["segments"] if fewest is None else min(fewest, p["segments"])
    # the bound is tight for the kernel it is compiled into (C = 10, fused): the largest batch
    # plans exactly that many waves wherever the tile kernel runs
    if fewest is not None:
        assert fewest == b["min_waves"], (fewest, b)


def test_batch_classes_at_config2_shapes(bound):
    for n, key in ((4096, "few"), (16384, "mid"), (65536, "large")):
        p = _lib.plan("fwd", 1, 0, F32, n, 10, 10)
        assert p["tile"] == 1 and p["segments"] == bound[10][key], (n, p["segments"])


def test_not_in_the_product():
    lib = _lib.load()  # the product library
    assert not hasattr(lib, "lv_ab_fwd_min_waves")
    with pytest.raises(_lib.LieVaeHipError):
        _lib.fwd_min_waves(10)
