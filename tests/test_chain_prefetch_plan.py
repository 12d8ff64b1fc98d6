"""Operand-prefetch depths of the forward tile kernel's chain (action_fwd.h chain_depth, a
compile-time choice per kernel and degree from the kernel's VGPR ceiling) and the A/B field
that turns them off (ActionArgs::chain_fetch, LV_TILE_PREFETCH=0), through the A/B library's
host-only entry lv_ab_fwd_chain: no GPU call, so this runs on CPU.  The knob is read once per
process, so each setting is planned in a child process."""
import json
import os
import subprocess
import sys

import pytest

F32, BF16 = 0, 1
OFF, HALF, FULL = 0, 1, 2
# (fused, F batch stride, dtype, n, L, C, cus): the BASELINE shapes and the benchmark's sweep
CONFIG1 = (1, 0, F32, 256, 3, 10, 256)
CONFIG2 = (1, 0, F32, 4096, 10, 10, 256)
CONFIG3 = (1, 0, F32, 512, 10, 10, 256)
CONFIG5 = (1, 0, BF16, 8192, 20, 10, 256)
SWEEP = ((1, 0, F32, 16384, 10, 10, 256), (1, 0, F32, 65536, 10, 10, 256))
RUNTIME_C = (1, 0, F32, 50, 6, 3, 256)
GRID_STRIDE = ((0, 121 * 10, F32, 4096, 10, 10, 256), (1, 0, F32, 4096, 20, 10, 256))

_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from lie_vae import _lib
print(json.dumps([_lib.fwd_chain(*q) for q in json.loads(sys.argv[2])]))
"""


def _plan(queries, knobs):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lie-vae_amd")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LV_")}
    env.update(knobs, LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", "liblievae_hip_ab.so"))
    r = subprocess.run([sys.executable, "-c", _SCRIPT, pkg, json.dumps(queries)], env=env, check=True,
                       capture_output=True, text=True, timeout=120)
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_depths_of_the_baseline_configs():
    """Up to l_max = 10 (ceiling 64 VGPRs: 8 waves per SIMD, which the 8-wave plan of batch
    16,384 needs for its 4 blocks per CU) every degree prefetches all its multiples.  The
    l_max = 20 kernel (ceiling 104: 4 waves per SIMD, it stands at 96 with no prefetch at
    its top degree) holds all of them up to l = 14, the first (l + 4) / 8 quads for 15-17
    and none from 18: 2(2l + 1) + 16 + held <= 104."""
    c1, c2, c3, c5, s1, s2, rc = _plan([CONFIG1, CONFIG2, CONFIG3, CONFIG5, *SWEEP, RUNTIME_C], {})
    for c, L in ((c1, 3), (c2, 10), (c3, 10), (s1, 10), (s2, 10), (rc, 6)):
        assert (c["tile"], c["chain_fetch"], c["vgpr_ceiling"]) == (1, 1, 64), c
        assert c["depths"] == [FULL] * (L + 1), c
    assert (c5["tile"], c5["chain_fetch"], c5["vgpr_ceiling"]) == (1, 1, 104), c5
    assert c5["depths"] == [FULL] * 15 + [HALF] * 3 + [OFF] * 3, c5
    for l, d in enumerate(c5["depths"]):
        held = {OFF: 0, HALF: 8 * ((l + 4) // 8), FULL: 2 * (l + 1)}[d]
        assert 2 * (2 * l + 1) + 16 + held <= c5["vgpr_ceiling"], (l, d)


def test_knob_turns_every_degree_off_and_the_grid_stride_kernel_has_none():
    on = _plan([CONFIG2, CONFIG5, *GRID_STRIDE], {})
    off = _plan([CONFIG2, CONFIG5, *GRID_STRIDE], {"LV_TILE_PREFETCH": "0"})
    assert [c["chain_fetch"] for c in on] == [1, 1, 0, 0]
    assert [c["chain_fetch"] for c in off] == [0, 0, 0, 0]
    assert [c["tile"] for c in on] == [c["tile"] for c in off] == [1, 1, 0, 0]
    assert [c["depths"] for c in on] == [c["depths"] for c in off]  # compile-time: the knob selects the copy


def test_field_sits_in_the_start_up_line_and_the_plan_is_unchanged():
    c = _plan([CONFIG2], {})[0]
    # the upper half of what was the 32-bit prio field: line 0 of ActionArgs, 2-byte aligned
    assert c["off_chain_fetch"] == 46
    from lie_vae import _lib
    p = _lib.plan("fwd", 1, 0, F32, 4096, 10, 10)
    assert (p["tile"], p["blocks"], p["segments"], p["lds_bytes"], p["aux"]) == (1, 683, 7, 30880, 1)
    p = _lib.plan("fwd", 1, 0, BF16, 8192, 20, 10)
    assert (p["tile"], p["blocks"]) == (1, 1366)


def test_not_in_the_product():
    from lie_vae import _lib
    lib = _lib.load()  # the product library
    assert not hasattr(lib, "lv_ab_fwd_chain")
    with pytest.raises(_lib.LieVaeHipError):
        _lib.fwd_chain(*CONFIG2)
    with open(_lib.LIB_PATH, "rb") as f:
        assert b"LV_TILE_PREFETCH" not in f.read()
