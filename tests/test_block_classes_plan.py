"""Planner rule of the forward tile kernel's block priority classes (action.hip plan_tile;
an A/B knob: LV_TILE_NCLASS, off by default and absent from the product library), through
the A/B library's host-only entry lv_ab_fwd_classes: no GPU call, so this runs on CPU.

With LV_TILE_NCLASS = 3 the classes are on exactly where the whole grid is resident at once
-- up to kTileFewGroupsPerCU = 4 sample groups per compute unit, the range of the 7-wave
plan -- and off beyond, and the grid-stride kernel never has them.  The two class fields
ride in the first 64-byte line of the kernel's launch arguments and the degree sets fill the
second, so the kernel's start-up still reads everything in its one batch of scalar loads.
The knobs are read once per process, so each setting is planned in a child process."""
import json
import os
import subprocess
import sys

import pytest

F32, BF16 = 0, 1
FEW_GROUPS_PER_CU = 4  # action.hip kTileFewGroupsPerCU
CUS = (256, 64, 304, 8)
# (L, C, dtype, fused): C = 10 and run-time C, both output types, fused and not
SHAPES = ((10, 10, F32, 1), (10, 10, BF16, 1), (20, 10, BF16, 1), (10, 10, F32, 0), (10, 7, F32, 1),
          (3, 16, F32, 0))
# (fused, F batch stride, L, C): a per-sample spectrum, a tile too large for LDS
GRID_STRIDE = ((0, 121 * 10, 10, 10), (1, 0, 20, 10), (0, 0, 20, 10), (0, 16 * 3, 3, 3))

_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from lie_vae import _lib
out = []
for q in json.loads(sys.argv[2]):
    fused, fstride, dt, n, L, C, cus = q
    c = _lib.fwd_classes(fused, fstride, dt, n, L, C, cus)
    c["plan_tile"] = _lib.plan("fwd", fused, fstride, dt, n, L, C)["tile"] if cus == 0 else None
    out.append(c)
print(json.dumps(out))
"""


def _edge(cus, C):
    return FEW_GROUPS_PER_CU * cus * (64 // C)  # the last n with <= 4 groups per CU


def _queries():
    on, off, grid = [], [], []
    for cus in CUS:
        for L, C, dt, fused in SHAPES:
            spg, edge = 64 // C, _edge(cus, C)
            on += [(fused, 0, dt, n, L, C, cus) for n in (1, spg, spg + 1, cus * spg, edge - 1, edge)]
            off += [(fused, 0, dt, n, L, C, cus) for n in (edge + 1, edge + spg, 2 * edge, 16 * edge + 1, 1 << 20)]
    for n in (1, 13, 4096, 65536):
        grid += [(fused, fstride, F32, n, L, C, 0) for fused, fstride, L, C in GRID_STRIDE]
    return on, off, grid


def _plan(queries, knobs):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lie-vae_amd")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LV_")}
    env.update(knobs, LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", "liblievae_hip_ab.so"))
    r = subprocess.run([sys.executable, "-c", _SCRIPT, pkg, json.dumps(queries)], env=env, check=True,
                       capture_output=True, text=True, timeout=120)
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("nclass", [3, 2])
def test_classes_on_exactly_up_to_the_few_groups_bound(nclass):
    on, off, grid = _queries()
    res = _plan(on + off + grid, {"LV_TILE_NCLASS": str(nclass)})
    for q, c in zip(on, res[:len(on)]):
        shift = q[-1].bit_length() - 1  # floor(log2(cus)): the block's turn on its CU
        assert (c["tile"], c["nclass"], c["class_map"]) == (1, nclass, shift), (q, c)
    for q, c in zip(off, res[len(on):len(on) + len(off)]):
        assert (c["tile"], c["nclass"], c["class_map"]) == (1, 0, 0), (q, c)
    for q, c in zip(grid, res[len(on) + len(off):]):
        assert (c["tile"], c["plan_tile"], c["nclass"], c["class_map"]) == (0, 0, 0, 0), (q, c)


def test_benchmark_sizes_and_the_mappings():
    """Config 2 (4,096 samples: 683 blocks on 256 CUs) takes the classes, the sweep sizes and
    config 5 (8,192 at l = 20: 1,366 blocks) do not; LV_TILE_CLASS_MAP and
    LV_TILE_CLASS_FLUSH reach the kernel's argument; the launch plan itself is unchanged."""
    qs = [(1, 0, F32, 4096, 10, 10, 256), (1, 0, F32, 6144, 10, 10, 256), (1, 0, F32, 6145, 10, 10, 256),
          (1, 0, F32, 16384, 10, 10, 256), (1, 0, F32, 65536, 10, 10, 256), (1, 0, BF16, 8192, 20, 10, 256)]
    r = _plan(qs, {"LV_TILE_NCLASS": "3", "LV_TILE_CLASS_MAP": "64", "LV_TILE_CLASS_FLUSH": "1"})
    assert [c["nclass"] for c in r] == [3, 3, 0, 0, 0, 0]
    assert [c["class_map"] for c in r] == [0x140, 0x140, 0, 0, 0, 0]
    r = _plan(qs, {"LV_TILE_NCLASS": "7", "LV_TILE_CLASS_MAP": "3"})  # at most 3 classes
    assert [(c["nclass"], c["class_map"]) for c in r[:3]] == [(3, 3), (3, 3), (0, 0)]
    from lie_vae import _lib
    p = _lib.plan("fwd", 1, 0, F32, 4096, 10, 10)
    assert (p["tile"], p["blocks"], p["segments"], p["lds_bytes"], p["aux"]) == (1, 683, 7, 30880, 1)


def test_classes_are_off_by_default_and_not_in_the_product():
    on, off, grid = _queries()
    for c in _plan(on + off + grid, {}):
        assert (c["nclass"], c["class_map"]) == (0, 0), c
    from lie_vae import _lib
    lib = _lib.load()  # the product library
    assert not hasattr(lib, "lv_ab_fwd_classes")
    with pytest.raises(_lib.LieVaeHipError):
        _lib.fwd_classes(1, 0, F32, 4096, 10, 10)
    with open(_lib.LIB_PATH, "rb") as f:
        assert b"LV_TILE_NCLASS" not in f.read()


def test_class_fields_sit_in_the_start_up_lines():
    c = _plan([(1, 0, F32, 4096, 10, 10, 256)], {})[0]
    assert 0 <= c["off_nclass"] < 64 and 0 <= c["off_class_map"] < 64
    assert c["off_nclass"] % 2 == 0 and c["off_class_map"] % 2 == 0 and c["off_nclass"] != c["off_class_map"]
    assert c["off_seg_mask"] == 64  # the degree sets are the second line
