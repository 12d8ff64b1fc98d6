"""Block priority classes of the forward tile kernel (action_fwd.h fwd_tile_body,
action.hip plan_tile; an A/B knob, LV_TILE_NCLASS): the blocks that share a CU run their
chains at different s_setprio levels.  That is scheduling only, so every output and every
saved angle must equal, bit for bit, what the product library -- whose kernels do not hold
the class code -- writes, for every class mapping the A/B library keeps (LV_TILE_NCLASS /
LV_TILE_CLASS_MAP / LV_TILE_CLASS_FLUSH) and for the A/B library with the classes off.  The
knobs are read once per process, so each setting runs in a child process that writes all
cases to one file.

Cases: 145 samples at l = 10 (25 blocks of 6 samples: every class of 2 and of 3, every XCD
residue, a ragged last group of one sample), fp32 and bf16 output; one sample; 19 samples at
l = 0 and 1; the bf16 l = 20 tile kernel at 13 samples; the non-fused lv_group_action_fwd at
145 samples.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from lie_vae import _lib
dev = torch.device("cuda:0")
F32, BF16 = 0, 1
res = {}
# (name, fused, n, L, dtype)
CASES = [("f145", 1, 145, 10, F32), ("f145_bf16", 1, 145, 10, BF16), ("f1", 1, 1, 10, F32),
         ("f19_l0", 1, 19, 0, F32), ("f19_l1", 1, 19, 1, F32), ("f13_l20_bf16", 1, 13, 20, BF16),
         ("g145", 0, 145, 10, F32)]
C = 10
for name, fused, n, L, dt in CASES:
    g = torch.Generator().manual_seed(1000 * L + n)
    M = (L + 1) ** 2
    v = torch.randn(n, 3, generator=g).to(dev)
    F = torch.randn(M, C, generator=g).to(dev)
    out = torch.full((n + 1, M, C), -12288.0, device=dev, dtype=torch.bfloat16 if dt == BF16 else torch.float32)
    ang = torch.full((n + 1, 3), -12288.0, device=dev)
    if fused:
        _lib.call("lv_fused_exp_action_fwd", None, v.data_ptr(), F.data_ptr(), 0, out.data_ptr(), dt,
                  ang.data_ptr(), n, L, C, 0, _lib.stream())
    else:
        _lib.call("lv_group_action_fwd", v.data_ptr(), F.data_ptr(), 0, out.data_ptr(), dt, n, L, C, 0,
                  _lib.stream())
    torch.cuda.synchronize()
    assert (out[n:].float() == -12288.0).all() and (ang[n:] == -12288.0).all(), name
    assert torch.isfinite(out[:n].float()).all(), name
    res[name] = out[:n].view(torch.int16 if dt == BF16 else torch.int32).cpu().numpy()
    if fused:
        res[name + "_ang"] = ang[:n].view(torch.int32).cpu().numpy()
    if hasattr(_lib.load(), "lv_ab_fwd_classes"):
        c = _lib.fwd_classes(fused, 0, dt, n, L, C)
        res[name + "_plan"] = np.array([c["tile"], c["nclass"], c["class_map"]])
    else:  # the product library: no classes in its kernels
        res[name + "_plan"] = np.array([_lib.plan("fwd", fused, 0, dt, n, L, C)["tile"], 0, 0])
np.savez(sys.argv[2], **res)
"""

CASE_NAMES = ("f145", "f145_bf16", "f1", "f19_l0", "f19_l1", "f13_l20_bf16", "g145")


def _run(tmp, tag, lib, knobs):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "lie-vae_amd")
    out = str(tmp / f"{tag}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LV_")}
    env.update(knobs, LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", lib))
    subprocess.run([sys.executable, "-c", _SCRIPT, pkg, out], env=env, check=True, capture_output=True,
                   text=True, timeout=300)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def product(gpu_device, tmp_path_factory):
    """The reference of every comparison, computed once: the product library."""
    r = _run(tmp_path_factory.mktemp("classes"), "product", "liblievae_hip.so", {})
    for name in CASE_NAMES:
        assert r[name + "_plan"][0] == 1, name  # every case runs the tile kernel
    return r


def _assert_same(r, ref, what):
    for name in CASE_NAMES:
        assert np.array_equal(r[name], ref[name]), (what, name)
        if name + "_ang" in ref:
            assert np.array_equal(r[name + "_ang"], ref[name + "_ang"]), (what, name, "angles")


def test_classes_off_in_the_ab_library(gpu_device, tmp_path, product):
    """The A/B library as it plans by default: no classes."""
    r = _run(tmp_path, "off", "liblievae_hip_ab.so", {})
    for name in CASE_NAMES:
        assert tuple(r[name + "_plan"]) == (1, 0, 0), name
    _assert_same(r, product, "off")


# every mapping the A/B library keeps: classes from the dealing round of 8 blocks (shift 3),
# from the block's turn on its CU (shift 8 = log2 of the MI355X's 256 CUs), from the
# workgroup's CU slot (64), with 2 and 3 classes, and the flush one priority above the chain
@pytest.mark.parametrize("knobs", [
    {"LV_TILE_NCLASS": "2", "LV_TILE_CLASS_MAP": "3"},
    {"LV_TILE_NCLASS": "3", "LV_TILE_CLASS_MAP": "3"},
    {"LV_TILE_NCLASS": "2", "LV_TILE_CLASS_MAP": "8"},
    {"LV_TILE_NCLASS": "3", "LV_TILE_CLASS_MAP": "8"},
    {"LV_TILE_NCLASS": "3", "LV_TILE_CLASS_MAP": "0"},   # shift 0: all three classes in 25 blocks' first 3
    {"LV_TILE_NCLASS": "2", "LV_TILE_CLASS_MAP": "64"},
    {"LV_TILE_NCLASS": "3", "LV_TILE_CLASS_MAP": "64"},
    {"LV_TILE_NCLASS": "3", "LV_TILE_CLASS_MAP": "3", "LV_TILE_CLASS_FLUSH": "1"},
    {"LV_TILE_NCLASS": "3", "LV_TILE_CLASS_MAP": "64", "LV_TILE_CLASS_FLUSH": "1"},
], ids=lambda k: json.dumps(k, separators=(",", ":")))
def test_every_mapping_against_the_product(gpu_device, tmp_path, product, knobs):
    r = _run(tmp_path, "ab", "liblievae_hip_ab.so", knobs)
    for name in CASE_NAMES:
        tile, nclass, cmap = r[name + "_plan"]
        assert tile == 1 and nclass == int(knobs["LV_TILE_NCLASS"]), name
        assert cmap & 0x7f == int(knobs["LV_TILE_CLASS_MAP"]), name
        assert bool(cmap & 0x100) == ("LV_TILE_CLASS_FLUSH" in knobs), name
    _assert_same(r, product, knobs)
