"""The product's forward tile kernel without the one-wave block's code (action_fwd.h
fwd_tile_body kMinWaves / kAngBehind): from l_max = 6 no product plan has a one-wave block, so
the mu-free fused kernel holds neither the angle maths behind the prologue barrier nor the
run-time choice of the angle waves (wave 1 writes alpha and gamma; wave 2 beta, from l_max = 8
always, at 6 and 7 only in plans of three waves and more).  The A/B library keeps all of it.
Angles and outputs of lv_fused_exp_action_fwd must equal the A/B library's bit for bit on both
sides of each boundary and in each batch class (few / mid / large groups per CU plan different
wave counts), and the A/B library's one-wave plan (LV_TILE_NSEG=1: every angle written behind
the barrier by wave 0) must give the same bits again.

Cases (fp32, C = 10, no mean rotation; waves few / large):
  l = 5   2 / 1 waves   the last l_max whose product kernel holds the one-wave code, and runs it
  l = 6   3 / 2         two waves: wave 1 writes all three angles
  l = 7   4 / 2
  l = 8   5 / 3         three waves: beta on wave 2, now a constant
  l = 10  7 / 4         config 2's kernel
n = 7 (two blocks, the second with one valid sample) and n = 24,583 (4,098 groups: the large
class at 256 CUs, last block one sample).  The large outputs are compared by a 64-bit sum of
their bit patterns and their last block in full, the angles in full.  Every case carries a
sentinel row past n.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SMALL, N_LARGE = 7, 24583
LS = (5, 6, 7, 8, 10)
CASES = {f"l{L}_n{n}": (n, L) for L in LS for n in (N_SMALL, N_LARGE)}

_SCRIPT = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from lie_vae import _lib
import test_gpu_tile_min_waves as T
dev = torch.device("cuda:0")
C = 10
res = {}
for name, (n, L) in T.CASES.items():
    g = torch.Generator().manual_seed(4100 + 10 * L + (n & 1023))
    v = torch.randn(n, 3, generator=g).to(dev)
    M = (L + 1) ** 2
    F = torch.randn(M, C, generator=g).to(dev)
    out = torch.full((n + 1, M, C), -12288.0, device=dev)
    ang = torch.full((n + 1, 3), -12288.0, device=dev)
    _lib.call("lv_fused_exp_action_fwd", None, v.data_ptr(), F.data_ptr(), 0, out.data_ptr(), _lib.LV_DTYPE_F32,
              ang.data_ptr(), n, L, C, 0, _lib.stream())
    torch.cuda.synchronize()
    assert (out[n:] == -12288.0).all() and (ang[n:] == -12288.0).all(), name
    assert torch.isfinite(out[:n]).all() and torch.isfinite(ang[:n]).all(), name
    bits = out[:n].view(torch.int32)
    res[name + "_sum"] = np.array([int(bits.to(torch.int64).sum().item())])
    res[name + "_tail"] = bits[max(0, n - 7):].cpu().numpy()
    res[name + "_ang"] = ang[:n].view(torch.int32).cpu().numpy()
    p = _lib.plan("fwd", 1, 0, _lib.LV_DTYPE_F32, n, L, C)
    res[name + "_plan"] = np.array([p["tile"], p["segments"]])
np.savez(sys.argv[3], **res)
"""


def _run(tmp, tag, lib, knobs):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "lie-vae_amd")
    out = str(tmp / f"{tag}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LV_")}
    env.update(knobs, LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", lib))
    subprocess.run([sys.executable, "-c", _SCRIPT, pkg, os.path.join(repo, "tests"), out], env=env, check=True,
                   capture_output=True, text=True, timeout=300, cwd=repo)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def product(gpu_device, tmp_path_factory):
    return _run(tmp_path_factory.mktemp("minwaves"), "product", "liblievae_hip.so", {})


def _assert_same(r, ref, what):
    for name in CASES:
        for part in ("_sum", "_tail", "_ang"):
            assert np.array_equal(r[name + part], ref[name + part]), (what, name, part)


def test_product_plans_cover_both_sides_of_each_boundary(product):
    """The wave counts the cases are chosen for (256 compute units): one wave only at l = 5,
    two waves at l = 6 and 7, three at l = 8."""
    waves = {name: tuple(product[name + "_plan"]) for name in CASES}
    want = {5: (2, 1), 6: (3, 2), 7: (4, 2), 8: (5, 3), 10: (7, 4)}
    for L, (few, large) in want.items():
        assert waves[f"l{L}_n{N_SMALL}"] == (1, few), (L, waves)
        assert waves[f"l{L}_n{N_LARGE}"] == (1, large), (L, waves)


def test_product_equals_ab_library_bitwise(gpu_device, tmp_path, product):
    """The A/B library at the product's wave counts: run-time angle waves, both placements
    compiled in."""
    ab = _run(tmp_path, "ab", "liblievae_hip_ab.so", {})
    for name in CASES:
        assert tuple(ab[name + "_plan"]) == tuple(product[name + "_plan"]), name
    _assert_same(product, ab, "product vs A/B library")


def test_one_wave_plan_of_the_ab_library_bitwise(gpu_device, tmp_path, product):
    """LV_TILE_NSEG=1: wave 0 writes every angle behind the prologue barrier, the code the
    product's kernels hold up to l_max = 5 only."""
    one = _run(tmp_path, "one", "liblievae_hip_ab.so", {"LV_TILE_NSEG": "1"})
    for name in CASES:
        assert tuple(one[name + "_plan"]) == (1, 1), name
    _assert_same(product, one, "product vs one-wave A/B plan")
