"""Operand prefetch of the forward tile kernel's chain (action_fwd.h fwd_tile_body `degree`,
action_chain.h xrot_fetch / xrot_apply / chain_pin): the multiples of the next rotation are
read from LDS before the J product in front of it instead of right before their use.  Only
the moment of the reads changes -- the FMAs and their order are those of depth 0 -- so every
output and every saved angle of lv_fused_exp_action_fwd must equal, bit for bit, what the
A/B library writes with the old order (LV_TILE_PREFETCH=0: depth 0 at every degree), and the
oracle parity of config 2 must hold at every shape.  The knobs are read once per process, so
each setting runs in a child process that writes all its cases to one file.

Cases (fp32, C = 10 unless noted; Sw = 6 samples per block):
  n = 7, l = 10          two blocks, the second with one valid sample (idle lanes mirror it)
  n = 23, l = 10         6 * 3 + 5, with and without a mean rotation, both transposes
  l = 0, 1, 2, 3         degree sets with tiny degrees (one quad of multiples, 1-row blocks)
  run-time C             C = 3, l = 6, n = 50 (column-major spectrum slices)
  bf16 output            l = 20, n = 13 (depth 2 up to l = 14, 1 for 15-17, 0 above)
  out + 4 / + 8 bytes    the LDS tile -- and the spectrum in its last sample slot -- shifted
                         by the output pointer's misalignment
  LV_TILE_NSEG = 2, 1    l = 10 in two waves and in one: degree sets of 5 and 11 degrees
                         (A/B library both sides: the product plans its own wave count)
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
# name: (n, L, C, dtype, with mean, transpose, output misalignment in floats)
CASES = {
    "n7": (7, 10, 10, F32, 0, 0, 0),
    "n23": (23, 10, 10, F32, 0, 0, 0),
    "n23_t": (23, 10, 10, F32, 0, 1, 0),
    "n23_mu": (23, 10, 10, F32, 1, 0, 0),
    "n23_mu_t": (23, 10, 10, F32, 1, 1, 0),
    "l0": (13, 0, 10, F32, 0, 0, 0),
    "l1": (13, 1, 10, F32, 0, 0, 0),
    "l2": (13, 2, 10, F32, 0, 0, 0),
    "l3": (13, 3, 10, F32, 0, 0, 0),
    "c3_l6": (50, 6, 3, F32, 0, 0, 0),
    "l20_bf16": (13, 20, 10, BF16, 0, 0, 0),
    "n23_mis4": (23, 10, 10, F32, 0, 0, 1),
    "n23_mis8": (23, 10, 10, F32, 0, 0, 2),
    "n23_mu_mis8": (23, 10, 10, F32, 1, 1, 2),
}


def _inputs(name):
    """Seeded host inputs of a case (the child processes and the oracle build the same)."""
    n, L, C, dt, with_mu, transpose, mis = CASES[name]
    g = torch.Generator().manual_seed(7000 + 100 * L + n + 10 * C)
    v = torch.randn(n, 3, generator=g)
    F = torch.randn((L + 1) ** 2, C, generator=g)
    w = torch.randn(n, 3, generator=g)
    return v, F, w


_SCRIPT = r"""
import sys, json, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[4]]
from lie_vae import _lib
from oracle import lie_ref
import test_gpu_chain_prefetch as T
dev = torch.device("cuda:0")
res = {}
for name, (n, L, C, dt, with_mu, transpose, mis) in T.CASES.items():
    v, F, w = T._inputs(name)
    M = (L + 1) ** 2
    mu = lie_ref.so3_exp(w).contiguous().to(dev) if with_mu else None
    v, F = v.to(dev), F.to(dev)
    odt = torch.bfloat16 if dt == T.BF16 else torch.float32
    buf = torch.full(((n + 1) * M * C + 4,), -12288.0, device=dev, dtype=odt)
    out = buf[mis:mis + (n + 1) * M * C].view(n + 1, M, C)
    ang = torch.full((n + 1, 3), -12288.0, device=dev)
    _lib.call("lv_fused_exp_action_fwd", _lib.ptr(mu), v.data_ptr(), F.data_ptr(), 0, out.data_ptr(), dt,
              ang.data_ptr(), n, L, C, transpose, _lib.stream())
    torch.cuda.synchronize()
    assert (out[n:].float() == -12288.0).all() and (ang[n:] == -12288.0).all(), name
    assert (buf[:mis].float() == -12288.0).all(), name
    assert torch.isfinite(out[:n].float()).all(), name
    res[name] = out[:n].contiguous().view(torch.int16 if dt == T.BF16 else torch.int32).cpu().numpy()
    res[name + "_ang"] = ang[:n].view(torch.int32).cpu().numpy()
    p = _lib.plan("fwd", 1, 0, dt, n, L, C)
    fetch = _lib.fwd_chain(1, 0, dt, n, L, C)["chain_fetch"] if hasattr(_lib.load(), "lv_ab_fwd_chain") else 1
    res[name + "_plan"] = np.array([p["tile"], p["segments"], fetch])
np.savez(sys.argv[3], **res)
"""


def _run(tmp, tag, lib, knobs):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "lie-vae_amd")
    out = str(tmp / f"{tag}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LV_")}
    env.update(knobs, LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", lib))
    subprocess.run([sys.executable, "-c", _SCRIPT, pkg, os.path.join(repo, "tests"), out, repo], env=env, check=True,
                   capture_output=True, text=True, timeout=300, cwd=repo)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def product(gpu_device, tmp_path_factory):
    """The product library (prefetch at its compile-time depths), computed once."""
    r = _run(tmp_path_factory.mktemp("prefetch"), "product", "liblievae_hip.so", {})
    for name in CASES:
        assert r[name + "_plan"][0] == 1, name  # every case runs the tile kernel
    return r


@pytest.fixture(scope="module")
def depth0(gpu_device, tmp_path_factory):
    """The A/B library with the old order: every LDS read right before its use."""
    r = _run(tmp_path_factory.mktemp("prefetch0"), "depth0", "liblievae_hip_ab.so", {"LV_TILE_PREFETCH": "0"})
    for name in CASES:
        assert tuple(r[name + "_plan"][[0, 2]]) == (1, 0), name
    return r


def _assert_same(r, ref, what):
    for name in CASES:
        assert np.array_equal(r[name], ref[name]), (what, name)
        assert np.array_equal(r[name + "_ang"], ref[name + "_ang"]), (what, name, "angles")


def test_product_equals_depth0_bitwise(product, depth0):
    _assert_same(product, depth0, "product vs depth 0")
    for name in CASES:
        assert tuple(product[name + "_plan"][:2]) == tuple(depth0[name + "_plan"][:2]), name


def test_ab_library_by_default_is_the_product(gpu_device, tmp_path, product):
    r = _run(tmp_path, "ab", "liblievae_hip_ab.so", {})
    for name in CASES:
        assert tuple(r[name + "_plan"]) == (1, product[name + "_plan"][1], 1), name
    _assert_same(r, product, "A/B default vs product")


@pytest.mark.parametrize("nseg", [2, 1])
def test_few_wave_plans_bitwise(gpu_device, tmp_path, product, depth0, nseg):
    """l = 10 in 2 waves and in 1 (LV_TILE_NSEG): degree sets of 5+ degrees per wave, with
    and without the prefetch; the degree sets do not change a value, so both also equal the
    product's 7-wave plan."""
    on = _run(tmp_path, "on", "liblievae_hip_ab.so", {"LV_TILE_NSEG": str(nseg)})
    off = _run(tmp_path, "off", "liblievae_hip_ab.so", {"LV_TILE_NSEG": str(nseg), "LV_TILE_PREFETCH": "0"})
    for name, (n, L, C, dt, with_mu, transpose, mis) in CASES.items():
        if L == 10 and C == 10:
            assert tuple(on[name + "_plan"]) == (1, nseg, 1) and tuple(off[name + "_plan"]) == (1, nseg, 0), name
    _assert_same(on, off, f"nseg {nseg}: prefetch vs depth 0")
    _assert_same(on, product, f"nseg {nseg} vs product")


@pytest.fixture(scope="module")
def oracle():
    """fp32 and fp64 oracle outputs of every case, computed once."""
    from oracle import lie_ref
    refs = {}
    for name, (n, L, C, dt, with_mu, transpose, mis) in CASES.items():
        v, F, w = _inputs(name)
        pair = []
        for ft in (torch.float32, torch.float64):
            z = lie_ref.so3_exp(v.to(ft))
            if with_mu:
                z = lie_ref.so3_exp(w).to(ft) @ z
            pair.append(lie_ref.block_wigner_apply(lie_ref.mat_to_eazyz(z), F.to(ft).expand(n, -1, -1), L,
                                                   bool(transpose)).numpy())
        refs[name] = pair
    return refs


@pytest.mark.parametrize("name", list(CASES))
def test_vs_oracle(product, oracle, name):
    """The tolerance of test_fused_vs_oracle_config2 (assert_parity_fp64).  The bf16 case
    cannot meet an fp32 bound by its format (8 significant bits): it takes the bound of
    test_action_bf16_output, 4e-3 normwise per sample."""
    from test_gpu_parity import assert_normwise, assert_parity_fp64
    n, L, C, dt, with_mu, transpose, mis = CASES[name]
    ref32, ref64 = oracle[name]
    if dt == BF16:
        y = torch.from_numpy(product[name].copy()).view(torch.bfloat16).float().numpy()
        assert_normwise(y.reshape(n, -1), ref64.reshape(n, -1), 4e-3, what=name)
    else:
        y = product[name].view(np.float32)
        assert_parity_fp64(y.reshape(n, -1), ref32.reshape(n, -1), ref64.reshape(n, -1), what=name)
