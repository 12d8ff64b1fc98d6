"""Start-up path of the forward tile kernel (action_fwd.h fwd_tile_body): the launch
arguments fetched in one batch, v / ang_out addressed through buffer resources based at the
group's first sample, the spectrum staged in as many slots as the block has threads for, the
angle maths of ang_out on either side of the prologue barrier (ang_order).  The shapes are the ones at which that
code can go wrong: ragged and tiny groups, every block shape (1 to 8 waves), run-time C,
degrees 0, 1 and the first from kTrigLdsMinL, a misaligned output, inputs that start
mid-allocation, and a batch whose output passes 2^31 bytes.

Outputs against oracle/lie_ref.py in fp64 with the config-2 parity test's rule (test_gpu_parity
assert_parity_fp64, tol 1e-5) for fp32 and the action matrix's 4e-3 for a bf16 output; every
variation of one shape (angles wanted or not, output alignment, input views, block shape,
angle placement) bit for bit against the plain run of that shape.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import assert_normwise, assert_parity_fp64, host

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
BF16_TOL = 4e-3  # tests/test_gpu_action_matrix.py check_run: a bf16 output against fp64
SENTINEL = -12288.0  # exact in bf16


class Shape:
    """Inputs of one (l, C) and the oracle's outputs on their first `rows` samples, computed
    once per (l, C, transpose)."""
    _cache = {}

    def __init__(self, L, C, n=13):
        g = torch.Generator().manual_seed(100 * L + C)
        self.L, self.C, self.n = L, C, n
        self.v = torch.randn(n, 3, generator=g)
        self.F = torch.randn((L + 1) ** 2, C, generator=g)
        self._ref = {}

    @classmethod
    def get(cls, L, C, n=13):
        key = (L, C, n)
        if key not in cls._cache:
            cls._cache[key] = cls(L, C, n)
        return cls._cache[key]

    def oracle(self, transpose, rows=None):
        """(fp32, fp64) oracle outputs of the samples `rows` (default: all), (len, M*C)."""
        key = (bool(transpose), None if rows is None else tuple(rows))
        if key not in self._ref:
            from oracle import lie_ref
            v = self.v if rows is None else self.v[list(rows)]
            res = []
            for dt in (torch.float32, torch.float64):
                a = lie_ref.mat_to_eazyz(lie_ref.so3_exp(v.to(dt)))
                y = lie_ref.block_wigner_apply(a, self.F.to(dt).expand(len(v), -1, -1), self.L,
                                               bool(transpose))
                res.append(y.double().numpy().reshape(len(v), -1))
            self._ref[key] = tuple(res)
        return self._ref[key]


def fwd(device, v, F, L, n, dtype=F32, want_ang=True, transpose=0, out_shift=0, out=None, ang=None):
    """lv_fused_exp_action_fwd (mu = NULL) on the first n rows of the device tensor v.  The
    output starts out_shift bytes into a 16-byte aligned allocation; one sample of padding
    after out and ang_out holds a sentinel the kernel must leave alone.  Returns (out, ang)."""
    from lie_vae import _lib
    M, C = F.shape
    esz = 2 if dtype == BF16 else 4
    tdt = torch.bfloat16 if dtype == BF16 else torch.float32
    if out is None:
        raw = torch.full(((n + 1) * M * C + 16,), SENTINEL, device=device, dtype=tdt)
        assert raw.data_ptr() % 16 == 0 and out_shift % esz == 0
        out = raw[out_shift // esz:out_shift // esz + (n + 1) * M * C].view(n + 1, M, C)
    if ang is None and want_ang:
        ang = torch.full((n + 1, 3), SENTINEL, device=device)
    _lib.call("lv_fused_exp_action_fwd", None, v.data_ptr(), F.data_ptr(), 0, out.data_ptr(), dtype,
              ang.data_ptr() if want_ang else None, n, L, C, int(transpose), _lib.stream())
    torch.cuda.synchronize(device)
    assert (out[n:].float() == SENTINEL).all(), "wrote past the last sample of out"
    if want_ang:
        assert (ang[n:] == SENTINEL).all(), "wrote past the last sample of ang_out"
        assert torch.isfinite(ang[:n]).all()
    return out[:n], (ang[:n] if want_ang else None)


def check_oracle(y, shape, transpose, dtype, what, rows=None):
    y32, y64 = shape.oracle(transpose, rows)
    y = host(y.float()).reshape(len(y64), -1)
    assert np.isfinite(y).all(), what
    if dtype == BF16:
        assert_normwise(y, y64, BF16_TOL, what=what)
    else:
        assert_parity_fp64(y, y32, y64, what=what)


@pytest.mark.parametrize("n", [1, 5, 6, 7, 13])
def test_ragged_and_tiny_groups(gpu_device, n):
    """One partial group, one full group, a full and a partial one: angles wanted and not,
    both transposes, both output types."""
    sh = Shape.get(10, 10)
    v, F = sh.v.to(gpu_device), sh.F.to(gpu_device)
    rows = range(n)
    full = fwd(gpu_device, v, F, 10, sh.n)[1]  # the angles of all 13 samples
    for transpose in (0, 1):
        for dtype in (F32, BF16):
            what = f"n={n} T={transpose} dtype={dtype}"
            y, ang = fwd(gpu_device, v, F, 10, n, dtype, True, transpose)
            check_oracle(y, sh, transpose, dtype, what, rows)
            y0, _ = fwd(gpu_device, v, F, 10, n, dtype, False, transpose)
            assert torch.equal(y0, y), what + ": the output depends on ang_out"
            # the saved angles are those of z = exp(v), whatever the group split, the output
            # type and the transpose
            assert torch.equal(ang, full[:n]), what


@pytest.mark.parametrize("L,C", [(3, 7), (10, 7), (0, 10), (1, 10), (13, 10)])
def test_runtime_c_and_edge_degrees(gpu_device, L, C):
    """Run-time C (C = 7: 9 samples per group, column-major spectrum slices) at l = 3 and 10;
    compile-time C at degrees 0, 1 and 13 (the first l >= kTrigLdsMinL); two groups each."""
    sh = Shape.get(L, C)
    v, F = sh.v.to(gpu_device), sh.F.to(gpu_device)
    for dtype in (F32, BF16):
        for transpose in (0, 1):
            y, _ = fwd(gpu_device, v, F, L, sh.n, dtype, True, transpose)
            check_oracle(y, sh, transpose, dtype, f"l={L} C={C} T={transpose} dtype={dtype}")


def test_product_block_shapes(gpu_device):
    """Every wave count the product plans at C = 10 stages the whole spectrum: the l_max and
    batch at which the planner picks 1, 2, ..., 8 waves (read from the plan), each against the
    oracle on its first and last 13 samples."""
    from lie_vae import _lib
    seen = set()
    for L, n in [(0, 13), (2, 13), (3, 13), (4, 13), (5, 13), (6, 13), (8, 13), (10, 13), (10, 16389),
                 (10, 65537)]:
        waves = _lib.plan("fwd", 1, 0, F32, n, L, 10)["segments"]
        if (waves, L) in seen:
            continue
        seen.add((waves, L))
        sh = Shape.get(L, 10, n)
        y, _ = fwd(gpu_device, sh.v.to(gpu_device), sh.F.to(gpu_device), L, n)
        rows = sorted(set(range(min(13, n))) | set(range(max(0, n - 13), n)))
        check_oracle(y[rows], sh, 0, F32, f"l={L} n={n} waves={waves}", rows)
    assert {w for w, _ in seen} >= {1, 2, 4, 7, 8}, seen


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_misaligned_output(gpu_device, dtype):
    """An output that starts 4, 8 and 12 bytes past a 16-byte boundary (tile_flush's head /
    body / tail split) holds the aligned run's values."""
    sh = Shape.get(10, 10)
    v, F = sh.v.to(gpu_device), sh.F.to(gpu_device)
    y0, a0 = fwd(gpu_device, v, F, 10, sh.n, dtype)
    check_oracle(y0, sh, 0, dtype, f"aligned dtype={dtype}")
    for shift in (4, 8, 12) + ((2, 14) if dtype == BF16 else ()):
        y, a = fwd(gpu_device, v, F, 10, sh.n, dtype, out_shift=shift)
        assert y.data_ptr() % 16 == shift
        assert torch.equal(y, y0) and torch.equal(a, a0), shift


def test_inputs_mid_allocation(gpu_device):
    """v and ang_out as views that start 5 and 3 samples into their allocations (60 and 36
    bytes: 4-byte aligned only), for every ragged n."""
    sh = Shape.get(10, 10)
    F = sh.F.to(gpu_device)
    vbig = torch.full((sh.n + 9, 3), 7.0, device=gpu_device)
    vbig[5:5 + sh.n] = sh.v.to(gpu_device)
    for n in (1, 7, 13):
        y0, a0 = fwd(gpu_device, sh.v.to(gpu_device), F, 10, n)
        abig = torch.full((n + 8, 3), SENTINEL, device=gpu_device)
        y, a = fwd(gpu_device, vbig[5:], F, 10, n, ang=abig[3:3 + n + 1])
        assert torch.equal(y, y0) and torch.equal(a, a0), n
        assert (abig[:3] == SENTINEL).all() and (abig[3 + n:] == SENTINEL).all(), n


def test_output_past_2gib(gpu_device):
    """450,000 samples at the config-2 width: the last group's output starts 2.18 GB into the
    tensor, past what a 32-bit byte offset from its base reaches.  First and last 12 samples
    against the oracle; the last sample of v / ang_out sits 5.4 MB in."""
    n, L, C = 450_000, 10, 10
    M = (L + 1) ** 2
    assert (n - 12) * M * C * 4 > 2 ** 31
    sh = Shape.get(L, C, n)
    v, F = sh.v.to(gpu_device), sh.F.to(gpu_device)
    out = torch.empty(n + 1, M, C, device=gpu_device)
    out[n:] = SENTINEL
    out[:12] = SENTINEL
    out[n - 12:n] = SENTINEL
    y, ang = fwd(gpu_device, v, F, L, n, out=out)
    rows = list(range(12)) + list(range(n - 12, n))
    check_oracle(y[rows], sh, 0, F32, "n=450,000", rows)
    small, ang_small = fwd(gpu_device, v[n - 12:].clone(), F, L, 12)
    assert torch.equal(y[n - 12:], small) and torch.equal(ang[n - 12:], ang_small)
    del out, y


_AB_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import test_fwd_prologue as t
from lie_vae import _lib
dev = torch.device("cuda:0")
res = {}
for n in (13, 16389):
    sh = t.Shape.get(10, 10, n)
    y, a = t.fwd(dev, sh.v.to(dev), sh.F.to(dev), 10, n)
    res[f"y{n}"], res[f"a{n}"] = y.cpu().numpy(), a.cpu().numpy()
    res[f"w{n}"] = _lib.plan("fwd", 1, 0, 0, n, 10, 10)["segments"]
np.savez(sys.argv[3], **res)
"""


def _ab_run(tmp_path, tag, lib, extra):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(repo, "lie-vae_amd")
    out = str(tmp_path / f"{tag}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LV_")}
    env.update(extra, LIEVAE_HIP_LIB=os.path.join(pkg, "lie_vae", lib))
    subprocess.run([sys.executable, "-c", _AB_SCRIPT, pkg, os.path.join(repo, "tests"), out], env=env,
                   check=True, capture_output=True, text=True, timeout=300)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def product_run(gpu_device, tmp_path_factory):
    return _ab_run(tmp_path_factory.mktemp("prologue"), "product", "liblievae_hip.so", {})


@pytest.mark.parametrize("knobs", [
    {"LV_TILE_ANG_ORDER": "0"},                        # the angle maths ahead of the barrier
    {"LV_TILE_ANG_ORDER": "1"},                        # ... behind it (lighter degree sets)
    {"LV_TILE_NSEG": "2"},                             # 2 waves: 10 staging slots per thread
    {"LV_TILE_NSEG": "2", "LV_TILE_ANG_ORDER": "1"},  # all three angles from wave 1, behind it
    {"LV_TILE_NSEG": "3", "LV_TILE_SPREAD": "1"},      # 3 waves, tasks spread over them
    {"LV_TILE_NSEG": "1"},                             # 1 wave: the staging loop past the slots
], ids=lambda k: json.dumps(k, separators=(",", ":")))
def test_block_shape_and_angle_placement_bitwise(gpu_device, tmp_path, product_run, knobs):
    """The A/B library (the same kernels with the planner's knobs and the timeline stamps
    compiled in) at forced block shapes and with the angle maths on either side of the
    prologue barrier: the product library's output and angles bit for bit, at 13 and 16,389
    samples.  (The product run itself is checked against the oracle above.)"""
    r = _ab_run(tmp_path, "ab", "liblievae_hip_ab.so", knobs)
    if "LV_TILE_NSEG" in knobs:
        assert r["w13"] == r["w16389"] == int(knobs["LV_TILE_NSEG"])
    for n in (13, 16389):
        assert np.array_equal(r[f"y{n}"], product_run[f"y{n}"]), (knobs, n)
        assert np.array_equal(r[f"a{n}"], product_run[f"a{n}"]), (knobs, n)
