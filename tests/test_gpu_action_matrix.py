"""The group-action kernels over their whole dispatch space, against the fp64 oracle.

The kernels are instantiated once per l_max (21 forward and 21 backward units, each with its
own literal J products) and dispatch at run time on C == 10 / run-time C, shared / per-sample
spectrum, fused / angle input, fp32 / bf16 output and the backward plan mode; the rest of
the suite is deep at l = 10, C = 10.  This module runs the case table of
tests/action_matrix_cases.py (which tests/test_plan.py classifies by dispatch branch on the
CPU): every degree, the persistent backward at every degree it serves, the channel classes
of the run-time-C kernels, looped grids and boundary angles.

Inputs per case, seeded from (L, C, n): Haar angles mat_to_eazyz(haar_matrices(n)), fused
inputs mu = haar_matrices(n) and v = 0.5 randn, spectrum and gout randn.  The oracle
(oracle/lie_ref.py, autograd) reads the same fp32 inputs cast up to fp64; its own fp32 run
is computed only where a 2x rule needs it.  Tolerances are the suite's: forward from angles
1e-5 per sample, angle gradient 1e-4 per sample (assert_grad_parity from 1,000 samples),
shared dF 1e-5 over the (M, C) matrix, per-sample dF 1e-4 per sample, bf16 output 4e-3 per
sample, fused forward assert_parity_fp64, fused gmu / gv assert_grad_parity; at l = 0 every
angle, v and mu gradient is exactly zero.

What it found: the fused backward missed assert_grad_parity at two seeded samples near
beta = 0 / pi (persistent section, l = 6 without a mean: gv off by 9.8e-4 against a
reference fp32 worst of 2.8e-4; l = 9 with a mean: gmu 2.2e-4 against 6.2e-5).  The forward
saved beta = acos(fp32 cos), 1.7e-5 off at beta = 0.009, and the exp -> ZYZ VJP ran in fp32;
with beta saved from the forward's own (cos, sin) pair and the VJP in fp64 the worst fused
gv / gmu over the whole table is 3e-5.  Each check prints its measured figure before it
asserts ("matrix: ..." lines, visible with -s / -rP)."""
import numpy as np
import pytest
import torch

import action_matrix_cases as amc
from test_gpu_parity import (_oracle_grads, assert_grad_parity, assert_normwise,
                             assert_parity_fp64, host, normwise)

pytestmark = pytest.mark.gpu


def _report(case, run, what, err, bound):
    print(f"matrix: {case.section} l={case.L} C={case.C} n={case.n} {run.path}"
          f"{'' if run.shared else ' per-sample'}{' T' if run.transpose else ''}"
          f"{' bf16' if run.bf16 else ''} {what} {err:.3e} (bound {bound:.1e})")


class Inputs:
    """The seeded inputs of one case (CPU, fp32), the per-sample tensors made on demand."""

    def __init__(self, case):
        from oracle import lie_ref
        self.case = case
        n, M, C = case.n, (case.L + 1) ** 2, case.C
        torch.manual_seed(amc.seed(case))  # haar_matrices draws from the global generator
        self.gen = torch.Generator().manual_seed(amc.seed(case))
        if case.section == "boundary":
            self.ang = torch.tensor(amc.boundary_angles(), dtype=torch.float32)
        else:
            self.ang = lie_ref.mat_to_eazyz(lie_ref.haar_matrices(n))
        self.mu = lie_ref.haar_matrices(n)
        self.v = 0.5 * torch.randn(n, 3, generator=self.gen)
        self.F = torch.randn(M, C, generator=self.gen)
        self.gout = torch.randn(n, M, C, generator=self.gen)
        self._Fs = None
        self._oracle = {}

    @property
    def Fs(self):
        if self._Fs is None:
            c = self.case
            self._Fs = torch.randn(c.n, (c.L + 1) ** 2, c.C, generator=self.gen)
        return self._Fs

    def leaves(self, run):
        """Differentiable inputs of the run besides the spectrum, in gradient order."""
        return {"angles": [self.ang], "fused_mu": [self.mu, self.v], "fused_nomu": [self.v]}[run.path]

    def oracle(self, run, dtype):
        """The oracle's forward (n, M*C) and autograd gradients (dF, [input gradients]) of
        the run in dtype: angles -> D·F, or the fused chain mu @ exp(v) -> ZYZ -> D·F
        (exp(v) without a mean).  One evaluation per (path, spectrum, transpose, dtype)."""
        from oracle import lie_ref
        key = (run.path, run.shared, run.transpose, dtype)
        if key not in self._oracle:
            n, L = self.case.n, self.case.L
            f = (self.F if run.shared else self.Fs).to(dtype).clone().requires_grad_(True)
            xs = [t.to(dtype).clone().requires_grad_(True) for t in self.leaves(run)]
            if run.path == "angles":
                a = xs[0]
            elif run.path == "fused_mu":
                a = lie_ref.mat_to_eazyz(lie_ref.so3_sample(xs[0], xs[1]))
            else:
                a = lie_ref.mat_to_eazyz(lie_ref.so3_exp(xs[0]))
            y = lie_ref.block_wigner_apply(a, f.expand(n, -1, -1) if run.shared else f, L, run.transpose)
            (y * self.gout.to(dtype)).sum().backward()
            self._oracle[key] = (y.detach().double().numpy().reshape(n, -1), f.grad.double().numpy(),
                                 [x.grad.double().numpy().reshape(n, -1) for x in xs])
        return self._oracle[key]


def hip_run(inp, run, device):
    """The run on the HIP path: output (n, M*C) as fp32, dF and the input gradients."""
    import lie_vae._ops as ops
    L = inp.case.L
    f = (inp.F if run.shared else inp.Fs).to(device).requires_grad_(run.bwd)
    xs = [t.to(device).requires_grad_(run.bwd) for t in inp.leaves(run)]
    od = torch.bfloat16 if run.bf16 else torch.float32
    if run.path == "angles":
        y = ops.group_action(xs[0], f, L, transpose=run.transpose, out_dtype=od)
    else:
        mu = xs[0] if run.path == "fused_mu" else None
        y = ops.fused_exp_action(mu, xs[-1], f, L, transpose=run.transpose, out_dtype=od)
    assert y.dtype == od and y.shape == inp.gout.shape
    if not run.bwd:
        return host(y.float()).reshape(inp.case.n, -1), None, None
    (y * inp.gout.to(device)).sum().backward()
    return (host(y.float()).reshape(inp.case.n, -1), host(f.grad),
            [host(x.grad).reshape(inp.case.n, -1) for x in xs])


def check_grads(case, run, gF, gx, gF64, gx64, gx32):
    """dF and the input gradients of one run against the oracle's (gx32: the oracle's own
    fp32 gradients where assert_grad_parity is the check, else None)."""
    n = case.n
    if run.shared:
        _report(case, run, "dF", normwise(gF[None], gF64[None]).max(), 1e-5)
        assert_normwise(gF[None], gF64[None], 1e-5, what=f"dF {case} {run}")
    else:
        _report(case, run, "dF per sample", normwise(gF.reshape(n, -1), gF64.reshape(n, -1)).max(), 1e-4)
        assert_normwise(gF.reshape(n, -1), gF64.reshape(n, -1), 1e-4, what=f"dF {case} {run}")
    names = {"angles": ["gang"], "fused_mu": ["gmu", "gv"], "fused_nomu": ["gv"]}[run.path]
    for k, name in enumerate(names):
        assert np.isfinite(gx[k]).all(), (name, case, run)
        if case.L == 0:
            # D_0 = 1: nothing depends on the rotation, and the normwise helpers divide by
            # the reference's norm
            assert not gx64[k].any() and not gx[k].any(), f"{name} not exactly zero at l = 0: {case} {run}"
            continue
        _report(case, run, name, normwise(gx[k], gx64[k]).max(), 1e-4)
        if gx32 is not None:
            _report(case, run, name + " oracle fp32", normwise(gx32[k], gx64[k]).max(), 1e-4)
            assert_grad_parity(gx[k], gx32[k], gx64[k], what=f"{name} {case} {run}")
        else:
            assert_normwise(gx[k], gx64[k], 1e-4, what=f"{name} {case} {run}")


def check_run(inp, run, device):
    """One run of the table, forward and (run.bwd) backward, against the fp64 oracle."""
    case = inp.case
    y, gF, gx = hip_run(inp, run, device)
    y64, gF64, gx64 = inp.oracle(run, torch.float64)
    fused = run.path != "angles"
    # the 2x rules read the oracle's own fp32 error: the fused path (fp32 Euler extraction
    # sets the floor) and angle gradients from 1,000 samples
    need32 = fused or case.n >= 1000
    assert np.isfinite(y).all(), (case, run)
    if run.fwd:
        if run.bf16:
            _report(case, run, "out", normwise(y, y64).max(), 4e-3)
            assert_normwise(y, y64, 4e-3, what=f"bf16 out {case} {run}")
        elif fused:
            y32 = inp.oracle(run, torch.float32)[0]
            _report(case, run, "out", normwise(y, y64).max(), 1e-5)
            _report(case, run, "out oracle fp32", normwise(y32, y64).max(), 1e-5)
            assert_parity_fp64(y, y32, y64, what=f"fused out {case} {run}")
        else:
            _report(case, run, "out", normwise(y, y64).max(), 1e-5)
            assert_normwise(y, y64, 1e-5, what=f"out {case} {run}")
    if run.bwd:
        gx32 = inp.oracle(run, torch.float32)[2] if need32 else None
        check_grads(case, run, gF, gx, gF64, gx64, gx32)


def _ids(cases):
    return [f"l{c.L}-C{c.C}-n{c.n}{'' if c.shared else '-per-sample'}" for c in cases]


# ------------------------------------------------- 1. every degree at the product's C
@pytest.mark.parametrize("case", amc.DEGREE_SWEEP, ids=_ids(amc.DEGREE_SWEEP))
def test_degree_sweep(gpu_device, case):
    """Each l_max instantiation at C = 10, n = 37 (six full groups and a ragged one): angle
    path with a shared and a per-sample spectrum (plan mode 0), the fused operator with
    (odd l) and without (even l) a mean, forward and backward; bf16 forward from angles and
    fused.  The backward's samples per group: 6 up to l = 15, fewer above (the reduced-group
    kernels ran)."""
    spg = amc.bwd_plan(case, amc.sweep_runs(case.L)[0])["samples_per_group"]
    assert spg == 6 if case.L <= 15 else 1 <= spg < 6, spg
    assert amc.bwd_plan(case, amc.sweep_runs(case.L)[1])["tile"] == 0
    inp = Inputs(case)
    for run in amc.runs(case):
        check_run(inp, run, gpu_device)


# ------------------------------------- 2. the persistent backward at every degree it serves
def _backward_twice(inp, run, device):
    """Two runs of the backward, bitwise equal; the first one's (dF, input gradients)."""
    res = [hip_run(inp, run, device)[1:] for _ in range(2)]
    (gF, gx), (gF2, gx2) = res
    assert np.array_equal(gF, gF2), ("dF not reproducible", inp.case, run)
    for a, b in zip(gx, gx2):
        assert np.array_equal(a, b), ("input gradients not reproducible", inp.case, run)
    return gF, gx


def _check_backward_whole_batch(inp, run, device):
    """Backward of a shared-spectrum run, twice (bitwise equal), against the oracle's fp64
    autograd over the whole batch (_oracle_grads): dF 1e-5, input gradients by
    assert_grad_parity."""
    case = inp.case
    gF, gx = _backward_twice(inp, run, device)
    if run.path == "angles":
        args = (None, None, inp.ang)
    else:  # no mean: the identity (mu @ exp(v) = exp(v) exactly), its gradient dropped
        mu = inp.mu if run.path == "fused_mu" else torch.eye(3).expand(case.n, 3, 3)
        args = (mu, inp.v, None)
    gF64, g64 = _oracle_grads(*args, inp.F, inp.gout, case.L, run.transpose)
    _, g32 = _oracle_grads(*args, inp.F, inp.gout, case.L, run.transpose, torch.float32)
    if run.path == "fused_nomu":
        g64, g32 = g64[1:], g32[1:]
    check_grads(case, run, gF, gx, gF64, g64, g32)


@pytest.mark.parametrize("case", amc.PERSIST, ids=_ids(amc.PERSIST))
def test_persistent_backward_every_degree(gpu_device, case):
    """Plan mode 3 (action_bwd_persist.h, its own degree sets per l) takes over from CUs + 1
    groups for 3 <= l <= 10; every other test of it runs l = 10.  At 6 (CUs + 1) + 5 samples,
    l = 3..9: the angle-path and the fused backward (VJP beside the reduce) against the
    oracle over the whole batch, bitwise reproducible; transposed for even l.  l = 0, 1, 2 at
    the same size stay on the one-group kernel (mode 1): the same comparison."""
    runs = amc.runs(case)
    assert amc.bwd_plan(case, runs[0])["tile"] == (3 if case.L >= 3 else 1)
    inp = Inputs(case)
    for run in runs:
        _check_backward_whole_batch(inp, run, gpu_device)


# ------------------------------------------ 3. channel classes of the run-time-C kernels
@pytest.mark.parametrize("C", amc.CHANNEL_CS)
def test_channel_classes(gpu_device, C):
    """Run-time C at every samples-per-group class (64, 32, 21, 9, 5, 4, 3, 2, and 1 from
    C = 33), two full groups and a ragged one, on both sides of l = 13 (spectrum in LDS below,
    from global memory from there; trig tables in LDS from there): the runs of the degree
    sweep at l = 1, 5, 12, 13, 16."""
    cases = [c for c in amc.CHANNELS if c.C == C]
    assert [c.L for c in cases] == list(amc.CHANNEL_LS)
    for case in cases:
        assert case.n == max(5, 2 * amc.fwd_plan(case, amc.sweep_runs(case.L)[0])["samples_per_group"] + 1)
        inp = Inputs(case)
        for run in amc.runs(case):
            check_run(inp, run, gpu_device)


@pytest.mark.parametrize("case", amc.L20_FUSED, ids=_ids(amc.L20_FUSED))
def test_l20_fused_grid_stride(gpu_device, case):
    """l = 20 with fp32 output: the fused forward is the grid-stride kernel (no tile plan
    fits), and at C = 11 the backward runs one sample per block."""
    (run,) = amc.runs(case)
    assert amc.fwd_plan(case, run)["tile"] == 0
    spg = amc.bwd_plan(case, run)["samples_per_group"]
    assert spg == 1 if case.C == 11 else 1 < spg < 6, spg
    check_run(Inputs(case), run, gpu_device)


@pytest.mark.parametrize("case", amc.EDGES, ids=_ids(amc.EDGES))
def test_channel_edges(gpu_device, case):
    """One or two channels at the ends of the degree range, the runs of the degree sweep: at
    l = 0 a block has one wave, too few for 64 // C samples (grid-stride forward, reduced
    backward group); at l = 19, 20 with C = 1 the bf16 forward is the grid-stride kernel."""
    runs = amc.runs(case)
    assert amc.fwd_plan(case, runs[-1])["tile"] == 0  # bf16, fused
    if case.L == 0:
        assert amc.bwd_plan(case, runs[0])["samples_per_group"] < 64 // case.C
    inp = Inputs(case)
    for run in runs:
        check_run(inp, run, gpu_device)


# ------------------------------------------------------------------- 4. looped grids
@pytest.mark.parametrize("case", amc.LOOPED, ids=_ids(amc.LOOPED))
def test_looped_grids(gpu_device, case):
    """Backward grids capped below the number of sample groups (4,096 blocks, 1,024 in the
    global-spectrum fallback, 3 per CU in the persistent kernel), so blocks loop over several
    groups: dF and the angle gradients against the oracle's fp64 autograd over the whole
    batch, bitwise reproducible run to run.  (The l = 20 case's whole-batch oracle, fp64 and
    fp32, takes 5 to 9 s on the host -- the whole test ran 5.5 s -- so it is compared whole
    like the others.)"""
    (run,) = amc.runs(case)
    p = amc.bwd_plan(case, run)
    assert p["blocks"] < amc.bwd_groups(case, p), p
    inp = Inputs(case)
    if run.shared:
        _check_backward_whole_batch(inp, run, gpu_device)
    else:
        gF, gx = _backward_twice(inp, run, gpu_device)
        _, gF64, gx64 = inp.oracle(run, torch.float64)
        check_grads(case, run, gF, gx, gF64, gx64, inp.oracle(run, torch.float32)[2])


# ---------------------------------------------------------------- 5. boundary angles
@pytest.mark.parametrize("case", amc.BOUNDARY, ids=_ids(amc.BOUNDARY))
def test_boundary_angles(gpu_device, case):
    """Angles on the edges of the extraction's ranges (amc.boundary_angles: alpha, gamma in
    {-pi, -pi/2, 0, pi/2, pi} x beta in {0, pi/2, pi}, and beta within 1e-6 of 0 and pi),
    given as angles, so no Euler extraction is involved: forward 1e-5 and angle gradient 1e-4
    per sample against the oracle on the same angles, everything finite; where the
    reference's gradient is exactly zero, |g| <= 1e-4 ||gout|| ||F||."""
    (run,) = amc.runs(case)
    inp = Inputs(case)
    assert inp.ang.shape == (case.n, 3)
    y, gF, (ga,) = hip_run(inp, run, gpu_device)
    y64, gF64, (ga64,) = inp.oracle(run, torch.float64)
    assert np.isfinite(y).all() and np.isfinite(ga).all() and np.isfinite(gF).all()
    _report(case, run, "out", normwise(y, y64).max(), 1e-5)
    assert_normwise(y, y64, 1e-5, what=f"out {case}")
    _report(case, run, "dF", normwise(gF[None], gF64[None]).max(), 1e-5)
    assert_normwise(gF[None], gF64[None], 1e-5, what=f"dF {case}")
    zero = ~ga64.any(axis=1)
    if zero.any():
        scale = np.linalg.norm(inp.gout.numpy().reshape(case.n, -1), axis=1) * np.linalg.norm(inp.F.numpy())
        worst = (np.linalg.norm(ga[zero], axis=1) / scale[zero]).max()
        _report(case, run, f"gang at {zero.sum()} zero-gradient samples / (|gout| |F|)", worst, 1e-4)
        assert worst <= 1e-4
    _report(case, run, "gang", normwise(ga[~zero], ga64[~zero]).max(), 1e-4)
    assert_normwise(ga[~zero], ga64[~zero], 1e-4, what=f"gang {case}")
