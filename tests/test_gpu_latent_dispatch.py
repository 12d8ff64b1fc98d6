"""GPU checks of the SO(3) normal latent kernels of csrc/pointwise.hip over their dispatch space
(lv_so3_log_posterior_*: wave and thread kernels, forward and backward; lv_softplus_*,
lv_n0_sample_*, lv_so3_sample_*; the grid-stride loop all of them share) against the fp64
oracle of tests/latent_cases.py, whose conditions tests/test_latent_cases_cpu.py asserts.

The density is graded per cell (a radius band of |v| x a class of sigma): a sample passes when
its error against fp64 is within the project's bounds for this op (values rtol 1e-5 + atol 1e-4,
gradients 1e-4 normwise per sample for gv and per b for gsigma) or within 2x the worst
fp32-oracle error of its own cell.  Every density test prints its worst ratio of error to bound
and takes its kernel from lv_so3_log_posterior_plan."""
import math

import numpy as np
import pytest
import torch

import latent_cases as lc

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL_F, TOL_G = 1e-5, 1e-4  # the project's normwise bounds, forward / gradients


def host(t):
    return t.detach().cpu().numpy()


_runs = {}


def density(device, k, ns, B, stride=1):
    """One forward + backward of the density on `latent_cases.inputs`, cached per shape (the
    tiled runs serve the grading and the cross-kernel tests); returns (plan, lp, gv, gsigma)."""
    import lie_vae._ops as ops
    from lie_vae import _lib
    key = (k, ns, B, stride)
    if key not in _runs:
        v, sigma, gout = lc.inputs(lc.case(k), ns, B, stride)
        vg = v.to(device).requires_grad_(True)
        sg = sigma.to(device).requires_grad_(True)
        lp = ops.so3_log_posterior(vg, sg, k)
        assert lp.shape == (ns, B) and lp.dtype == F32
        (lp * gout.to(device)).sum().backward()
        _runs[key] = (_lib.so3_log_posterior_plan(ns, B, k), host(lp), host(vg.grad), host(sg.grad))
    return _runs[key]


def check_density(device, k, ns, B, fwd_wave, bwd_wave, stride=1):
    plan, lp, gv, gs = density(device, k, ns, B, stride)
    assert (plan["fwd_wave"], plan["bwd_wave"]) == (int(fwd_wave), int(bwd_wave)), plan
    for a in (lp, gv, gs):
        assert np.isfinite(a).all()
    res = lc.grade(lc.case(k), ns, B, lp, gv, gs, stride)
    print(f"k={k} ns={ns} B={B} fwd {'wave' if fwd_wave else 'thread'} bwd "
          f"{'wave' if bwd_wave else 'thread'}: worst error / bound " +
          ", ".join(f"{w} {r:.3f}" for w, (r, _) in res.items()))
    for what, (r, where) in res.items():
        assert r <= 1.0, where
    return res


# ------------------------------------------------------------------ the density
@pytest.mark.parametrize("k", lc.KS)
def test_density_k_sweep(gpu_device, k):
    """ns = 3, B = 240 (20 samples a cell on average) at every k class: 0 (one live lane, -inf
    in the other 63), 1, 2, 10, 31 (63 of 64 lanes), 32 and 33 (first thread-kernel sizes), 64
    (the limit); k <= 31 wave, k >= 32 thread, both directions.  The broad sigma class makes the
    outermost term carry weight (test_latent_cases_cpu.py test_last_term_is_visible).

    Measured worst error / bound on an MI355X, (lp, gv, gsigma):
    k = 0 (0.16, 0.50, 0.01), 1 (0.13, 0.50, 0.03), 2 (0.15, 0.68, 0.14), 10 (0.33, 0.50, 0.36),
    31 (0.49, 0.56, 0.50), 32 (0.51, 0.55, 0.50), 33 (0.51, 0.59, 0.68), 64 (0.51, 0.52, 0.50).
    (With the weights' exponents all in fp32, k = 1 stood at gv 1.09: sample (s = 0, b = 199),
    cell pi-1e-3 x aniso; test_density_backward_weights_at_two_modes.)"""
    check_density(gpu_device, k, lc.NS0, lc.B0, k <= 31, k <= 31)


TILED = {"wave_fwd_at_limit": (256, 256, True, True),
         "thread_fwd_wave_bwd": (257, 256, False, True),
         "wave_bwd_at_limit": (1, 65536, True, True),
         "thread_fwd_thread_bwd": (2, 65537, False, False)}


@pytest.mark.parametrize("name", TILED)
def test_density_size_dispatch(gpu_device, name):
    """k = 10 at the size thresholds, the 720 base samples tiled (each element keeps its cell
    and the cell's reference error): ns*B = 65536 exactly (wave forward at its limit), ns*B
    above with small B (thread forward, wave backward, gsigma summed over 257 s), B = 65536
    (wave backward at its limit) and B = 65537 (thread both ways).  Repeats of a sample within a
    run are bitwise equal.  Measured worst error / bound (lp, gv, gsigma): (0.33, 0.50, 0.46),
    (0.33, 0.50, 0.49), (0.24, 0.50, 0.32), (0.33, 0.50, 0.33) in the order above."""
    ns, B, fw, bw = TILED[name]
    check_density(gpu_device, 10, ns, B, fw, bw)
    _, lp, gv, _ = density(gpu_device, 10, ns, B)
    if ns > lc.NS0:
        assert np.array_equal(lp[:-lc.NS0], lp[lc.NS0:])
    if B > lc.B0:
        assert np.array_equal(lp[:, :-lc.B0], lp[:, lc.B0:])


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


@pytest.mark.parametrize("wave,thread", [("wave_fwd_at_limit", "thread_fwd_wave_bwd"),
                                         ("wave_bwd_at_limit", "thread_fwd_thread_bwd")])
def test_wave_and_thread_forward_agree(gpu_device, wave, thread):
    """The same (v, sigma) through the wave forward and the thread forward.  Both evaluate the
    same 2k+1 fp32 terms l_t and the same exact maximum m; they differ in the order in which
    they add the e_t = exp(l_t - m), all in [0, 1] with the largest equal to 1.  Each order makes
    at most 2k roundings of partial sums <= S, so |S_w - S_t| <= (2k+1) 2^-23 S, first order with
    a factor 2 to spare; log S then moves by at most (2k+1) 2^-23.  logf is within 3 ulp
    (the OpenCL bound the device library keeps) of a value <= log(2k+1), on each side: 6
    ulp(log(2k+1)).  The final m + log S rounds once on each side: ulp(out).  So
        |out_w - out_t| <= (2k+1) 2^-23 + 6 ulp(log(2k+1)) + ulp(out),
    about 4e-6 + ulp(out) at k = 10.  Measured: at most 4.8e-7 (one ulp of a value in [4, 8)),
    0.11 of the bound; 6-7% of the 65,536 pairs differ at all."""
    k = 10
    nsw, Bw = TILED[wave][:2]
    nst, Bt = TILED[thread][:2]
    pw, lw = density(gpu_device, k, nsw, Bw)[:2]
    pt, lt = density(gpu_device, k, nst, Bt)[:2]
    assert pw["fwd_wave"] == 1 and pt["fwd_wave"] == 0
    # element (s, b) is base sample (s mod 3, b mod 240) in both
    lt = lt[:nsw, :Bw]
    bound = (2 * k + 1) * 2.0 ** -23 + 6 * ulp32(math.log(2 * k + 1)) + ulp32(lw)
    d = np.abs(lw.astype(np.float64) - lt)
    print(f"{wave} vs {thread}: max |wave - thread| {d.max():.3e}, worst / bound "
          f"{(d / bound).max():.3f}, {np.count_nonzero(d)} of {d.size} differ")
    assert (d <= bound).all(), (d / bound).max()


@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("ns,B", [(1, 1), (1, 3), (17, 5), (2, 67)])
def test_density_ragged_shapes(gpu_device, ns, B, k):
    """One element, fewer elements than one block's 4 waves, B no multiple of 4 with gsigma
    summed over 17 s, and 67 b (17 wave blocks, the last a quarter full), on the wave (k = 10)
    and thread (k = 40) kernels; the columns are base columns 7b mod 240, so they span cells.
    Measured worst error / bound over the eight runs: lp 0.51, gv 0.52, gsigma 0.10."""
    check_density(gpu_device, k, ns, B, k <= 31, k <= 31, stride=7)


@pytest.mark.parametrize("k,B", [(1, 64), (40, 64)])
def test_density_backward_weights_at_large_lse(gpu_device, k, B):
    """Regression: the backward's weights are exp(l_t - m) / sum.  Formed as exp(l_t - lse)
    with lse = m + log(sum) rounded to fp32, they were all off by the rounding of lse, up to
    half an ulp of |log q|: 4.9e-4 relative at |log q| ~ 1e4 (sigma 0.02 .. 0.03, |v| ~ pi), in
    gv and gsigma alike, on the wave (k = 1) and the thread (k = 40) kernel.  The flat 1e-4
    holds here (test_latent_cases_cpu.py test_large_lse_case_is_well_conditioned).  Measured:
    gv 2.4e-7 and gsigma 2.1e-7; with the weights formed the old way 2.4e-4 both, and up to
    3.0e-4 in the k sweep's cell pi-1e-3 x narrow (gsigma, k = 31)."""
    import lie_vae._ops as ops
    v, sigma = lc.large_lse_case(B)
    _, dv64, ds64 = lc.per_sample(v, sigma, k, F64)
    vg = v.to(gpu_device).requires_grad_(True)
    sg = sigma.to(gpu_device).requires_grad_(True)
    ops.so3_log_posterior(vg, sg, k).sum().backward()
    egv = lc.rel_rows(host(vg.grad)[0], dv64)
    egs = lc.rel_rows(host(sg.grad), ds64)
    print(f"large lse, k={k}: worst gv error {egv.max():.2e}, gsigma {egs.max():.2e} (bound 1e-4)")
    assert egv.max() <= TOL_G and egs.max() <= TOL_G


@pytest.mark.parametrize("k", [1, 40])
def test_density_backward_weights_at_two_modes(gpu_device, k):
    """Regression: the backward takes the Gaussian part of its weights' exponents in fp64.  With
    |v| near pi the terms t = 0 and t = -1 carry comparable weight with opposite slopes, the
    gradient follows l_0 - l_-1, and fp32 terms of size 1e2..1e3 leave that difference 1e-4
    off: the fp32 oracle is 3.7e-4 off fp64 on this case, the kernel with fp32 terms was 3.8e-4
    (and 1.22e-4 against a bound of 1.12e-4 on one sample of the k sweep at k = 1, cell
    pi-1e-3 x aniso).  Flat 1e-4, wave (k = 1) and thread (k = 40) kernel.  Measured: gv
    1.6e-6, gsigma 2.2e-7."""
    import lie_vae._ops as ops
    v, sigma = lc.two_mode_case()
    _, dv64, ds64 = lc.per_sample(v, sigma, k, F64)
    vg = v.to(gpu_device).requires_grad_(True)
    sg = sigma.to(gpu_device).requires_grad_(True)
    ops.so3_log_posterior(vg, sg, k).sum().backward()
    egv = lc.rel_rows(host(vg.grad)[0], dv64)
    egs = lc.rel_rows(host(sg.grad), ds64)
    print(f"two modes, k={k}: worst gv error {egv.max():.2e}, gsigma {egs.max():.2e} (bound 1e-4)")
    assert egv.max() <= TOL_G and egs.max() <= TOL_G


@pytest.mark.parametrize("k", [10, 40])
def test_density_empty_shapes(gpu_device, k):
    """ns = 0, B = 5: empty value, empty gv, and gsigma -- a sum over no samples -- exactly zero
    over a buffer pre-filled with NaN (the entry point's hipMemsetAsync path); through autograd
    too.  B = 0: everything empty, nothing launched."""
    import lie_vae._ops as ops
    from lie_vae import _lib
    d = gpu_device
    sigma = lc.case(k).sigma[:5].to(d)
    empty = torch.empty(0, 5, 3, device=d)
    gs = torch.full((5, 3), float("nan"), device=d)
    _lib.call("lv_so3_log_posterior_bwd", empty.data_ptr(), sigma.data_ptr(),
              torch.empty(0, 5, device=d).data_ptr(), empty.data_ptr(), gs.data_ptr(), 0, 5, k,
              _lib.stream())
    assert torch.equal(gs, torch.zeros(5, 3, device=d))
    assert _lib.so3_log_posterior_plan(0, 5, k)["bwd_blocks"] == 0
    v = empty.clone().requires_grad_(True)
    s = sigma.clone().requires_grad_(True)
    lp = ops.so3_log_posterior(v, s, k)
    assert lp.shape == (0, 5)
    lp.sum().backward()
    assert v.grad.shape == (0, 5, 3) and torch.equal(s.grad, torch.zeros(5, 3, device=d))
    v = torch.empty(3, 0, 3, device=d, requires_grad=True)
    s = torch.empty(0, 3, device=d, requires_grad=True)
    lp = ops.so3_log_posterior(v, s, k)
    assert lp.shape == (3, 0)
    lp.sum().backward()
    assert v.grad.shape == (3, 0, 3) and s.grad.shape == (0, 3)


# ------------------------------------------------------------------ softplus
def softplus_run(device, x, gs):
    import lie_vae._ops as ops
    xg = x.detach().clone().to(device).requires_grad_(True)
    y = ops.unary(xg, ops.SOFTPLUS)
    (y * gs.to(device)).sum().backward()
    return y.detach(), xg.grad


def softplus_ref(x, gs, dtype):
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    y = torch.nn.functional.softplus(xr)
    (y * gs.to(dtype)).sum().backward()
    return y.detach().double(), xr.grad.double()


def rel_err(y, ref):
    return ((y.double() - ref).abs() / ref.abs().clamp_min(1e-300))


def test_softplus_threshold_and_tails(gpu_device):
    """The edge inputs one by one (-100, -20, 0, 20 and its two fp32 neighbours, 20.5, 88, 89
    past the overflow of expf, 1e4) and a bulk uniform on [-30, 30), forward and backward,
    against torch's fp64 softplus and its autograd: each edge input within 1e-5 (1e-4 for the
    gradient) relative, or within 2x the error of torch's own fp32 softplus at that input; the
    bulk with the 2x rule over the bulk.  Everything finite; above the threshold the value is x
    and the gradient is gs, exactly.  Measured: only x = -100 (a denormal result, 3.7e-44) is
    off by more than 7e-8: 1.7e-2 where torch's fp32 has 5.5e-2, gradient 1.4e-2 on both sides;
    worst error / bound 0.16 and 0.50.  (At x = 20 itself z / (z + 1) rounds to 1 in fp32, so
    `x >= 20` in place of `x > 20` is the same function to an ulp: no test can tell them.)"""
    pts = torch.from_numpy(lc.softplus_points())
    x = torch.cat((pts, lc.softplus_bulk(5000)))
    gen = torch.Generator().manual_seed(5)
    gs = (torch.randn(len(x), generator=gen, dtype=F64) + 2.0).to(F32)
    y, gx = (t.cpu() for t in softplus_run(gpu_device, x, gs))
    y64, g64 = softplus_ref(x, gs, F64)
    y32, g32 = softplus_ref(x, gs, F32)
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    above = x > 20
    assert above.sum() > 500 and (~above).sum() > 500  # a sixth of the bulk lies above
    assert torch.equal(y[above], x[above]) and torch.equal(gx[above], gs[above])
    npt = len(pts)
    for what, out, r64, r32, tol in (("softplus", y, y64, y32, TOL_F), ("grad", gx, g64, g32, TOL_G)):
        e, eref = rel_err(out, r64), rel_err(r32, r64)
        floor = torch.cat((eref[:npt], eref[npt:].max().expand(len(x) - npt)))
        bound = torch.maximum(torch.full_like(e, tol), 2 * floor)
        print(f"{what}: worst rel err {float(e.max()):.2e} (torch fp32 {float(eref.max()):.2e}), "
              f"worst err / bound {float((e / bound).max()):.3f}; edge inputs "
              + " ".join(f"{float(a):g}:{float(b):.1e}" for a, b in zip(pts, e[:npt])))
        assert (e <= bound).all(), (what, x[(e > bound)], e[e > bound])


def test_softplus_grid_stride(gpu_device):
    """n = 65536 * 256 + 257: the grid is capped at 65,536 blocks of 256 threads, so the first
    257 threads take a second trip of the grid-stride loop every kernel of pointwise.hip and
    vmf.hip shares.  Forward and backward over the whole array against torch's fp64 softplus on
    the device (2x rule against torch's fp32), and bitwise against the same kernels run alone on
    the first and the last 1024 elements.  Measured worst relative error 1.4e-7 (value) and
    2.4e-7 (gradient), the same as torch's fp32; 0.3 s."""
    n = 65536 * 256 + 257
    gen = torch.Generator(device=gpu_device).manual_seed(9)
    x = (torch.rand(n, generator=gen, device=gpu_device) - 0.5) * 60
    gs = torch.randn(n, generator=gen, device=gpu_device) + 2.0
    y, gx = softplus_run(gpu_device, x, gs)
    assert y.shape == (n,) and torch.isfinite(y).all() and torch.isfinite(gx).all()
    for sl in (slice(0, 1024), slice(n - 1024, n)):
        ya, ga = softplus_run(gpu_device, x[sl].clone(), gs[sl].clone())
        assert torch.equal(ya, y[sl]) and torch.equal(ga, gx[sl])
    y64, g64 = softplus_ref(x, gs, F64)
    y32, g32 = softplus_ref(x, gs, F32)
    for what, out, r64, r32, tol in (("softplus", y, y64, y32, TOL_F), ("grad", gx, g64, g32, TOL_G)):
        e, floor = rel_err(out, r64), float(rel_err(r32, r64).max())
        bound = max(tol, 2 * floor)
        i = int(e.argmax())
        print(f"{what}: worst rel err {float(e[i]):.2e} at element {i} of {n} "
              f"(torch fp32 {floor:.2e}), err / bound {float(e[i]) / bound:.3f}")
        assert float(e[i]) <= bound
        assert float(e[n - 257:].max()) <= bound  # the second trip


# ------------------------------------------------------------------ n0_sample
@pytest.mark.parametrize("ns,B", [(1, 1), (17, 67)])
def test_n0_sample(gpu_device, ns, B):
    """v = eps * sigma is one fp32 multiply: bitwise the IEEE product.  gsigma[b, j] = sum_s
    gv * eps: ns products and ns - 1 additions in fp32, each rounding at most 2^-24 of a partial
    sum <= sum_s |gv * eps|, so |gsigma - fp64| <= ns 2^-24 sum_s |gv * eps| (first order; a
    fused multiply-add only removes roundings).  Measured worst error / bound 0.71 (one
    product) and 0.13."""
    import lie_vae._ops as ops
    from oracle import lie_ref
    gen = torch.Generator().manual_seed(100 * ns + B)
    lo, hi = 0.03, 30.0
    sigma = (lo * (hi / lo) ** torch.rand(B, 3, generator=gen, dtype=F64)).to(F32)
    eps = torch.randn(ns, B, 3, generator=gen)
    gv = torch.randn(ns, B, 3, generator=gen)
    sg = sigma.to(gpu_device).requires_grad_(True)
    v = ops.n0_sample(sg, eps.to(gpu_device))
    assert v.shape == (ns, B, 3) and torch.equal(v.detach().cpu(), eps * sigma)
    (v * gv.to(gpu_device)).sum().backward()
    s64 = sigma.double().requires_grad_(True)
    (lie_ref.n0_sample(s64, eps.double()) * gv.double()).sum().backward()
    err = (sg.grad.cpu().double() - s64.grad).abs()
    bound = ns * 2.0 ** -24 * (gv.double() * eps.double()).abs().sum(0)
    print(f"n0_sample ns={ns} B={B}: worst gsigma err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------ so3_sample
def so3_sample_case(ns, B):
    """mu (B, 3, 3) Haar, v from the radius bands, and a cotangent gz redrawn (from the fp64
    oracle alone) until ||gv64|| >= 0.05 ||gz|| for every sample.  At |v| near 2 pi the exp map
    is nearly singular: its two tangential singular values are sin(theta) / theta and
    (1 - cos(theta)) / theta, about 0.002 in the two 2 pi bands, so gv is as small as the
    radial part <gz, dz / dtheta> happens to be, and relative to such a gv any fp32 evaluation
    of the 9-term products carries ~ 9 * 2^-24 ||gz|| / ||gv||: a sample with ||gv|| = 0.002
    ||gz|| tests the draw, not the kernel."""
    from oracle import lie_ref
    v, band = lc.band_vectors(ns, B)
    torch.manual_seed(1000 * ns + B)
    mu = lie_ref.haar_matrices(B, dtype=F64).to(F32)
    gz = torch.randn(ns, B, 3, 3, dtype=F64).to(F32)
    for _ in range(50):
        gv64 = torch.from_numpy(so3_sample_ref(mu, v, gz, F64)[2])
        weak = gv64.norm(dim=-1) < 0.05 * gz.double().flatten(2).norm(dim=-1)
        if not weak.any():
            return mu, v, gz, band
        gz[weak] = torch.randn(int(weak.sum()), 3, 3, dtype=F64).to(F32)
    raise AssertionError("so3_sample_case: no well-conditioned cotangent found")


def so3_sample_ref(mu, v, gz, dtype):
    from oracle import lie_ref
    m = mu.detach().clone().to(dtype).requires_grad_(True)
    w = v.detach().clone().to(dtype).requires_grad_(True)
    z = lie_ref.so3_sample(m, w)
    (z * gz.to(dtype)).sum().backward()
    return [t.detach().double().numpy() for t in (z, m.grad, w.grad)]


def so3_sample_run(device, mu, v, gz, dtype):
    import lie_vae._ops as ops
    m = mu.detach().clone().to(device, dtype).requires_grad_(True)
    w = v.detach().clone().to(device, dtype).requires_grad_(True)
    z = ops.so3_sample(m, w)
    assert z.dtype == dtype and z.shape == (*v.shape[:2], 3, 3)
    (z * gz.to(device, dtype)).sum().backward()
    assert m.grad.dtype == dtype and w.grad.dtype == dtype
    return [host(t).astype(np.float64) for t in (z, m.grad, w.grad)]


@pytest.mark.parametrize("ns,B", [(1, 1), (17, 67)])
def test_so3_sample_fp32_bands(gpu_device, ns, B):
    """z = mu exp(v), gmu (summed over s) and gv with |v| from the radius bands of the density
    (band = b mod 9), against the oracle's fp64 autograd: normwise per sample (per b for gmu)
    within the project's 1e-5 / 1e-4, or within 2x the worst fp32-oracle error of its band.
    Measured at (17, 67): z 8.0e-7 (band 9.0; the oracle 6.6e-7), gmu 5.0e-7, gv 2.4e-5 (band
    0.004; the oracle 2.6e-5); worst error / bound 0.08, 0.005, 0.24."""
    mu, v, gz, band = so3_sample_case(ns, B)
    got = so3_sample_run(gpu_device, mu, v, gz, F32)
    r64 = so3_sample_ref(mu, v, gz, F64)
    r32 = so3_sample_ref(mu, v, gz, F32)
    band_s = np.tile(band, ns)
    for what, y, a64, a32, tol, bnd, rows in (("z", *[a[0] for a in (got, r64, r32)], TOL_F, band_s, ns * B),
                                              ("gmu", *[a[1] for a in (got, r64, r32)], TOL_G, band, B),
                                              ("gv", *[a[2] for a in (got, r64, r32)], TOL_G, band_s, ns * B)):
        assert np.isfinite(y).all(), what
        e = lc.rel_rows(y.reshape(rows, -1), a64.reshape(rows, -1))
        eref = lc.rel_rows(a32.reshape(rows, -1), a64.reshape(rows, -1))
        floor = np.zeros(lc.NBAND)
        np.maximum.at(floor, bnd, eref)
        bound = np.maximum(tol, 2 * floor[bnd])
        i = int(np.argmax(e / bound))
        print(f"so3_sample {what} ns={ns} B={B}: worst err / bound {e[i] / bound[i]:.3f} in band "
              f"{lc.BANDS[bnd[i]][0]} (err {e[i]:.2e}, fp32 oracle of the band {floor[bnd[i]]:.2e})")
        assert (e <= bound).all(), (what, lc.BANDS[bnd[i]][0], e[i], bound[i])


@pytest.mark.parametrize("ns,B", [(1, 1), (17, 67)])
def test_so3_sample_fp64_bands(gpu_device, ns, B):
    """The fp64 twin on the same bands, at the tolerances of test_gpu_parity.py
    test_fp64_maps_follow_input_dtype: values within 1e-12 and gradients within 1e-10 of the
    oracle's fp64 autograd, relative to max(largest entry, 1)."""
    mu, v, gz, _ = so3_sample_case(ns, B)
    got = so3_sample_run(gpu_device, mu, v, gz, F64)
    ref = so3_sample_ref(mu, v, gz, F64)
    for what, y, r, tol in zip(("z", "gmu", "gv"), got, ref, (1e-12, 1e-10, 1e-10)):
        err, scale = np.abs(y - r).max(), max(np.abs(r).max(), 1.0)
        print(f"so3_sample fp64 {what} ns={ns} B={B}: max abs err {err:.2e}, / bound {err / (tol * scale):.3f}")
        assert err <= tol * scale, what
