"""The conv-layer kernels (csrc/deconv.hip, csrc/bn.hip) over their dispatch space, through
the C ABI (lie_vae._lib.call) so that shapes the Python modules would refuse or never
produce are reached too.  The shapes are tests/conv_layer_cases.py.

Convolution and sum kernels run on small INTEGER operands: every product and every fp32
partial sum is then an exact integer (each test asserts the bound that makes it so, below
2^24), the float64 reference is exact, and the kernel rounds once to bf16 (round to nearest
even; not at all in fp32) -- so its output must equal reference.to(dtype) bit for bit,
whatever the summation order, the tiling or the number of partial slabs.  BatchNorm cannot
be exact; it keeps the bounds of test_fused_bn_leaky_relu_matches_float64.

Every output buffer is filled with NaN and followed by a NaN guard band: an element the
kernel does not write, or a write past the end, fails the comparison."""
import functools

import pytest
import torch

import conv_layer_cases as cases
from lie_vae import _lib

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
EXACT = 2 ** 24   # integers below this are exact in fp32
GUARD = 64


# ------------------------------------------------------------------------------ helpers
def _ints(g, shape, lim):
    """Integers in [-lim, lim] as float64."""
    return torch.randint(-lim, lim + 1, shape, generator=g).double()


def _out(dev, shape, dtype):
    """NaN-filled output of `shape` with a NaN guard band behind it: (buffer, view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), float("nan"), device=dev, dtype=dtype)
    return buf, buf[:n].view(shape)


def _guard_intact(buf):
    return bool(buf[-GUARD:].isnan().all())


def _nhwc(t, dtype, dev):
    """(N, C, H, W) float64 -> dense (N, H, W, C) on the device."""
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)


def _nchw(t):
    """Dense (N, H, W, C) device tensor -> (N, C, H, W) on the CPU."""
    return t.permute(0, 3, 1, 2).cpu()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _assert_exact_regime(terms, amax, bmax, extra, *refs):
    """The condition that makes the bitwise comparison valid: the sum of absolute products
    (terms·amax·bmax, + extra for a bias) and every reference value stay below 2^24."""
    assert terms * amax * bmax + extra < EXACT, (terms, amax, bmax, extra)
    for r in refs:
        assert float(r.abs().max()) < EXACT


@functools.lru_cache(maxsize=None)
def _deconv_data(c, lim_x=4, lim_w=3):
    """Integer operands and the float64 forward of a transposed-convolution case."""
    g = torch.Generator().manual_seed(c.N * 131 + c.H * 17 + c.W * 7 + c.Cin * 3 + c.Cout)
    x = _ints(g, (c.N, c.Cin, c.H, c.W), lim_x)
    w = _ints(g, (c.Cin, c.Cout, 4, 4), lim_w)
    b = _ints(g, (c.Cout,), 4) if c.bias else None
    ref = torch.nn.functional.conv_transpose2d(x, w, b, 2, 1)
    if getattr(c, "flags", 0) & cases.RELU_OUT:
        ref = ref.clamp_min(0)
    # an output pixel sees 2 x 2 taps of Cin channels
    _assert_exact_regime(4 * c.Cin, lim_x, lim_w, 4, ref)
    return x, w, b, ref


# ------------------------------------------------------------------ A. bf16 MFMA forward
def _ids(cs):
    return ["-".join(str(int(v)) for v in c) for c in cs]


@pytest.mark.parametrize("c", cases.MFMA_BF16, ids=_ids(cases.MFMA_BF16))
def test_mfma_bf16_forward_exact(gpu_device, c):
    """lv_deconv4s2_fwd_bf16_ex (default variant: 128-row tiles, 2-stage ring, XCD-grouped
    grid) on integer operands: bitwise equal to the float64 conv_transpose2d cast to bf16.
    Ragged and exact row tiles, grid padding, one to 25 K steps, Cout % 8 == 4, null bias,
    fused ReLU, images where every tap is partly outside."""
    lib, dev = _lib.load(), gpu_device
    x, w, b, ref = _deconv_data(c)
    xg, wg = _nhwc(x, BF16, dev), w.to(BF16).to(dev)
    bg = None if b is None else b.float().to(dev)
    wt = torch.empty(lib.lv_deconv4s2_packed_weight_elems(c.Cin), device=dev, dtype=BF16)
    buf, y = _out(dev, (c.N, 2 * c.H, 2 * c.W, c.Cout), BF16)
    st = _lib.stream()
    _lib.call("lv_deconv4s2_pack_weight_bf16", wg.data_ptr(), wt.data_ptr(), c.Cin, c.Cout, st)
    _lib.call("lv_deconv4s2_fwd_bf16_ex", xg.data_ptr(), wt.data_ptr(), _ptr(bg), y.data_ptr(),
              c.N, c.H, c.W, c.Cin, c.Cout, c.flags, st)
    torch.cuda.synchronize(dev)
    assert _guard_intact(buf)
    got, want = _nchw(y), ref.to(BF16)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"


def test_mfma_bf16_forward_empty_batch(gpu_device):
    """N = 0 is a no-op that returns LV_OK (no pointer is read)."""
    _lib.call("lv_deconv4s2_fwd_bf16_ex", None, None, None, None, 0, 4, 4, 200, 200, 0, _lib.stream())
    _lib.call("lv_deconv4s2_fwd_f32", None, None, None, None, None, 0, 4, 4, 200, 200, 0, _lib.stream())
    _lib.call("lv_deconv4s2_small_fwd_bf16", None, None, None, None, 0, 4, 4, 200, 3, _lib.stream())


@pytest.mark.parametrize("c", cases.MFMA_BF16_DGRAD, ids=_ids(cases.MFMA_BF16_DGRAD))
def test_mfma_bf16_encoder_dgrad_exact(gpu_device, c):
    """The same kernel as the encoder's input gradient (nets._Conv4s2: Conv2d(Cout, Cin, 4,
    2, 1) whose weight is read as this layer's): gx bitwise equal to float64 autograd of
    conv2d on integer gy and w.  (gw / gb there are MIOpen's and are not requested.)"""
    from lie_vae.experiments.nets import _Conv4s2
    dev = gpu_device
    g = torch.Generator().manual_seed(c.Cin * 5 + c.Cout)
    x = _ints(g, (c.N, c.Cout, 2 * c.H, 2 * c.W), 4)
    w = _ints(g, (c.Cin, c.Cout, 4, 4), 3)       # Conv2d weight (out, in, 4, 4)
    gy = _ints(g, (c.N, c.Cin, c.H, c.W), 4)
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.conv2d(xr, w, None, 2, 1).backward(gy)
    _assert_exact_regime(4 * c.Cin, 4, 3, 0, xr.grad)
    xd = x.to(BF16).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = _Conv4s2.apply(xd, w.to(BF16).to(dev), None)
    y.backward(gy.to(BF16).to(dev).contiguous(memory_format=torch.channels_last))
    assert torch.equal(xd.grad.cpu(), xr.grad.to(BF16))


# ------------------------------------------------------------------ B. fp32 MFMA forward
@pytest.mark.parametrize("c", cases.MFMA_F32, ids=_ids(cases.MFMA_F32))
def test_mfma_f32_forward_exact(gpu_device, c):
    """lv_deconv4s2_fwd_f32 on integer operands: y (NCHW) bitwise equal to the float64
    reference cast to fp32 (no rounding happens at all), and the channels-last twin (where
    Cout % 4 == 0) bitwise equal to y.  Cin = 4 is one K step of 16; Cout from 1 to 208."""
    lib, dev = _lib.load(), gpu_device
    x, w, b, ref = _deconv_data(c)
    xg, wg = _nhwc(x, F32, dev), w.float().to(dev)
    bg = None if b is None else b.float().to(dev)
    wt = torch.empty(lib.lv_deconv4s2_packed_weight_elems_f32(c.Cin), device=dev, dtype=F32)
    buf, y = _out(dev, (c.N, c.Cout, 2 * c.H, 2 * c.W), F32)
    twin = c.Cout % 4 == 0
    bufcl, ycl = _out(dev, (c.N, 2 * c.H, 2 * c.W, c.Cout), F32) if twin else (None, None)
    st = _lib.stream()
    _lib.call("lv_deconv4s2_pack_weight_f32", wg.data_ptr(), wt.data_ptr(), c.Cin, c.Cout, st)
    _lib.call("lv_deconv4s2_fwd_f32", xg.data_ptr(), wt.data_ptr(), _ptr(bg), y.data_ptr(), _ptr(ycl),
              c.N, c.H, c.W, c.Cin, c.Cout, c.flags, st)
    torch.cuda.synchronize(dev)
    assert _guard_intact(buf)
    got, want = y.cpu(), ref.float()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"
    if twin:
        assert _guard_intact(bufcl)
        assert torch.equal(_bits(_nchw(ycl)), _bits(got)), "channels-last twin"


# ------------------------------------------------------------------ C. small-Cout forward
@pytest.mark.parametrize("c", cases.SMALL_FWD, ids=_ids(cases.SMALL_FWD))
def test_small_forward_exact(gpu_device, c):
    """lv_deconv4s2_small_fwd_bf16 (8 x 16-quad blocks, K padded to 32 channels per
    neighbour) on integer operands: bitwise.  Cout 1..4, zero-padded channel chunks, whole
    and ragged blocks, a 1x1 image, several images, null bias."""
    lib, dev = _lib.load(), gpu_device
    x, w, b, ref = _deconv_data(c)
    xg, wg = _nhwc(x, BF16, dev), w.to(BF16).to(dev)
    bg = None if b is None else b.float().to(dev)
    wq = torch.empty(lib.lv_deconv4s2_small_packed_weight_elems(c.Cin), device=dev, dtype=BF16)
    buf, y = _out(dev, (c.N, 2 * c.H, 2 * c.W, c.Cout), BF16)
    st = _lib.stream()
    _lib.call("lv_deconv4s2_small_pack_weight_bf16", wg.data_ptr(), wq.data_ptr(), c.Cin, c.Cout, st)
    _lib.call("lv_deconv4s2_small_fwd_bf16", xg.data_ptr(), wq.data_ptr(), _ptr(bg), y.data_ptr(),
              c.N, c.H, c.W, c.Cin, c.Cout, st)
    torch.cuda.synchronize(dev)
    assert _guard_intact(buf)
    got, want = _nchw(y), ref.to(BF16)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"


# ------------------------------------------------------------------ D. small-Cout backward
@functools.lru_cache(maxsize=None)
def _small_bwd_data(c):
    """Integer x, w, gy of a backward case and float64 autograd's gx, gw, gb.  With
    LV_DECONV_MASK_GX x is a ReLU output and gx is masked by x > 0."""
    g = torch.Generator().manual_seed(c.N + c.H * 17 + c.W * 7 + c.Cin * 3 + c.Cout + c.flags)
    x = _ints(g, (c.N, c.Cin, c.H, c.W), 4)
    if c.flags & cases.MASK_GX:
        x = x.clamp_min(0)
    w = _ints(g, (c.Cin, c.Cout, 4, 4), 3)
    gy = _ints(g, (c.N, c.Cout, 2 * c.H, 2 * c.W), 4)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), torch.zeros(c.Cout, dtype=torch.float64,
                                                                                             requires_grad=True)
    torch.nn.functional.conv_transpose2d(xr, wr, br, 2, 1).backward(gy)
    gx = xr.grad * (x > 0) if c.flags & cases.MASK_GX else xr.grad
    # dgrad: 9 neighbours x 16 (phase, channel) columns per input pixel; wgrad: one product
    # per pixel of the batch (the looped case: 684·165·16 = 1.8e6); bias: 4 values per pixel
    P = c.N * c.H * c.W
    _assert_exact_regime(9 * 16, 4, 3, 0, gx)
    _assert_exact_regime(P, 4, 4, 0, wr.grad)
    _assert_exact_regime(4 * P, 4, 1, 0, br.grad)
    return x, w, gy, gx, wr.grad, br.grad


def _small_bwd_inputs(dev, c):
    x, w, gy = _small_bwd_data(c)[:3]
    return _nhwc(x, BF16, dev), w.to(BF16).to(dev), _nhwc(gy, BF16, dev)


def _run_small_bwd(dev, c, xg, wg, gyg, want_gx=True, want_gw=True, want_gb=True):
    """One lv_deconv4s2_small_bwd_bf16_ex call; (gx NCHW, gw, gb) on the CPU (None = skipped)."""
    lib, st = _lib.load(), _lib.stream()
    wd = bx = gx = bw = gw = bb = gb = ws = None
    if want_gx:
        wd = torch.empty(lib.lv_deconv4s2_small_dgrad_weight_elems(c.Cin), device=dev, dtype=BF16)
        _lib.call("lv_deconv4s2_small_pack_dgrad_weight_bf16", wg.data_ptr(), wd.data_ptr(), c.Cin, c.Cout, st)
        bx, gx = _out(dev, (c.N, c.H, c.W, c.Cin), BF16)
    if want_gw:
        bw, gw = _out(dev, (c.Cin, c.Cout, 4, 4), BF16)
        ws = torch.empty(max(1, lib.lv_deconv4s2_small_bwd_workspace_elems(c.N, c.H, c.W, c.Cin, c.Cout)),
                         device=dev, dtype=F32)
    if want_gb:
        bb, gb = _out(dev, (c.Cout,), F32)
    _lib.call("lv_deconv4s2_small_bwd_bf16_ex", xg.data_ptr(), gyg.data_ptr(), _ptr(wd), _ptr(gx), _ptr(gw),
              _ptr(gb), _ptr(ws), c.N, c.H, c.W, c.Cin, c.Cout, c.flags, st)
    torch.cuda.synchronize(dev)
    for b in (bx, bw, bb):
        assert b is None or _guard_intact(b)
    return (None if gx is None else _nchw(gx), None if gw is None else gw.cpu(),
            None if gb is None else gb.cpu())


def _assert_small_bwd_exact(dev, c):
    gx_ref, gw_ref, gb_ref = _small_bwd_data(c)[3:]
    gx, gw, gb = _run_small_bwd(dev, c, *_small_bwd_inputs(dev, c))
    for name, got, want in (("gx", gx, gx_ref.to(BF16)), ("gw", gw, gw_ref.to(BF16)), ("gb", gb, gb_ref.float())):
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {want.numel()} elements differ"


@pytest.mark.parametrize("c", cases.SMALL_BWD, ids=_ids(cases.SMALL_BWD))
def test_small_backward_exact(gpu_device, c):
    """lv_deconv4s2_small_bwd_bf16_ex on integer operands: gx, gw (bf16) and gb (fp32)
    bitwise equal to float64 autograd of conv_transpose2d.  One to sixteen channel tiles
    (idle dgrad waves, wgrad's second accumulator set, the bias column in the last tile),
    every Cout, tiles ragged in height and width."""
    _assert_small_bwd_exact(gpu_device, c)


@pytest.mark.parametrize("c", cases.SMALL_BWD_LOOP, ids=_ids(cases.SMALL_BWD_LOOP))
def test_small_backward_persistent_loop_exact(gpu_device, c):
    """The persistent tile loops: more than 2·8·CUs tiles, so every block of the dgrad and
    of the wgrad walks at least two tiles (the next tile's quads loaded a tile ahead, LDS
    reused), four of the six tiles per image ragged.  gx, gw, gb bitwise; once with
    LV_DECONV_MASK_GX (gx masked by x > 0, x a ReLU output)."""
    assert c.N * cases.LOOP_TILES_IMG > 2 * 8 * _lib.load().lv_compute_units()
    _assert_small_bwd_exact(gpu_device, c)


def test_small_backward_partial_calls(gpu_device):
    """gx only (null gw, gb and workspace), gw + gb only (null gx and dgrad weight) and gw
    without gb: the same bits as the full call, which is exact."""
    dev, c = gpu_device, cases.SMALL_BWD_PARTIAL
    _assert_small_bwd_exact(dev, c)
    inp = _small_bwd_inputs(dev, c)
    gx, gw, gb = _run_small_bwd(dev, c, *inp)
    gx1, gw1, gb1 = _run_small_bwd(dev, c, *inp, want_gw=False, want_gb=False)
    assert gw1 is None and gb1 is None and torch.equal(_bits(gx1), _bits(gx))
    gx2, gw2, gb2 = _run_small_bwd(dev, c, *inp, want_gx=False)
    assert gx2 is None and torch.equal(_bits(gw2), _bits(gw)) and torch.equal(_bits(gb2), _bits(gb))
    gx3, gw3, gb3 = _run_small_bwd(dev, c, *inp, want_gx=False, want_gb=False)
    assert gx3 is None and gb3 is None and torch.equal(_bits(gw3), _bits(gw))


def test_small_backward_empty_batch(gpu_device):
    """N = 0: gw and gb are zeroed (x and gy are not read)."""
    dev, c = gpu_device, cases.SMALL_BWD_PARTIAL._replace(N=0)
    one = torch.zeros(8, device=dev, dtype=BF16)   # empty tensors have a null data pointer
    gx, gw, gb = _run_small_bwd(dev, c, one, torch.ones(c.Cin, c.Cout, 4, 4, device=dev, dtype=BF16), one)
    assert gx.numel() == 0 and not gw.any() and not gb.any()
    assert gw.shape == (c.Cin, c.Cout, 4, 4) and gb.shape == (c.Cout,)


# ------------------------------------------------------------------ E. per-channel sum
def _channel_sum(dev, g):
    P, C = g.shape
    ws = torch.empty(max(1, _lib.load().lv_channel_sum_workspace_elems(P, C)), device=dev, dtype=F32)
    buf, out = _out(dev, (C,), F32)
    _lib.call("lv_channel_sum_bf16", _ptr(g) if P else None, out.data_ptr(), ws.data_ptr(), P, C, _lib.stream())
    torch.cuda.synchronize(dev)
    assert _guard_intact(buf)
    return out.cpu()


@pytest.mark.parametrize("P,C", cases.CHANNEL_SUM)
def test_channel_sum_exact(gpu_device, P, C):
    """lv_channel_sum_bf16 on integers in [-8, 8]: bitwise equal to the float64 column sum.
    One row, rows around one block, R = 1 (C = 2048) and R = 32 (C = 8), the 1024-block cap
    with empty trailing blocks."""
    g = _ints(torch.Generator().manual_seed(P + C), (P, C), 8)
    ref = g.sum(0)
    _assert_exact_regime(P, 8, 1, 0, ref)
    assert torch.equal(_channel_sum(gpu_device, g.to(BF16).to(gpu_device)), ref.float())


def test_channel_sum_empty(gpu_device):
    """P = 0: zeros, nothing read."""
    out = _channel_sum(gpu_device, torch.empty(0, 200, device=gpu_device, dtype=BF16))
    assert out.shape == (200,) and not out.any()


# ------------------------------------------------------------------ F. BatchNorm + LeakyReLU
EPS, SLOPE, MOMENTUM = 1e-5, 0.2, 0.1


def _bn_forward(dev, x, gamma, beta, rm, rv, training=1):
    """lv_bn_lrelu_fwd_bf16 on a (P, C) bf16 device tensor: (y, save_mean, save_invstd)."""
    lib = _lib.load()
    P, C = x.shape
    n_ws = lib.lv_bn_workspace_elems(P, C)
    geo = cases.bn_geom(P, C)
    assert geo is not None and cases.bn_nblk_from_workspace(n_ws, C) == geo[4]
    ws = torch.empty(n_ws, device=dev, dtype=F32)
    by, y = _out(dev, (P, C), BF16)
    bm, mean = _out(dev, (C,), F32)
    bi, invstd = _out(dev, (C,), F32)
    _lib.call("lv_bn_lrelu_fwd_bf16", x.data_ptr(), _ptr(gamma), _ptr(beta), _ptr(rm), _ptr(rv), training,
              MOMENTUM, EPS, SLOPE, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), P, C,
              _lib.stream())
    torch.cuda.synchronize(dev)
    assert _guard_intact(by) and _guard_intact(bm) and _guard_intact(bi)
    return y, mean, invstd


def _bn_backward(dev, g, x, gamma, beta, mean, invstd, want_params=True):
    """lv_bn_lrelu_bwd_bf16: (gx, ggamma, gbeta)."""
    P, C = x.shape
    ws = torch.empty(_lib.load().lv_bn_workspace_elems(P, C), device=dev, dtype=F32)
    bx, gx = _out(dev, (P, C), BF16)
    bg, gg = _out(dev, (C,), F32) if want_params else (None, None)
    bb, gb = _out(dev, (C,), F32) if want_params else (None, None)
    _lib.call("lv_bn_lrelu_bwd_bf16", g.data_ptr(), x.data_ptr(), _ptr(gamma), _ptr(beta), mean.data_ptr(),
              invstd.data_ptr(), SLOPE, gx.data_ptr(), _ptr(gg), _ptr(gb), ws.data_ptr(), P, C, _lib.stream())
    torch.cuda.synchronize(dev)
    for b in (bx, bg, bb):
        assert b is None or _guard_intact(b)
    return gx, gg, gb


def _within(name, got, ref, rel, absr):
    """|got - ref| <= rel |ref| + absr rms(ref), elementwise (the project's conv-layer bound)."""
    gd = got.double().cpu()
    err = (gd - ref).abs()
    bad = err > rel * ref.abs() + absr * ref.square().mean().sqrt()
    print(f"  {name}: max err {float(err.max()):.3e}, rms(ref) {float(ref.square().mean().sqrt()):.3e}, "
          f"{int(bad.sum())} of {bad.numel()} off")
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} off, max err {float(err.max()):.3e}"


def _bn_data(C, P, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(P, C, generator=g) * 1.5 + 0.7).to(BF16)
    gy = torch.randn(P, C, generator=g).to(BF16)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    rm = torch.randn(C, generator=g) * 0.1
    rv = torch.rand(C, generator=g) + 0.5
    return x, gy, gamma, beta, rm, rv


def _bn_stats64(x64):
    mean = x64.mean(0)
    var = x64.var(0, unbiased=False)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def _check_bn_training(dev, C, P, affine=True, running=True, param_grads=True):
    """Forward + backward in training mode against the float64 formulas and the bounds of
    test_fused_bn_leaky_relu_matches_float64 (the activation mask from the kernel's own y)."""
    x, gy, gamma, beta, rm, rv = _bn_data(C, P, C * 3 + P)
    dv = lambda t: t.to(dev)
    xg, gg = dv(x), dv(gy)
    gam, bet = (dv(gamma), dv(beta)) if affine else (None, None)
    rmg, rvg = (dv(rm), dv(rv)) if running else (None, None)
    y, mean_k, inv_k = _bn_forward(dev, xg, gam, bet, rmg, rvg)
    gx, ggam, gbet = _bn_backward(dev, gg, xg, gam, bet, mean_k, inv_k, want_params=param_grads)
    x64, g64 = x.double(), gy.double()
    w64 = gamma.double() if affine else torch.ones(C, dtype=torch.float64)
    b64 = beta.double() if affine else torch.zeros(C, dtype=torch.float64)
    mean, var, inv = _bn_stats64(x64)
    xhat = (x64 - mean) * inv
    z = xhat * w64 + b64
    print(f"BN C={C} P={P} affine={affine} running={running}")
    _within("y", y, torch.where(z > 0, z, SLOPE * z), 2.0 ** -8, 1e-3)
    if running:
        torch.testing.assert_close(rmg.double().cpu(), 0.9 * rm.double() + 0.1 * mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(rvg.double().cpu(), 0.9 * rv.double() + 0.1 * var * P / (P - 1),
                                   rtol=1e-5, atol=1e-6)
    gz = torch.where(y.double().cpu() > 0, g64, SLOPE * g64)
    gb = gz.sum(0)
    gw = (gz * xhat).sum(0)
    _within("gx", gx, (w64 * inv) * (gz - gb / P - xhat * gw / P), 2.0 ** -7, 2e-3)
    if param_grads:
        _within("ggamma", ggam, gw, 1e-4, 1e-4)
        _within("gbeta", gbet, gb, 1e-4, 1e-4)


@pytest.mark.parametrize("C,P,why", cases.BN_GEOMETRY, ids=[f"C{c[0]}-P{c[1]}" for c in cases.BN_GEOMETRY])
def test_bn_geometry_classes(gpu_device, C, P, why):
    """Every (T, R) class of the reductions' thread geometry at its smallest supported P:
    T = 1, odd C (8 pixels per period), R = 1, partly idle blocks."""
    _check_bn_training(gpu_device, C, P)


@pytest.mark.parametrize("C,P", cases.BN_UNROLL)
def test_bn_reduce_unroll_boundaries(gpu_device, C, P):
    """4R - 1, 4R and 4R + 1 period groups: the 4-way unrolled loop of bn_reduce_part_kernel
    with a remainder of three, none, and a second block."""
    _check_bn_training(gpu_device, C, P)


@pytest.mark.parametrize("C,P,nblk", cases.BN_NBLK)
def test_bn_finalize_block_counts(gpu_device, C, P, nblk):
    """1, 15, 16, 17, 63, 64 and 65 reduction blocks: the 16 slices of bn_finalize_kernel
    empty, just full, and at its 4-way unroll boundary.  The block count is read back from
    lv_bn_workspace_elems so the case cannot drift off its branch."""
    assert cases.bn_nblk_from_workspace(_lib.load().lv_bn_workspace_elems(P, C), C) == nblk
    _check_bn_training(gpu_device, C, P)


@pytest.mark.parametrize("C,P", cases.BN_GRID_STRIDE)
def test_bn_apply_grid_stride(gpu_device, C, P):
    """More than 2048 x 256 vectors: threads of bn_apply_kernel take a second vector and use
    the running channel offset, in the forward and the backward apply."""
    _check_bn_training(gpu_device, C, P)


@pytest.mark.parametrize("C,P", cases.BN_EVAL)
def test_bn_eval_mode(gpu_device, C, P):
    """training = 0 (bn_eval_coef_kernel; no Python caller): y = lrelu(a x + b) from the
    running statistics, against float64 at the usual y bound; the running statistics are
    left unchanged."""
    dev = gpu_device
    x, _, gamma, beta, rm, rv = _bn_data(C, P, C + P)
    rmg, rvg = rm.to(dev), rv.to(dev)
    y, _, _ = _bn_forward(dev, x.to(dev), gamma.to(dev), beta.to(dev), rmg, rvg, training=0)
    a = gamma.double() / torch.sqrt(rv.double() + EPS)
    z = x.double() * a + (beta.double() - rm.double() * a)
    _within("y", y, torch.where(z > 0, z, SLOPE * z), 2.0 ** -8, 1e-3)
    assert torch.equal(rmg.cpu(), rm) and torch.equal(rvg.cpu(), rv)


def test_bn_null_parameters(gpu_device):
    """Null gamma / beta (an affine=False layer), null running statistics in training mode,
    null ggamma / gbeta in the backward."""
    C, P = cases.BN_NULL_PARAMS
    _check_bn_training(gpu_device, C, P, affine=False)
    _check_bn_training(gpu_device, C, P, running=False)
    _check_bn_training(gpu_device, C, P, param_grads=False)


def _stat_errors(mean, invstd, x64):
    """Max relative error of the saved statistics against float64: the mean relative to the
    channel's rms (its rounding error scales with the data, not with a mean near zero), the
    inverse standard deviation relative to itself."""
    m64, v64, i64 = _bn_stats64(x64)
    scale = torch.sqrt(v64 + m64 * m64).clamp_min(1e-30)
    return (float(((mean.double().cpu() - m64).abs() / scale).max()),
            float(((invstd.double().cpu() - i64).abs() / i64).max()))


def _assert_stats_within_twice_torch(dev, x):
    """The 2x rule: torch.native_batch_norm's saved statistics on the same bf16 input set the
    noise floor; the library's error is at most twice that, floor 1e-6 relative."""
    P, C = x.shape
    xg = x.to(dev)
    _, mean_k, inv_k = _bn_forward(dev, xg, None, None, None, None)
    _, mean_t, inv_t = torch.native_batch_norm(xg.view(P, C, 1, 1), None, None, None, None, True, MOMENTUM, EPS)
    assert mean_t.dtype == F32 and inv_t.dtype == F32
    e_k, e_t = _stat_errors(mean_k, inv_k, x.double()), _stat_errors(mean_t, inv_t, x.double())
    print(f"BN stats C={C} P={P}: mean err library {e_k[0]:.3e} torch {e_t[0]:.3e}; "
          f"invstd err library {e_k[1]:.3e} torch {e_t[1]:.3e}")
    assert e_k[0] <= max(2 * e_t[0], 1e-6), ("save_mean", e_k[0], e_t[0])
    assert e_k[1] <= max(2 * e_t[1], 1e-6), ("save_invstd", e_k[1], e_t[1])
    return mean_k, inv_k


@pytest.mark.parametrize("C,P", cases.BN_STATS)
def test_bn_saved_statistics_within_twice_torch(gpu_device, C, P):
    """save_mean / save_invstd against float64 on the same bf16 input, relative error (mean:
    over the channel's rms), bounded by twice torch.native_batch_norm's on the GPU, floor 1e-6.
    Measured on MI355X, library | torch:
      C = 50, P = 65536:  mean 8.4e-8 | 4.1e-8,  invstd 2.1e-7 | 1.1e-7
      C = 9,  P = 904:    mean 7.4e-8 | 6.4e-8,  invstd 9.6e-7 | 5.7e-8  (inside the floor only)
      C = 16, P = 4096:   mean 3.7e-8 | 3.3e-8,  invstd 1.4e-7 | 5.9e-8"""
    x = _bn_data(C, P, C + 7 * P)[0]
    _assert_stats_within_twice_torch(gpu_device, x)


def test_bn_stress_inputs(gpu_device):
    """Channels that strain the shifted one-pass variance: mean 30 with standard deviation
    0.25; a constant channel (variance 0); a channel whose pixel 0 lies 32 sigma from the
    rest -- with x[0, c] alone as the shift, E[d^2] - E[d]^2 cancels there -- and two more
    with the outlier at the last and at the middle pixel.  Saved statistics
    under the 2x rule against torch.native_batch_norm, y at the usual bound.
    Measured on MI355X (C = 16, P = 65536), library | torch: with the shift x[0, c] mean
    1.3e-7 | 3.4e-8, invstd 6.1e-5 | 9.0e-8 (outside the rule); with bn_shift's median of
    three pixels mean 3.9e-8 | 3.4e-8, invstd 1.1e-7 | 9.0e-8."""
    dev = gpu_device
    C, P = cases.BN_STRESS
    g = torch.Generator().manual_seed(11)
    x = torch.randn(P, C, generator=g) * 1.5 + 0.7
    x[:, 0] = 30.0 + 0.25 * torch.randn(P, generator=g)
    x[:, 1] = 3.0
    x[:, 2] = torch.randn(P, generator=g)
    x[0, 2] = 32.0
    x[:, 3:5] = torch.randn(P, 2, generator=g)   # the same at the other two sampled pixels
    x[P - 1, 3] = 32.0
    x[P // 2, 4] = -32.0
    x = x.to(BF16)
    _assert_stats_within_twice_torch(dev, x)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    y, _, _ = _bn_forward(dev, x.to(dev), gamma.to(dev), beta.to(dev), None, None)
    mean, _, inv = _bn_stats64(x.double())
    z = (x.double() - mean) * inv * gamma.double() + beta.double()
    _within("y", y, torch.where(z > 0, z, SLOPE * z), 2.0 ** -8, 1e-3)


# ------------------------------------------------------------------ G. determinism
def test_small_backward_is_deterministic(gpu_device):
    """A looped small-Cout backward run twice: gx, gw and gb bit-identical."""
    dev, c = gpu_device, cases.SMALL_BWD_LOOP[0]
    inp = _small_bwd_inputs(dev, c)
    a, b = _run_small_bwd(dev, c, *inp), _run_small_bwd(dev, c, *inp)
    for name, u, v in zip(("gx", "gw", "gb"), a, b):
        assert torch.equal(_bits(u), _bits(v)), name


def test_bn_is_deterministic(gpu_device):
    """A 65-block BatchNorm forward + backward run twice: y, the saved and the running
    statistics, gx, ggamma and gbeta bit-identical."""
    dev = gpu_device
    C, P = cases.BN_DETERMINISM
    x, gy, gamma, beta, rm, rv = _bn_data(C, P, 5)
    runs = []
    for _ in range(2):
        rmg, rvg = rm.to(dev), rv.to(dev)
        xg, gam, bet = x.to(dev), gamma.to(dev), beta.to(dev)
        y, mean, inv = _bn_forward(dev, xg, gam, bet, rmg, rvg)
        runs.append((y, mean, inv, rmg, rvg) + _bn_backward(dev, gy.to(dev), xg, gam, bet, mean, inv))
    for i, (u, v) in enumerate(zip(*runs)):
        assert torch.equal(_bits(u), _bits(v)), i
