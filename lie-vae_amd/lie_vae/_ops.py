"""torch.autograd.Functions over the C ABI.  Forward and backward both run the HIP
kernels of liblievae_hip.so on the caller's current stream; nothing here computes on
the CPU.  The per-sample maps follow the input dtype as the reference's do (fp64 in ->
the ``*_f64`` kernels, fp64 out; anything else -> fp32); the Wigner-D / group-action
path is fp32 (the reference's own J is fp32, ``lie_tools.py:10-14``) and the S2S2
Gram–Schmidt is fp64, as in the reference (``reparameterize.py:195-197``)."""
import torch

from . import _lib
from ._lib import call, ptr, stream

F32 = torch.float32


def _prep(t, dtype=F32):
    _lib.require_device(t)
    return t.contiguous() if t.dtype == dtype else t.to(dtype).contiguous()


def _empty(shape, like, dtype=F32):
    return torch.empty(shape, device=like.device, dtype=dtype)


F64 = torch.float64


def _map_dtype(*ts):
    """Compute dtype of a per-sample map: fp64 if any floating input is fp64 (torch's
    promotion for the reference's expressions), else fp32."""
    return F64 if any(t is not None and t.dtype == F64 for t in ts) else F32


def _k(name, dtype):
    return name + "_f64" if dtype == F64 else name


def _flat(t, last):
    """View (..., *last) as (n, *last); returns the batch shape too."""
    lead = t.shape[: t.dim() - len(last)]
    n = 1
    for d in lead:
        n *= d
    return t.reshape(n, *last), lead, n


# ------------------------------------------------------------- unary maps
class _Unary(torch.autograd.Function):
    """Generic per-sample map x (n, *IN) -> y (n, *OUT) with a VJP kernel; fp32 or fp64
    following the input."""

    @staticmethod
    def forward(ctx, x, spec):
        fwd, bwd, ishape, oshape = spec
        dt = _map_dtype(x) if fwd in _F64_MAPS else F32
        xf, lead, n = _flat(_prep(x, dt), ishape)
        y = _empty((n, *oshape), xf, dt)
        call(_k(fwd, dt), ptr(xf), ptr(y), n, stream())
        ctx.save_for_backward(xf)
        ctx.spec, ctx.lead, ctx.n, ctx.dt = spec, lead, n, dt
        return y.reshape(*lead, *oshape)

    @staticmethod
    def backward(ctx, gy):
        (xf,) = ctx.saved_tensors
        fwd, bwd, ishape, oshape = ctx.spec
        gyf = _prep(gy, ctx.dt).reshape(ctx.n, *oshape)
        gx = _empty((ctx.n, *ishape), xf, ctx.dt)
        call(_k(bwd, ctx.dt), ptr(xf), ptr(gyf), ptr(gx), ctx.n, stream())
        return gx.reshape(*ctx.lead, *ishape), None


SO3_EXP = ("lv_so3_exp_fwd", "lv_so3_exp_bwd", (3,), (3, 3))
QUAT_TO_MAT = ("lv_quat_to_mat_fwd", "lv_quat_to_mat_bwd", (4,), (3, 3))
MAT_TO_QUAT = ("lv_mat_to_quat_fwd", "lv_mat_to_quat_bwd", (3, 3), (4,))
QUAT_TO_EAZYZ = ("lv_quat_to_eazyz_fwd", "lv_quat_to_eazyz_bwd", (4,), (3,))
MAT_TO_EAZYZ = ("lv_mat_to_eazyz_fwd", "lv_mat_to_eazyz_bwd", (3, 3), (3,))
SOFTPLUS = ("lv_softplus_fwd", "lv_softplus_bwd", (), ())
SO3_LOG = ("lv_so3_log_fwd", "lv_so3_log_bwd", (3, 3), (3,))
SO3_PROJECT = ("lv_so3_project_fwd", "lv_so3_project_bwd", (3, 3), (3, 3))
# maps with fp64 twins
_F64_MAPS = {s[0] for s in (SO3_EXP, QUAT_TO_MAT, MAT_TO_QUAT, QUAT_TO_EAZYZ, MAT_TO_EAZYZ,
                            SO3_LOG, SO3_PROJECT)}


def unary(x, spec):
    return _Unary.apply(x, spec)


# ----------------------------------------------------------- binary maps
class _S2S1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, axis, cs):
        dt = _map_dtype(axis, cs)
        a, lead, n = _flat(_prep(axis, dt), (3,))
        c, _, _ = _flat(_prep(cs, dt), (2,))
        r = _empty((n, 3, 3), a, dt)
        call(_k("lv_s2s1_fwd", dt), ptr(a), ptr(c), ptr(r), n, stream())
        ctx.save_for_backward(a, c)
        ctx.lead, ctx.n, ctx.dt = lead, n, dt
        return r.reshape(*lead, 3, 3)

    @staticmethod
    def backward(ctx, g):
        a, c = ctx.saved_tensors
        gf = _prep(g, ctx.dt).reshape(ctx.n, 3, 3)
        ga, gc = _empty((ctx.n, 3), a, ctx.dt), _empty((ctx.n, 2), a, ctx.dt)
        call(_k("lv_s2s1_bwd", ctx.dt), ptr(a), ptr(c), ptr(gf), ptr(ga), ptr(gc), ctx.n,
             stream())
        return ga.reshape(*ctx.lead, 3), gc.reshape(*ctx.lead, 2)


class _S2S2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v1, v2):
        f64 = torch.float64
        a, lead, n = _flat(_prep(v1, f64), (3,))
        b, _, _ = _flat(_prep(v2, f64), (3,))
        r = _empty((n, 3, 3), a, f64)
        call("lv_s2s2_fwd_f64", ptr(a), ptr(b), ptr(r), n, stream())
        ctx.save_for_backward(a, b)
        ctx.lead, ctx.n = lead, n
        return r.reshape(*lead, 3, 3)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        gf = _prep(g, torch.float64).reshape(ctx.n, 3, 3)
        g1, g2 = torch.empty_like(a), torch.empty_like(b)
        call("lv_s2s2_bwd_f64", ptr(a), ptr(b), ptr(gf), ptr(g1), ptr(g2), ctx.n, stream())
        return g1.reshape(*ctx.lead, 3), g2.reshape(*ctx.lead, 3)


class _SO3Sample(torch.autograd.Function):
    """z[s, b] = mu[b] @ exp(v[s, b]) — reparameterize.py:269-273."""

    @staticmethod
    def forward(ctx, mu, v):
        dt = _map_dtype(mu, v)
        mu = _prep(mu, dt)
        v = _prep(v, dt)
        ns, B = v.shape[0], v.shape[1]
        assert mu.shape == (B, 3, 3) and v.shape == (ns, B, 3)
        z = _empty((ns, B, 3, 3), v, dt)
        call(_k("lv_so3_sample_fwd", dt), ptr(mu), ptr(v), ptr(z), ns, B, stream())
        ctx.save_for_backward(mu, v)
        ctx.dt = dt
        return z

    @staticmethod
    def backward(ctx, gz):
        mu, v = ctx.saved_tensors
        ns, B = v.shape[0], v.shape[1]
        gz = _prep(gz, ctx.dt)
        gmu, gv = torch.empty_like(mu), torch.empty_like(v)
        call(_k("lv_so3_sample_bwd", ctx.dt), ptr(mu), ptr(v), ptr(gz), ptr(gmu), ptr(gv), ns,
             B, stream())
        return gmu, gv


class _SO3RelLog(torch.autograd.Function):
    """v[s, b] = log(mu[b]^T z[s, b]), the inverse of _SO3Sample; tangent-space gradients
    (include/lievae.h lv_so3_rel_log_bwd)."""

    @staticmethod
    def forward(ctx, mu, z):
        dt = _map_dtype(mu, z)
        mu = _prep(mu, dt)
        z = _prep(z, dt)
        ns, B = z.shape[0], z.shape[1]
        v = _empty((ns, B, 3), z, dt)
        call(_k("lv_so3_rel_log_fwd", dt), ptr(mu), ptr(z), ptr(v), ns, B, stream())
        ctx.save_for_backward(mu, z)
        ctx.dt = dt
        return v

    @staticmethod
    def backward(ctx, gv):
        mu, z = ctx.saved_tensors
        ns, B = z.shape[0], z.shape[1]
        gv = _prep(gv, ctx.dt)
        gmu, gz = torch.empty_like(mu), torch.empty_like(z)
        call(_k("lv_so3_rel_log_bwd", ctx.dt), ptr(mu), ptr(z), ptr(gv), ptr(gmu), ptr(gz), ns,
             B, stream())
        return gmu, gz


def so3_rel_log(mu, z):
    """mu (B,3,3), z (ns,B,3,3) rotations -> v (ns,B,3) with z = mu exp(v), |v| <= pi;
    differentiable in both."""
    assert z.dim() == 4 and tuple(z.shape[2:]) == (3, 3), \
        f"so3_rel_log: z must be (ns, B, 3, 3), got {tuple(z.shape)}"
    assert tuple(mu.shape) == (z.shape[1], 3, 3), \
        f"so3_rel_log: mu must be ({z.shape[1]},3,3), got {tuple(mu.shape)}"
    _lib.require_device(mu, z)
    return _SO3RelLog.apply(mu, z)


class _SO3Angle(torch.autograd.Function):
    """theta = rotation angle of A^T B, in [0, pi] (include/lievae.h lv_so3_angle_fwd)."""

    @staticmethod
    def forward(ctx, A, B):
        dt = _map_dtype(A, B)
        a, lead, n = _flat(_prep(A, dt), (3, 3))
        b, _, _ = _flat(_prep(B, dt), (3, 3))
        th = _empty((n,), a, dt)
        call(_k("lv_so3_angle_fwd", dt), ptr(a), ptr(b), ptr(th), n, stream())
        ctx.save_for_backward(a, b)
        ctx.lead, ctx.n, ctx.dt = lead, n, dt
        return th.reshape(lead)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        gf = _prep(g, ctx.dt).reshape(ctx.n)
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        call(_k("lv_so3_angle_bwd", ctx.dt), ptr(a), ptr(b), ptr(gf), ptr(ga), ptr(gb), ctx.n,
             stream())
        return ga.reshape(*ctx.lead, 3, 3), gb.reshape(*ctx.lead, 3, 3)


def so3_angle(A, B):
    """A, B (...,3,3) rotations of one shape -> the rotation angle of A^T B (...), in [0, pi];
    differentiable in both (gradient 0 where the angle is 0)."""
    assert A.dim() >= 2 and tuple(A.shape[-2:]) == (3, 3) and A.shape == B.shape, \
        f"so3_angle: A and B must be (...,3,3) of one shape, got {tuple(A.shape)} and {tuple(B.shape)}"
    _lib.require_device(A, B)
    return _SO3Angle.apply(A, B)


# ------------------------------------------------- rotation moment, mean, alignment
MOMENT_MAX_NS = 8  # csrc/so3_stats.hip kMomentMaxNs


def so3_moment(X, Y=None, weights=None, C=None, flags=0, project=True):
    """S[s] = sum_i w_i op(X_i) C_s op(Y_i) (include/lievae.h lv_so3_moment): X, Y (n,3,3), weights
    (n) or None, C (ns,3,3) or None (the identity, ns = 1), flags of _lib.LV_MOMENT_XT / _YT /
    _CT.  Returns S (ns,3,3) fp64, wsum () fp64 and R (ns,3,3) = project(S) in the inputs'
    dtype (None with project=False).  Two launches on the current stream, no host sync, bitwise
    reproducible.  Forward only: inputs that require grad are refused."""
    assert X.dim() == 3 and tuple(X.shape[1:]) == (3, 3), \
        f"so3_moment: X must be (n,3,3), got {tuple(X.shape)}"
    n = X.shape[0]
    assert Y is None or tuple(Y.shape) == (n, 3, 3), \
        f"so3_moment: Y must be ({n},3,3), got {tuple(Y.shape)}"
    assert weights is None or tuple(weights.shape) == (n,), \
        f"so3_moment: weights must be ({n},), got {tuple(weights.shape)}"
    ns = 1 if C is None else C.shape[0]
    assert C is None or (C.dim() == 3 and tuple(C.shape[1:]) == (3, 3)
                         and 1 <= ns <= MOMENT_MAX_NS), \
        f"so3_moment: C must be (ns,3,3) with 1 <= ns <= {MOMENT_MAX_NS}, got {tuple(C.shape)}"
    _lib.require_device(X, Y, weights, C)
    if any(t is not None and t.requires_grad for t in (X, Y, weights, C)):
        raise RuntimeError("so3_moment (so3_mean, align_rotations) has no backward; detach the "
                           "inputs")
    dt = _map_dtype(X, Y, weights, C)
    X, Y, weights, C = (None if t is None else _prep(t, dt) for t in (X, Y, weights, C))
    dev = X.device
    S = torch.empty((ns, 3, 3), device=dev, dtype=F64)
    wsum = torch.empty((), device=dev, dtype=F64)
    R = torch.empty((ns, 3, 3), device=dev, dtype=dt) if project else None
    nb = int(_lib.load().lv_so3_moment_workspace(n, ns))
    ws = torch.empty(max(nb, 8), device=dev, dtype=torch.uint8)
    call(_k("lv_so3_moment", dt), ptr(X), ptr(Y), ptr(weights), ptr(C), ns, flags, ptr(S),
         ptr(wsum), ptr(R), n, ptr(ws), nb, _lib.stream_of(dev))
    return S, wsum, R


def so3_mean(R, weights=None):
    """Chordal mean of rotations: (n,3,3) -> (3,3), the projection of sum_i w_i R_i."""
    return so3_moment(R, weights=weights)[2][0]


def _half_turn_starts(device, dtype):
    """The identity and the half-turns about x, y, z, (4,3,3); built by device kernels only
    (no host-to-device copy, so it can be captured in a graph)."""
    s = torch.arange(4, device=device)[:, None]
    j = torch.arange(3, device=device)[None, :]
    return torch.diag_embed(((s == 0) | (s == j + 1)).to(dtype) * 2 - 1)


def align_rotations(Z, G, side='both', weights=None, rounds=16):
    """(A, B, rms) minimising sum_i w_i |Z_i - A G_i B|_F^2 over rotations; Z, G (n,3,3).
    'left' fixes B = I and 'right' fixes A = I: one closed-form Procrustes step each (one
    lv_so3_moment).  'both' alternates the two steps `rounds` times from four starts of B --
    the identity and the half-turns about x, y, z, carried as ns = 4 through the same launches
    -- and keeps the start of lowest residual, selected on the device.  rms =
    sqrt(residual / sum w), from the last moment: residual = 6 wsum - 2 tr(B^T S) (a difference:
    an exact fit reads as ~sqrt(eps) of the rotations' dtype, not 0).  No host sync: capturable
    in a graph.  Forward only."""
    assert side in ('both', 'left', 'right'), f"align_rotations: side {side!r}"
    assert Z.dim() == 3 and tuple(Z.shape[1:]) == (3, 3) and G.shape == Z.shape, \
        f"align_rotations: Z and G must be (n,3,3) of one shape, got {tuple(Z.shape)} and " \
        f"{tuple(G.shape)}"
    _lib.require_device(Z, G, weights)
    dt = _map_dtype(Z, G, weights)
    XT, YT, CT = _lib.LV_MOMENT_XT, _lib.LV_MOMENT_YT, _lib.LV_MOMENT_CT
    if side != 'both':
        if side == 'left':
            S, wsum, R = so3_moment(Z, G, weights, None, YT)
        else:
            S, wsum, R = so3_moment(G, Z, weights, None, XT)
        eye = torch.eye(3, device=Z.device, dtype=dt)
        res = 6 * wsum - 2 * (R[0].double() * S[0]).sum()
        rms = torch.sqrt(res.clamp(min=0) / wsum).to(dt)
        return (R[0], eye, rms) if side == 'left' else (eye, R[0], rms)
    assert rounds >= 1, "align_rotations: rounds must be >= 1"
    Bs = _half_turn_starts(Z.device, dt)
    for _ in range(rounds):
        As = so3_moment(Z, G, weights, Bs, YT | CT)[2]
        S, wsum, Bs = so3_moment(G, Z, weights, As, XT | CT)
    res = 6 * wsum - 2 * (Bs.double() * S).sum((-1, -2))
    k = torch.argmin(res).reshape(1)
    A, B = As.index_select(0, k)[0], Bs.index_select(0, k)[0]
    rms = torch.sqrt(res.index_select(0, k)[0].clamp(min=0) / wsum).to(dt)
    return A, B, rms


class _N0Sample(torch.autograd.Function):
    """v[s, b] = eps[s, b] * sigma[b] — reparameterize.py:137-141 (eps given)."""

    @staticmethod
    def forward(ctx, sigma, eps):
        sigma = _prep(sigma)
        eps = _prep(eps)
        ns, B = eps.shape[0], eps.shape[1]
        v = torch.empty_like(eps)
        call("lv_n0_sample_fwd", ptr(sigma), ptr(eps), ptr(v), ns, B, stream())
        ctx.save_for_backward(eps)
        return v

    @staticmethod
    def backward(ctx, gv):
        (eps,) = ctx.saved_tensors
        ns, B = eps.shape[0], eps.shape[1]
        gs = _empty((B, 3), eps)
        call("lv_n0_sample_bwd", ptr(eps), ptr(_prep(gv)), ptr(gs), ns, B, stream())
        return gs, None


class _SO3LogPosterior(torch.autograd.Function):
    """log q(exp(v) | sigma), 2k+1 wrapped terms — reparameterize.py:233-263."""

    @staticmethod
    def forward(ctx, v, sigma, k):
        v = _prep(v)
        sigma = _prep(sigma)
        ns, B = v.shape[0], v.shape[1]
        out = _empty((ns, B), v)
        call("lv_so3_log_posterior_fwd", ptr(v), ptr(sigma), ptr(out), ns, B, k, stream())
        ctx.save_for_backward(v, sigma)
        ctx.k = k
        return out

    @staticmethod
    def backward(ctx, g):
        v, sigma = ctx.saved_tensors
        ns, B = v.shape[0], v.shape[1]
        gv, gs = torch.empty_like(v), torch.empty_like(sigma)
        call("lv_so3_log_posterior_bwd", ptr(v), ptr(sigma), ptr(_prep(g)), ptr(gv), ptr(gs),
             ns, B, ctx.k, stream())
        return gv, gs, None


# ------------------------------------------------------- vMF latent on S^3
I32 = torch.int32


class _VmfSample(torch.autograd.Function):
    """z[s, b] ~ vMF(mu[b], kappa[b]) from the standard normals noise[s, b] (6 trials + 3 per
    sample) -- reparameterize.py:90-93; also returns the accepted trial's index."""

    @staticmethod
    def forward(ctx, mu, kappa, noise):
        mu, kappa, noise = _prep(mu), _prep(kappa), _prep(noise)
        ns, B, W = noise.shape
        trials = (W - 3) // 6
        z = _empty((ns, B, 4), noise)
        acc = _empty((ns, B), noise, I32)
        call("lv_vmf_sample_fwd", ptr(mu), ptr(kappa), ptr(noise), ptr(z), ptr(acc), ns, B, trials,
             stream())
        ctx.save_for_backward(mu, kappa, noise, acc)
        ctx.mark_non_differentiable(acc)
        ctx.trials = trials
        return z, acc

    @staticmethod
    def backward(ctx, gz, _gacc):
        mu, kappa, noise, acc = ctx.saved_tensors
        ns, B = acc.shape
        new = torch.zeros_like if ns == 0 else torch.empty_like  # no samples: nothing is launched
        gmu, gk = new(mu), new(kappa)
        call("lv_vmf_sample_bwd", ptr(mu), ptr(kappa), ptr(noise), ptr(acc), ptr(_prep(gz)),
             ptr(gmu), ptr(gk), ns, B, ctx.trials, stream())
        return gmu, gk, None


class _VmfKL(torch.autograd.Function):
    """KL(vMF(., kappa) || U(S^3)) per datum -- reparameterize.py:79-82."""

    @staticmethod
    def forward(ctx, kappa):
        kappa = _prep(kappa)
        kl = torch.empty_like(kappa)
        call("lv_vmf_kl_fwd", ptr(kappa), ptr(kl), kappa.shape[0], stream())
        ctx.save_for_backward(kappa)
        return kl

    @staticmethod
    def backward(ctx, g):
        (kappa,) = ctx.saved_tensors
        gk = torch.empty_like(kappa)
        call("lv_vmf_kl_bwd", ptr(kappa), ptr(_prep(g)), ptr(gk), kappa.shape[0], stream())
        return gk


class _VmfLogProb(torch.autograd.Function):
    """log q(z[s, b] | mu[b], kappa[b]) -- reparameterize.py:84-85."""

    @staticmethod
    def forward(ctx, mu, kappa, z):
        mu, kappa, z = _prep(mu), _prep(kappa), _prep(z)
        ns, B = z.shape[0], z.shape[1]
        out = _empty((ns, B), z)
        call("lv_vmf_log_prob_fwd", ptr(mu), ptr(kappa), ptr(z), ptr(out), ns, B, stream())
        ctx.save_for_backward(mu, kappa, z)
        return out

    @staticmethod
    def backward(ctx, g):
        mu, kappa, z = ctx.saved_tensors
        ns, B = z.shape[0], z.shape[1]
        new = torch.zeros_like if ns == 0 else torch.empty_like
        gmu, gk, gz = new(mu), new(kappa), torch.empty_like(z)
        call("lv_vmf_log_prob_bwd", ptr(mu), ptr(kappa), ptr(z), ptr(_prep(g)), ptr(gmu), ptr(gk),
             ptr(gz), ns, B, stream())
        return gmu, gk, gz


VMF_MAX_TRIALS = 64  # csrc/vmf.hip kVmfMaxTrials
_VMF_ACCEPTED = None


def _check_vmf(mu, kappa, B, what):
    assert tuple(mu.shape) == (B, 4), f"{what}: mu must be ({B},4), got {tuple(mu.shape)}"
    assert tuple(kappa.shape) == (B,), f"{what}: kappa must be ({B},), got {tuple(kappa.shape)}"


def vmf_sample(mu, kappa, noise):
    """mu (B,4) unit, kappa (B), noise (ns, B, 6 T + 3) standard normals -> z (ns, B, 4) on
    S^3; T = the number of rejection trials, 1..64, read off the noise's width.  Differentiable
    in mu and kappa (pathwise).  vmf_last_accepted() gives the accepted trial per sample."""
    global _VMF_ACCEPTED
    assert noise.dim() == 3, f"vmf_sample: noise must be (ns, B, 6T+3), got {tuple(noise.shape)}"
    W = noise.shape[2]
    assert W >= 9 and (W - 3) % 6 == 0 and (W - 3) // 6 <= VMF_MAX_TRIALS, \
        f"vmf_sample: noise width must be 6T+3 with 1 <= T <= {VMF_MAX_TRIALS}, got {W}"
    _check_vmf(mu, kappa, noise.shape[1], "vmf_sample")
    _lib.require_device(mu, kappa, noise)
    z, _VMF_ACCEPTED = _VmfSample.apply(mu, kappa, noise.detach())
    return z


def vmf_last_accepted():
    """(ns, B) int32 of the last vmf_sample call: the index of the accepted trial, or T where
    none of the T was accepted and the last proposal was used.  Carries no gradient."""
    return _VMF_ACCEPTED


def vmf_kl(kappa):
    """kappa (B) -> KL(vMF || uniform on S^3) (B); differentiable."""
    assert kappa.dim() == 1, f"vmf_kl: kappa must be (B,), got {tuple(kappa.shape)}"
    _lib.require_device(kappa)
    return _VmfKL.apply(kappa)


def vmf_log_prob(mu, kappa, z):
    """mu (B,4), kappa (B), z (ns, B, 4) -> log q(z) (ns, B); differentiable in all three."""
    assert z.dim() == 3 and z.shape[2] == 4, \
        f"vmf_log_prob: z must be (ns, B, 4), got {tuple(z.shape)}"
    _check_vmf(mu, kappa, z.shape[1], "vmf_log_prob")
    _lib.require_device(mu, kappa, z)
    return _VmfLogProb.apply(mu, kappa, z)


# ------------------------------------------------------------ group action
_WS_BYTES = {}   # (n, L, C, shared F) -> lv_group_action_bwd_workspace
_WS_BUF = {}     # (device index, raw stream) -> cached uint8 workspace (eager calls only)


def _bwd_workspace(n, L, C, shared, device):
    """The backward's workspace: its size queried once per shape, the buffer reused per
    (device, stream) for eager calls (stream order serialises its users).  Under graph
    capture a fresh allocation from the graph's pool keeps replays independent of eager
    calls on other streams."""
    key = (n, L, C, shared)
    nb = _WS_BYTES.get(key)
    if nb is None:
        nb = _WS_BYTES[key] = int(_lib.load().lv_group_action_bwd_workspace(n, L, C, shared))
    st = _lib.stream_of(device)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(nb, 1), device=device, dtype=torch.uint8), nb, st
    bkey = (device.index, st)
    buf = _WS_BUF.get(bkey)
    if buf is None or buf.numel() < nb:
        buf = _WS_BUF[bkey] = torch.empty(max(nb, 1 << 20), device=device, dtype=torch.uint8)
    return buf, nb, st


class _GroupAction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, angles, spec, L, transpose, out_dtype):
        angles = _prep(angles)
        n = angles.shape[0]
        M = (L + 1) ** 2
        C = spec.shape[-1]
        stride = 0 if spec.dim() == 2 else M * C
        dt = _lib.LV_DTYPE_BF16 if out_dtype == torch.bfloat16 else _lib.LV_DTYPE_F32
        out = _empty((n, M, C), angles, out_dtype)
        call("lv_group_action_fwd", ptr(angles), ptr(spec), stride, ptr(out), dt, n, L, C,
             int(transpose), stream())
        ctx.save_for_backward(angles, spec)
        ctx.L, ctx.transpose, ctx.stride = L, transpose, stride
        return out

    @staticmethod
    def backward(ctx, gout):
        angles, spec = ctx.saved_tensors
        n, L, C = angles.shape[0], ctx.L, spec.shape[-1]
        gout = _prep(gout)
        gang = torch.empty_like(angles)
        gspec = torch.empty_like(spec)
        ws, ws_bytes, st = _bwd_workspace(n, L, C, int(ctx.stride == 0), angles.device)
        call("lv_group_action_bwd", ptr(angles), ptr(spec), ctx.stride, ptr(gout), ptr(gang),
             ptr(gspec), n, L, C, int(ctx.transpose), ws.data_ptr(), ws_bytes, st)
        return gang, gspec, None, None, None


def _check_spectrum(spectrum, n, L, what):
    """The shape contract of block_wigner_matrix_multiply (lie_tools.py:226-253), where
    the reference's bmm would raise: spectrum (M, C) or (n, M, C) with M = (L+1)^2.  A
    stride-0 batch expand of (M, C) (ActionNet's item_rep, decoders.py:53) collapses to
    the shared form.  Checked here because the kernels trust these sizes."""
    M = (L + 1) ** 2
    assert spectrum.dim() in (2, 3), f"{what}: spectrum must be (M,C) or (n,M,C), " \
                                     f"got {tuple(spectrum.shape)}"
    assert spectrum.shape[-2] == M, f"{what}: spectrum rows {spectrum.shape[-2]} != " \
                                    f"(L+1)^2 = {M}"
    if spectrum.dim() == 3:
        assert spectrum.shape[0] == n, f"{what}: spectrum batch {spectrum.shape[0]} != " \
                                       f"number of samples {n}"
        if spectrum.stride(0) == 0:
            # (M,C) passed once; autograd routes dF through expand back to item_rep
            spectrum = spectrum.as_strided(spectrum.shape[1:], spectrum.stride()[1:])
    return spectrum


def _check_out_dtype(out_dtype, what):
    """The kernels write fp32 or bf16 output only; anything else would be written with
    the wrong element size (checked before either path, Python or C++ operator)."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"{what}: out_dtype must be torch.float32 or torch.bfloat16, "
                         f"got {out_dtype}")


def group_action(angles, spectrum, L, transpose=False, out_dtype=F32):
    """block_wigner_matrix_multiply on the HIP path; angles (n,3), spectrum (M,C),
    (n,M,C) or a stride-0 expand of (M,C)."""
    assert angles.dim() == 2 and angles.shape[1] == 3, \
        f"angles must be (n,3), got {tuple(angles.shape)}"
    _check_out_dtype(out_dtype, "group_action")
    spectrum = _check_spectrum(spectrum, angles.shape[0], L, "group_action")
    _lib.require_device(angles, spectrum)
    return _GroupAction.apply(angles, _contig(spectrum), L, transpose, out_dtype)


def _contig(t):
    return t.contiguous() if t.dtype == F32 else t.float().contiguous()


def _f32c(t):
    """t itself when already fp32 and contiguous (the common case: no dispatcher call)."""
    return t if t.dtype == F32 and t.is_contiguous() else t.to(F32).contiguous()


class _FusedExpAction(torch.autograd.Function):
    """mu@exp(v) -> ZYZ -> block D·F in one launch; backward = one tile-kernel launch
    (group-action backward) + one launch of the dF slab reduce with the exp -> ZYZ VJP
    beside it.
    Host path kept short (the eager training direction is host-bound at config 2): no
    conversion calls on already-fp32 contiguous inputs, the workspace cached per stream."""

    @staticmethod
    def forward(ctx, mu, v, spec, L, transpose, out_dtype):
        v = _f32c(v)
        n = v.shape[0]
        mu_c = _f32c(mu) if mu is not None else None
        M = (L + 1) ** 2
        C = spec.shape[-1]
        dev = v.device
        out = torch.empty((n, M, C), device=dev, dtype=out_dtype)
        ang = torch.empty((n, 3), device=dev, dtype=F32)
        call("lv_fused_exp_action_fwd", None if mu_c is None else mu_c.data_ptr(), v.data_ptr(),
             spec.data_ptr(), 0, out.data_ptr(),
             _lib.LV_DTYPE_BF16 if out_dtype == torch.bfloat16 else _lib.LV_DTYPE_F32,
             ang.data_ptr(), n, L, C, int(transpose), _lib.stream_of(dev))
        ctx.save_for_backward(mu_c, v, spec, ang)
        ctx.L, ctx.transpose = L, transpose
        return out

    @staticmethod
    def backward(ctx, gout):
        mu, v, spec, ang = ctx.saved_tensors
        n, L, C = v.shape[0], ctx.L, spec.shape[-1]
        gout = _f32c(gout)
        dev = v.device
        gspec, gv = torch.empty_like(spec), torch.empty_like(v)
        gmu = torch.empty_like(mu) if mu is not None else None
        ws, ws_bytes, st = _bwd_workspace(n, L, C, 1, dev)
        call("lv_fused_exp_action_bwd", None if mu is None else mu.data_ptr(), v.data_ptr(),
             ang.data_ptr(), spec.data_ptr(), gout.data_ptr(),
             None if gmu is None else gmu.data_ptr(), gv.data_ptr(), gspec.data_ptr(), n, L, C,
             int(ctx.transpose), ws.data_ptr(), ws_bytes, st)
        return gmu, gv, gspec, None, None, None


_TORCH_OPS = _lib.load_torch_ops()  # liblievae_torch.so: the op as a C++ autograd function


def fused_exp_action(mu, v, spectrum, L, transpose=False, out_dtype=F32):
    """(mu (n,3,3) or None, v (n,3), spectrum (M,C) or a stride-0 expand of it) ->
    (n, M, C).  The fused kernel takes a shared spectrum only (ActionNet's item_rep);
    a per-sample spectrum goes through group_action.  Runs as the C++ operator
    torch.ops.lievae.fused_exp_action (csrc/torch_ops.cpp: forward, backward and autograd
    bookkeeping without Python frames) when liblievae_torch.so is built, else through the
    Python autograd.Function below -- the same kernels either way."""
    assert v.dim() == 2 and v.shape[1] == 3, f"v must be (n,3), got {tuple(v.shape)}"
    n = v.shape[0]
    if mu is not None:
        assert tuple(mu.shape) == (n, 3, 3), f"mu must be ({n},3,3), got {tuple(mu.shape)}"
    _check_out_dtype(out_dtype, "fused_exp_action")
    spectrum = _check_spectrum(spectrum, n, L, "fused_exp_action")
    if spectrum.dim() != 2:
        raise ValueError("fused_exp_action takes a shared (M,C) spectrum; use group_action "
                         "for a per-sample (n,M,C) spectrum")
    _lib.require_device(v, spectrum, mu)
    if _TORCH_OPS:
        return torch.ops.lievae.fused_exp_action(mu, v, spectrum, L, bool(transpose),
                                                 out_dtype == torch.bfloat16)
    return _FusedExpAction.apply(mu, v, _f32c(spectrum), L, transpose, out_dtype)


class _WignerD(torch.autograd.Function):
    """angles (n, 3) -> D: one degree's block (n, (2l+1)^2) or the packed blocks 0..L
    (n, sum (2l+1)^2).  fp32 whatever the input dtype; the angle gradient comes back in the
    input's dtype, with the values computed in fp32."""

    @staticmethod
    def forward(ctx, angles, l, packed):
        a = _prep(angles)
        n = a.shape[0]
        width = (l + 1) * (2 * l + 1) * (2 * l + 3) // 3 if packed else (2 * l + 1) ** 2
        D = _empty((n, width), a)
        call("lv_wigner_d_fwd" if packed else "lv_wigner_d_block_fwd", ptr(a), ptr(D), n, l,
             _lib.stream_of(a.device))
        ctx.save_for_backward(a)
        ctx.l, ctx.packed, ctx.in_dtype = l, packed, angles.dtype
        return D

    @staticmethod
    def backward(ctx, gD):
        (a,) = ctx.saved_tensors
        gD = _prep(gD)  # contiguous fp32: the upstream may be a transposed view
        gang = torch.empty_like(a)
        call("lv_wigner_d_bwd" if ctx.packed else "lv_wigner_d_block_bwd", ptr(a), ptr(gD),
             ptr(gang), a.shape[0], ctx.l, _lib.stream_of(a.device))
        return gang.to(ctx.in_dtype), None, None


def _check_angles(angles, what):
    assert angles.dim() == 2 and angles.shape[1] == 3, \
        f"{what}: angles must be (n,3), got {tuple(angles.shape)}"
    _lib.require_device(angles)


def wigner_blocks(angles, L):
    """Packed D_0..D_L for each angle triple, (n, sum (2l+1)^2); differentiable in the
    angles (lv_wigner_d_bwd)."""
    _check_angles(angles, "wigner_blocks")
    return _WignerD.apply(angles, L, True)


def wigner_block(angles, l):
    """D_l alone for each angle triple, (n, (2l+1)^2) row-major, in one launch;
    differentiable in the angles (lv_wigner_d_block_bwd)."""
    _check_angles(angles, "wigner_block")
    return _WignerD.apply(angles, l, False)


# ------------------------------------------------------ encoder regularisers
def rotate_images(img, cs, align_corners=False, flags=0):
    """EquivarianceLoss.rotate on the HIP path (losses/equivariance_loss.py:50-57): img
    (N, C, H, W) rotated per image by the angle of cs (N, 2) = (cos, sin), bilinear taps,
    zeros outside.  No backward (the reference never differentiates the image): an input
    that requires grad is refused.  flags: _lib.LV_ROTATE_DIRECT forces the direct path."""
    assert img.dim() == 4, f"img must be (N,C,H,W), got {tuple(img.shape)}"
    assert tuple(cs.shape) == (img.shape[0], 2), \
        f"cs must be ({img.shape[0]},2), got {tuple(cs.shape)}"
    if img.requires_grad or cs.requires_grad:
        raise RuntimeError("rotate_images has no backward (the reference rotates its input "
                           "image with angles drawn without gradient); detach the inputs")
    _lib.require_device(img, cs)
    img, cs = _f32c(img), _f32c(cs)
    N, C, H, W = img.shape
    out = torch.empty_like(img)
    call("lv_rotate_bilinear_fwd", ptr(img), ptr(cs), ptr(out), N, C, H, W,
         int(bool(align_corners)), flags, _lib.stream_of(img.device))
    return out


# ------------------------------------------------------ sphere-cube renderer
def render_spherecube(g, size=64, rgb=True, samples=2, flags=0):
    """Images of the sphere-cube scene seen from the poses g (csrc/render.hip; the data the
    reference's SphereCubeDataset reads from disk): g (n,3,3) camera frames, or (n,4)
    scalar-last quaternions (through quaternions_to_group_matrix) -> (n, 3 | 1, size, size)
    fp32 in [0, 1] on g's device, each pixel the mean of samples x samples sub-samples.  One
    launch, no host sync; forward only (no gradient reaches g).  flags:
    _lib.LV_RENDER_SCALAR forces the one-pixel path (same bits)."""
    quats = g.dim() == 2 and g.shape[1] == 4
    assert quats or (g.dim() == 3 and tuple(g.shape[1:]) == (3, 3)), \
        f"g must be matrices (n,3,3) or quaternions (n,4), got {tuple(g.shape)}"
    _lib.require_device(g)
    g = g.detach()
    R = _f32c(unary(g, QUAT_TO_MAT) if quats else g)
    n, C = R.shape[0], 3 if rgb else 1
    out = torch.empty((n, C, size, size), device=R.device, dtype=F32)
    call("lv_render_spherecube_fwd", ptr(R), ptr(out), n, size, C, samples, flags,
         _lib.stream_of(R.device))
    return out


# ------------------------------------------------------ triangle-mesh renderer
def mesh_pack(vertices, faces, albedo, records, bad_counter):
    """One mesh into its slice of a record tensor (csrc/render_mesh.hip mesh_pack_k): vertices
    (V,3) fp32, faces (T,3) int32, albedo (T,3) fp32 -> records (T,16) fp32 (a contiguous,
    16-byte aligned view); ``bad_counter`` (one int32 element) counts the triangles with a
    face index outside [0, V).  No host sync."""
    _lib.require_device(vertices, faces, albedo, records, bad_counter)
    V, T = vertices.shape[0], faces.shape[0]
    assert vertices.dtype == F32 and vertices.is_contiguous() and tuple(vertices.shape) == (V, 3)
    assert faces.dtype == torch.int32 and faces.is_contiguous() and tuple(faces.shape) == (T, 3)
    assert albedo.dtype == F32 and albedo.is_contiguous() and tuple(albedo.shape) == (T, 3)
    assert records.dtype == F32 and records.is_contiguous() and tuple(records.shape) == (T, 16)
    assert bad_counter.dtype == torch.int32 and bad_counter.numel() == 1
    call("lv_mesh_pack", ptr(vertices), V, ptr(faces), ptr(albedo), T, ptr(records),
         ptr(bad_counter), _lib.stream_of(records.device))


def render_mesh(g, meshes, mesh_id=None, size=64, rgb=True, samples=2, flags=0, max_blocks=0):
    """Images of packed triangle meshes seen from the poses g (csrc/render_mesh.hip): g (n,3,3)
    camera frames or (n,4) scalar-last quaternions, ``meshes`` a meshes.MeshSet on g's device,
    ``mesh_id`` (n,) integers choosing each image's mesh (None: mesh 0; an id outside [0, K)
    renders the background) -> (n, 3 | 1, size, size) fp32 in [0, 1].  One launch, no host
    sync; forward only.  flags: _lib.LV_MESH_SCALAR forces the one-pixel path (same bits);
    max_blocks caps the grid (0: the default cap)."""
    quats = g.dim() == 2 and g.shape[1] == 4
    assert quats or (g.dim() == 3 and tuple(g.shape[1:]) == (3, 3)), \
        f"g must be matrices (n,3,3) or quaternions (n,4), got {tuple(g.shape)}"
    _lib.require_device(g, meshes.records, mesh_id)
    g = g.detach()
    R = _f32c(unary(g, QUAT_TO_MAT) if quats else g)
    n, C = R.shape[0], 3 if rgb else 1
    if mesh_id is not None:
        assert mesh_id.dim() == 1 and mesh_id.shape[0] == n and not mesh_id.is_floating_point(), \
            f"mesh_id must be (n,) integers, got {tuple(mesh_id.shape)} {mesh_id.dtype}"
        mesh_id = mesh_id.to(torch.int64).contiguous()
    out = torch.empty((n, C, size, size), device=R.device, dtype=F32)
    call("lv_render_mesh_fwd", ptr(R), ptr(mesh_id), ptr(meshes.records), ptr(meshes.ranges),
         meshes.K, meshes.total_records, ptr(out), n, size, C, samples, flags, max_blocks,
         _lib.stream_of(R.device))
    return out


# ------------------------------------------------- spherical harmonics on S^2
def _s2_points(x, what):
    assert x.dim() == 2 and x.shape[1] == 3, f"{what}: x must be (P,3), got {tuple(x.shape)}"
    return _f32c(x.detach())


def s2_harmonics(x, L):
    """x (P,3) -> Y (P,(L+1)^2), the real harmonics of csrc/s2.hip; forward only."""
    x = _s2_points(x, "s2_harmonics")
    _lib.require_device(x)
    P = x.shape[0]
    Y = torch.empty((P, (L + 1) ** 2), device=x.device, dtype=F32)
    call("lv_s2_harmonics_fwd", ptr(x), ptr(Y), P, L, _lib.stream_of(x.device))
    return Y


def _s2_synthesis_raw(spec, x, L, scale=None):
    """spec (M,C) or (B,M,C), x (P,3), both fp32 contiguous -> (P,C) or (B,P,C); `scale` (P)
    multiplies the rows of the result (the analysis VJP)."""
    shared = spec.dim() == 2
    B, C, P = (1 if shared else spec.shape[0]), spec.shape[-1], x.shape[0]
    out = torch.empty((B, P, C), device=spec.device, dtype=F32)
    call("lv_s2_synthesis_fwd", ptr(spec), 0 if shared else spec.shape[1] * C, ptr(x), ptr(out),
         B, P, L, C, _lib.stream_of(spec.device))
    if scale is not None:
        out = out * scale[None, :, None]
    return out[0] if shared else out


def _s2_analysis_raw(values, x, w, L):
    """values (P,C) or (B,P,C), x (P,3), w (P) or None, all fp32 contiguous -> (M,C) or
    (B,M,C)."""
    shared = values.dim() == 2
    B, P, C = (1 if shared else values.shape[0]), values.shape[-2], values.shape[-1]
    M = (L + 1) ** 2
    dev = values.device
    if P == 0:  # the empty sum; nothing is launched
        F = torch.zeros((B, M, C), device=dev, dtype=F32)
    else:
        F = torch.empty((B, M, C), device=dev, dtype=F32)
        nb = int(_lib.load().lv_s2_analysis_workspace(B, P, L, C))
        ws = torch.empty(max(nb, 8), device=dev, dtype=torch.uint8)
        call("lv_s2_analysis_fwd", ptr(values), ptr(x), ptr(w), ptr(F), B, P, L, C, ptr(ws), nb,
             _lib.stream_of(dev))
    return F[0] if shared else F


class _S2Synthesis(torch.autograd.Function):
    """values = Y(x) spectrum; the VJP in the spectrum is the analysis kernel with unit
    weights.  A shared (M,C) spectrum comes back as (P,C)."""

    @staticmethod
    def forward(ctx, spec, x, L):
        ctx.save_for_backward(x)
        ctx.L = L
        return _s2_synthesis_raw(spec, x, L)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return _s2_analysis_raw(_f32c(g), x, None, ctx.L), None, None


class _S2Analysis(torch.autograd.Function):
    """spectrum = Y(x)^T diag(w) values; the VJP in the values is the synthesis kernel, its rows
    scaled by w."""

    @staticmethod
    def forward(ctx, values, x, w, L):
        ctx.save_for_backward(x, w)
        ctx.L = L
        return _s2_analysis_raw(values, x, w, L)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return _s2_synthesis_raw(_f32c(g), x, ctx.L, scale=w), None, None, None


def _s2_degrees(rows, what):
    L = int(round(rows ** 0.5)) - 1
    assert L >= 0 and (L + 1) ** 2 == rows, f"{what}: spectrum rows {rows} != (L+1)^2"
    return L


def s2_synthesis(spectrum, x):
    """spectrum (M,C), (B,M,C) or a stride-0 expand of (M,C); x (P,3) shared by the batch ->
    (P,C) for a shared spectrum, else (B,P,C).  Differentiable in the spectrum only."""
    assert spectrum.dim() in (2, 3), \
        f"s2_synthesis: spectrum must be (M,C) or (B,M,C), got {tuple(spectrum.shape)}"
    L = _s2_degrees(spectrum.shape[-2], "s2_synthesis")
    x = _s2_points(x, "s2_synthesis")
    _lib.require_device(spectrum, x)
    expand = None
    if spectrum.dim() == 3 and spectrum.stride(0) == 0:
        # (M,C) passed once; autograd routes the gradient through the views back to the block
        expand = spectrum.shape[0]
        spectrum = spectrum.as_strided(spectrum.shape[1:], spectrum.stride()[1:])
    out = _S2Synthesis.apply(_contig(spectrum), x, L)
    return out if expand is None else out.expand(expand, -1, -1)


def s2_analysis(values, x, weights, L):
    """values (P,C) or (B,P,C), x (P,3), weights (P) or None -> (M,C) or (B,M,C).
    Differentiable in the values only."""
    assert values.dim() in (2, 3), \
        f"s2_analysis: values must be (P,C) or (B,P,C), got {tuple(values.shape)}"
    x = _s2_points(x, "s2_analysis")
    P = x.shape[0]
    assert values.shape[-2] == P, f"s2_analysis: values rows {values.shape[-2]} != points {P}"
    assert weights is None or tuple(weights.shape) == (P,), \
        f"s2_analysis: weights must be ({P},), got {tuple(weights.shape)}"
    _lib.require_device(values, x, weights)
    if weights is not None:
        weights = _f32c(weights.detach())
    return _S2Analysis.apply(_contig(values), x, weights, L)


class _EquivarianceDiff(torch.autograd.Function):
    """diffs[n] = sum (g_n enc_n - enc_rot_n)^2, g = s2s1rodrigues(e_x, cs) --
    losses/equivariance_loss.py:28-36.  cs carries no gradient (theta is drawn)."""

    @staticmethod
    def forward(ctx, cs, enc, enc_rot):
        cs, enc, enc_rot = _prep(cs), _prep(enc), _prep(enc_rot)
        n = cs.shape[0]
        diffs = _empty((n,), enc)
        call("lv_equivariance_diff_fwd", ptr(cs), ptr(enc), ptr(enc_rot), ptr(diffs), n,
             _lib.stream_of(enc.device))
        ctx.save_for_backward(cs, enc, enc_rot)
        return diffs

    @staticmethod
    def backward(ctx, g):
        cs, enc, enc_rot = ctx.saved_tensors
        ge, gr = torch.empty_like(enc), torch.empty_like(enc_rot)
        call("lv_equivariance_diff_bwd", ptr(cs), ptr(enc), ptr(enc_rot), ptr(_prep(g)), ptr(ge),
             ptr(gr), cs.shape[0], _lib.stream_of(enc.device))
        return None, ge, gr


def equivariance_diff(cs, enc, enc_rot):
    """cs (n, 2), enc and enc_rot (n, 3, 3) -> diffs (n); differentiable in both encodings."""
    n = cs.shape[0]
    assert tuple(cs.shape) == (n, 2), f"cs must be (n,2), got {tuple(cs.shape)}"
    assert tuple(enc.shape) == (n, 3, 3) and tuple(enc_rot.shape) == (n, 3, 3), \
        f"enc and enc_rot must be ({n},3,3), got {tuple(enc.shape)} and {tuple(enc_rot.shape)}"
    _lib.require_device(cs, enc, enc_rot)
    return _EquivarianceDiff.apply(cs.detach(), enc, enc_rot)


class _PairSqdist(torch.autograd.Function):
    """diffs[i] = sum (enc[2i] - enc[2i+1])^2 -- losses/encoder_continuity_loss.py:18-20."""

    @staticmethod
    def forward(ctx, enc):
        enc = _prep(enc)
        rows, D = enc.shape
        diffs = _empty((rows // 2,), enc)
        call("lv_pair_sqdist_fwd", ptr(enc), ptr(diffs), rows, D, _lib.stream_of(enc.device))
        ctx.save_for_backward(enc)
        return diffs

    @staticmethod
    def backward(ctx, g):
        (enc,) = ctx.saved_tensors
        ge = torch.empty_like(enc)
        call("lv_pair_sqdist_bwd", ptr(enc), ptr(_prep(g)), ptr(ge), enc.shape[0], enc.shape[1],
             _lib.stream_of(enc.device))
        return ge


def pair_sqdist(enc):
    """enc (2n, D) -> diffs (n): squared distance of adjacent rows."""
    assert enc.dim() == 2, f"enc must be (rows, D), got {tuple(enc.shape)}"
    _lib.require_device(enc)
    return _PairSqdist.apply(enc)


s2s1 = _S2S1.apply
s2s2 = _S2S2.apply
so3_sample = _SO3Sample.apply
n0_sample = _N0Sample.apply
so3_log_posterior = _SO3LogPosterior.apply
