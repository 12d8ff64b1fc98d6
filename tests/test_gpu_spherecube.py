"""GPU checks of the sphere-cube renderer (csrc/render.hip) and the datasets built on it.

The reference is tests/spherecube_ref.py, the scene restated in fp64 numpy.  A ray within a
rounding of a silhouette or a cube edge may land on either side of it, so values are compared
off the restatement's edge mask, which every comparison first holds under 2 % of its pixels
(tests/test_spherecube_cpu.py holds it there on the CPU too).  Off-edge tolerance: 1e-5
absolute on values in [0, 1], about ten times what the restatement run in fp32 shows against
itself in fp64 (1.05e-6 at 64 x 64, S = 2).
"""
import numpy as np
import pytest
import torch

import spherecube_ref as sr

pytestmark = pytest.mark.gpu

TOL = 1e-5
SCALAR = 1  # LV_RENDER_SCALAR


def _render(R, size, S, rgb, dev, flags=0):
    import lie_vae._ops as ops
    g = torch.as_tensor(np.asarray(R), dtype=torch.float32).to(dev)
    return ops.render_spherecube(g, size=size, rgb=rgb, samples=S, flags=flags)


@pytest.fixture(scope="module")
def cases(gpu_device):
    """name -> (R, size, S, rgb, fp64 image, edge mask, device image); rendered once."""
    out = {}
    for name, (R, size, S, rgb) in sr.parity_cases().items():
        R = R.astype(np.float32).astype(np.float64)  # the poses the device sees
        ref, mask = sr.render(R, size, S, rgb)
        out[name] = (R, size, S, rgb, ref, mask, _render(R, size, S, rgb, gpu_device))
    torch.cuda.synchronize()
    return out


def _close(x, ref, mask, what):
    err, share = sr.off_edge_error(x.cpu().numpy(), ref, mask)
    print(f"{what}: off-edge max error {err:.3e}, masked share {share:.4%}")
    assert share <= sr.MASK_CAP, (what, share)
    assert err <= TOL, (what, err)


def test_parity_with_the_restatement(cases):
    """Five Haar poses, the identity and the six face-on views at 64 x 64, S = 2; grey at
    8 x 8, S = 1; the one-pixel path at 7 x 7, S = 3, whose centre ray at the identity has a
    zero component; S = 4 at 12 x 12."""
    from lie_vae import _lib
    for name, (R, size, S, rgb, ref, mask, x) in cases.items():
        assert tuple(x.shape) == (R.shape[0], 3 if rgb else 1, size, size) and x.dtype == torch.float32
        assert torch.isfinite(x).all(), name
        assert _lib.render_plan(R.shape[0], size, 3 if rgb else 1, S)["wide"] == int(size % 4 == 0)
        _close(x, ref, mask, name)
        assert 0.25 <= float((x.amax(1) > 0).float().mean()) <= 0.75, name


def test_paths_agree_and_calls_repeat_bitwise(cases, gpu_device):
    """LV_RENDER_SCALAR gives the four-pixel path's bits at size 8 and 64 (both channel
    counts), and a second call gives the first call's bits."""
    for name in ("64x64 S=2 rgb", "8x8 S=1 grey"):
        R, size, S, rgb, _, _, x = cases[name]
        for c_rgb in (True, False):
            wide = x if c_rgb == rgb else _render(R, size, S, c_rgb, gpu_device)
            assert torch.equal(_render(R, size, S, c_rgb, gpu_device, SCALAR), wide), (name, c_rgb)
            assert torch.equal(_render(R, size, S, c_rgb, gpu_device), wide), (name, c_rgb)
    R, size, S, rgb, _, _, x = cases["7x7 S=3 rgb"]
    assert torch.equal(_render(R, size, S, rgb, gpu_device), x)
    # an output that is not 16-byte aligned takes one-pixel runs, same bits
    from lie_vae import _lib
    R, size, S, rgb, _, _, x = cases["64x64 S=2 rgb"]
    g = torch.as_tensor(R, dtype=torch.float32).to(gpu_device)
    buf = torch.zeros(x.numel() + 1, device=gpu_device)
    _lib.call("lv_render_spherecube_fwd", g.data_ptr(), buf[1:].data_ptr(), g.shape[0], size, 3, S,
              0, _lib.stream_of(gpu_device))
    assert torch.equal(buf[1:].view_as(x), x) and float(buf[0]) == 0.0


def test_grey_is_the_channel_mean_and_quaternions_are_poses(gpu_device):
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    q = lt.random_quaternions(6, device=gpu_device)
    rgb = lt.render_spherecube(q, size=16, samples=2)
    grey = lt.render_spherecube(q, size=16, rgb=False, samples=2)
    assert tuple(grey.shape) == (6, 1, 16, 16)
    # same sums; torch divides by a scalar as a multiplication by fl(1/3), so the two quotients
    # carry three roundings of 2^-24 between them on values <= 0.95: under 2^-22
    mean = ((rgb[:, 0] + rgb[:, 1]) + rgb[:, 2]) / 3
    assert float((grey[:, 0] - mean).abs().max()) <= 2.0 ** -22
    assert torch.equal(rgb, ops.render_spherecube(lt.quaternions_to_group_matrix(q), size=16))
    assert lt.render_spherecube(q[:0], size=16).shape == (0, 3, 16, 16)


def test_strided_grid_on_the_wide_path(gpu_device):
    """More tiles than the 65,536-block grid, so blocks stride: the smallest such n at
    64 x 64 from the plan (16,385 RGB images, 0.8 GB).  The first and last two images equal
    the one-pixel path's render of the same poses (a grid without a stride), every value is
    finite, and the middle holds the right images too (a strided sample against a small call)."""
    from lie_vae import _lib
    import lie_vae.lie_tools as lt
    cap = _lib.render_plan(10 ** 6, 64, 3, 2)["blocks"]      # the largest grid
    per_image = _lib.render_plan(1, 64, 3, 2)["blocks"]      # tiles of one image
    n = cap // per_image + 1                                 # the first n with more tiles than blocks
    assert _lib.render_plan(n, 64, 3, 2) == {"wide": 1, "blocks": cap, "threads": 256, "lds_bytes": 0}
    assert _lib.render_plan(n - 1, 64, 3, 2)["blocks"] == (n - 1) * per_image == cap
    assert (cap, per_image, n) == (65536, 4, 16385)
    gen = torch.Generator(device=gpu_device).manual_seed(5)
    g = lt.random_group_matrices(n, device=gpu_device, generator=gen)
    x = lt.render_spherecube(g)
    assert torch.isfinite(x).all()
    import lie_vae._ops as ops
    pick = torch.cat([torch.arange(2), torch.arange(n // 2, n // 2 + 2), torch.arange(n - 2, n)]).to(gpu_device)
    small = ops.render_spherecube(g[pick], flags=SCALAR)
    assert torch.equal(x[pick], small)
    assert float(small.amax()) > 0.5


def test_quarter_turns_roll_the_image(cases, gpu_device):
    """render(R Rz(90 k)) is render(R) turned k quarter turns clockwise (the direction
    tests/test_spherecube_cpu.py pins on the restatement), off-edge at 1e-5; the image-rotation
    kernel of the equivariance loss agrees: rotate_images with (cos, sin) = (0, -1) is the
    exact clockwise quarter turn."""
    import lie_vae._ops as ops
    for name in ("64x64 S=2 rgb", "12x12 S=4 rgb"):
        R, size, S, rgb, ref, mask, x = cases[name]
        for k in (1, 2, 3):
            Rk = (R @ sr.rot_z(k)).astype(np.float32).astype(np.float64)
            xk = _render(Rk, size, S, rgb, gpu_device)
            _, mk = sr.render(Rk, size, S, rgb)
            both = mk | np.rot90(mask, -k, axes=(1, 2))
            rolled = torch.rot90(x, -k, dims=(2, 3))
            _close(xk, rolled.cpu().numpy().astype(np.float64), both, f"{name} k={k} vs rot90")
            c, s = ((1, 0), (0, -1), (-1, 0), (0, 1))[k]
            cs = torch.tensor([[float(c), float(s)]], device=gpu_device).expand(x.shape[0], 2).contiguous()
            turned = ops.rotate_images(x, cs)
            assert torch.equal(turned, rolled), (name, k)
            _close(xk, turned.cpu().numpy().astype(np.float64), both, f"{name} k={k} vs rotate_images")


def test_non_finite_and_wild_poses_stay_finite(gpu_device):
    """Any finite R gives a finite image; a non-finite R gives a finite image here (a hit test
    that sees a NaN fails), and its neighbours in the batch are untouched."""
    import lie_vae._ops as ops
    good = torch.as_tensor(sr.haar_poses(1, 0)[0], dtype=torch.float32)
    rows = [good, torch.zeros(3, 3), torch.full((3, 3), 1e30), torch.full((3, 3), -3e38),
            good * 1e-30, torch.full((3, 3), float("nan")), torch.full((3, 3), float("inf")),
            torch.tensor([[1., 0, 0], [0, float("nan"), 0], [0, 0, 1]]),
            torch.tensor([[1., 0, 0], [0, 1, 0], [0, 0, 1e-45]]), torch.randn(3, 3) * 10, good]
    g = torch.stack(rows).to(gpu_device)
    for size, S, flags in ((16, 2, 0), (7, 3, 0), (16, 2, SCALAR)):
        x = ops.render_spherecube(g, size=size, samples=S, flags=flags)
        assert torch.isfinite(x).all()
        assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0
        alone = ops.render_spherecube(g[:1], size=size, samples=S, flags=flags)
        assert torch.equal(x[0], alone[0]) and torch.equal(x[-1], alone[0])


def test_datasets_on_device(gpu_device, tmp_path):
    """generate(n=10): the reference's item shapes and dtypes, image == render(group_el) bit
    for bit; pairs are a geodesic step of the drawn length apart and prep_batch flattens them;
    save / load round-trips."""
    import lie_vae.lie_tools as lt
    from torch.utils.data import DataLoader

    from lie_vae.experiments.datasets import ScPairsDataset, SphereCubeDataset, spherecube_batch
    gen = torch.Generator(device=gpu_device).manual_seed(3)
    ds = SphereCubeDataset.generate(10, size=16, device=gpu_device, generator=gen)
    assert len(ds) == 10
    name, g, x = ds[4]
    assert name == 0 and tuple(g.shape) == (3, 3) and tuple(x.shape) == (3, 16, 16)
    assert g.dtype == torch.float32 and x.dtype == torch.float32 and x.device == gpu_device
    assert torch.equal(ds.tensors[1], lt.render_spherecube(ds.tensors[0], size=16))
    gen.manual_seed(3)
    assert torch.equal(ds.tensors[0], lt.random_group_matrices(10, device=gpu_device, generator=gen))
    assert SphereCubeDataset.generate(3, device=gpu_device)[0][2].shape == (3, 64, 64)
    p = str(tmp_path / "sc.pt")
    ds.save(p)
    back = SphereCubeDataset(path=p, device=gpu_device)
    assert all(torch.equal(a, b) for a, b in zip(ds.tensors, back.tensors))

    step_size = 2 * np.pi / 60
    gen.manual_seed(8)
    pairs = ScPairsDataset.generate(10, size=16, device=gpu_device, generator=gen)
    gen.manual_seed(8)
    a = lt.random_group_matrices(10, device=gpu_device, generator=gen)
    step = torch.randn(10, 3, device=gpu_device, generator=gen) * step_size
    names, gs, imgs = pairs[7]
    assert names.dtype == torch.int64 and names.tolist() == [0, 0]
    assert tuple(gs.shape) == (2, 3, 3) and tuple(imgs.shape) == (2, 3, 16, 16)
    pg, px = pairs.tensors
    assert torch.equal(pg[:, 0], a)
    dist = lt.geodesic_distance(pg[:, 0], pg[:, 1])
    assert float((dist - step.norm(dim=-1)).abs().max()) <= 1e-5
    assert torch.equal(px.reshape(20, 3, 16, 16), lt.render_spherecube(pg.reshape(20, 3, 3), size=16))
    names, gs, imgs = pairs.prep_batch(next(iter(DataLoader(pairs, batch_size=5))))
    assert tuple(names.shape) == (10,) and tuple(gs.shape) == (10, 3, 3)
    assert tuple(imgs.shape) == (10, 3, 16, 16) and torch.equal(gs[3], pg[1, 1])
    p = str(tmp_path / "pairs.pt")
    pairs.save(p)
    back = ScPairsDataset(path=p, device=gpu_device)
    assert all(torch.equal(a, b) for a, b in zip(pairs.tensors, back.tensors))

    gen.manual_seed(3)
    g, x = spherecube_batch(10, gpu_device, generator=gen, size=16)
    assert torch.equal(g, ds.tensors[0]) and torch.equal(x, ds.tensors[1])


def test_chunked_generation_matches_one_call(gpu_device, monkeypatch):
    """Datasets render in chunks (4,096 images in flight); a small chunk with a ragged tail
    gives the one-call images."""
    import lie_vae.lie_tools as lt
    from lie_vae.experiments import datasets
    assert datasets.RENDER_CHUNK == 4096
    monkeypatch.setattr(datasets, "RENDER_CHUNK", 4)
    gen = torch.Generator(device=gpu_device).manual_seed(1)
    ds = datasets.SphereCubeDataset.generate(10, size=8, device=gpu_device, generator=gen)
    assert torch.equal(ds.tensors[1], lt.render_spherecube(ds.tensors[0], size=8))


def test_vae_end_to_end_and_graph_replay(gpu_device):
    """The conv VAE on a rendered batch: a finite ELBO that backpropagates, evaluate_poses
    gives four finite numbers, and a captured render replays to the eager bits."""
    import lie_vae.lie_tools as lt
    from lie_vae.experiments.datasets import spherecube_batch
    from lie_vae.experiments.pose_eval import evaluate_poses
    from lie_vae.experiments.vae import VAE
    torch.manual_seed(0)
    gen = torch.Generator(device=gpu_device).manual_seed(0)
    g, x = spherecube_batch(4, gpu_device, generator=gen)
    assert tuple(g.shape) == (4, 3, 3) and tuple(x.shape) == (4, 3, 64, 64)
    model = VAE(latent_mode='so3', decoder_mode='action', rgb=True).to(gpu_device)
    recon, kl, _ = model.elbo(x)
    loss = (recon + kl).mean()
    assert torch.isfinite(loss)
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)
    stats = evaluate_poses(model, x, g)
    assert len(stats) == 4 and all(np.isfinite(v) for v in stats.values())

    eager = lt.render_spherecube(g).clone()
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        lt.render_spherecube(g)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lt.render_spherecube(g)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    g.copy_(g.flip(0))  # new poses in the static buffer, same graph
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager.flip(0))
