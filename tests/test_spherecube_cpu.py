"""CPU checks of the sphere-cube renderer (csrc/render.hip): the launch plan against its closed
form, every argument check of the C entry points (they run before any launch, so no device is
needed), the refusal of CPU tensors, and the invariants of the numpy restatement in
tests/spherecube_ref.py that the GPU parity tests lean on -- above all that its edge mask stays
small on the poses those tests use, so the mask cannot hide a failure."""
import ctypes

import numpy as np
import pytest
import torch

import spherecube_ref as sr

SCALAR = 1  # LV_RENDER_SCALAR


def test_library_exports_the_render_entry_points():
    from lie_vae import _lib
    lib = _lib.load()
    for name in ("lv_render_spherecube_fwd", "lv_render_plan"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
    assert _lib.LV_RENDER_SCALAR == SCALAR
    import lie_vae.lie_tools as lt
    assert callable(lt.render_spherecube) and "render_spherecube" in lt.__all__


def test_render_plan_closed_form():
    """[wide?, blocks, threads, LDS bytes]: the four-pixel path exactly when size % 4 == 0 and
    LV_RENDER_SCALAR is clear; a tile is 256 runs of one image, so an image takes
    ceil(runs / 256) tiles, and the grid is the tile count capped at 65,536 (blocks stride
    over the rest -- at n = 70,000 on either path); R travels in registers, no LDS."""
    from lie_vae import _lib
    strided = set()
    for n in (0, 1, 5, 70000):
        for size in (1, 7, 8, 64):
            for channels in (1, 3):
                for flags in (0, SCALAR):
                    for samples in (1, 2, 4):
                        p = _lib.render_plan(n, size, channels, samples, flags)
                        wide = size % 4 == 0 and not flags
                        runs = size * size // (4 if wide else 1)
                        tiles = n * -(-runs // 256)
                        assert p == {"wide": int(wide), "blocks": min(65536, tiles), "threads": 256,
                                     "lds_bytes": 0}, (n, size, channels, flags, samples, p)
                        if tiles > 65536:
                            strided.add((size, wide))
    # n = 70,000 strides at every size (one tile per image is already more tiles than blocks)
    assert strided == {(1, False), (7, False), (8, False), (8, True), (64, False), (64, True)}
    assert _lib.render_plan(16384, 64, 3, 2)["blocks"] == 65536  # the last grid without a stride
    assert _lib.render_plan(3, 64, 3, 2) == {"wide": 1, "blocks": 12, "threads": 256, "lds_bytes": 0}


def test_render_argument_checks_before_any_launch():
    """Every LV_ERR_ARG case of the two entry points, with dummy non-null pointers that are
    never dereferenced; an empty batch is LV_OK with nothing launched."""
    from lie_vae import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(16)
    buf = (ctypes.c_int64 * 4)()
    fwd, plan = lib.lv_render_spherecube_fwd, lib.lv_render_plan

    def refused(rc, word):
        msg = lib.lv_last_error()
        assert rc == -1 and msg and word in msg, (rc, msg)

    for n in (-1, -70000):
        refused(fwd(P, P, n, 64, 3, 2, 0, None), b"n must")
        refused(plan(n, 64, 3, 2, 0, buf), b"n must")
    for size in (0, -8, 1025, 4096):
        refused(fwd(P, P, 2, size, 3, 2, 0, None), b"size must")
        refused(plan(2, size, 3, 2, 0, buf), b"size must")
    for channels in (0, 2, 4, -1):
        refused(fwd(P, P, 2, 64, channels, 2, 0, None), b"channels must")
        refused(plan(2, 64, channels, 2, 0, buf), b"channels must")
    for samples in (0, 5, -2):
        refused(fwd(P, P, 2, 64, 3, samples, 0, None), b"samples must")
        refused(plan(2, 64, 3, samples, 0, buf), b"samples must")
    for flags in (2, 3, -1):
        refused(fwd(P, P, 2, 64, 3, 2, flags, None), b"flags")
        refused(plan(2, 64, 3, 2, flags, buf), b"flags")
    refused(fwd(None, P, 2, 64, 3, 2, 0, None), b"null")
    refused(fwd(P, None, 2, 64, 3, 2, 0, None), b"null")
    refused(plan(2, 64, 3, 2, 0, None), b"null")
    # n * channels * size^2 floats beyond int64 byte offsets
    for n, size, channels in ((2 ** 62, 64, 3), (2 ** 61 // 4096 + 1, 64, 1), (2 ** 41, 1024, 3)):
        refused(fwd(P, P, n, size, channels, 2, 0, None), b"index range")
        refused(plan(n, size, channels, 2, 0, buf), b"index range")
    assert plan(2 ** 61 // 4096 - 1, 64, 1, 2, 0, buf) == 0 and buf[1] == 65536
    # empty batches: LV_OK before the pointers are looked at
    assert fwd(None, None, 0, 64, 3, 2, 0, None) == 0
    assert fwd(P, P, 0, 7, 1, 3, SCALAR, None) == 0
    assert plan(0, 64, 3, 2, 0, buf) == 0 and buf[1] == 0


def test_cpu_tensors_fail_loudly():
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    from lie_vae.experiments.datasets import ScPairsDataset, SphereCubeDataset, spherecube_batch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lt.render_spherecube(torch.eye(3)[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.render_spherecube(torch.tensor([[0., 0., 0., 1.]]), size=8, rgb=False, samples=1)
    with pytest.raises(AssertionError, match="g must"):
        ops.render_spherecube(torch.randn(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SphereCubeDataset.generate(4, size=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ScPairsDataset.generate(4, size=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spherecube_batch(4, "cpu")


def test_datasets_host_side(tmp_path):
    """Item layout of the reference's datasets (experiments/datasets.py:42-65, 114-127) on
    tensors given directly, the class attributes its training script reads, prep_batch, and
    the save / weights_only load round trip."""
    from torch.utils.data import DataLoader

    from lie_vae.experiments.datasets import ScPairsDataset, SphereCubeDataset
    g, x = torch.randn(5, 3, 3), torch.rand(5, 3, 8, 8)
    ds = SphereCubeDataset(tensors=(g, x))
    assert (ds.rgb, ds.single_id, ds.num_workers) == (True, True, 0) and len(ds) == 5
    name, gi, xi = ds[3]
    assert name == 0 and torch.equal(gi, g[3]) and torch.equal(xi, x[3])
    batch = ds.prep_batch(next(iter(DataLoader(ds, batch_size=4))))
    assert batch[0].dtype == torch.int64 and tuple(batch[0].shape) == (4,)
    assert tuple(batch[1].shape) == (4, 3, 3) and tuple(batch[2].shape) == (4, 3, 8, 8)
    p = str(tmp_path / "sc.pt")
    ds.save(p)
    back = SphereCubeDataset(path=p)
    assert len(back) == 5 and all(torch.equal(a, b) for a, b in zip(ds.tensors, back.tensors))

    pg, px = torch.randn(6, 2, 3, 3), torch.rand(6, 2, 3, 8, 8)
    pairs = ScPairsDataset(tensors=(pg, px))
    assert (pairs.rgb, pairs.single_id, pairs.num_workers) == (True, True, 0) and len(pairs) == 6
    names, gs, imgs = pairs[2]
    assert names.dtype == torch.int64 and names.tolist() == [0, 0]
    assert torch.equal(gs, pg[2]) and torch.equal(imgs, px[2])
    names, gs, imgs = pairs.prep_batch(next(iter(DataLoader(pairs, batch_size=4))))
    assert tuple(names.shape) == (8,) and tuple(gs.shape) == (8, 3, 3)
    assert tuple(imgs.shape) == (8, 3, 8, 8)
    assert torch.equal(gs[2], pg[1, 0]) and torch.equal(gs[3], pg[1, 1])  # pairs stay adjacent
    p = str(tmp_path / "pairs.pt")
    pairs.save(p)
    back = ScPairsDataset(path=p)
    assert all(torch.equal(a, b) for a, b in zip(pairs.tensors, back.tensors))


# ------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def rendered():
    """Every parity case of tests/test_gpu_spherecube.py, rendered once in fp64."""
    return {name: sr.render(R, size, S, rgb) for name, (R, size, S, rgb) in sr.parity_cases().items()}


def test_mask_cap_on_the_chosen_seeds(rendered):
    """The edge mask covers at most 2 % of the pixels of every parity case (and of each case's
    quarter turns, which the roll tests compare), so it cannot hide a wrong image; and the
    scene fills a fair part of the frame."""
    for name, (R, size, S, rgb) in sr.parity_cases().items():
        img, mask = rendered[name]
        assert mask.mean() <= sr.MASK_CAP, (name, mask.mean())
        assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
        assert 0.25 <= (img.max(axis=1) > 0).mean() <= 0.75, name
        for k in (1, 2, 3):
            _, mk = sr.render(R @ sr.rot_z(k), size, S, rgb)
            both = mk | np.rot90(mask, -k, axes=(1, 2))
            assert both.mean() <= sr.MASK_CAP, (name, k, both.mean())


def test_fp32_restatement_within_a_tenth_of_the_tolerance(rendered):
    """The bar of the GPU comparison (1e-5 off-edge) is about ten times what the same
    arithmetic in fp32 numpy shows against fp64."""
    for name, (R, size, S, rgb) in sr.parity_cases().items():
        img, mask = rendered[name]
        img32, _ = sr.render(R, size, S, rgb, dtype=np.float32)
        assert img32.dtype == np.float32
        err, _ = sr.off_edge_error(img32, img, mask)
        assert err <= 2e-6, (name, err)


def test_quarter_turn_about_the_view_axis_is_rot90(rendered):
    """render(R Rz(90 k)) is render(R) turned by k quarter turns CLOCKWISE (np.rot90 with -k):
    turning the camera anticlockwise about its view axis turns the picture clockwise.  The
    opposite direction is off by whole colours."""
    for name, (R, size, S, rgb) in sr.parity_cases().items():
        img, mask = rendered[name]
        for k in (1, 2, 3):
            imk, mk = sr.render(R @ sr.rot_z(k), size, S, rgb)
            both = mk | np.rot90(mask, -k, axes=(1, 2))
            err, _ = sr.off_edge_error(imk, np.rot90(img, -k, axes=(2, 3)), both)
            assert err <= 1e-12, (name, k, err)
            if k != 2:
                wrong, _ = sr.off_edge_error(imk, np.rot90(img, k, axes=(2, 3)), both)
                assert wrong > 0.1, (name, k, wrong)


def test_grey_is_the_channel_mean():
    R = sr.haar_poses(3, 5)
    for size, S in ((8, 1), (12, 2)):
        rgb, m1 = sr.render(R, size, S, True)
        grey, m2 = sr.render(R, size, S, False)
        assert grey.shape == (3, 1, size, size) and np.array_equal(m1, m2)
        np.testing.assert_allclose(grey[:, 0], rgb.mean(axis=1), rtol=0, atol=1e-15)


def test_identity_view():
    """Camera on +z looking down: the sphere (grey) at the image centre in front of the +z
    face (blue, shaded 0.3 + 0.7 * 3 / sqrt 14), background in the corners; odd size with odd
    S sends the centre ray through exact zeros without a NaN."""
    blue = np.array([.1, .1, .9]) * (0.3 + 0.7 * 3 / np.sqrt(14))
    for size, S in ((7, 3), (64, 2), (9, 1)):
        img, mask = sr.render(np.eye(3)[None], size, S)
        assert np.isfinite(img).all()
        c = size // 2
        centre = img[0, :, c, c]
        assert centre[0] == centre[1] == centre[2] and 0.7 < centre[0] <= 0.95
        assert np.array_equal(img[0, :, 0, 0], np.zeros(3))
        # on the row through the centre the sphere spans |u| <= 0.152 and the face
        # |u| <= 0.25 (of 0.4): the ray at u = 0.2 sees the face, the one at u = 0.3 nothing
        col, hit = sr.trace(np.eye(3)[None], np.array([0.75, 0.875]) * size, np.array([0.5, 0.5]) * size, size)
        assert hit[0].tolist() == [4, sr.ID_BACKGROUND]
        np.testing.assert_allclose(col[0, 0], blue, rtol=0, atol=1e-15)
    # the centre ray at odd size and S = 1 has d = (0, 0, -1) exactly: hits the sphere's pole
    col, hit = sr.trace(np.eye(3)[None], np.array([3.5]), np.array([3.5]), 7)
    assert hit[0, 0] == sr.ID_SPHERE
    np.testing.assert_allclose(col[0, 0], 0.95 * (0.3 + 0.7 * 3 / np.sqrt(14)), atol=1e-15)


def test_face_on_views_show_each_face():
    """The six axis views (rays with exact zero components) see the six faces in turn."""
    R = sr.face_on_poses()
    for f in range(6):
        # u = -0.22, v = 0.22: on the face, outside the sphere that sits in front of +z
        col, hit = sr.trace(R[f:f + 1], np.array([14.25]), np.array([14.25]), 64)
        assert hit[0, 0] == f, (f, hit)
    img, mask = sr.render(R, 64, 2)
    assert np.isfinite(img).all()
