"""GPU checks of the triangle-mesh renderer (csrc/render_mesh.hip), of meshes.MeshSet and of
the datasets built on them.

The reference is tests/mesh_ref.py, packing and tracing restated in fp64 numpy.  A ray within a
rounding of a silhouette or of an edge between triangles may land on either side of it, so
values are compared off the restatement's edge mask, which every comparison first holds under
2 % of its pixels (tests/test_mesh_cpu.py holds it there on the CPU too).  Off-edge tolerance:
1e-5 absolute on values in [0, 1], as for the sphere-cube renderer; the restatement run in fp32
differs from fp64 by 1.4e-7 at most on these cases (asserted in tests/test_mesh_cpu.py), so the
bar is 74 times the format's own error.
"""
import numpy as np
import pytest
import torch

import mesh_ref as mr
import spherecube_ref as sr

pytestmark = pytest.mark.gpu

TOL = 1e-5
SCALAR = 1  # LV_MESH_SCALAR


def _mesh(spec):
    from lie_vae import meshes
    return meshes.Mesh(*mr.case_arrays(spec))


def _poses(R, dev):
    return torch.as_tensor(np.asarray(R), dtype=torch.float32).to(dev)


def _render(R, ms, size, S, rgb, dev, mesh_id=None, flags=0, max_blocks=0):
    import lie_vae._ops as ops
    return ops.render_mesh(_poses(R, dev), ms, mesh_id, size=size, rgb=rgb, samples=S, flags=flags,
                           max_blocks=max_blocks)


@pytest.fixture(scope="module")
def cases(gpu_device):
    """name -> (R, MeshSet, size, S, rgb, fp64 image, edge mask, device image); the reference
    and the device image are computed once."""
    from lie_vae import meshes
    out = {}
    for name, (spec, R, size, S, rgb) in mr.parity_cases().items():
        R = R.astype(np.float32).astype(np.float64)  # the poses the device sees
        rec, bad = mr.pack(*mr.case_arrays(spec))
        assert bad == 0
        ref, mask = mr.render(R, rec, size, S, rgb)
        ms = meshes.MeshSet([_mesh(spec)], gpu_device)
        out[name] = (R, ms, size, S, rgb, ref, mask, _render(R, ms, size, S, rgb, gpu_device))
    torch.cuda.synchronize()
    return out


def _close(x, ref, mask, what):
    err, share = mr.off_edge_error(x.cpu().numpy(), ref, mask)
    print(f"{what}: off-edge max error {err:.3e}, masked share {share:.4%}")
    assert share <= mr.MASK_CAP, (what, share)
    assert err <= TOL, (what, err)


def test_parity_with_the_restatement(cases, gpu_device):
    """cube() at the 12 sphere-cube parity poses (64 x 64, S = 2); the icosahedron at 16 x 16
    S = 2, 7 x 7 S = 3 (the one-pixel path), 12 x 12 S = 4 and grey at 8 x 8 S = 1;
    icosphere(2) (320 triangles) at 32 x 32; one large triangle from both sides; soups of 63,
    64, 65 and 257 triangles (no staging: the records come by scalar loads, so there is no
    chunk size to straddle).  The packed records match the restatement too."""
    from lie_vae import _lib
    assert set(cases) == set(mr.parity_cases())
    for name, (R, ms, size, S, rgb, ref, mask, x) in cases.items():
        C = 3 if rgb else 1
        assert tuple(x.shape) == (R.shape[0], C, size, size) and x.dtype == torch.float32, name
        assert torch.isfinite(x).all(), name
        assert _lib.render_mesh_plan(R.shape[0], size, C, S)["wide"] == int(size % 4 == 0)
        rec, _ = mr.pack(*mr.case_arrays(mr.parity_cases()[name][0]))
        assert tuple(ms.records.shape) == rec.shape and ms.ranges.tolist() == [[0, rec.shape[0]]]
        # records: fp32 arithmetic on values <= 4, a handful of roundings each
        assert float(np.abs(ms.records.cpu().numpy() - rec).max()) <= 2e-6, name
        _close(x, ref, mask, name)
        assert float((x.amax(1) > 0).float().mean()) >= 0.05, name
    # the triangle's front and back colours, exactly the record's
    R, ms, size, S, rgb, ref, mask, x = cases["triangle 16x16 S=2 rgb"]
    assert torch.equal(x[0, :, 8, 8], ms.records[0, 9:12]) and torch.equal(x[1, :, 8, 8], ms.records[0, 12:15])
    assert float((ms.records[0, 9:12] - ms.records[0, 12:15]).min()) > 0.1


def test_empty_mesh_and_empty_batch(gpu_device):
    """T = 0 renders the background; n = 0 gives an empty tensor."""
    import lie_vae.lie_tools as lt
    from lie_vae import meshes
    empty = meshes.Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    g = _poses(mr.haar_poses(3, 0), gpu_device)
    for size, S, rgb in ((16, 2, True), (7, 3, False)):
        x = lt.render_mesh(g, empty, size=size, samples=S, rgb=rgb)
        assert tuple(x.shape) == (3, 3 if rgb else 1, size, size) and x.dtype == torch.float32
        assert not x.any()
    ms = meshes.MeshSet([empty, meshes.cube(), empty], gpu_device)
    assert ms.ranges.tolist() == [[0, 0], [0, 12], [12, 0]] and ms.total_records == 12
    x = lt.render_mesh(g, ms, torch.tensor([0, 1, 2], device=gpu_device), size=16)
    assert not x[0].any() and x[1].any() and not x[2].any()
    x = lt.render_mesh(g[:0], ms, size=16)
    assert tuple(x.shape) == (0, 3, 16, 16) and x.dtype == torch.float32
    assert lt.render_mesh(g[:0], ms, torch.zeros(0, dtype=torch.long, device=gpu_device), rgb=False).shape == (0, 1, 64, 64)


def test_cube_agrees_with_render_spherecube(cases, gpu_device):
    """The two device renderers on the pixels of the CPU anchor test (no sub-sample on the
    sphere, outside both restatements' edge masks: 94.6 % of them) at 1e-5."""
    import lie_vae.lie_tools as lt
    R, sc_img, cube_img, keep = mr.cube_anchor()
    name = "cube 64x64 S=2 rgb"
    assert np.array_equal(R, cases[name][0])
    x = cases[name][-1]
    sc = lt.render_spherecube(_poses(R, gpu_device), size=64, samples=2)
    diff = (x - sc).abs().amax(1).cpu().numpy()
    print(f"cube against render_spherecube: max diff {diff[keep].max():.3e} on {keep.mean():.2%} of the pixels")
    assert keep.mean() >= 0.80
    assert diff[keep].max() <= TOL
    assert diff[~keep].max() > 0.1  # the sphere is there in one and not in the other


def test_paths_agree_and_calls_repeat_bitwise(cases, gpu_device):
    """LV_MESH_SCALAR gives the four-pixel path's bits (both channel counts), a second call
    gives the first call's bits, an output that is not 16-byte aligned takes one-pixel runs
    with the same bits, and two blocks striding over the three tiles of three 16 x 16 images
    give the default grid's bits on either path."""
    from lie_vae import _lib
    for name in ("cube 64x64 S=2 rgb", "icosahedron 8x8 S=1 grey", "icosahedron 12x12 S=4 rgb",
                 "soup65 16x16 S=2 rgb"):
        R, ms, size, S, rgb, _, _, x = cases[name]
        for c_rgb in (True, False):
            wide = x if c_rgb == rgb else _render(R, ms, size, S, c_rgb, gpu_device)
            assert torch.equal(_render(R, ms, size, S, c_rgb, gpu_device, flags=SCALAR), wide), (name, c_rgb)
            assert torch.equal(_render(R, ms, size, S, c_rgb, gpu_device), wide), (name, c_rgb)
    R, ms, size, S, rgb, _, _, x = cases["icosahedron 7x7 S=3 rgb"]
    assert torch.equal(_render(R, ms, size, S, rgb, gpu_device), x)
    # a misaligned out
    R, ms, size, S, rgb, _, _, x = cases["cube 64x64 S=2 rgb"]
    g = _poses(R, gpu_device)
    buf = torch.zeros(x.numel() + 2, device=gpu_device)
    _lib.call("lv_render_mesh_fwd", g.data_ptr(), None, ms.records.data_ptr(), ms.ranges.data_ptr(),
              ms.K, ms.total_records, buf[1:].data_ptr(), g.shape[0], size, 3, S, 0, 0,
              _lib.stream_of(gpu_device))
    assert torch.equal(buf[1:-1].view_as(x), x) and float(buf[0]) == 0.0 and float(buf[-1]) == 0.0
    # the strided grid
    R3 = mr.haar_poses(3, 4)
    ms = cases["icosahedron 16x16 S=2 rgb"][1]
    assert _lib.render_mesh_plan(3, 16, 3, 2)["blocks"] == 3
    assert _lib.render_mesh_plan(3, 16, 3, 2, max_blocks=2)["blocks"] == 2
    for flags in (0, SCALAR):
        full = _render(R3, ms, 16, 2, True, gpu_device, flags=flags)
        assert torch.equal(_render(R3, ms, 16, 2, True, gpu_device, flags=flags, max_blocks=2), full)
        assert torch.equal(_render(R3, ms, 16, 2, True, gpu_device, flags=flags, max_blocks=1), full)
        assert full[2].any()


def test_mixed_batch_and_ids_outside_the_set(gpu_device):
    """K = 3 meshes and mesh_id = [2,0,1,1,2,0,...]: image i is, bit for bit, the single-mesh
    render of its mesh at its pose; ids -1 and K render all-zero images and leave their
    neighbours untouched; int32 ids and quaternion poses give the same images."""
    import lie_vae.lie_tools as lt
    from lie_vae import meshes
    three = [meshes.cube(), meshes.icosahedron().normalized(1.5), _mesh(("soup", 65, 3))]
    ms = meshes.MeshSet(three, gpu_device)
    assert ms.K == 3 and ms.ranges.tolist() == [[0, 12], [12, 20], [32, 65]] and ms.total_records == 97
    singles = [meshes.MeshSet([m], gpu_device) for m in three]
    g = _poses(mr.haar_poses(12, 6), gpu_device)
    ids = torch.tensor([2, 0, 1, 1, 2, 0] * 2, device=gpu_device)
    for size, S, rgb in ((16, 2, True), (7, 3, True), (8, 1, False)):
        x = lt.render_mesh(g, ms, ids, size=size, samples=S, rgb=rgb)
        alone = [lt.render_mesh(g, s, size=size, samples=S, rgb=rgb) for s in singles]
        for i, k in enumerate(ids.tolist()):
            assert torch.equal(x[i], alone[k][i]), (size, i, k)
            assert x[i].any()
        assert not torch.equal(alone[0], alone[1])
        wild = ids.clone()
        wild[3], wild[7], wild[11] = -1, 3, 2 ** 40
        y = lt.render_mesh(g, ms, wild, size=size, samples=S, rgb=rgb)
        for i in range(12):
            assert (not y[i].any()) if i in (3, 7, 11) else torch.equal(y[i], x[i]), (size, i)
        assert torch.equal(lt.render_mesh(g, ms, ids.to(torch.int32), size=size, samples=S, rgb=rgb), x)
    q = lt.group_matrix_to_quaternions(g)
    x = lt.render_mesh(q, ms, ids, size=16)
    assert torch.equal(x, lt.render_mesh(lt.quaternions_to_group_matrix(q), ms, ids, size=16))
    # a Mesh is packed on the fly
    assert torch.equal(lt.render_mesh(g, three[1], size=16), lt.render_mesh(g, singles[1], size=16))


def test_non_finite_and_wild_inputs_stay_finite(gpu_device):
    """The pose rows of the sphere-cube renderer's wild-pose test on an icosahedron, and meshes
    with a NaN vertex, an infinite vertex and two kinds of zero-area triangle: every image is
    finite and in [0, 1], the good rows are unchanged, and a triangle without a finite positive area
    cannot be hit and changes no bit of its mesh's image."""
    import lie_vae.lie_tools as lt
    from lie_vae import meshes
    good = torch.as_tensor(sr.haar_poses(1, 0)[0], dtype=torch.float32)
    rows = [good, torch.zeros(3, 3), torch.full((3, 3), 1e30), torch.full((3, 3), -3e38),
            good * 1e-30, torch.full((3, 3), float("nan")), torch.full((3, 3), float("inf")),
            torch.tensor([[1., 0, 0], [0, float("nan"), 0], [0, 0, 1]]),
            torch.tensor([[1., 0, 0], [0, 1, 0], [0, 0, 1e-45]]), torch.randn(3, 3) * 10, good]
    g = torch.stack(rows).to(gpu_device)
    ico = meshes.icosahedron().normalized(1.5)

    def with_triangle(extra_vertices, face):
        v = np.concatenate([ico.vertices, np.asarray(extra_vertices, dtype=np.float32).reshape(-1, 3)])
        return meshes.Mesh(v, np.concatenate([ico.faces, [face]]), np.concatenate([ico.albedo, [[1, 1, 1]]]))

    nan_vertex = with_triangle([(float("nan"), 0, 3)], (0, 1, 12))
    inf_vertex = with_triangle([(float("inf"), 0, 3)], (0, 1, 12))
    repeated = with_triangle([(0, 0, 3)], (12, 12, 1))
    collinear = with_triangle([(0, 0, 1.75), (0, 0, 2), (0, 0, 2.5)], (12, 13, 14))
    ms = meshes.MeshSet([ico, nan_vertex, inf_vertex, repeated, collinear], gpu_device)
    assert torch.isfinite(ms.records[:, 9:]).all() and float(ms.records[:, 9:].min()) >= 0.0
    assert float(ms.records[:, 9:].max()) <= 1.0
    for k in (1, 2, 3, 4):  # no finite positive area: zero edges and colours
        last = ms.records[int(ms.ranges[k].sum()) - 1]
        assert not last[3:].any(), k
    for size, S, flags in ((16, 2, 0), (7, 3, 0), (16, 2, SCALAR)):
        base = None
        for k in range(5):
            ids = torch.full((g.shape[0],), k, device=gpu_device)
            x = lt._ops.render_mesh(g, ms, ids, size=size, samples=S, flags=flags)
            assert torch.isfinite(x).all(), (size, k)
            assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0, (size, k)
            alone = lt._ops.render_mesh(g[:1], ms, ids[:1], size=size, samples=S, flags=flags)
            assert torch.equal(x[0], alone[0]) and torch.equal(x[-1], alone[0]) and x[0].any()
            if k == 0:
                base = x
            else:
                assert torch.equal(x, base), (size, k)


def test_meshset_refuses_face_indices_outside_the_vertices(gpu_device):
    """A face index equal to V and one equal to -1: the pack kernel checks an index before it
    addresses anything (it writes a zero record and counts), and MeshSet raises naming the
    mesh.  No out-of-bounds access is provoked."""
    from lie_vae import _ops, meshes
    cube = meshes.cube()
    for bad_index in (8, -1, 2 ** 31 - 1, -2 ** 31):
        faces = cube.faces.copy()
        faces[5, 1] = bad_index
        with pytest.raises(ValueError, match="mesh 1: 1 of its 12 triangles"):
            meshes.MeshSet([cube, meshes.Mesh(cube.vertices, faces, cube.albedo)], gpu_device)
    with pytest.raises(ValueError, match="32 bits"):
        faces = cube.faces.copy()
        faces[0, 0] = 2 ** 31
        meshes.MeshSet([meshes.Mesh(cube.vertices, faces, cube.albedo)], gpu_device)
    # the kernel alone: the bad triangles' records are zero, the others are packed, the count is theirs
    faces = cube.faces.copy()
    faces[2, 0], faces[9, 2] = 8, -1
    rec = torch.full((12, 16), 7.0, device=gpu_device)
    bad = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    _ops.mesh_pack(torch.from_numpy(cube.vertices).to(gpu_device),
                   torch.from_numpy(faces.astype(np.int32)).to(gpu_device),
                   torch.from_numpy(cube.albedo).to(gpu_device), rec, bad)
    want, nbad = mr.pack(cube.vertices, faces, cube.albedo)
    assert int(bad) == nbad == 2 and not rec[2].any() and not rec[9].any()
    assert float(np.abs(rec.cpu().numpy() - want).max()) <= 2e-6


def test_quarter_turns_roll_the_image(cases, gpu_device):
    """render_mesh(R Rz(90 k)) is render_mesh(R) turned k quarter turns clockwise, off both
    edge masks at 1e-5, as for the sphere-cube renderer."""
    for name in mr.QUARTER_TURN_CASES:
        R, ms, size, S, rgb, ref, mask, x = cases[name]
        rec = ms.records.cpu().numpy().astype(np.float64)
        for k in (1, 2, 3):
            Rk = (R @ sr.rot_z(k)).astype(np.float32).astype(np.float64)
            xk = _render(Rk, ms, size, S, rgb, gpu_device)
            both = mr.edge_mask(Rk, rec, size, S) | np.rot90(mask, -k, axes=(1, 2))
            rolled = torch.rot90(x, -k, dims=(2, 3))
            _close(xk, rolled.cpu().numpy().astype(np.float64), both, f"{name} k={k} vs rot90")
            if k != 2:
                wrong = torch.rot90(x, k, dims=(2, 3)).cpu().numpy().astype(np.float64)
                assert mr.off_edge_error(xk.cpu().numpy(), wrong, both)[0] > 0.1, (name, k)


def test_datasets_on_device(gpu_device, tmp_path, monkeypatch):
    """MeshDataset.generate with 3 meshes, n = 12 at 16 x 16: the reference's item shapes and
    dtypes, x == render_mesh(g, meshes, names) bit for bit, the same seed gives the same items,
    save / load round-trips, chunked generation equals one-call generation, and mesh_batch
    draws what generate draws."""
    import lie_vae.lie_tools as lt
    from lie_vae import meshes
    from lie_vae.experiments import datasets
    from lie_vae.experiments.datasets import MeshDataset, mesh_batch
    three = [meshes.tetrahedron().normalized(1.5), meshes.cube(), meshes.icosphere(1).normalized(1.5)]
    ms = meshes.MeshSet(three, gpu_device)
    gen = torch.Generator(device=gpu_device).manual_seed(3)
    ds = MeshDataset.generate(ms, 12, size=16, device=gpu_device, generator=gen)
    assert len(ds) == 12 and (ds.single_id, ds.rgb, ds.num_workers) == (False, True, 0)
    name, g, x = ds[4]
    assert name.dtype == torch.int64 and name.dim() == 0 and 0 <= int(name) < 3
    assert tuple(g.shape) == (3, 3) and tuple(x.shape) == (3, 16, 16)
    assert g.dtype == torch.float32 and x.dtype == torch.float32 and x.device == gpu_device
    names, gs, xs = ds.tensors
    assert names.dtype == torch.int64 and tuple(names.shape) == (12,) and set(names.tolist()) == {0, 1, 2}
    assert torch.equal(xs, lt.render_mesh(gs, ms, names, size=16))
    assert all(xs[i].any() for i in range(12))
    gen.manual_seed(3)
    again = MeshDataset.generate(ms, 12, size=16, device=gpu_device, generator=gen)
    assert all(torch.equal(a, b) for a, b in zip(ds.tensors, again.tensors))
    # a list of Mesh is packed by generate
    gen.manual_seed(3)
    listed = MeshDataset.generate(three, 12, size=16, device=gpu_device, generator=gen)
    assert all(torch.equal(a, b) for a, b in zip(ds.tensors, listed.tensors))
    p = str(tmp_path / "meshes.pt")
    ds.save(p)
    back = MeshDataset(path=p, device=gpu_device)
    assert all(torch.equal(a, b) for a, b in zip(ds.tensors, back.tensors))
    from torch.utils.data import DataLoader
    batch = ds.prep_batch(next(iter(DataLoader(ds, batch_size=5))))
    assert tuple(batch[0].shape) == (5,) and tuple(batch[1].shape) == (5, 3, 3)
    assert tuple(batch[2].shape) == (5, 3, 16, 16) and torch.equal(batch[0], names[:5])
    gen.manual_seed(3)
    bn, bg, bx = mesh_batch(12, gpu_device, ms, generator=gen, size=16)
    assert torch.equal(bn, names) and torch.equal(bg, gs) and torch.equal(bx, xs)
    # chunks of 5 with a ragged tail
    assert datasets.RENDER_CHUNK == 4096
    monkeypatch.setattr(datasets, "RENDER_CHUNK", 5)
    gen.manual_seed(3)
    chunked = MeshDataset.generate(ms, 12, size=16, device=gpu_device, generator=gen)
    assert all(torch.equal(a, b) for a, b in zip(ds.tensors, chunked.tensors))


def test_vae_end_to_end_and_graph_replay(gpu_device):
    """The conv VAE on a rendered 4-image mesh_batch: a finite ELBO that backpropagates,
    evaluate_poses gives four finite numbers, and a captured render_mesh replays to the eager
    bits after the poses change in place."""
    import lie_vae.lie_tools as lt
    from lie_vae import meshes
    from lie_vae.experiments.datasets import mesh_batch
    from lie_vae.experiments.pose_eval import evaluate_poses
    from lie_vae.experiments.vae import VAE
    torch.manual_seed(0)
    ms = meshes.MeshSet([meshes.cube(), meshes.icosahedron().normalized(1.5)], gpu_device)
    gen = torch.Generator(device=gpu_device).manual_seed(0)
    names, g, x = mesh_batch(4, gpu_device, ms, generator=gen)
    assert tuple(names.shape) == (4,) and tuple(g.shape) == (4, 3, 3) and tuple(x.shape) == (4, 3, 64, 64)
    model = VAE(latent_mode='so3', decoder_mode='action', rgb=True).to(gpu_device)
    recon, kl, _ = model.elbo(x)
    loss = (recon + kl).mean()
    assert torch.isfinite(loss)
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)
    stats = evaluate_poses(model, x, g)
    assert len(stats) == 4 and all(np.isfinite(v) for v in stats.values())

    names = torch.tensor([0, 1, 1, 0], device=gpu_device)
    eager = lt.render_mesh(g, ms, names).clone()
    assert not torch.equal(eager[0], eager.flip(0)[0])
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        lt.render_mesh(g, ms, names)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = lt.render_mesh(g, ms, names)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    g.copy_(g.flip(0))  # new poses in the static buffer, same graph; the ids are a palindrome
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager.flip(0))
