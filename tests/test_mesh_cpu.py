"""CPU checks of the triangle-mesh renderer (csrc/render_mesh.hip): the built-in solids, the
OBJ reader, the launch plan and every argument check of the three C entry points (they run
before any launch, so no device is needed), the refusal of CPU tensors, and the invariants of
the numpy restatement in tests/mesh_ref.py that the GPU parity tests lean on: it agrees with
the trusted sphere-cube restatement on the cube, its edge mask stays small on the compared
cases, and its fp32 run is far inside the GPU tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_ref as mr
import spherecube_ref as sr

SCALAR = 1  # LV_MESH_SCALAR
TOL = 1e-5  # the GPU comparison's bar (tests/test_gpu_mesh.py)


# ------------------------------------------------------------------ solids and files
def _edges(mesh):
    f = mesh.faces
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0)


def test_builtin_solids():
    """Vertex, edge and face counts with V - E + F = 2, every edge shared by two triangles
    in opposite directions, positive signed volume (outward winding), distinct palette colours
    and the radius after ``normalized``."""
    from lie_vae import meshes
    want = {"cube": (8, 18, 12), "tetrahedron": (4, 6, 4), "octahedron": (6, 12, 8),
            "icosahedron": (12, 30, 20), "icosphere0": (12, 30, 20), "icosphere1": (42, 120, 80),
            "icosphere2": (162, 480, 320)}
    built = {"cube": meshes.cube(), "tetrahedron": meshes.tetrahedron(),
             "octahedron": meshes.octahedron(), "icosahedron": meshes.icosahedron(),
             "icosphere0": meshes.icosphere(0), "icosphere1": meshes.icosphere(1),
             "icosphere2": meshes.icosphere(2)}
    for name, m in built.items():
        V, E, F = m.vertices.shape[0], _edges(m).shape[0], m.faces.shape[0]
        assert (V, E, F) == want[name] and V - E + F == 2, (name, V, E, F)
        assert m.vertices.dtype == np.float32 and m.faces.dtype == np.int64
        assert m.albedo.shape == (F, 3) and m.albedo.dtype == np.float32
        f = m.faces
        directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert len({tuple(e) for e in directed}) == 3 * F, name           # no directed edge twice
        assert {tuple(e) for e in directed} == {tuple(e[::-1]) for e in directed}, name
        assert m.signed_volume() > 0, name
        if name != "cube":
            assert len({tuple(c) for c in m.albedo}) == F, name           # the palette is distinct
        for radius in (1.5, 0.7):
            nm = m.normalized(radius)
            norms = np.linalg.norm(nm.vertices.astype(np.float64), axis=1)
            assert abs(norms.max() - radius) <= 1e-6 * radius, (name, radius)
            box = (nm.vertices.min(axis=0) + nm.vertices.max(axis=0)) / 2
            assert np.abs(box).max() <= 1e-6, name
            assert np.array_equal(nm.faces, m.faces) and np.array_equal(nm.albedo, m.albedo)
    assert abs(meshes.cube().signed_volume() - 8.0) < 1e-12
    assert abs(np.linalg.norm(meshes.icosphere(2).vertices, axis=1) - 1).max() < 1e-6
    # the cube carries the sphere-cube scene's albedos in its face order, two triangles a face
    c = meshes.cube()
    assert np.array_equal(c.albedo, np.repeat(np.asarray(sr.FACE_ALBEDO, dtype=np.float32), 2, axis=0))
    for t in range(12):
        tri = c.vertices[c.faces[t]]
        axis, sign = t // 4, (1, -1)[(t // 2) % 2]
        assert np.array_equal(tri[:, axis], np.full(3, sign, dtype=np.float32)), t
    # container checks
    one = meshes.Mesh(c.vertices, c.faces, (0.2, 0.4, 0.6))
    assert one.albedo.shape == (12, 3) and np.allclose(one.albedo[7], (0.2, 0.4, 0.6))
    with pytest.raises(ValueError, match="albedo"):
        meshes.Mesh(c.vertices, c.faces, np.zeros((5, 3)))
    with pytest.raises(ValueError, match="albedo"):
        meshes.Mesh(c.vertices, c.faces, (0.2, 1.4, 0.6))
    with pytest.raises(ValueError, match="integers"):
        meshes.Mesh(c.vertices, c.faces.astype(np.float64))
    assert meshes.Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)).faces.shape == (0, 3)


def _triangle_set(mesh):
    """The triangles as a set of coordinate triples, each rotated to start at its smallest
    vertex (the winding is kept)."""
    out = set()
    for tri in mesh.vertices[mesh.faces].astype(np.float64):
        pts = [tuple(p) for p in tri]
        k = pts.index(min(pts))
        out.add(tuple(pts[k:] + pts[:k]))
    return out


def _quad_cube_obj():
    """cube() written as six quads (each the two triangles of a face joined along their
    shared diagonal, starting at the fan's apex), every face in another token style, with the
    lines a reader has to ignore."""
    from lie_vae import meshes
    c = meshes.cube()
    lines = ["# a cube of six quads", "mtllib none.mtl", "o cube"]
    lines += ["v %g %g %.1f" % tuple(v) for v in c.vertices]
    lines += ["vt 0 0", "vt 1 0", "vn 0 0 1", "vn 1 0 0", "s off", "usemtl red"]
    styles = ("{i}/1/2", "{n}/2/1", "{i}", "{n}//1", "{i}/2", "{n}")
    for k in range(6):
        quad = [c.faces[2 * k][0], c.faces[2 * k][1], c.faces[2 * k][2], c.faces[2 * k + 1][2]]
        lines.append("f " + " ".join(styles[k].format(i=q + 1, n=q - 8) for q in quad)
                     + ("   # trailing comment" if k == 2 else ""))
    return "\n".join(lines) + "\n"


def test_load_obj(tmp_path):
    """A quad cube with v/vt/vn, v//vn and v/vt tokens and negative indices equals ``cube()``
    up to the order of the triangles (the fan of a quad (a, b, c, d) is (a, b, c), (a, c, d),
    cube()'s own split); a pentagon becomes three triangles; malformed files raise."""
    from lie_vae import meshes
    p = tmp_path / "cube.obj"
    p.write_text(_quad_cube_obj())
    m = meshes.load_obj(str(p))
    assert m.vertices.shape == (8, 3) and m.faces.shape == (12, 3)
    assert m.signed_volume() == 8.0
    assert _triangle_set(m) == _triangle_set(meshes.cube())
    p = tmp_path / "pentagon.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 2 1 0\nv 1 2 0\nv 0 1 0\nf 1 2 3 4 5\n")
    assert meshes.load_obj(str(p)).faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4]]
    bad = {"index past the vertices": "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n",
           "index zero": "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n",
           "negative past the start": "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n",
           "face before its vertices": "v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n",
           "two-vertex face": "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n",
           "short vertex": "v 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
           "not a number": "v 0 0 zero\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
           "not an index": "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x/1\n",
           "no faces": "v 0 0 0\nv 1 0 0\nv 0 1 0\n",
           "empty": "# nothing\n"}
    for what, text in bad.items():
        p = tmp_path / "bad.obj"
        p.write_text(text)
        with pytest.raises(ValueError, match="bad.obj"):
            meshes.load_obj(str(p))


# ------------------------------------------------------------------ the C entry points
def test_library_exports_the_mesh_entry_points():
    from lie_vae import _lib
    lib = _lib.load()
    for name in ("lv_mesh_pack", "lv_render_mesh_fwd", "lv_render_mesh_plan"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
    assert _lib.LV_MESH_SCALAR == SCALAR
    import lie_vae.lie_tools as lt
    assert callable(lt.render_mesh) and "render_mesh" in lt.__all__


def test_render_mesh_plan_closed_form():
    """[wide?, blocks, threads, LDS bytes]: render_plan's tiling (a tile is 256 runs of one
    image; four-pixel runs exactly when size % 4 == 0 and LV_MESH_SCALAR is clear) with the
    grid capped at max_blocks when 0 < max_blocks < 65,536, else at 65,536; no LDS."""
    from lie_vae import _lib
    for n in (0, 1, 3, 70000):
        for size in (1, 7, 16, 64):
            for channels in (1, 3):
                for flags in (0, SCALAR):
                    for max_blocks in (0, 1, 2, 65535, 65536, 10 ** 9):
                        p = _lib.render_mesh_plan(n, size, channels, 2, flags, max_blocks)
                        wide = size % 4 == 0 and not flags
                        tiles = n * -(-(size * size // (4 if wide else 1)) // 256)
                        cap = max_blocks if 0 < max_blocks < 65536 else 65536
                        assert p == {"wide": int(wide), "blocks": min(cap, tiles), "threads": 256,
                                     "lds_bytes": 0}, (n, size, channels, flags, max_blocks, p)
                        if not max_blocks:
                            assert p == _lib.render_plan(n, size, channels, 2, flags)
    # three 16 x 16 images are three tiles: two blocks stride over them
    assert _lib.render_mesh_plan(3, 16, 3, 2)["blocks"] == 3
    assert _lib.render_mesh_plan(3, 16, 3, 2, max_blocks=2)["blocks"] == 2
    # ranges that fit
    assert _lib.render_mesh_plan(1, 16, 3, 2, K=3, total_records=10, ranges=[(0, 4), (4, 0), (4, 6)])["blocks"] == 1


def test_mesh_argument_checks_before_any_launch():
    """Every LV_ERR_ARG case of the three entry points, with dummy non-null pointers that are
    never dereferenced; an empty batch and an empty mesh are LV_OK with nothing launched."""
    from lie_vae import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(16)
    buf = (ctypes.c_int64 * 4)()
    fwd, plan, pack = lib.lv_render_mesh_fwd, lib.lv_render_mesh_plan, lib.lv_mesh_pack

    def refused(rc, word):
        msg = lib.lv_last_error()
        assert rc == -1 and msg and word in msg, (rc, msg)

    def both(word, K=1, total=12, n=2, size=64, channels=3, samples=2, flags=0, max_blocks=0):
        refused(fwd(P, P, P, P, K, total, P, n, size, channels, samples, flags, max_blocks, None), word)
        refused(plan(None, K, total, n, size, channels, samples, flags, max_blocks, buf), word)

    for n in (-1, -70000):
        both(b"n must", n=n)
    for size in (0, -8, 1025, 4096):
        both(b"size must", size=size)
    for channels in (0, 2, 4, -1):
        both(b"channels must", channels=channels)
    for samples in (0, 5, -2):
        both(b"samples must", samples=samples)
    for K in (0, -1):
        both(b"K must", K=K)
    for total in (-1, 2 ** 31):
        both(b"total_records", total=total)
    for flags in (2, 3, -1):
        both(b"flags", flags=flags)
    both(b"max_blocks", max_blocks=-1)
    for n, size, channels in ((2 ** 62, 64, 3), (2 ** 61 // 4096 + 1, 64, 1), (2 ** 41, 1024, 3)):
        both(b"index range", n=n, size=size, channels=channels)
    # null and misaligned pointers (mesh_id may be null: every image shows mesh 0)
    refused(fwd(None, None, P, P, 1, 12, P, 2, 64, 3, 2, 0, 0, None), b"null")
    refused(fwd(P, None, None, P, 1, 12, P, 2, 64, 3, 2, 0, 0, None), b"null")
    refused(fwd(P, None, P, None, 1, 12, P, 2, 64, 3, 2, 0, 0, None), b"null")
    refused(fwd(P, None, P, P, 1, 12, None, 2, 64, 3, 2, 0, 0, None), b"null")
    refused(fwd(P, None, ctypes.c_void_p(20), P, 1, 12, P, 2, 64, 3, 2, 0, 0, None), b"aligned")
    refused(plan(None, 1, 12, 2, 64, 3, 2, 0, 0, None), b"null")
    # a range past the records, a negative start, a negative count
    for pairs, which in (([0, 5, 5, 8], b"range 1"), ([-1, 3, 3, 9], b"range 0"),
                         ([0, 12, 12, -1], b"range 1"), ([0, 13, 0, 0], b"range 0"),
                         ([2 ** 31 - 1, 2 ** 31 - 1, 0, 0], b"range 0")):
        host = (ctypes.c_int32 * 4)(*pairs)
        refused(plan(host, 2, 12, 2, 64, 3, 2, 0, 0, buf), which)
    host = (ctypes.c_int32 * 4)(0, 5, 5, 7)
    assert plan(host, 2, 12, 2, 64, 3, 2, 0, 0, buf) == 0 and list(buf) == [1, 8, 256, 0]
    # empty batches: LV_OK before the pointers are looked at
    assert fwd(None, None, None, None, 1, 0, None, 0, 64, 3, 2, 0, 0, None) == 0
    assert plan(None, 1, 0, 0, 7, 1, 3, SCALAR, 5, buf) == 0 and list(buf) == [0, 0, 256, 0]
    # packing
    for V in (-1, 2 ** 31 // 3 + 1):
        refused(pack(P, V, P, P, 4, P, P, None), b"V must")
    for T in (-1, 2 ** 31 // 16 + 1):
        refused(pack(P, 8, P, P, T, P, P, None), b"T must")
    for k in (2, 3, 5, 6):
        args = [P, 8, P, P, 4, P, P, None]
        args[k] = None
        refused(pack(*args), b"null")
    refused(pack(None, 8, P, P, 4, P, P, None), b"null")
    refused(pack(P, 8, P, P, 4, ctypes.c_void_p(24), P, None), b"aligned")
    assert pack(None, 0, None, None, 0, None, None, None) == 0    # an empty mesh


def test_cpu_tensors_fail_loudly():
    import lie_vae._ops as ops
    import lie_vae.lie_tools as lt
    from lie_vae import meshes
    from lie_vae.experiments.datasets import MeshDataset, mesh_batch
    cube = meshes.cube()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lt.render_mesh(torch.eye(3)[None], cube)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lt.render_mesh(torch.tensor([[0., 0., 0., 1.]]), cube, size=8, rgb=False, samples=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshes.MeshSet([cube], "cpu")
    with pytest.raises(ValueError, match="at least one"):
        meshes.MeshSet([], "cuda:0")
    with pytest.raises(AssertionError, match="g must"):
        ops.render_mesh(torch.randn(4, 3), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MeshDataset.generate([cube], 4, size=8, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_batch(4, "cpu", [cube])


def test_mesh_dataset_host_side(tmp_path):
    """Item layout of the reference's ShapeDataset (experiments/datasets.py:72-85) on tensors
    given directly, the class attributes its training script reads, prep_batch, and the save /
    weights_only load round trip."""
    from torch.utils.data import DataLoader

    from lie_vae.experiments.datasets import MeshDataset
    names = torch.tensor([2, 0, 1, 1, 2])
    g, x = torch.randn(5, 3, 3), torch.rand(5, 3, 8, 8)
    ds = MeshDataset(tensors=(names, g, x))
    assert (ds.rgb, ds.single_id, ds.num_workers) == (True, False, 0) and len(ds) == 5
    name, gi, xi = ds[3]
    assert int(name) == 1 and name.dtype == torch.int64 and torch.equal(gi, g[3]) and torch.equal(xi, x[3])
    batch = ds.prep_batch(next(iter(DataLoader(ds, batch_size=4))))
    assert batch[0].dtype == torch.int64 and batch[0].tolist() == [2, 0, 1, 1]
    assert tuple(batch[1].shape) == (4, 3, 3) and tuple(batch[2].shape) == (4, 3, 8, 8)
    p = str(tmp_path / "meshes.pt")
    ds.save(p)
    back = MeshDataset(path=p)
    assert len(back) == 5 and all(torch.equal(a, b) for a, b in zip(ds.tensors, back.tensors))
    with pytest.raises(AssertionError, match="tensors must"):
        MeshDataset(tensors=(names.float(), g, x))


# ------------------------------------------------------------------ the restatement
@pytest.fixture(scope="module")
def rendered():
    """name -> (R, records, size, S, rgb, fp64 image, edge mask) of every parity case of
    tests/test_gpu_mesh.py, rendered once."""
    out = {}
    for name, (spec, R, size, S, rgb) in mr.parity_cases().items():
        R = R.astype(np.float32).astype(np.float64)
        rec, bad = mr.pack(*mr.case_arrays(spec))
        assert bad == 0
        out[name] = (R, rec, size, S, rgb) + mr.render(R, rec, size, S, rgb)
    return out


def test_cube_anchor_agrees_with_the_spherecube_restatement():
    """``cube()`` through this restatement against the sphere-cube restatement at that scene's
    12 parity poses (64 x 64, S = 2), on the pixels without a sub-sample on the sphere and
    outside both edge masks: the two cubes (slabs there, 12 triangles here) give the same fp64
    colours to 1e-12 (measured: 0) on at least 80 % of the pixels (measured: 94.6 %, at least
    87.6 % in every image)."""
    R, sc_img, cube_img, keep = mr.cube_anchor()
    assert R.shape == (12, 3, 3) and keep.shape == (12, 64, 64)
    share, least = keep.mean(), keep.reshape(12, -1).mean(axis=1).min()
    diff = np.abs(sc_img - cube_img).max(axis=1)
    print(f"anchor: {share:.2%} of the pixels compared (least image {least:.2%}), "
          f"max diff {diff[keep].max():.3e}")
    assert share >= 0.80 and least >= 0.80, (share, least)
    assert diff[keep].max() <= 1e-12
    # and the comparison is not vacuous: the compared pixels show all six faces
    seen = {tuple(np.round(c, 9)) for c in np.moveaxis(cube_img, 1, -1)[keep]}
    shade = 0.3 + 0.7 * np.maximum(0.0, np.array([1.0, -1.0] * 3) * np.repeat(sr.LIGHT, 2))
    for f in range(6):
        assert tuple(np.round(np.asarray(sr.FACE_ALBEDO[f]) * shade[f], 9)) in seen, f
    assert (0.0, 0.0, 0.0) in seen


def test_mask_cap_and_coverage_on_the_chosen_seeds(rendered):
    """The edge mask covers at most 2 % of the pixels of every parity case (measured: 0 to
    1.8 %), so it cannot hide a wrong image, at least 5 % of the pixels are not background, and
    the quarter turns the GPU test compares stay under the cap too."""
    for name, (R, rec, size, S, rgb, img, mask) in rendered.items():
        share, lit = mask.mean(), (img.max(axis=1) > 0).mean()
        print(f"{name}: masked {share:.4%}, not background {lit:.2%}")
        assert share <= mr.MASK_CAP, (name, share)
        assert lit >= 0.05, (name, lit)
        assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
    for name in mr.QUARTER_TURN_CASES:
        R, rec, size, S, rgb, img, mask = rendered[name]
        for k in (1, 2, 3):
            Rk = (R @ sr.rot_z(k)).astype(np.float32).astype(np.float64)
            imk, mk = mr.render(Rk, rec, size, S, rgb)
            both = mk | np.rot90(mask, -k, axes=(1, 2))
            assert both.mean() <= mr.MASK_CAP, (name, k, both.mean())
            err, _ = mr.off_edge_error(imk, np.rot90(img, -k, axes=(2, 3)), both)
            assert err <= 1e-12, (name, k, err)


def test_fp32_restatement_within_a_tenth_of_the_tolerance(rendered):
    """The bar of the GPU comparison (1e-5 off-edge) is at least ten times what the same
    arithmetic in fp32 numpy (packing and tracing) shows against fp64 on the same cases:
    measured 1.4e-7 at most (icosahedron 12 x 12, S = 4), so the bar is 74 times that."""
    worst = 0.0
    for name, (R, rec, size, S, rgb, img, mask) in rendered.items():
        spec = mr.parity_cases()[name][0]
        rec32, _ = mr.pack(*mr.case_arrays(spec), dtype=np.float32)
        img32, _ = mr.render(R, rec32, size, S, rgb, dtype=np.float32, mask=False)
        assert rec32.dtype == np.float32 and img32.dtype == np.float32
        err, _ = mr.off_edge_error(img32, img, mask)
        print(f"{name}: fp32 against fp64 off-edge {err:.3e}")
        worst = max(worst, err)
    assert worst > 0.0 and TOL >= 10 * worst, worst


def test_front_and_back_of_one_triangle(rendered):
    """The single triangle faces +z: the identity pose sees its front colour, the half turn
    about x its back colour; both are albedo times ambient + Lambert of +-n.l."""
    R, rec, size, S, rgb, img, mask = rendered["triangle 16x16 S=2 rgb"]
    alb = np.asarray(mr.TRIANGLE[2][0], dtype=np.float64)
    front = alb * (0.3 + 0.7 * 3 / np.sqrt(14))
    back = alb * 0.3
    np.testing.assert_allclose(rec[0, 9:12], front, rtol=0, atol=1e-15)
    np.testing.assert_allclose(rec[0, 12:15], back, rtol=0, atol=1e-15)
    np.testing.assert_allclose(img[0, :, 8, 8], front, rtol=0, atol=1e-15)
    np.testing.assert_allclose(img[1, :, 8, 8], back, rtol=0, atol=1e-15)
    assert np.array_equal(img[:, :, 0, 0], np.zeros((2, 3)))


def test_pack_marks_bad_indices_and_degenerate_triangles():
    """A face index equal to V or to -1 zeroes the record and is counted; a zero-area triangle
    keeps v0 and gets zero edges and zero colours; neither is ever hit."""
    from lie_vae import meshes
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 0)], dtype=np.float32)
    faces = np.array([(0, 1, 2), (0, 1, 4), (-1, 1, 2), (0, 1, 3), (2, 1, 0)])
    m = meshes.Mesh(v, faces, (0.5, 0.5, 0.5))  # the container keeps the indices: packing checks them
    assert np.array_equal(m.faces, faces)
    rec, bad = mr.pack(m.vertices, m.faces, m.albedo)
    assert bad == 2 and not rec[1].any() and not rec[2].any()
    assert rec[0, 9:15].min() > 0 and not rec[3, 3:15].any()
    _, hit = mr.trace(np.eye(3)[None], rec, np.tile(np.arange(16) + .5, 16),
                      np.repeat(np.arange(16) + .5, 16), 16)
    assert set(np.unique(hit)) <= {mr.NO_HIT, 0}   # triangle 4 coincides with 0: the lower index wins
    assert (hit == 0).any()
