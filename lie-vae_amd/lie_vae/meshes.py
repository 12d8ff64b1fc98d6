"""Triangle meshes for the device renderer (csrc/render_mesh.hip).

``Mesh`` is a host-side container (numpy); ``cube`` ... ``icosphere`` build the usual solids
with outward windings; ``load_obj`` reads the ``v`` and ``f`` lines of a Wavefront file;
``MeshSet`` packs K meshes into the record and range tensors ``lie_tools.render_mesh`` takes.
Extension: the reference has no meshes, its ShapeDataset reads images rendered elsewhere.
"""
import numpy as np
import torch

from . import _lib, _ops

__all__ = ["Mesh", "MeshSet", "cube", "tetrahedron", "octahedron", "icosahedron", "icosphere",
           "load_obj", "palette", "CUBE_FACE_ALBEDO"]

# the sphere-cube scene's face colours, faces +x, -x, +y, -y, +z, -z (csrc/render.hip)
CUBE_FACE_ALBEDO = ((.9, .1, .1), (.1, .8, .8), (.1, .8, .1), (.8, .1, .8), (.1, .1, .9), (.9, .9, .1))


def palette(count):
    """(count, 3) float32 albedos, distinct and RNG-free: hues a golden-ratio step apart at
    saturation 0.75 and value 0.9."""
    h = (np.arange(count, dtype=np.float64) * 0.6180339887498949) % 1.0
    k = (np.array([5.0, 3.0, 1.0])[None, :] + h[:, None] * 6.0) % 6.0
    rgb = 0.9 * (1.0 - 0.75 * np.clip(np.minimum(k, 4.0 - k), 0.0, 1.0))
    return rgb.astype(np.float32)


class Mesh:
    """vertices (V,3) float32, faces (T,3) int64 (indices into vertices; checked on the
    device when the mesh is packed), albedo (T,3) float32 in [0, 1]: given per triangle, as
    one colour (3,), or None for ``palette(T)``."""

    def __init__(self, vertices, faces, albedo=None):
        self.vertices = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
        faces = np.asarray(faces)
        if faces.size and not np.issubdtype(faces.dtype, np.integer):
            raise ValueError(f"faces must be integers, got {faces.dtype}")
        self.faces = np.ascontiguousarray(faces.reshape(-1, 3).astype(np.int64))
        T = self.faces.shape[0]
        if albedo is None:
            albedo = palette(T)
        albedo = np.asarray(albedo, dtype=np.float32)
        if albedo.shape == (3,):
            albedo = np.broadcast_to(albedo, (T, 3))
        if albedo.shape != (T, 3):
            raise ValueError(f"albedo must be (T,3) = ({T},3), (3,) or None, got {albedo.shape}")
        if not (np.isfinite(albedo).all() and albedo.min(initial=0.0) >= 0.0 and albedo.max(initial=0.0) <= 1.0):
            raise ValueError("albedo must lie in [0, 1]")
        self.albedo = np.ascontiguousarray(albedo)

    def normalized(self, radius=1.5):
        """The mesh centred on its bounding box and scaled so that its largest vertex norm is
        ``radius`` (the camera's view covers a ball of radius about 1.9)."""
        v = self.vertices.astype(np.float64)
        v = v - (v.min(axis=0) + v.max(axis=0)) / 2
        v = v * (radius / np.sqrt((v * v).sum(axis=1)).max())
        return Mesh(v, self.faces, self.albedo)

    def signed_volume(self):
        """Sum of v0 . (v1 x v2) / 6 (fp64): positive for a closed mesh wound outwards."""
        a, b, c = (self.vertices[self.faces[:, k]].astype(np.float64) for k in range(3))
        return float((a * np.cross(b, c)).sum() / 6.0)


def _convex(vertices, edge, albedo=None):
    """The convex solid whose faces are the vertex triples at mutual distance ``edge``, in
    index order, each wound outwards (the solid contains the origin)."""
    v = np.asarray(vertices, dtype=np.float64)
    n = len(v)
    dist = np.sqrt(((v[:, None] - v[None]) ** 2).sum(-1))
    near = np.abs(dist - edge) < 1e-9
    faces = []
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                if near[i, j] and near[j, k] and near[i, k]:
                    out = np.dot(np.cross(v[j] - v[i], v[k] - v[i]), v[i] + v[j] + v[k]) > 0
                    faces.append((i, j, k) if out else (i, k, j))
    return Mesh(v, faces, albedo)


def tetrahedron():
    """4 vertices, 4 faces, vertex norm sqrt 3."""
    return _convex([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.sqrt(8.0))


def octahedron():
    """6 vertices, 8 faces, vertex norm 1."""
    return _convex([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.sqrt(2.0))


def icosahedron():
    """12 vertices, 20 faces, vertex norm 1."""
    p = (1 + np.sqrt(5.0)) / 2
    v = [c for a in (1, -1) for b in (p, -p) for c in ((0, a, b), (a, b, 0), (b, 0, a))]
    return _convex(np.asarray(v) / np.sqrt(1 + p * p), 2 / np.sqrt(1 + p * p))


def icosphere(level):
    """The icosahedron with every triangle split in four ``level`` times and the new vertices
    pushed onto the unit sphere: 20 * 4**level triangles."""
    base = icosahedron()
    verts = [tuple(p) for p in base.vertices.astype(np.float64)]
    faces = [tuple(f) for f in base.faces]
    for _ in range(level):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = (np.asarray(verts[a]) + np.asarray(verts[b])) / 2
                verts.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(verts) - 1
            return mid[key]

        split = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            split += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = split
    return Mesh(verts, faces)


def cube():
    """[-1,1]^3 as 12 triangles, two per face, faces in the sphere-cube scene's order +x, -x,
    +y, -y, +z, -z with that scene's albedos."""
    verts = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
    faces, albedo = [], []
    for axis in range(3):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        for sign in (1, -1):
            ring = []
            for sb, sc in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = [0, 0, 0]
                p[axis], p[b], p[c] = sign, sb, sc
                ring.append(verts.index(tuple(p)))
            if sign < 0:
                ring.reverse()
            faces += [(ring[0], ring[1], ring[2]), (ring[0], ring[2], ring[3])]
            albedo += [CUBE_FACE_ALBEDO[2 * axis + (sign < 0)]] * 2
    return Mesh(verts, faces, albedo)


def load_obj(path):
    """The ``v x y z`` and ``f ...`` lines of a Wavefront OBJ file as a Mesh.  Face tokens may
    be ``i``, ``i/j``, ``i//k`` or ``i/j/k`` (only the vertex index is used), 1-based or
    negative (relative to the vertices read so far); a polygon becomes a triangle fan.  All
    other lines are ignored.  A malformed ``v`` or ``f`` line raises ValueError."""
    verts, faces = [], []
    with open(path, "r", errors="replace") as fh:
        for lineno, line in enumerate(fh, 1):
            tok = line.split("#", 1)[0].split()
            if not tok or tok[0] not in ("v", "f"):
                continue
            try:
                if tok[0] == "v":
                    if len(tok) < 4:
                        raise ValueError("a vertex needs three coordinates")
                    verts.append([float(t) for t in tok[1:4]])
                else:
                    if len(tok) < 4:
                        raise ValueError("a face needs at least three vertices")
                    idx = []
                    for t in tok[1:]:
                        i = int(t.split("/")[0])
                        i = i - 1 if i > 0 else len(verts) + i  # 0 is no index: it lands on len(verts)
                        if i < 0 or i >= len(verts):
                            raise ValueError(f"vertex index {t!r} outside the {len(verts)} vertices read")
                        idx.append(i)
                    faces += [(idx[0], idx[k], idx[k + 1]) for k in range(1, len(idx) - 1)]
            except ValueError as e:
                raise ValueError(f"{path}:{lineno}: {e}") from None
    if not verts or not faces:
        raise ValueError(f"{path}: no vertices or no faces")
    return Mesh(verts, faces)


class MeshSet:
    """K meshes packed for the renderer on ``device``: ``records`` (total,16) fp32 (one
    mesh_pack launch per mesh), ``ranges`` (K,2) int32 = (first record, count).  Construction
    reads the bad-index counters once -- the set's only host sync -- and raises ValueError
    naming the first mesh with a face index outside its vertices."""

    def __init__(self, meshes, device):
        meshes = [meshes] if isinstance(meshes, Mesh) else list(meshes)
        if not meshes:
            raise ValueError("MeshSet needs at least one mesh")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("lie_vae ops run only on the MI355X HIP path (got device "
                               f"{device}). There is no CPU fallback.")
        counts = [m.faces.shape[0] for m in meshes]
        starts = [int(s) for s in np.concatenate([[0], np.cumsum(counts)[:-1]])]
        self.K, self.total_records = len(meshes), int(sum(counts))
        pairs = list(zip(starts, counts))
        # the host-side check of the ranges against the record count (and of the limits)
        _lib.render_mesh_plan(0, 1, 1, 1, K=self.K, total_records=self.total_records, ranges=pairs)
        self.triangles = tuple(counts)
        self.records = torch.zeros((max(self.total_records, 1), 16), device=device, dtype=torch.float32)
        self.ranges = torch.tensor(pairs, dtype=torch.int32).reshape(self.K, 2).to(device)
        bad = torch.zeros(self.K, device=device, dtype=torch.int32)
        for k, (m, start, T) in enumerate(zip(meshes, starts, counts)):
            if T == 0:
                continue
            if m.faces.max() > np.iinfo(np.int32).max or m.faces.min() < np.iinfo(np.int32).min:
                raise ValueError(f"mesh {k}: a face index does not fit 32 bits")
            _ops.mesh_pack(torch.from_numpy(m.vertices).to(device),
                           torch.from_numpy(m.faces.astype(np.int32)).to(device),
                           torch.from_numpy(m.albedo).to(device),
                           self.records[start:start + T], bad[k:k + 1])
        bad = bad.cpu().tolist()
        for k, b in enumerate(bad):
            if b:
                raise ValueError(f"mesh {k}: {b} of its {counts[k]} triangles have a face index "
                                 f"outside its {meshes[k].vertices.shape[0]} vertices")

    @property
    def device(self):
        return self.records.device
