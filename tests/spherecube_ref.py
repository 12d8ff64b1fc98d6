"""numpy restatement of the sphere-cube scene of csrc/render.hip, fp64 by
default, with the per-pixel edge mask the comparisons need.

Scene: the cube [-1,1]^3 with one albedo per face and a sphere of radius 0.6 at (0,0,1), lit
by l = (1,2,3)/sqrt(14) in the object frame (Lambert + 0.3 ambient, no specular).  The pose R
is the camera frame: the camera sits at 5 R[:,2], looks along its own -z with +y up, and is a
pinhole of half-width 0.4 at unit distance.  A pixel is the mean of its S x S regular
sub-samples, added row by row.

A ray within a rounding of a silhouette or a cube edge may land on either side of it, so
``render`` also returns a mask of the pixels with a sub-sample whose hit id (face 0-5, sphere 6,
background 7) changes when the sample moves by +-EDGE_SHIFT pixel in x or in y; value
comparisons leave those pixels out (and assert that they are few: ``MASK_CAP``).
"""
import numpy as np

TAU = 0.4                     # half-width of the image plane at unit distance
CAM_DIST = 5.0
SPHERE_C = (0.0, 0.0, 1.0)
SPHERE_R = 0.6
SPHERE_ALBEDO = (0.95, 0.95, 0.95)
# faces +x, -x, +y, -y, +z, -z (id = 2 axis + (0 for +, 1 for -))
FACE_ALBEDO = ((.9, .1, .1), (.1, .8, .8), (.1, .8, .1), (.8, .1, .8), (.1, .1, .9), (.9, .9, .1))
LIGHT = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
AMBIENT, DIFFUSE = 0.3, 0.7
ID_SPHERE, ID_BACKGROUND = 6, 7
EDGE_SHIFT = 1e-3             # pixels
MASK_CAP = 0.02               # largest share of masked pixels a comparison accepts


def trace(R, kx, ky, size, dtype=np.float64):
    """Colours (n, P, 3) and hit ids (n, P) of the rays through the image-plane positions
    (kx, ky) (pixel units, arrays of P values) for the poses R (n, 3, 3)."""
    f = dtype
    R = np.asarray(R, dtype=f)
    kx, ky = np.asarray(kx, dtype=f), np.asarray(ky, dtype=f)
    u = ((kx / f(size) - f(0.5)) * f(2 * TAU))[None, :, None]
    v = ((f(0.5) - ky / f(size)) * f(2 * TAU))[None, :, None]
    o = (f(CAM_DIST) * R[:, :, 2])[:, None, :]                      # (n, 1, 3)
    d = (u * R[:, None, :, 0] + v * R[:, None, :, 1]) - R[:, None, :, 2]   # (n, P, 3)
    inf = f(np.inf)
    with np.errstate(all="ignore"):
        # ---- cube: slabs; a zero component never meets 0 * inf
        inv = f(1) / d
        par = (d == 0) | np.isinf(inv)
        t1 = (f(-1) - o) * inv
        t2 = (f(1) - o) * inv
        inside = np.abs(o) <= 1
        tn = np.where(par, np.where(inside, -inf, inf), np.minimum(t1, t2))
        tf = np.where(par, np.where(inside, inf, -inf), np.maximum(t1, t2))
        axis = np.zeros(tn.shape[:2], dtype=np.int64)
        t_in = tn[..., 0].copy()
        for a in (1, 2):
            better = tn[..., a] > t_in
            axis = np.where(better, a, axis)
            t_in = np.where(better, tn[..., a], t_in)
        t_out = np.minimum(np.minimum(tf[..., 0], tf[..., 1]), tf[..., 2])
        cube = (t_in <= t_out) & (t_out > 0)
        d_ax = np.take_along_axis(d, axis[..., None], -1)[..., 0]
        face = 2 * axis + np.where(d_ax < 0, 0, 1)
        # ---- sphere: r^2 - |oc - (oc.d / d.d) d|^2, near root
        oc = o - np.asarray(SPHERE_C, dtype=f)
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        od = (oc[..., 0] * d[..., 0] + oc[..., 1] * d[..., 1]) + oc[..., 2] * d[..., 2]
        s = od / dd
        p = oc - s[..., None] * d
        disc = f(SPHERE_R * SPHERE_R) - ((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])
        t_s = -s - np.sqrt(disc / dd)
        sphere = (disc >= 0) & (t_s > 0)
        nrm = (oc + t_s[..., None] * d) / f(SPHERE_R)
        light = LIGHT.astype(f)
        nl = (nrm[..., 0] * light[0] + nrm[..., 1] * light[1]) + nrm[..., 2] * light[2]
        shade_s = f(AMBIENT) + f(DIFFUSE) * np.maximum(f(0), nl)
    # ---- nearest hit
    take_s = sphere & (~cube | (t_s < t_in))
    hit = np.where(take_s, ID_SPHERE, np.where(cube, face, ID_BACKGROUND))
    sgn = np.array([1.0, -1.0] * 3)
    face_shade = AMBIENT + DIFFUSE * np.maximum(0.0, sgn * np.repeat(LIGHT, 2))
    table = np.zeros((8, 3))
    table[:6] = np.asarray(FACE_ALBEDO) * face_shade[:, None]
    col = table.astype(f)[hit]
    col = np.where(take_s[..., None], np.asarray(SPHERE_ALBEDO, dtype=f) * shade_s[..., None], col)
    return col.astype(f), hit


def _positions(size, S, dtype):
    """(ky, kx) of every sub-sample, laid out (i, a, j, b)."""
    f = dtype
    pix = np.arange(size).astype(f)
    off = ((np.arange(S).astype(f) + f(0.5)) / f(S))
    k = pix[:, None] + off[None, :]                       # (size, S)
    ky = np.broadcast_to(k[:, :, None, None], (size, S, size, S)).reshape(-1)
    kx = np.broadcast_to(k[None, None, :, :], (size, S, size, S)).reshape(-1)
    return ky, kx


def render(R, size=64, samples=2, rgb=True, dtype=np.float64):
    """Images (n, 3 | 1, size, size) and the edge mask (n, size, size), True = leave out."""
    f = dtype
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    n, S = R.shape[0], samples
    ky, kx = _positions(size, S, f)
    col, hit = trace(R, kx, ky, size, f)
    col = col.reshape(n, size, S, size, S, 3)
    acc = np.zeros((n, size, size, 3), dtype=f)
    for a in range(S):            # the kernel's order: rows of sub-samples, then columns
        for b in range(S):
            acc = acc + col[:, :, a, :, b, :]
    img = np.moveaxis(acc / f(S * S), -1, 1)
    if not rgb:
        img = (((img[:, 0] + img[:, 1]) + img[:, 2]) / f(3))[:, None]
    # edge mask, always from fp64 positions
    ky64, kx64 = _positions(size, S, np.float64)
    _, hit0 = trace(R, kx64, ky64, size)
    edge = np.zeros(hit0.shape, dtype=bool)
    for dx, dy in ((EDGE_SHIFT, 0), (-EDGE_SHIFT, 0), (0, EDGE_SHIFT), (0, -EDGE_SHIFT)):
        _, h = trace(R, kx64 + dx, ky64 + dy, size)
        edge |= h != hit0
    mask = edge.reshape(n, size, S, size, S).any(axis=(2, 4))
    return np.ascontiguousarray(img), mask


def haar_poses(n, seed):
    """n Haar rotations (fp64) from a seeded numpy generator: normalised Gaussian quaternions."""
    q = np.random.default_rng(seed).standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
                    -1).reshape(n, 3, 3)


def face_on_poses():
    """The six views along a coordinate axis (entries 0 and +-1 exactly), camera on +x, -x,
    +y, -y, +z, -z in turn."""
    out = []
    for k in range(3):
        for s in (1.0, -1.0):
            z = np.zeros(3)
            z[k] = s
            x = np.zeros(3)
            x[(k + 1) % 3] = 1.0
            out.append(np.stack([x, np.cross(z, x), z], 1))
    return np.stack(out)


def parity_cases():
    """name -> (R (n,3,3) fp64, size, samples, rgb): the cases the device is compared on.  The
    seeds are chosen so that the edge mask of each case (and of its quarter turns) stays under
    MASK_CAP; tests/test_spherecube_cpu.py asserts that."""
    eye = np.eye(3)[None]
    return {
        "64x64 S=2 rgb": (np.concatenate([haar_poses(5, 0), eye, face_on_poses()]), 64, 2, True),
        "8x8 S=1 grey": (haar_poses(3, 1), 8, 1, False),
        "7x7 S=3 rgb": (np.concatenate([haar_poses(3, 2), eye]), 7, 3, True),
        "12x12 S=4 rgb": (haar_poses(2, 3), 12, 4, True),
    }


def rot_z(k):
    """Rz(90 deg k), exact."""
    c, s = ((1, 0), (0, 1), (-1, 0), (0, -1))[k % 4]
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def off_edge_error(x, ref, mask):
    """Largest |x - ref| over the unmasked pixels (all channels) and the masked share."""
    diff = np.abs(np.asarray(x, dtype=np.float64) - ref).max(axis=1)
    return float(np.where(mask, 0.0, diff).max()), float(mask.mean())
