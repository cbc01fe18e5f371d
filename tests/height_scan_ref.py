"""A numpy float32 restatement of the terrain height scan, written from legged_gym's published formulas (``_init_height_points``, ``_get_heights``,
``quat_apply_yaw``) and Isaac Gym's ``quat_apply`` and ``normalize``, independently of csrc/height_scan.h: the comparator of
tests/test_height_scan.py and tests/test_height_scan_gpu.py.  Every array is float32 and every operation one numpy operation, so each result is
rounded once, in legged_gym's order; the cell index alone is float64, as the plant forms it.

    points  = meshgrid(x, y) flattened, x the outer index
    quat    = root[:, 3:7] with [:, :2] = 0, divided by its norm clamped to >= 1e-9
    rotated = quat_apply(quat, (px, py, 0)):  t = cross(xyz, b) * 2;  b + w * t + cross(xyz, t)
    world   = rotated[:, :, :2] + root[:, None, :2]
    cell    = clip(trunc(((world + origin) - x0) / hscale), 0, count - 2), values that are negative or not a number going to 0 and values past the
              last node to the last node BEFORE the cast (include/mpc_terrain.h)
    height  = min(H[i, j], H[i + 1, j], H[i, j + 1]) * vscale
    column  = clip(clip(root_z - offset - height, -clip, clip) * scale, -obs_clip, obs_clip)
"""
import numpy as np

F = np.float32
DEFAULT_X = [-0.8, -0.7, -0.6, -0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
DEFAULT_Y = [-0.5, -0.4, -0.3, -0.2, -0.1, 0.0, 0.1, 0.2, 0.3, 0.4, 0.5]
# the four point grids of the tests: legged_gym's 17 x 11 (pad 5), 4 x 4 (pad 0), 1 x 1 (pad 15), 16 x 13 = 208 (the most the row takes)
GRIDS = {
    "17x11": (DEFAULT_X, DEFAULT_Y),
    "4x4": ([-0.3, -0.1, 0.1, 0.3], [-0.15, -0.05, 0.05, 0.15]),
    "1x1": ([0.25], [-0.125]),
    "16x13": ([round(-0.75 + 0.1 * i, 2) for i in range(16)], [round(-0.6 + 0.1 * j, 1) for j in range(13)]),
}
OFFSET, CLIP, SCALE, OBS_CLIP = 0.5, 1.0, 5.0, 5.0


def height_points(x, y):
    """[len(x) * len(y), 2] float32: p = i * len(y) + j is (x[i], y[j])."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    out = np.zeros((len(x) * len(y), 2), F)
    for i in range(len(x)):
        for j in range(len(y)):
            out[i * len(y) + j] = (x[i], y[j])
    return out


def padded_width(in_width, P):
    return -(-(in_width + P) // 16) * 16


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def quat_apply_yaw(quat, points):
    """quat [n, 4] xyzw float32, points [P, 2] float32 -> [n, P, 3] float32."""
    assert quat.dtype == F and points.dtype == F
    with np.errstate(all="ignore"):
        q = quat.copy()
        q[:, :2] = F(0)
        norm = np.sqrt(q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])              # (the two zero squares add nothing)
        q = q / np.fmax(norm, F(1e-9))[:, None]
        n, P = len(q), len(points)
        b = np.zeros((n, P, 3), F)
        b[:, :, :2] = points[None]
        xyz = np.broadcast_to(q[:, None, :3], (n, P, 3))
        t = _cross(xyz, b) * F(2)
        out = b + q[:, None, 3:] * t + _cross(xyz, t)
    assert out.dtype == F
    return out


def axis_index(v32, origin, x0, hscale, count):
    """The cell along one axis: v32 [n, P] float32 world-less-origin coordinates, origin [n] float64."""
    with np.errstate(all="ignore"):
        u = ((v32.astype(np.float64) + origin[:, None]) - x0) / hscale
        u = np.where(u > 0, u, 0.0)                                         # negative, -inf and NaN
        u = np.minimum(u, count - 1)                                        # +inf and everything past the last node
    return np.clip(u.astype(np.int64), 0, count - 2)


def scan(field, root, origin, points, obs_in, offset=OFFSET, clip=CLIP, scale=SCALE, obs_clip=OBS_CLIP):
    """field: dict(heights int16 [rows, cols], hscale, vscale, x0, y0); root [n, 13] float32; origin [n, 2] float64; points [P, 2] float32; obs_in
    [n, in_width] float32.  Returns dict(wide [n, padded_width] float32, heights [n, P] float32, i, j [n, P] int64)."""
    H = field["heights"]
    assert H.dtype == np.int16 and root.dtype == F and origin.dtype == np.float64 and obs_in.dtype == F
    n, P, in_width = len(root), len(points), obs_in.shape[1]
    with np.errstate(all="ignore"):
        world = quat_apply_yaw(root[:, 3:7], points)[:, :, :2] + root[:, None, :2]
    assert world.dtype == F
    i = axis_index(world[:, :, 0], origin[:, 0], field["x0"], field["hscale"], H.shape[0])
    j = axis_index(world[:, :, 1], origin[:, 1], field["y0"], field["hscale"], H.shape[1])
    lowest = np.minimum(np.minimum(H[i, j], H[i + 1, j]), H[i, j + 1])
    assert lowest.dtype == np.int16
    heights = lowest.astype(F) * F(field["vscale"])
    with np.errstate(all="ignore"):
        d = (root[:, 2:3] - F(offset)) - heights
        col = np.fmin(np.fmax(d, -F(clip)), F(clip)) * F(scale)
        col = np.fmin(np.fmax(col, -F(obs_clip)), F(obs_clip))
    wide = np.zeros((n, padded_width(in_width, P)), F)
    wide[:, :in_width] = obs_in
    wide[:, in_width:in_width + P] = col
    assert heights.dtype == F and col.dtype == F
    return dict(wide=wide, heights=heights, i=i, j=j)


# ---- the crafted field and batch ------------------------------------------------------------------------------------------------------------------
ROWS, COLS, HSCALE, VSCALE, X0, Y0 = 12, 9, 0.25, 0.005, -0.5, -0.25       # spans x in [-0.5, 2.25], y in [-0.25, 1.75]


def crafted_field():
    H = np.random.default_rng(11).integers(-60, 61, (ROWS, COLS)).astype(np.int16)
    H[4, 3] = -32768                                                        # the lowest of every cell that touches it
    H[6, 5] = H[7, 5] = H[6, 6] = 32767                                     # the lowest of cell (6, 5) alone
    return dict(heights=H, hscale=HSCALE, vscale=VSCALE, x0=X0, y0=Y0)


def _root(x, y, z, quat=(0.0, 0.0, 0.0, 1.0)):
    r = np.zeros(13, F)
    r[:3] = (x, y, z)
    r[3:7] = quat
    r[7:] = (0.3, -0.2, 0.1, 0.05, -0.04, 0.03)                             # velocities: not the scan's business
    return r


def _border_origin(p, r, node, ulps):
    """The float64 origin that puts `node` exactly `-ulps` float32 steps from where the float32 sum p + r lands (yaw 0: the rotation is exact), so
    that the point lands on the border (0), one float32 ulp below it (-1) or one above (1).  Sums of two float32 numbers do not reach every
    neighbour of a node, so the border is moved and not the point; every difference here is exact in float64."""
    w = F(F(p) + F(r))
    at = w if ulps == 0 else np.nextafter(w, F(-np.inf if ulps > 0 else np.inf), dtype=F)
    return float(node) - float(at)


def _yaw_quat(yaw):
    return (0.0, 0.0, float(np.sin(yaw / 2)), float(np.cos(yaw / 2)))


PATTERN = 27
PROBE = 0                                                                  # the point whose landing the border rows craft
NODE_X = lambda k: X0 + HSCALE * k                                          # noqa: E731
NODE_Y = lambda k: Y0 + HSCALE * k                                          # noqa: E731


def crafted(n, points):
    """n environments cycling through PATTERN kinds of rows.  Returns dict(root [n, 13] float32, origin [n, 2] float64, kind [n], expect {row: (axis,
    cell)} for the rows whose origin puts a cell border on, or one float32 ulp beside, where the PROBE point lands)."""
    px, py = points[PROBE]
    root, origin, kind, expect = np.zeros((n, 13), F), np.zeros((n, 2), np.float64), np.zeros(n, np.int64), {}
    for r in range(n):
        k, cyc = r % PATTERN, r // PATTERN
        kx, ky = 3 + cyc % 6, 2 + cyc % 5                                   # the node the border rows aim at
        cx, cy, z = 1.0 + 0.037 * cyc, 0.75 - 0.021 * cyc, 0.45 + 0.05 * ((r * 7) % 13)
        kind[r] = k
        if k == 0:
            root[r] = _root(cx, cy, z)
        elif k in (1, 2, 3):                                                # the probe's x exactly on node kx, one ulp below, one above
            root[r] = _root(cx, cy, z)
            origin[r, 0] = _border_origin(px, cx, NODE_X(kx), (0, -1, 1)[k - 1])
            expect[r] = (0, kx - 1 if k == 2 else kx)
        elif k in (4, 5, 6):                                                # the same along y
            root[r] = _root(cx, cy, z)
            origin[r, 1] = _border_origin(py, cy, NODE_Y(ky), (0, -1, 1)[k - 4])
            expect[r] = (1, ky - 1 if k == 5 else ky)
        elif k == 7:                                                        # yaw 180 degrees: the rotation is exact, the point lands at root - p
            root[r] = _root(cx, cy, z, (0.0, 0.0, 1.0, 0.0))
        elif k == 8:
            root[r] = _root(cx, cy, z, _yaw_quat(0.7 + 0.4 * cyc))
        elif k == 9:                                                        # pitched and rolled: x and y of the quaternion are ignored
            q = np.array([0.21, -0.17, 0.43, 0.86])
            root[r] = _root(cx, cy, z, tuple(q / np.linalg.norm(q)))
        elif k == 10:                                                       # z = w = 0: the 1e-9 clamp leaves the points unrotated
            root[r] = _root(cx, cy, z, (0.6, 0.8, 0.0, 0.0))
        elif k in (11, 12, 13, 14, 15, 16):                                 # beyond the four edges and two corners
            x, y = ((-5.0, cy), (7.0, cy), (cx, -4.0), (cx, 6.0), (9.0, 8.0), (-9.0, -8.0))[k - 11]
            root[r] = _root(x, y, z, _yaw_quat(0.3))
        elif k == 17:                                                       # a far origin: the index is float64, float32 would lose the position
            origin[r] = (1000.125, -1000.125)
            root[r] = _root(-999.2 + 0.013 * cyc, 1000.9, z, _yaw_quat(-1.1))
        elif k == 18:
            root[r] = _root(np.nan, cy, z)
        elif k == 19:
            root[r] = _root(cx, np.inf, z)
        elif k == 20:
            root[r] = _root(-np.inf, np.nan, z, _yaw_quat(2.0))
        elif k == 21:
            root[r] = _root(cx, cy, z, (0.0, 0.0, np.nan, 0.8))
        elif k == 22:
            root[r] = _root(cx, cy, z, (0.0, 0.0, 0.5, np.inf))
        elif k == 23:                                                       # a root height that is not a number: fmaxf / fminf give -clip * scale
            root[r] = _root(cx, cy, np.nan)
        elif k == 24:                                                       # not normalised: normalize divides
            root[r] = _root(cx, cy, z, (0.0, 0.0, 3.0, 4.0))
        elif k == 25:                                                       # over the int16 extremes: cells (4, 3) and (6, 5)
            root[r] = _root(NODE_X(4) + 0.1 - px, NODE_Y(3) + 0.1 - py, z)
        else:
            root[r] = _root(NODE_X(6) + 0.1 - px, NODE_Y(5) + 0.1 - py, z)
    return dict(root=root, origin=origin, kind=kind, expect=expect)


def sentinel_obs(n, in_width=48):
    return (1000.0 + np.arange(n, dtype=np.float64)[:, None] + np.arange(in_width)[None] / 64.0).astype(F)
