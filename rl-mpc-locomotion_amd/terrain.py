"""Height-field terrain for the toy plant (include/mpc_terrain.h, csrc/toy_sim.h's HeightField): the container, the surface in numpy, a
generator and a placement of robot origins.

The surface, one definition for the header, this module and the documents.  ``H[rows][cols]`` int16, row index along x, ``hscale`` metres
per cell, ``vscale`` metres per unit, node (0, 0) at world ``(x0, y0)``.  In float64, in this order::

    u = ((x + ox) - x0) / hscale;  if not u > 0: u = 0;  if u > rows - 1: u = rows - 1
    i = int(u);  if i > rows - 2: i = rows - 2;  fu = u - i                  (the same for v, j, fv with y, oy, y0, cols)
    z00 = vscale H[i][j], z10 = vscale H[i+1][j], z01 = vscale H[i][j+1], z11 = vscale H[i+1][j+1]
    fu >= fv:  z = z00 + fu (z10 - z00) + fv (z11 - z10),  gx = (z10 - z00) / hscale,  gy = (z11 - z10) / hscale
    else:      z = z00 + fv (z01 - z00) + fu (z11 - z01),  gx = (z11 - z01) / hscale,  gy = (z01 - z00) / hscale
    normal = (-gx, -gy, 1) / |.|

The clamp is in floating point before the integer conversion, so NaN, infinities and 1e300 land on the field and outside it the surface
continues with the border's heights.  A cell is split along the diagonal (i, j) - (i+1, j+1): that is how Isaac Gym's
``convert_heightfield_to_trimesh`` splits it (triangles (ind0, ind3, ind1) and (ind0, ind2, ind3)), restated here from its published
definition -- isaacgym is not a dependency and nothing is checked against it.  Its ``slope_threshold`` correction is not modelled; for the
reference's parameters (threshold 1.5) no cell of ``Terrain.reference`` is steep enough for it to apply.

``random_uniform_terrain`` restates Isaac Gym's generator of the same name by its published algorithm with numpy only; parity is in
construction, not in the draws (``numpy.random.default_rng(seed)``, not the global generator).
"""
import numpy as np

from ._lib import cd, ci, text, vp

# the entry points of include/mpc_terrain.h (bound by toy_sim.lib(), whose handle they act on; not in _lib.SYMBOLS, which lists include/mpc_batch.h)
DECLS = {
    "mpc_terrain_attach": (ci, [vp, ci, ci, vp, cd, cd, cd, cd, vp]),
    "mpc_terrain_query": (ci, [vp, vp, ci, vp, vp, vp]),
    "mpc_terrain_last_error": (text, []),
}
SYMBOLS = list(DECLS)


class Terrain:
    """A plain container: ``heights`` int16 [rows, cols], ``hscale``, ``vscale``, ``x0``, ``y0``, and the surface in numpy."""

    def __init__(self, heights, hscale, vscale, x0=0.0, y0=0.0):
        h = np.asarray(heights)
        if h.ndim != 2 or h.shape[0] < 2 or h.shape[1] < 2:
            raise ValueError("heights: a [rows, cols] array with rows, cols >= 2")
        if h.dtype != np.int16:
            if not np.array_equal(h, np.rint(h)) or np.abs(h).max() > 32767:
                raise ValueError("heights must hold int16 values")
            h = h.astype(np.int16)
        self.heights = np.ascontiguousarray(h)
        self.rows, self.cols = self.heights.shape
        self.hscale, self.vscale, self.x0, self.y0 = float(hscale), float(vscale), float(x0), float(y0)
        if not (np.isfinite(self.hscale) and self.hscale > 0 and np.isfinite(self.vscale) and self.vscale > 0):
            raise ValueError("hscale and vscale must be finite and > 0")
        if not (np.isfinite(self.x0) and np.isfinite(self.y0)):
            raise ValueError("x0 and y0 must be finite")

    def __deepcopy__(self, memo):
        return self                    # (read-only by convention: a copied robot model shares its terrain)

    # ---- the surface ------------------------------------------------------------------------------------------------------------------
    def _index_scalar(self, x, o, x0, count):
        u = ((x + o) - x0) / self.hscale
        if not u > 0:
            u = 0.0
        if u > count - 1:
            u = float(count - 1)
        i = int(u)
        if i > count - 2:
            i = count - 2
        return i, u - i

    def _index(self, x, o, x0, count):
        with np.errstate(invalid="ignore", over="ignore"):
            u = ((x + o) - x0) / self.hscale
            u = np.where(u > 0, u, 0.0)
            u = np.where(u > count - 1, float(count - 1), u)
        i = np.minimum(u.astype(np.int64), count - 2)
        return i, u - i

    def cell(self, x, y, origin=(0.0, 0.0)):
        """(i, j, fu, fv): the cell under (x, y) + origin and the fractions inside it.  Scalars give Python scalars (the numpy model's path, the
        same IEEE operations one at a time), arrays give arrays."""
        ox, oy = origin
        if np.ndim(x) == 0 and np.ndim(y) == 0:
            i, fu = self._index_scalar(float(x), float(ox), self.x0, self.rows)
            j, fv = self._index_scalar(float(y), float(oy), self.y0, self.cols)
            return i, j, fu, fv
        x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
        i, fu = self._index(x, ox, self.x0, self.rows)
        j, fv = self._index(y, oy, self.y0, self.cols)
        return i, j, fu, fv

    def surface(self, x, y, origin=(0.0, 0.0)):
        """(z, gx, gy, upper) at (x, y) + origin; ``upper`` marks the triangle with fu >= fv."""
        i, j, fu, fv = self.cell(x, y, origin)
        H, vs, hs = self.heights, self.vscale, self.hscale
        if np.ndim(i) == 0:
            z00, z10, z01, z11 = vs * float(H[i, j]), vs * float(H[i + 1, j]), vs * float(H[i, j + 1]), vs * float(H[i + 1, j + 1])
            if fu >= fv:
                return z00 + fu * (z10 - z00) + fv * (z11 - z10), (z10 - z00) / hs, (z11 - z10) / hs, True
            return z00 + fv * (z01 - z00) + fu * (z11 - z01), (z11 - z01) / hs, (z01 - z00) / hs, False
        z00, z10, z01, z11 = (vs * H[i, j].astype(np.float64), vs * H[i + 1, j].astype(np.float64), vs * H[i, j + 1].astype(np.float64),
                              vs * H[i + 1, j + 1].astype(np.float64))
        upper = fu >= fv
        z = np.where(upper, z00 + fu * (z10 - z00) + fv * (z11 - z10), z00 + fv * (z01 - z00) + fu * (z11 - z01))
        gx = np.where(upper, (z10 - z00) / hs, (z11 - z01) / hs)
        gy = np.where(upper, (z11 - z10) / hs, (z01 - z00) / hs)
        return z, gx, gy, upper

    def height(self, x, y, origin=(0.0, 0.0)):
        return self.surface(x, y, origin)[0]

    def normal(self, x, y, origin=(0.0, 0.0)):
        """Unit normal (-gx, -gy, 1) / |.|, shape [..., 3]."""
        _, gx, gy, _ = self.surface(x, y, origin)
        n = np.stack([-np.asarray(gx, np.float64), -np.asarray(gy, np.float64), np.ones_like(gx, dtype=np.float64)], -1)
        return n / np.sqrt(n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2])[..., None]

    def max_cell_slope(self):
        """The largest |height difference| / hscale between two neighbouring nodes (along x or y), what the mesh's slope_threshold compares."""
        z = self.heights.astype(np.float64) * self.vscale
        return float(max(np.abs(np.diff(z, axis=0)).max(), np.abs(np.diff(z, axis=1)).max()) / self.hscale)

    @property
    def extent(self):
        """((x_min, x_max), (y_min, y_max)) of the field's nodes."""
        return ((self.x0, self.x0 + (self.rows - 1) * self.hscale), (self.y0, self.y0 + (self.cols - 1) * self.hscale))

    # ---- presets ----------------------------------------------------------------------------------------------------------------------
    @classmethod
    def reference(cls, seed=0):
        """The reference's ``add_random_uniform_terrain`` (RL_Environment/sim_utils.py:192-212): 50 m x 50 m at 0.1 m, 0.005 m units, heights
        -0.2 .. 0 m in 0.05 m steps on a 0.3 m grid, the mesh transform (-50/3, -50/3) as (x0, y0)."""
        return cls.random_uniform(500, 500, min_height=-0.2, max_height=0.0, step=0.05, seed=seed, x0=-50.0 / 3, y0=-50.0 / 3)

    @classmethod
    def mild(cls, seed=0, rows=500, cols=500):
        """The same generator with -0.04 .. 0 m in 0.01 m steps."""
        return cls.random_uniform(rows, cols, min_height=-0.04, max_height=0.0, step=0.01, seed=seed, x0=-(rows * 0.1) / 3, y0=-(cols * 0.1) / 3)

    @classmethod
    def random_uniform(cls, rows, cols, min_height, max_height, step, seed, hscale=0.1, vscale=0.005, downsampled_scale=0.3, x0=0.0, y0=0.0):
        return cls(random_uniform_terrain(rows, cols, hscale, vscale, min_height, max_height, step, downsampled_scale, seed), hscale, vscale, x0, y0)


def random_uniform_terrain(rows, cols, hscale, vscale, min_height, max_height, step, downsampled_scale, seed):
    """Isaac Gym's ``terrain_utils.random_uniform_terrain`` restated from its published algorithm: a uniform choice over
    ``arange(int(min / vs), int(max / vs) + int(step / vs), int(step / vs))`` on the downsampled grid
    (``int(rows hscale / downsampled_scale)`` x ``int(cols hscale / downsampled_scale)`` nodes spanning the field), linear interpolation onto
    ``linspace(0, rows hscale, rows)`` x ``linspace(0, cols hscale, cols)`` -- separable, with ``np.interp`` along x and then along y, where
    the original calls scipy's ``interp2d(kind='linear')`` -- then ``rint`` and int16.  Returns int16 [rows, cols]."""
    if downsampled_scale is None:
        downsampled_scale = hscale
    lo, hi, st = int(min_height / vscale), int(max_height / vscale), int(step / vscale)
    if st <= 0 or hi < lo:
        raise ValueError("step must be at least one vertical unit and max_height >= min_height")
    heights_range = np.arange(lo, hi + st, st)
    nx, ny = int(rows * hscale / downsampled_scale), int(cols * hscale / downsampled_scale)
    if nx < 2 or ny < 2:
        raise ValueError("the downsampled grid needs at least 2 x 2 nodes")
    coarse = np.random.default_rng(seed).choice(heights_range, (nx, ny)).astype(np.float64)
    x, y = np.linspace(0, rows * hscale, nx), np.linspace(0, cols * hscale, ny)
    xu, yu = np.linspace(0, rows * hscale, rows), np.linspace(0, cols * hscale, cols)
    along_x = np.stack([np.interp(xu, x, coarse[:, b]) for b in range(ny)], 1)          # [rows, ny]
    full = np.stack([np.interp(yu, y, along_x[a]) for a in range(rows)], 0)             # [rows, cols]
    return np.rint(full).astype(np.int16)


def spread_origins(n, terrain, margin=1.0):
    """A row-major grid of n origins [n, 2] inside the field, `margin` metres from its border.  The toy's robots do not collide, so thousands of
    them may share one field (4096 environments at Isaac Gym's own spacing would span 256 m, far outside a 50 m field)."""
    (xa, xb), (ya, yb) = terrain.extent
    if not (xb - xa > 2 * margin and yb - ya > 2 * margin):
        raise ValueError("margin leaves no room inside the field")
    side = int(np.ceil(np.sqrt(n)))
    xs, ys = np.linspace(xa + margin, xb - margin, side), np.linspace(ya + margin, yb - margin, side)
    k = np.arange(n)
    return np.stack([xs[k // side], ys[k % side]], 1)
