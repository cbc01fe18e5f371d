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

    # The reference's demo terrains (RL_Environment/sim_utils.py:146-190, ``add_terrain``): 2 m x ``width`` m at 0.05 m cells and 0.005 m units,
    # ``step_height = 0.07``, ``step_width = 0.3``, ``slope = step_height (2 / step_width) / 2``; the mesh transform ``(x_offset, -1)`` is
    # ``(x0, y0)``, ``invert`` reverses the rows (:175-176), and the mesh's z shift (:185-188) is added to the heights as whole units.
    @classmethod
    def _reference_demo(cls, name, x_offset, invert, width):
        hscale, vscale, terrain_width, step_height, step_width = 0.05, 0.005, 2.0, 0.07, 0.3
        rows, cols = int(terrain_width / hscale), int(width / hscale)                            # :153-154
        slope = step_height * (terrain_width / step_width) / terrain_width                       # :159-161
        if name == "slope":
            h, dz = sloped_terrain(rows, cols, hscale, vscale, slope), 0.0
        elif name == "stair":
            h, dz = stairs_terrain(rows, cols, hscale, vscale, step_width, step_height), -0.09
        else:
            h, dz = pyramid_stairs_terrain(rows, cols, hscale, vscale, step_width, step_height), 0.01
        if invert:
            h = h[::-1]
        return cls(h + np.int16(int(round(dz / vscale))), hscale, vscale, x0=x_offset, y0=-1.0)

    @classmethod
    def reference_slope(cls, x_offset=2.0, invert=False, width=2.8):
        """``add_terrain(name="slope")`` (sim_utils.py:146-167, :175-184, :190): ``sloped_terrain`` with slope 0.07 / 0.3, the top 93 units."""
        return cls._reference_demo("slope", x_offset, invert, width)

    @classmethod
    def reference_stairs(cls, invert=False, x_offset=2.0, width=2.8):
        """``add_terrain(name="stair")`` (sim_utils.py:146-169, :175-186, :190): eight steps of 5 rows and 14 units, lowered by 0.09 m (18 units).
        The reference's demo places it at ``x_offset=3.95, invert=True`` (RL_MPC_Locomotion.py:39)."""
        return cls._reference_demo("stair", x_offset, invert, width)

    @classmethod
    def reference_pyramid(cls, x_offset=2.0, invert=False, width=2.8):
        """``add_terrain(name="pyramid")`` (sim_utils.py:146-165, :170-171, :175-184, :187-190): ``pyramid_stairs_terrain``, raised by 0.01 m (2 units)."""
        return cls._reference_demo("pyramid", x_offset, invert, width)

    @classmethod
    def reference_uneven(cls, seed=0):
        """``add_uneven_terrains`` (sim_utils.py:214-240): four 12 m x 12 m tiles at 0.25 m and 0.005 m units stacked along x -- random uniform
        (-0.1 .. 0.1 m, step 0.2, on a 0.5 m grid; :227), slope -0.5 (:228), stairs of 0.75 m x -0.35 m with the rows reversed (:229-230), pyramid
        stairs of 0.75 m x -0.5 m (:231) -- and the mesh transform (-1, -7) as (x0, y0) (:238-239)."""
        hscale, vscale, terrain_width = 0.25, 0.005, 12.0
        rows, cols = int(terrain_width / hscale), int(terrain_width / hscale)
        tiles = [random_uniform_terrain(rows, cols, hscale, vscale, -0.1, 0.1, 0.2, 0.5, seed),
                 sloped_terrain(rows, cols, hscale, vscale, -0.5),
                 stairs_terrain(rows, cols, hscale, vscale, 0.75, -0.35)[::-1],
                 pyramid_stairs_terrain(rows, cols, hscale, vscale, 0.75, -0.5)]
        return cls(np.concatenate(tiles, 0), hscale, vscale, x0=-1.0, y0=-terrain_width / 2 - 1.0)


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


# ---- Isaac Gym's other terrain_utils generators, restated from their published algorithms -------------------------------------------------
# Each returns int16 [rows, cols], row index along x.  ``int()`` is Python's truncation of the float quotient as Python computes it, as in the
# originals: ``int(0.3 / 0.05)`` is 5 (the quotient is 5.999999999999999), so the reference's "0.3 m" steps are 5 cells wide.  As for
# ``random_uniform_terrain``, parity is in construction and nothing is checked against isaacgym.  Not modelled, here or in the plant: the mesh's
# ``slope_threshold`` correction (a stair riser is therefore a one-cell ramp; at the reference's own parameters the steepest cell is
# 0.07 / 0.05 = 1.4 < 1.5, so its meshes are not corrected either), foot-edge collision (the toy's feet touch the surface from above only), and
# ``stepping_stones_terrain`` / ``wave_terrain``.
def sloped_terrain(rows, cols, hscale, vscale, slope):
    """``terrain_utils.sloped_terrain``: row i at ``int16(max_h i / rows)`` with ``max_h = int(slope (hscale / vscale) rows)``; the int16
    conversion truncates toward zero."""
    max_h = int(slope * (hscale / vscale) * rows)
    col = (max_h * np.arange(rows).reshape(rows, 1) / rows).astype(np.int16)
    return np.ascontiguousarray(np.broadcast_to(col, (rows, cols)))


def pyramid_sloped_terrain(rows, cols, hscale, vscale, slope, platform_size=1.0):
    """``terrain_utils.pyramid_sloped_terrain``: ``int16(max_h xx yy)`` with the two ramps ``(c - |c - i|) / c`` about ``c = int(rows / 2)``,
    ``int(cols / 2)`` and ``max_h = int(slope (hscale / vscale) (rows / 2))``, clipped to the value at the platform's corner."""
    cx, cy = int(rows / 2), int(cols / 2)
    xx = ((cx - np.abs(cx - np.arange(rows))) / cx).reshape(rows, 1)
    yy = ((cy - np.abs(cy - np.arange(cols))) / cy).reshape(1, cols)
    max_h = int(slope * (hscale / vscale) * (rows / 2))
    h = (max_h * xx * yy).astype(np.int16)
    p = int(platform_size / hscale / 2)
    v = int(h[rows // 2 - p, cols // 2 - p])
    return np.clip(h, min(v, 0), max(v, 0)).astype(np.int16)


def stairs_terrain(rows, cols, hscale, vscale, step_width, step_height):
    """``terrain_utils.stairs_terrain``: steps of ``sw = int(step_width / hscale)`` rows, step k at ``(k + 1) int(step_height / vscale)``; the rows
    past the last whole step stay 0."""
    sw, sh = int(step_width / hscale), int(step_height / vscale)
    if sw < 1:
        raise ValueError("step_width must be at least one cell")
    h = np.zeros((rows, cols), np.int16)
    for k in range(rows // sw):
        h[k * sw:(k + 1) * sw, :] = (k + 1) * sh
    return h


def pyramid_stairs_terrain(rows, cols, hscale, vscale, step_width, step_height, platform_size=1.0):
    """``terrain_utils.pyramid_stairs_terrain``: while both sides of the window are longer than ``int(platform_size / hscale)`` the window shrinks
    by ``sw`` on every side, the height grows by ``sh`` and is written into the window (the last window may be empty)."""
    return _pyramid_stairs(rows, cols, hscale, vscale, step_width, step_height, platform_size)[0]


def _pyramid_stairs(rows, cols, hscale, vscale, step_width, step_height, platform_size):
    """(field, rings): the loop of pyramid_stairs_terrain and how many times it ran."""
    sw, sh, p = int(step_width / hscale), int(step_height / vscale), int(platform_size / hscale)
    if sw < 1:
        raise ValueError("step_width must be at least one cell")
    h = np.zeros((rows, cols), np.int16)
    height, a, b, c, d, rings = 0, 0, rows, 0, cols, 0
    while (b - a) > p and (d - c) > p:
        a, b, c, d = a + sw, b - sw, c + sw, d - sw
        height += sh
        rings += 1
        if b > a and d > c:              # (Python's slice of a crossed window is empty; written out so that negative indices never wrap)
            h[a:b, c:d] = height
    return h, rings


def discrete_obstacles_terrain(rows, cols, hscale, vscale, max_height, min_size, max_size, num_rects, platform_size=1.0, seed=0):
    """``terrain_utils.discrete_obstacles_terrain``: ``num_rects`` rectangles with sides from ``range(int(min_size / hscale), int(max_size / hscale), 4)``,
    corners from ``range(0, rows - w, 4)`` x ``range(0, cols - l, 4)`` and heights from ``[-mh, -mh // 2, mh // 2, mh]``, ``mh = int(max_height / vscale)``;
    the central platform is set to 0 last.  The draws come from ``numpy.random.default_rng(seed)``, per rectangle: width, length, start_i, start_j, height."""
    mh, lo, hi, p = int(max_height / vscale), int(min_size / hscale), int(max_size / hscale), int(platform_size / hscale)
    heights, sizes = [-mh, -mh // 2, mh // 2, mh], list(range(lo, hi, 4))
    if not sizes or rows - max(sizes) < 1 or cols - max(sizes) < 1:
        raise ValueError("no rectangle size fits: need min_size < max_size in cells and a field larger than the largest rectangle")
    rng = np.random.default_rng(seed)
    h = np.zeros((rows, cols), np.int16)
    for _ in range(num_rects):
        w, l = int(rng.choice(sizes)), int(rng.choice(sizes))
        i, j = int(rng.choice(range(0, rows - w, 4))), int(rng.choice(range(0, cols - l, 4)))
        h[i:i + w, j:j + l] = int(rng.choice(heights))
    h[max((rows - p) // 2, 0):(rows + p) // 2, max((cols - p) // 2, 0):(cols + p) // 2] = 0
    return h


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


# ---- a grid of tiles ordered by difficulty ---------------------------------------------------------------------------------------------
MAX_NODES = 4096                       # MPC_TERRAIN_MAX_NODES of include/mpc_terrain.h, per axis


def _smooth_slope(sign):
    return lambda difficulty, rows, cols, hscale, vscale, seed: pyramid_sloped_terrain(rows, cols, hscale, vscale, sign * difficulty * 0.4, platform_size=3.0)


def _rough_slope(difficulty, rows, cols, hscale, vscale, seed):
    base = pyramid_sloped_terrain(rows, cols, hscale, vscale, difficulty * 0.4, platform_size=3.0).astype(np.int64)
    return (base + random_uniform_terrain(rows, cols, hscale, vscale, -0.05, 0.05, 0.005, 0.2, seed)).astype(np.int16)


def _stairs(sign):
    return lambda difficulty, rows, cols, hscale, vscale, seed: pyramid_stairs_terrain(rows, cols, hscale, vscale, 0.31, sign * (0.05 + 0.18 * difficulty),
                                                                                      platform_size=3.0)


def _discrete(difficulty, rows, cols, hscale, vscale, seed):
    return discrete_obstacles_terrain(rows, cols, hscale, vscale, 0.05 + difficulty * 0.2, 1.0, 2.0, 20, platform_size=3.0, seed=seed)


def legged_gym_generators():
    """(generators, proportions): legged_gym's five kinds of ``make_terrain`` with its default ``terrain_proportions`` (0.1, 0.1, 0.35, 0.25, 0.2)
    -- smooth pyramid slope (``difficulty 0.4``; downwards on the first half of its share, hence six entries), the same slope with +-0.05 m of
    random uniform roughness, pyramid stairs of 0.31 m x ``0.05 + 0.18 difficulty`` downwards and upwards, discrete obstacles of
    ``0.05 + 0.2 difficulty`` -- restated from its published parameters; stepping stones and gaps (proportion 0 there) are not built."""
    return [_smooth_slope(-1.0), _smooth_slope(1.0), _rough_slope, _stairs(-1.0), _stairs(1.0), _discrete], (0.05, 0.05, 0.1, 0.35, 0.25, 0.2)


class TerrainGrid:
    """legged_gym's ``Terrain`` (its curriculum layout) restated from its published layout: ``num_levels x num_types`` tiles of ``tile_length`` (x) by
    ``tile_width`` (y) metres inside a flat border of ``border_size`` metres, in one int16 field.  Level (row of tiles) i runs along x and has
    ``difficulty = i / num_levels``; type column j takes the generator whose cumulative share of ``proportions`` first exceeds ``j / num_types + 0.001``.
    ``generators``: callables ``(difficulty, rows, cols, hscale, vscale, seed) -> int16 [rows, cols]`` (default: ``legged_gym_generators()``; without
    ``proportions`` the list is shared out evenly over the columns).  Each tile's seed is ``seed 1000003 + level num_types + type``.

    ``terrain`` is the ``Terrain`` (node (0, 0) at ``(-border_size, -border_size)``, so tile (i, j) spans ``[i L, (i + 1) L) x [j W, (j + 1) W)`` as in
    legged_gym); ``tile_origins`` [levels, types, 2] float64 the tile centres ``((i + 0.5) L, (j + 0.5) W)`` in that frame; ``env_length = tile_length``.
    legged_gym's 10 x 20 tiles of 8 m at 0.1 m with a 25 m border are 1300 x 2100 nodes; a field beyond ``MAX_NODES`` per axis is a ``ValueError``.
    What the generators' text says is not modelled holds here too (no slope correction, no foot-edge collision)."""

    def __init__(self, num_levels=10, num_types=20, tile_length=8.0, tile_width=8.0, hscale=0.1, vscale=0.005, border_size=25.0, generators=None,
                 proportions=None, seed=0):
        self.num_levels, self.num_types = int(num_levels), int(num_types)
        if self.num_levels < 1 or self.num_types < 1:
            raise ValueError("num_levels and num_types must be at least 1")
        self.tile_length, self.tile_width, self.border_size = float(tile_length), float(tile_width), float(border_size)
        self.hscale, self.vscale, self.seed = float(hscale), float(vscale), int(seed)
        self.env_length, self.env_width = self.tile_length, self.tile_width
        if generators is None:
            if proportions is not None:
                raise ValueError("proportions come with the generators they share out")
            generators, proportions = legged_gym_generators()
        generators = list(generators)
        if not generators or not all(callable(g) for g in generators):
            raise ValueError("generators: a non-empty list of callables (difficulty, rows, cols, hscale, vscale, seed) -> int16 [rows, cols]")
        if proportions is None:
            proportions = [1.0 / len(generators)] * len(generators)
        if len(proportions) != len(generators):
            raise ValueError("one proportion per generator")
        cumulative = [float(np.sum(proportions[:k + 1])) for k in range(len(proportions))]
        self.tile_rows, self.tile_cols, self.border = int(self.tile_length / self.hscale), int(self.tile_width / self.hscale), int(self.border_size / self.hscale)
        rows, cols = self.num_levels * self.tile_rows + 2 * self.border, self.num_types * self.tile_cols + 2 * self.border
        if self.tile_rows < 2 or self.tile_cols < 2:
            raise ValueError("a tile needs at least 2 x 2 cells")
        if rows > MAX_NODES or cols > MAX_NODES:
            raise ValueError(f"the field would be {rows} x {cols} nodes; the plant takes at most {MAX_NODES} per axis (MPC_TERRAIN_MAX_NODES)")
        self.kind = []                     # per type column: the index of its generator
        for j in range(self.num_types):
            choice = j / self.num_types + 0.001
            self.kind.append(next((k for k, c in enumerate(cumulative) if choice < c), len(generators) - 1))
        field = np.zeros((rows, cols), np.int16)
        self.tile_origins = np.zeros((self.num_levels, self.num_types, 2), np.float64)
        for j in range(self.num_types):
            for i in range(self.num_levels):
                tile = np.asarray(generators[self.kind[j]](i / self.num_levels, self.tile_rows, self.tile_cols, self.hscale, self.vscale, self.tile_seed(i, j)))
                if tile.shape != (self.tile_rows, self.tile_cols) or tile.dtype != np.int16:
                    raise ValueError(f"the generator of type {j} must return int16 [{self.tile_rows}, {self.tile_cols}]")
                a, c = self.border + i * self.tile_rows, self.border + j * self.tile_cols
                field[a:a + self.tile_rows, c:c + self.tile_cols] = tile
                self.tile_origins[i, j] = ((i + 0.5) * self.tile_length, (j + 0.5) * self.tile_width)
        self.terrain = Terrain(field, self.hscale, self.vscale, x0=-self.border * self.hscale, y0=-self.border * self.hscale)

    def tile_seed(self, level, type_):
        return self.seed * 1000003 + level * self.num_types + type_

    def assign(self, n, max_init_level=0, seed=0):
        """(levels0 [n] int32, types [n] int32) as legged_gym's ``_get_env_origins`` hands them out: ``types = floor(arange(n) / (n / num_types))``, ``levels0``
        uniform in ``0 .. max_init_level`` (from ``numpy.random.default_rng(seed)``)."""
        n, max_init_level = int(n), int(max_init_level)
        if n < 1 or not 0 <= max_init_level < self.num_levels:
            raise ValueError("n >= 1 and 0 <= max_init_level < num_levels")
        types = np.minimum(np.floor(np.arange(n) / (n / self.num_types)), self.num_types - 1).astype(np.int32)
        levels0 = np.random.default_rng(seed).integers(0, max_init_level + 1, n).astype(np.int32)
        return levels0, types
