"""The terrain generators, the reference's presets and the grid of tiles (rl_mpc_locomotion_amd.terrain), numpy only: the integer conversions the
reference's own numbers go through (a rounding int(round(...)) fails them), the shapes, and the layout of TerrainGrid."""
import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import terrain as TR
from rl_mpc_locomotion_amd.terrain import Terrain, TerrainGrid


def blocks(h, sw):
    """The per-step value of a staircase along x: every block of sw rows is constant (asserted); the values of the whole blocks."""
    k = h.shape[0] // sw
    vals = []
    for b in range(k):
        blk = h[b * sw:(b + 1) * sw]
        assert (blk == blk[0, 0]).all(), b
        vals.append(int(blk[0, 0]))
    return vals


def test_python_truncates_the_quotients_as_the_reference_does():
    assert int(0.3 / 0.05) == 5 and round(0.3 / 0.05) == 6                 # the reference's 0.3 m steps are 5 cells wide
    assert int(0.07 / 0.005) == 14 and int(0.75 / 0.25) == 3 and int(-0.35 / 0.005) == -70 and int(-0.5 / 0.005) == -100
    assert int(2.0 / 0.05) == 40 and int(12.0 / 0.25) == 48 and int(1.0 / 0.25) == 4


def test_stairs():
    h = TR.stairs_terrain(40, 56, 0.05, 0.005, 0.3, 0.07)                  # add_terrain("stair")
    assert h.dtype == np.int16 and h.shape == (40, 56)
    vals = blocks(h, 5)
    assert len(vals) == 8 and vals == [14 * (k + 1) for k in range(8)] and np.diff(vals).tolist() == [14] * 7
    h = TR.stairs_terrain(48, 48, 0.25, 0.005, 0.75, -0.35)                # add_uneven_terrains' stairs
    vals = blocks(h, 3)
    assert len(vals) == 16 and vals == [-70 * (k + 1) for k in range(16)]
    h = TR.stairs_terrain(43, 7, 0.05, 0.005, 0.3, 0.07)                   # rows past the last whole step stay 0
    assert blocks(h, 5) == [14 * (k + 1) for k in range(8)] and (h[40:] == 0).all()
    with pytest.raises(ValueError):
        TR.stairs_terrain(40, 40, 0.05, 0.005, 0.01, 0.07)


def test_reference_stairs_slope_and_pyramid():
    s = Terrain.reference_stairs()
    assert (s.rows, s.cols, s.hscale, s.vscale, s.x0, s.y0) == (40, int(2.8 / 0.05), 0.05, 0.005, 2.0, -1.0)
    assert blocks(s.heights, 5) == [14 * (k + 1) - 18 for k in range(8)]   # the mesh's z = -0.09 m is 18 units
    inv = Terrain.reference_stairs(invert=True, x_offset=3.95)             # RL_MPC_Locomotion.py:39
    assert np.array_equal(inv.heights, s.heights[::-1]) and inv.x0 == 3.95 and inv.heights[0, 0] == 8 * 14 - 18
    assert abs(s.max_cell_slope() - 1.4) < 1e-12 and s.max_cell_slope() < 1.5      # a riser is a one-cell ramp below the mesh's slope_threshold
    sl = Terrain.reference_slope()
    slope = 0.07 * (2.0 / 0.3) / 2.0
    assert int(slope * (0.05 / 0.005) * 40) == 93
    assert np.array_equal(sl.heights[:, 0], np.trunc(93 * np.arange(40) / 40).astype(np.int16)) and (sl.heights == sl.heights[:, :1]).all()
    assert sl.heights.max() == 90 and (sl.x0, sl.y0) == (2.0, -1.0) and sl.heights.shape == s.heights.shape
    assert np.array_equal(Terrain.reference_slope(invert=True).heights, sl.heights[::-1])
    py = Terrain.reference_pyramid()
    assert np.array_equal(py.heights, TR.pyramid_stairs_terrain(40, py.cols, 0.05, 0.005, 0.3, 0.07) + 2)      # z = +0.01 m is 2 units
    assert py.heights.min() == 2


def test_sloped_terrain_truncates_toward_zero():
    h = TR.sloped_terrain(48, 5, 0.25, 0.005, -0.5)
    max_h = int(-0.5 * (0.25 / 0.005) * 48)
    assert max_h == -1200 and np.array_equal(h[:, 2], np.trunc(-1200 * np.arange(48) / 48).astype(np.int16))
    h = TR.sloped_terrain(7, 3, 0.1, 0.005, -0.13)                         # quotients that are not whole: toward zero, not floor
    m = int(-0.13 * (0.1 / 0.005) * 7)
    want = [int(m * i / 7) for i in range(7)]
    assert h[:, 0].tolist() == want and want != [int(np.floor(m * i / 7)) for i in range(7)]


def rings_of(h, sw, sh):
    """Ring k (the cells whose distance to the nearest border is in [k sw, (k + 1) sw)) must sit at k sh, up to the top."""
    rows, cols = h.shape
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    depth = np.minimum(np.minimum(i, rows - 1 - i), np.minimum(j, cols - 1 - j)) // sw
    top = int(h[rows // 2, cols // 2]) // sh
    assert np.array_equal(h, np.minimum(depth, top) * sh)
    return top


def test_pyramid_stairs():
    h, rings = TR._pyramid_stairs(40, 56, 0.05, 0.005, 0.3, 0.07, 1.0)     # sw 5, sh 14, p 20: 40 -> 30 -> 20 stops
    assert rings == 2 and rings_of(h, 5, 14) == 2 and h.max() == 28
    assert np.array_equal(h, h[::-1]) and np.array_equal(h, h[:, ::-1])
    h, rings = TR._pyramid_stairs(48, 48, 0.25, 0.005, 0.75, -0.5, 1.0)    # add_uneven_terrains: sw 3, sh -100, p 4
    sides, n = 48, 0
    while sides > 4:
        sides, n = sides - 6, n + 1
    assert rings == n == 8                                                 # 48, 42, .. 6 pass the test; the eighth window is empty
    assert rings_of(h, 3, -100) == 7 and h.min() == -700
    assert np.array_equal(h, h[::-1]) and np.array_equal(h, h[:, ::-1]) and np.array_equal(h, TR.pyramid_stairs_terrain(48, 48, 0.25, 0.005, 0.75, -0.5))
    h, rings = TR._pyramid_stairs(41, 37, 0.1, 0.005, 0.31, 0.1, 1.0)      # odd sides: still rings of width sw
    assert rings_of(h, 3, 20) == rings and rings == 5
    h, rings = TR._pyramid_stairs(20, 20, 0.1, 0.005, 0.3, 0.1, 3.0)       # the field is smaller than the platform: untouched
    assert rings == 0 and not h.any()


def test_pyramid_slope_is_clipped_to_the_platform_value():
    rows = cols = 80
    h = TR.pyramid_sloped_terrain(rows, cols, 0.1, 0.005, 0.4, platform_size=3.0)
    max_h = int(0.4 * (0.1 / 0.005) * 40)
    i = np.arange(rows)
    ramp = (40 - np.abs(40 - i)) / 40
    raw = (max_h * ramp[:, None] * ramp[None, :]).astype(np.int16)
    p = int(3.0 / 0.1 / 2)
    v = int(raw[40 - p, 40 - p])
    assert p == 15 and 0 < v < max_h
    assert np.array_equal(h, np.clip(raw, 0, v)) and h.max() == v and (h[40 - p:40 + p + 1, 40 - p:40 + p + 1] == v).all()
    down = TR.pyramid_sloped_terrain(rows, cols, 0.1, 0.005, -0.4, platform_size=3.0)
    raw_d = (int(-0.4 * (0.1 / 0.005) * 40) * ramp[:, None] * ramp[None, :]).astype(np.int16)
    vd = int(raw_d[40 - p, 40 - p])
    assert vd < 0 and np.array_equal(down, np.clip(raw_d, vd, 0)) and down.min() == vd
    assert not TR.pyramid_sloped_terrain(rows, cols, 0.1, 0.005, 0.0).any()


def test_discrete_obstacles():
    args = dict(max_height=0.15, min_size=1.0, max_size=2.0, num_rects=20, platform_size=3.0)
    h = TR.discrete_obstacles_terrain(80, 80, 0.1, 0.005, seed=4, **args)
    mh = int(0.15 / 0.005)
    assert h.dtype == np.int16 and set(np.unique(h).tolist()) <= {-mh, -mh // 2, 0, mh // 2, mh} and len(np.unique(h)) >= 4
    assert -mh // 2 == -15 and mh // 2 == 15
    assert not h[(80 - 30) // 2:(80 + 30) // 2, (80 - 30) // 2:(80 + 30) // 2].any() and h.any()
    assert np.array_equal(h, TR.discrete_obstacles_terrain(80, 80, 0.1, 0.005, seed=4, **args))
    assert not np.array_equal(h, TR.discrete_obstacles_terrain(80, 80, 0.1, 0.005, seed=5, **args))
    # the draws, in their order: width, length, start_i, start_j, height
    rng = np.random.default_rng(4)
    sizes = list(range(10, 20, 4))
    w, l = int(rng.choice(sizes)), int(rng.choice(sizes))
    i, j = int(rng.choice(range(0, 80 - w, 4))), int(rng.choice(range(0, 80 - l, 4)))
    one = TR.discrete_obstacles_terrain(80, 80, 0.1, 0.005, 0.15, 1.0, 2.0, 1, platform_size=0.0, seed=4)
    want = np.zeros((80, 80), np.int16)
    want[i:i + w, j:j + l] = int(rng.choice([-mh, -mh // 2, mh // 2, mh]))
    assert np.array_equal(one, want)
    with pytest.raises(ValueError):
        TR.discrete_obstacles_terrain(12, 12, 0.1, 0.005, 0.15, 1.0, 2.0, 3)


def test_reference_uneven():
    u = Terrain.reference_uneven(seed=3)
    assert (u.rows, u.cols, u.hscale, u.vscale) == (192, 48, 0.25, 0.005) and (u.x0, u.y0) == (-1.0, -7.0)
    b = [u.heights[k * 48:(k + 1) * 48] for k in range(4)]
    assert np.array_equal(b[0], TR.random_uniform_terrain(48, 48, 0.25, 0.005, -0.1, 0.1, 0.2, 0.5, 3)) and set(np.unique(b[0]).tolist()) - {-20, 20}
    assert np.abs(b[0]).max() <= 20
    assert int(-0.5 * (0.25 / 0.005) * 48) == -1200 and np.array_equal(b[1], TR.sloped_terrain(48, 48, 0.25, 0.005, -0.5))
    assert b[1][0, 0] == 0 and b[1][47, 0] == int(-1200 * 47 / 48)
    stairs = TR.stairs_terrain(48, 48, 0.25, 0.005, 0.75, -0.35)
    assert np.array_equal(b[2], stairs[::-1]) and b[2][0, 0] == -70 * 16 and b[2][47, 0] == -70
    assert np.array_equal(b[3], TR.pyramid_stairs_terrain(48, 48, 0.25, 0.005, 0.75, -0.5)) and b[3].min() == -700
    assert not np.array_equal(u.heights, Terrain.reference_uneven(seed=4).heights)


def flat(value):
    return lambda difficulty, rows, cols, hscale, vscale, seed: np.full((rows, cols), value, np.int16)


def test_terrain_grid_layout():
    seen = []

    def ramp(difficulty, rows, cols, hscale, vscale, seed):                # a tile that is different everywhere
        seen.append((difficulty, rows, cols, seed))
        return (np.arange(rows)[:, None] * 3 + np.arange(cols)[None, :] + int(round(difficulty * 1000)) + 1).astype(np.int16)

    def other(difficulty, rows, cols, hscale, vscale, seed):
        return (-ramp(difficulty, rows, cols, hscale, vscale, seed)).astype(np.int16)

    g = TerrainGrid(num_levels=3, num_types=2, tile_length=4.0, tile_width=3.0, hscale=0.1, vscale=0.005, border_size=2.0, generators=[ramp, other], seed=5)
    t = g.terrain
    assert (t.rows, t.cols) == (3 * 40 + 2 * 20, 2 * 30 + 2 * 20) and (t.x0, t.y0) == (-2.0, -2.0) and g.env_length == 4.0
    assert g.tile_origins.shape == (3, 2, 2) and g.tile_origins.dtype == np.float64 and g.kind == [0, 1]
    H = t.heights
    assert not H[:20].any() and not H[-20:].any() and not H[:, :20].any() and not H[:, -20:].any()          # the border
    assert H[20:-20, 20:-20].all()
    for i in range(3):
        for j in range(2):
            assert g.tile_origins[i, j].tolist() == [(i + 0.5) * 4.0, (j + 0.5) * 3.0]
            tile = (ramp if j == 0 else other)(i / 3, 40, 30, 0.1, 0.005, g.tile_seed(i, j))
            a, c = 20 + i * 40, 20 + j * 30
            assert np.array_equal(H[a:a + 40, c:c + 30], tile)
            # the origin is the tile's centre node, and the surface there is the generator's own centre value
            x, y = g.tile_origins[i, j]
            assert t.cell(x, y)[:2] == (a + 20, c + 15) and abs(t.height(x, y) - 0.005 * int(tile[20, 15])) < 1e-12
    assert {s[0] for s in seen} == {0.0, 1 / 3, 2 / 3} and len({s[3] for s in seen[:6]}) == 6


def test_terrain_grid_defaults_assign_and_limits():
    g = TerrainGrid(num_levels=2, num_types=20, tile_length=8.0, tile_width=8.0, border_size=1.0)
    assert g.kind == [0, 1, 2, 2, 3, 3, 3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 5, 5, 5, 5]          # legged_gym's proportions 0.1, 0.1, 0.35, 0.25, 0.2
    H = g.terrain.heights
    assert not H[10:90, 10:170].any() and H[90:170, 10:90].min() < 0 and H[90:170, 90:170].max() > 0      # smooth slopes: flat at difficulty 0, then down / up
    assert H[10:90, 170:330].any() and H[13, 333] == -10 and H[13, 893] == 10      # roughness; stairs of 0.05 m down and up
    assert H[10:90, 330:890].max() == 0 and H[10:90, 890:1290].min() == 0 and not (H[10:90, 330:1290] % 10).any()
    for n, T in ((10, 4), (64, 20), (7, 3), (4096, 20), (5, 8)):
        gg = TerrainGrid(3, T, 2.0, 2.0, border_size=1.0, generators=[flat(3)])
        lv, ty = gg.assign(n, max_init_level=2, seed=1)
        assert lv.dtype == ty.dtype == np.int32 and np.array_equal(ty, np.floor(np.arange(n) / (n / T)).astype(np.int32))
        assert lv.min() >= 0 and lv.max() <= 2 and ty.max() < T and (np.diff(ty) >= 0).all()
        assert np.array_equal(lv, gg.assign(n, 2, seed=1)[0]) and not gg.assign(n, 0, seed=1)[0].any()
    assert len(np.unique(TerrainGrid(3, 2, 2.0, 2.0, border_size=1.0, generators=[flat(1)]).assign(200, 2, 0)[0])) == 3
    with pytest.raises(ValueError):
        gg.assign(8, max_init_level=3)
    # legged_gym's own field fits the plant's limit; one more row of tiles per axis does not
    assert TR.MAX_NODES == 4096
    rows, cols = 10 * 80 + 2 * 250, 20 * 80 + 2 * 250
    assert (rows, cols) == (1300, 2100)
    big = TerrainGrid(10, 20, 8.0, 8.0, border_size=25.0, generators=[flat(0)])
    assert (big.terrain.rows, big.terrain.cols) == (1300, 2100)
    with pytest.raises(ValueError, match="4096"):
        TerrainGrid(10, 46, 8.0, 8.0, border_size=25.0, generators=[flat(0)])
    with pytest.raises(ValueError, match="4096"):
        TerrainGrid(46, 2, 8.0, 8.0, border_size=25.0, generators=[flat(0)])
    with pytest.raises(ValueError):
        TerrainGrid(2, 2, 2.0, 2.0, generators=[lambda *a: np.zeros((3, 3), np.int16)])
    with pytest.raises(ValueError):
        TerrainGrid(0, 2)
