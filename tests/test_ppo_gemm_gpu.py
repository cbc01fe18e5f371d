"""csrc/ppo_gemm.h's kernels on the MI355X, one instantiation at a time, against the same product in float64 on the CPU, element by element.

tests/device/ppo_gemm_harness.hip is compiled once per run with hipcc and loaded through ctypes; the test fills the pgemm::Launch and names the
kind and the tile (narrow = gemm_kernel<KIND, 2, 1>, wide = gemm_kernel<KIND, 2, 2>) itself, so the launch plan (csrc/ppo_gemm_plan.h) is not involved
and the 128 x 128 tile and the 512- and 1024-row chunks run at shapes far below those at which the plan picks them.  The axis sets stand at the two
shape tables; they include what the 240-column observation rows of training with a height scan add: K = 240 through the row index, N = 240, and a
weight gradient of nin = 240 with ldb = 240 in 1024- and in 256-row chunks.

The tolerance is derived, not measured.  A float32 sum of n products, in any order and fused or not, lies within gamma_n * sum |a_k b_k| of the exact
sum, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  Hence, per element,
  forward          gamma_{K+1} (sum |x w| + |bias|)                       (the bias is one more term)
  backward data    gamma_{K+2} sum |dy w| |f|, f = 1 for y > 0, y + 1 otherwise     (one rounding for y + 1, one for the product with it)
  backward weight  gamma_len sum |dy x| per chunk partial, len the chunk's own row count; its dbias partial gamma_len sum |dy|
  reduced dW, db   the sum of the chunks' bounds plus one ulp (the float64 chunk sum is rounded once), and bit for bit the float32 rounding of the
                   float64 sum of the kernel's own partials in chunk order
The inputs make the bound bite: magnitudes are drawn from +-[0.5, 2] times one scale per operand, and every case asserts of its own inputs that each
single product (and the bias) is at least 3 x the bound of the element it belongs to, so a dropped, doubled or misplaced term cannot pass.  Every
operand has NaN in its padding columns and in rows past its end; the outputs are pre-filled with a sentinel that must survive, bit for bit, everywhere
outside the M x N region.  Largest measured error / bound per kind and tile: DESIGN.md section 8.3."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, U, draw as _draw, gamma, ulp32  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "device", "ppo_gemm_harness.hip")
HIPCC = "/opt/rocm/bin/hipcc"

FORWARD, BACKWARD_DATA, BACKWARD_WEIGHT = 0, 1, 2                 # pgemm::Kind
KIND_NAMES = ("forward", "backward data", "backward weight")
TILES = {"narrow": 0, "wide": 1}                                  # gemm_kernel<KIND, 2, 1>, gemm_kernel<KIND, 2, 2>
SENTINEL = 0x7FA5C3E1                                             # a NaN with a payload: no kernel result has these bits

# Two problems per launch, so one problem's workgroups leave early; the second slot of one case is empty (tiles_m = 0).  pad: the leading
# dimensions are round4(width) + 4 instead of round4(width).  idx (forward): the rows of X are read through an int64 index.
# Forward and backward data, (M, N, K).  Over the cases: M in {1, 31, 33, 127, 128, 129, 257}, N in {1, 12, 16, 63, 65, 127, 128, 129, 144, 240},
# K in {1, 2, 3, 4, 5, 16, 31, 32, 33, 48, 63, 65, 100, 240}, each with every kind and tile (tests/test_ppo_gemm_plan.py checks that of this table).
FB_CASES = (
    dict(shapes=((1, 12, 1), (257, 144, 100)), pad=False, idx=(True, False)),
    dict(shapes=((31, 1, 2), (129, 129, 65)), pad=True, idx=(False, True)),
    dict(shapes=((33, 16, 3), (128, 128, 63)), pad=False, idx=(False, False)),
    dict(shapes=((127, 63, 4), (31, 65, 48)), pad=True, idx=(True, True)),
    dict(shapes=((128, 127, 5), (33, 12, 33)), pad=False, idx=(False, False)),
    dict(shapes=((129, 16, 31), (1, 144, 32)), pad=True, idx=(False, True)),
    dict(shapes=((129, 65, 33), None), pad=True, idx=(True, False)),
    # the wide observation rows (240 columns with the default height scan): the first layer's reduction, 7 1/2 trips of 32 through the index with
    # lda = 240 as the update passes it, and 240 output columns (the narrow tile's fourth column tile holds 48, the wide tile's second 112)
    dict(shapes=((129, 65, 240), (33, 128, 16)), pad=False, idx=(True, False)),
    dict(shapes=((257, 240, 48), (31, 12, 240)), pad=True, idx=(False, True)),
)
# Backward weight, (nout, nin, rows, chunk_rows).  nout in {1, 12, 16, 127, 129}, nin in {16, 48, 65, 128, 144, 240}, rows in {1, 31, 33, 255, 256, 257, 1023,
# 1025, 2049} and 512, 1024; every chunk length with a row count that leaves a last chunk of one row (257 / 256, 1025 / 512, 2049 / 1024) and with one
# that fills the last chunk (256 / 256, 512 / 512, 1024 / 1024).  idx: the rows of X are read through the index.  db: the dbias partials are asked for.
BW_CASES = (
    dict(shapes=((1, 16, 1, 256), (129, 144, 2049, 1024)), pad=False, idx=(False, False), db=(True, True)),
    dict(shapes=((12, 48, 31, 256), (127, 128, 1025, 512)), pad=True, idx=(True, True), db=(True, True)),
    dict(shapes=((16, 65, 33, 512), (129, 16, 257, 256)), pad=False, idx=(False, False), db=(True, False)),
    dict(shapes=((127, 128, 255, 256), (12, 65, 256, 256)), pad=True, idx=(False, True), db=(True, True)),
    dict(shapes=((129, 144, 1023, 1024), (16, 48, 1024, 1024)), pad=False, idx=(True, False), db=(True, True)),
    dict(shapes=((1, 128, 512, 512), (127, 16, 1024, 512)), pad=True, idx=(False, False), db=(True, True)),
    dict(shapes=((12, 144, 2049, 256), None), pad=True, idx=(True, False), db=(True, True)),
    # the first layer's weight gradient on the wide rows: nin = 240 read through the index with ldb = 240 (pad=False) in 1024-row chunks, the last of
    # one row, as mpc_ppo_update_grads plans it from 15 361 rows on; and nin = 240 in 256-row chunks, as it plans it below that
    dict(shapes=((129, 240, 2049, 1024), (12, 16, 33, 256)), pad=False, idx=(True, False), db=(True, True)),
    dict(shapes=((127, 240, 1025, 256), (1, 48, 31, 512)), pad=True, idx=(False, True), db=(True, True)),
)

WORST = {}                                                        # (kind, tile) -> largest error / bound seen, printed as evidence


class Problem(C.Structure):                                       # pgemm::Problem, field for field
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("aux", C.c_void_p), ("idx", C.c_void_p), ("dbias", C.c_void_p),
                ("idx_limit", C.c_longlong), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("lda", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int),
                ("ldaux", C.c_int), ("elu", C.c_int), ("tiles_m", C.c_int), ("tiles_n", C.c_int), ("chunks", C.c_int), ("chunk_rows", C.c_int)]


class Launch(C.Structure):
    _fields_ = [("p", Problem * 2)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    d = tmp_path_factory.mktemp("ppo_gemm_harness")
    so = d / "ppo_gemm_harness.so"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, HARNESS, "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.ppo_gemm_harness_sizeof_launch.restype = C.c_int
    L.ppo_gemm_harness_launch.argtypes = [C.POINTER(Launch), C.c_int, C.c_int, C.c_void_p]; L.ppo_gemm_harness_launch.restype = C.c_int
    L.ppo_gemm_harness_reduce.argtypes = [C.c_int] + [C.c_void_p] * 5; L.ppo_gemm_harness_reduce.restype = C.c_int
    assert L.ppo_gemm_harness_sizeof_launch() == C.sizeof(Launch)
    return L


# ------------------------------------------------------------------ inputs and float64 references (host only; shared by the two tiles)

def _index(rng, rows, limit):
    """An int64 row index with repeats, unsorted, with values below 0 and at or above limit (the kernel clamps to [0, limit))."""
    idx = rng.integers(-2, limit + 2, rows).astype(np.int64)
    if rows >= 4:
        idx[0], idx[1], idx[2] = limit + 7, -5, idx[3]
        assert (np.diff(idx) < 0).any() and (np.diff(idx) > 0).any()
    elif rows == 1:
        idx[0] = limit + 7
    return idx


def _ld(width, pad):
    return (width + 3) // 4 * 4 + (4 if pad else 0)


def _terms_bite(min_term, bound, what):
    """The case's own inputs: every single term at least 3 x the bound of its element, and none subnormal."""
    live = bound > 0
    assert (min_term[live] >= 3.0 * bound[live]).all(), f"{what}: a term of {min_term[live].min():.3e} under 3 x its bound, ratio {(min_term[live] / bound[live]).min():.2f}"
    assert min_term.min() >= 2.0 ** -126, what


@functools.lru_cache(maxsize=None)
def forward_case(i):
    case, out = FB_CASES[i], []
    for slot, shape in enumerate(case["shapes"]):
        if shape is None:
            out.append(None)
            continue
        M, N, K = shape
        rng = np.random.default_rng(1000 + 10 * i + slot)
        limit = M + 5 if case["idx"][slot] else M
        X, W, b = _draw(rng, (limit, K), 1.3), _draw(rng, (N, K), 10.0 / np.sqrt(K) / 1.3), _draw(rng, (N,), 4.0)
        idx = _index(rng, M, limit) if case["idx"][slot] else None
        Xr = X if idx is None else X[np.clip(idx, 0, limit - 1)]
        Xd, Wd, bd = Xr.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
        exact = Xd @ Wd.T + bd
        bound = gamma(K + 1) * (np.abs(Xd) @ np.abs(Wd).T + np.abs(bd))
        min_term = np.minimum(np.outer(np.abs(Xd).min(1), np.abs(Wd).min(1)), np.abs(bd)[None, :])      # (a lower bound of the smallest term)
        _terms_bite(min_term, bound, f"forward case {i} slot {slot}")
        assert (exact > 0).any() and (exact <= 0).any(), f"forward case {i} slot {slot}: one ELU branch only"
        out.append(dict(M=M, N=N, K=K, limit=limit, X=X, W=W, b=b, idx=idx, exact=exact, bound=bound))
    assert any(o is not None and (o["exact"] < -17.5).any() for o in out), f"forward case {i}: no pre-activation below -17"
    return out


@functools.lru_cache(maxsize=None)
def backward_data_case(i):
    case, out = FB_CASES[i], []
    for slot, shape in enumerate(case["shapes"]):
        if shape is None:
            out.append(None)
            continue
        M, N, K = shape
        rng = np.random.default_rng(2000 + 10 * i + slot)
        dY, W = _draw(rng, (M, K), 0.37), _draw(rng, (K, N), 1.9)
        y = np.where(rng.random((M, N)) < 0.5, np.abs(_draw(rng, (M, N), 1.0)), -rng.uniform(0.02, 0.98, (M, N)).astype(np.float32)).astype(np.float32)
        planted = np.array([0.0, -1.0, 1e-30, -1e-30, -0.0, np.nextafter(np.float32(-1.0), np.float32(0.0))], np.float32)
        flat = y.reshape(-1)
        pos = rng.permutation(flat.size)[:planted.size]
        flat[pos] = planted[:pos.size]                                               # exactly 0 and -1, just above and just below 0, just above -1
        yd = y.astype(np.float64)
        f = np.where(yd > 0, 1.0, yd + 1.0)
        dYd, Wd = dY.astype(np.float64), W.astype(np.float64)
        s, sabs = dYd @ Wd, np.abs(dYd) @ np.abs(Wd)
        _terms_bite(np.outer(np.abs(dYd).min(1), np.abs(Wd).min(0)), gamma(K + 2) * sabs, f"backward data case {i} slot {slot}")
        out.append(dict(M=M, N=N, K=K, dY=dY, W=W, y=y, exact=s * f, bound=gamma(K + 2) * sabs * np.abs(f)))
    assert sum(int((o["y"] == -1).sum()) for o in out if o) >= 1 and sum(int((o["y"] == 0).sum()) for o in out if o) >= 2
    return out


@functools.lru_cache(maxsize=None)
def backward_weight_case(i):
    case, out = BW_CASES[i], []
    for slot, shape in enumerate(case["shapes"]):
        if shape is None:
            out.append(None)
            continue
        nout, nin, rows, chunk_rows = shape
        rng = np.random.default_rng(3000 + 10 * i + slot)
        limit = rows + 5 if case["idx"][slot] else rows
        dY, X = _draw(rng, (rows, nout), 0.37), _draw(rng, (limit, nin), 1.6)
        idx = _index(rng, rows, limit) if case["idx"][slot] else None
        Xr = X if idx is None else X[np.clip(idx, 0, limit - 1)]
        dYd, Xd = dY.astype(np.float64), Xr.astype(np.float64)
        chunks = -(-rows // chunk_rows)
        exact, bound, db_exact, db_bound = (np.zeros(s) for s in ((chunks, nout, nin), (chunks, nout, nin), (chunks, nout), (chunks, nout)))
        for c in range(chunks):
            a, x = dYd[c * chunk_rows:(c + 1) * chunk_rows], Xd[c * chunk_rows:(c + 1) * chunk_rows]
            n = a.shape[0]                                                            # the chunk's actual row count
            exact[c], bound[c] = a.T @ x, gamma(n) * (np.abs(a).T @ np.abs(x))
            db_exact[c], db_bound[c] = a.sum(0), gamma(n) * np.abs(a).sum(0)
            _terms_bite(np.outer(np.abs(a).min(0), np.abs(x).min(0)), bound[c], f"backward weight case {i} slot {slot} chunk {c}")
            _terms_bite(np.abs(a).min(0), db_bound[c], f"backward weight case {i} slot {slot} chunk {c} dbias")
        assert chunks == 1 or rows - (chunks - 1) * chunk_rows in (1, chunk_rows)
        out.append(dict(M=nout, N=nin, K=rows, limit=limit, chunk_rows=chunk_rows, chunks=chunks, dY=dY, X=X, idx=idx, exact=exact, bound=bound,
                        db_exact=db_exact, db_bound=db_bound, total=dYd.T @ Xd, db_total=dYd.sum(0)))
    return out


# ------------------------------------------------------------------ device buffers

def _poisoned(a, ld, extra_rows=2):
    """a [rows][width] on the device inside [rows + extra_rows][ld] of NaN."""
    a = np.atleast_2d(a)
    buf = np.full((a.shape[0] + extra_rows, ld), np.nan, np.float32)
    buf[:a.shape[0], :a.shape[1]] = a
    return torch.from_numpy(buf).to(DEV)


def _sentinel(*shape):
    t = torch.empty(shape, dtype=torch.float32, device=DEV)
    t.view(torch.int32).fill_(SENTINEL)
    return t


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _untouched(t, region, what):
    """Every word of t outside region (a boolean mask) is still the sentinel, bit for bit; nothing inside it is."""
    bits = _bits(t)
    assert (bits[~region] == SENTINEL).all(), f"{what}: {int((bits[~region] != SENTINEL).sum())} words outside the result were written"
    assert (bits[region] != SENTINEL).all(), f"{what}: {int((bits[region] == SENTINEL).sum())} words of the result were never written"


def _region(shape, *extent):
    m = np.zeros(shape, bool)
    m[tuple(slice(0, e) for e in extent)] = True
    return m


def _within(got, exact, bound, key, what):
    """Every element against its own bound; where the bound is 0 the result is exactly (+-) 0."""
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), f"{what}: a NaN or an infinity reached the result"
    err = np.abs(got - exact)
    zero = bound == 0
    assert (got[zero] == 0).all(), what
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{what}: largest error / bound {ratio:.3f}; {KIND_NAMES[key[0]]} {key[1]} so far {WORST[key]:.3f}")
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside their bound, first at {tuple(np.argwhere(bad)[0])}, worst ratio {ratio:.3f}"


def _tiles(p, M, N, tile):
    p.tiles_m, p.tiles_n = (M + 127) // 128, (N + (128 if TILES[tile] else 64) - 1) // (128 if TILES[tile] else 64)


def _run(harness, launch, kind, tile):
    rc = harness.ppo_gemm_harness_launch(C.byref(launch), kind, TILES[tile], None)
    assert rc == 0, f"the harness refused or failed the launch: {rc}"


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("case", range(len(FB_CASES)))
@pytest.mark.parametrize("tile", sorted(TILES))
def test_forward_matches_float64(harness, tile, case):
    spec, probs = FB_CASES[case], forward_case(case)
    outs = {}
    for elu in (0, 1):
        launch, keep = Launch(), []
        for slot, o in enumerate(probs):
            if o is None:
                continue
            M, N, K = o["M"], o["N"], o["K"]
            lda, ldb, ldc = _ld(K, spec["pad"]), _ld(K, spec["pad"]), _ld(N, spec["pad"])
            A, B, bias, Cbuf = _poisoned(o["X"], lda), _poisoned(o["W"], ldb), _poisoned(o["b"][None, :], _ld(N, True), 0), _sentinel(M + 2, ldc)
            idx = torch.from_numpy(o["idx"]).to(DEV) if o["idx"] is not None else None
            p = launch.p[slot]
            p.A, p.B, p.C, p.aux, p.idx, p.idx_limit = A.data_ptr(), B.data_ptr(), Cbuf.data_ptr(), bias.data_ptr(), idx.data_ptr() if idx is not None else None, o["limit"]
            p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.elu, p.chunks = M, N, K, lda, ldb, ldc, elu, 1
            _tiles(p, M, N, tile)
            keep.append((slot, Cbuf, (A, B, bias, idx)))
        _run(harness, launch, FORWARD, tile)
        torch.cuda.synchronize()
        for slot, Cbuf, _ in keep:
            o = probs[slot]
            _untouched(Cbuf, _region(tuple(Cbuf.shape), o["M"], o["N"]), f"forward {tile} case {case} slot {slot} elu {elu}")
            outs[(slot, elu)] = Cbuf.cpu().numpy()[:o["M"], :o["N"]]
    for slot, o in enumerate(probs):
        if o is None:
            continue
        what = f"forward {tile} case {case} slot {slot} {(o['M'], o['N'], o['K'])}"
        v, y = outs[(slot, 0)], outs[(slot, 1)]
        _within(v, o["exact"], o["bound"], (FORWARD, tile), what)
        # ELU on the kernel's own pre-activation: the identity bit for bit above 0, expm1 within 2 float32 ulp elsewhere (ROCm documents expm1f at
        # 1 ulp; one more for the rounding of the comparison value)
        pos = v > 0
        assert pos.any() and (~pos).any(), what
        assert (y[pos].view(np.int32) == v[pos].view(np.int32)).all(), f"{what}: ELU changed a positive pre-activation"
        want = np.expm1(v[~pos].astype(np.float64))
        off = np.abs(y[~pos].astype(np.float64) - want) / ulp32(want)
        print(f"{what}: ELU off by at most {off.max():.3f} ulp over {int((~pos).sum())} elements, {int((v < -17.5).sum())} of them below -17.5")
        assert (off <= 2.0).all(), f"{what}: ELU off by {off.max():.3f} ulp"


@pytest.mark.parametrize("case", range(len(FB_CASES)))
@pytest.mark.parametrize("tile", sorted(TILES))
def test_backward_data_matches_float64(harness, tile, case):
    spec, probs = FB_CASES[case], backward_data_case(case)
    launch, keep = Launch(), []
    for slot, o in enumerate(probs):
        if o is None:
            continue
        M, N, K = o["M"], o["N"], o["K"]
        lda, ldb, ldc, ldaux = _ld(K, spec["pad"]), _ld(N, spec["pad"]), _ld(N, spec["pad"]), _ld(N, not spec["pad"])
        A, B, aux, Cbuf = _poisoned(o["dY"], lda), _poisoned(o["W"], ldb), _poisoned(o["y"], ldaux), _sentinel(M + 2, ldc)
        p = launch.p[slot]
        p.A, p.B, p.C, p.aux = A.data_ptr(), B.data_ptr(), Cbuf.data_ptr(), aux.data_ptr()
        p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.ldaux, p.chunks = M, N, K, lda, ldb, ldc, ldaux, 1
        _tiles(p, M, N, tile)
        keep.append((slot, Cbuf, (A, B, aux)))
    _run(harness, launch, BACKWARD_DATA, tile)
    torch.cuda.synchronize()
    for slot, Cbuf, _ in keep:
        o = probs[slot]
        what = f"backward data {tile} case {case} slot {slot} {(o['M'], o['N'], o['K'])}"
        _untouched(Cbuf, _region(tuple(Cbuf.shape), o["M"], o["N"]), what)
        got = Cbuf.cpu().numpy()[:o["M"], :o["N"]]
        _within(got, o["exact"], o["bound"], (BACKWARD_DATA, tile), what)
        assert (got[o["y"] == -1] == 0).all(), what                                 # a factor of exactly 0


@pytest.mark.parametrize("case", range(len(BW_CASES)))
@pytest.mark.parametrize("tile", sorted(TILES))
def test_backward_weight_and_the_chunk_sum_match_float64(harness, tile, case):
    spec, probs = BW_CASES[case], backward_weight_case(case)
    launch, keep = Launch(), []
    for slot, o in enumerate(probs):
        if o is None:
            continue
        M, N, K, chunks = o["M"], o["N"], o["K"], o["chunks"]
        lda, ldb, ldc = _ld(M, spec["pad"]), _ld(N, spec["pad"]), _ld(N, spec["pad"])
        A, B = _poisoned(o["dY"], lda), _poisoned(o["X"], ldb)
        Cbuf, db = _sentinel(chunks + 1, M, ldc), _sentinel(chunks + 1, M) if spec["db"][slot] else None
        idx = torch.from_numpy(o["idx"]).to(DEV) if o["idx"] is not None else None
        p = launch.p[slot]
        p.A, p.B, p.C, p.idx, p.idx_limit, p.dbias = A.data_ptr(), B.data_ptr(), Cbuf.data_ptr(), idx.data_ptr() if idx is not None else None, o["limit"], db.data_ptr() if db is not None else None
        p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.chunks, p.chunk_rows = M, N, K, lda, ldb, ldc, chunks, o["chunk_rows"]
        _tiles(p, M, N, tile)
        keep.append((slot, Cbuf, db, ldc, (A, B, idx)))
    _run(harness, launch, BACKWARD_WEIGHT, tile)
    # the chunk sum on the kernel's own partials, on the same stream
    parts, outs, numel, nchunks = [], [], [], []
    for slot, Cbuf, db, ldc, _ in keep:
        o = probs[slot]
        parts.append(Cbuf); outs.append(_sentinel(o["M"] * ldc + 8)); numel.append(o["M"] * ldc); nchunks.append(o["chunks"])
        if db is not None:
            parts.append(db); outs.append(_sentinel(o["M"] + 8)); numel.append(o["M"]); nchunks.append(o["chunks"])
    n = len(parts)
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    ints = lambda v: (C.c_int * n)(*v)
    rc = harness.ppo_gemm_harness_reduce(n, ptrs(parts), ptrs(outs), ints(numel), ints(nchunks), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    reduced = dict(zip([id(t) for t in parts], outs))
    key = (BACKWARD_WEIGHT, tile)
    for slot, Cbuf, db, ldc, _ in keep:
        o = probs[slot]
        M, N, chunks = o["M"], o["N"], o["chunks"]
        what = f"backward weight {tile} case {case} slot {slot} {(M, N, o['K'])} in {chunks} chunks of {o['chunk_rows']}"
        _untouched(Cbuf, _region(tuple(Cbuf.shape), chunks, M, N), what)
        part = Cbuf.cpu().numpy()[:chunks, :, :N]
        _within(part, o["exact"], o["bound"], key, what + ": partials")
        out = reduced[id(Cbuf)]
        assert (_bits(out)[M * ldc:] == SENTINEL).all(), what
        got = out.cpu().numpy()[:M * ldc].reshape(M, ldc)[:, :N]
        s = np.zeros((M, N))
        for c in range(chunks):
            s += part[c].astype(np.float64)
        assert (got.view(np.int32) == s.astype(np.float32).view(np.int32)).all(), f"{what}: the chunk sum is not the rounded float64 sum of the partials"
        _within(got, o["total"], o["bound"].sum(0) + ulp32(o["total"]), key, what + ": reduced dW")
        if db is None:
            continue
        _untouched(db, _region(tuple(db.shape), chunks, M), what + ": dbias")
        dpart = db.cpu().numpy()[:chunks]
        _within(dpart, o["db_exact"], o["db_bound"], key, what + ": dbias partials")
        out = reduced[id(db)]
        assert (_bits(out)[M:] == SENTINEL).all(), what
        got = out.cpu().numpy()[:M]
        s = np.zeros(M)
        for c in range(chunks):
            s += dpart[c].astype(np.float64)
        assert (got.view(np.int32) == s.astype(np.float32).view(np.int32)).all(), f"{what}: the dbias chunk sum is not the rounded float64 sum"
        _within(got, o["db_total"], o["db_bound"].sum(0) + ulp32(o["db_total"]), key, what + ": reduced dbias")
