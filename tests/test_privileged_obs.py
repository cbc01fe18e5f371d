"""The critic's privileged observation row without a GPU (csrc/privileged_obs.h, csrc/mpc_privileged_obs.h, rl_mpc_locomotion_amd.privileged_obs):
the layout against the numpy restatement of tests/privileged_obs_ref.py, the header's arithmetic compiled with g++ against the same restatement bit
for bit, and every refusal of the C ABI, which comes back before the device is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rl_mpc_locomotion_amd  # noqa: F401
from rl_mpc_locomotion_amd import _lib, privileged_obs as V
from tests import privileged_obs_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "rl-mpc-locomotion_amd", "csrc")
E_ARG = -1


def test_row_layout():
    assert [V.privileged_width(P) for P in (0, 15, 187)] == [64, 80, 240]
    for P in (0, 1, 6, 7, 15, 16, 22, 23, 187, 203, 208):
        scan, contact, phase, pad, w = ref.offsets(P)
        assert V.privileged_width(P) == w == ref.width(P) == V.lib().mpc_privobs_width(P) and w % 16 == 0 and 0 <= w - (48 + P + 5) < 16
        assert (V.SCAN_OFFSET, V.contact_offset(P), V.phase_offset(P)) == (scan, contact, phase)
        assert V.NUM_TASK_OBS == scan == 48 and contact == 48 + P and phase == contact + V.NUM_CONTACTS and pad == phase + 1 == 48 + P + V.NUM_EXTRA
    assert V.privileged_width(187) == 48 + 187 + 5                         # the default 17 x 11 scan: no pad at all
    for bad in (-1, 209):
        with pytest.raises(ValueError):
            V.privileged_width(bad)
        assert V.lib().mpc_privobs_width(bad) == E_ARG and b"mpc_privobs_width" in V.lib().mpc_privobs_last_error()
    assert V.inverse_length(2000) == ref.inverse_length(2000) == np.float32(1.0 / 2000.0) and V.inverse_length(3).dtype == np.float32


def test_restatement_on_a_hand_built_row():
    P, n = 15, 3
    obs = ref.sentinel_obs(n, 64)
    contact = np.array([[1, 0, 0, 1], [0, 0, 0, 0], [7, 1, 1, 1]], np.int32)
    progress = np.array([0, 5, 1999], np.int64)
    inv = ref.inverse_length(2000)
    got = ref.row(obs, contact, progress, inv, P)
    assert got.shape == (n, 80) and got.dtype == np.float32
    assert got[:, :63].tobytes() == obs[:, :63].tobytes()
    assert got[:, 63:67].tolist() == [[1, 0, 0, 1], [0, 0, 0, 0], [1, 1, 1, 1]]
    assert got[:, 67].tolist() == [0.0, float(np.float32(5) * inv), float(np.float32(1999) * inv)] and (got[:, 68:] == 0).all()


SHIM = r"""
#include "privileged_obs.h"
extern "C" {
int shim_width(int P) { return privobs::width(P); }
// out [n][width(P)]: the live columns copied, the rest through tail_column; i32 is the sim's record [9][n]
void shim_rows(int n, int P, int obs_width, const float *obs, const int *i32, const long long *progress, float inv_len, float *out) {
  const int live = privobs::kTaskObs + P, w = privobs::width(P);
  for (int r = 0; r < n; ++r)
    for (int col = 0; col < w; ++col)
      out[(long)r * w + col] = col < live ? obs[(long)r * obs_width + col] : privobs::tail_column(col, live, i32, n, r, progress[r], inv_len);
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("privobs_shim")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.shim_width.argtypes, L.shim_width.restype = [C.c_int], C.c_int
    L.shim_rows.argtypes, L.shim_rows.restype = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p], None
    return L


@pytest.mark.parametrize("P", (0, 15, 187))
def test_header_arithmetic_equals_the_restatement(shim, P):
    n, max_len = 65, 2000
    rng = np.random.default_rng(P)
    w_in = 48 if P == 0 else -(-(48 + P) // 16) * 16
    obs = ref.sentinel_obs(n, w_in, seed=P)
    i32 = rng.integers(0, 2, (9, n)).astype(np.int32)                      # the sim's layout: entry l of robot r at [l][r]
    i32[4:] = rng.integers(0, 50, (5, n))                                  # lift4 and fell: not read
    progress = rng.integers(0, max_len, n).astype(np.int64)
    progress[:3] = (0, 1, max_len - 1)
    inv = ref.inverse_length(max_len)
    assert shim.shim_width(P) == ref.width(P)
    out = np.full((n, ref.width(P)), np.nan, np.float32)
    shim.shim_rows(n, P, w_in, obs.ctypes.data, i32.ctypes.data, progress.ctypes.data, inv, out.ctypes.data)
    want = ref.row(obs, i32[:4].T, progress, inv, P)
    assert out.tobytes() == want.tobytes()
    assert 0 < want[:, 48 + P:48 + P + 4].mean() < 1 and len(np.unique(want[:, 48 + P + 4])) > 30


def test_refusals_come_back_before_the_device_is_touched():
    """No GPU is needed for any of these: create and destroy are host-only, and run validates everything before it looks at its handle's device."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "mpc_privileged_obs.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mpc_privobs_[a-z_]+)\s*\(", header))) == sorted(V.SYMBOLS)
    assert not set(V.SYMBOLS) & set(_lib.SYMBOLS)
    L = V.lib()
    for s in V.SYMBOLS:
        assert getattr(L, s).argtypes is not None, s
    err = L.mpc_privobs_last_error
    h = C.c_void_p()
    assert L.mpc_privobs_create(None, 4) == E_ARG and L.mpc_privobs_create(C.byref(h), 0) == E_ARG and b"n must be" in err()
    assert not h.value
    assert L.mpc_privobs_create(C.byref(h), 4) == 0 and h.value                 # host-only: no device needed
    assert L.mpc_privobs_bind(None, 0x1000) == E_ARG and L.mpc_privobs_bind(h, None) == E_ARG and b"null sim" in err()
    p, q = 0x10000, 0x20000
    run = lambda *a: L.mpc_privobs_run(*a, None)
    assert run(None, p, 48, 0, p, 0.001, q) == E_ARG
    assert run(h, None, 48, 0, p, 0.001, q) == E_ARG and run(h, p, 48, 0, None, 0.001, q) == E_ARG and run(h, p, 48, 0, p, 0.001, None) == E_ARG
    assert run(h, p, 48, -1, p, 0.001, q) == E_ARG and run(h, p, 48, 209, p, 0.001, q) == E_ARG and b"P must" in err()
    assert run(h, p, 47, 0, p, 0.001, q) == E_ARG and run(h, p, 62, 15, p, 0.001, q) == E_ARG and run(h, p, 50, 0, p, 0.001, q) == E_ARG and b"obs_width" in err()
    assert run(h, p + 4, 48, 0, p, 0.001, q) == E_ARG and run(h, p, 48, 0, p, 0.001, q + 8) == E_ARG and b"16-byte" in err()
    assert run(h, p, 48, 0, p + 4, 0.001, q) == E_ARG and b"8-byte" in err()
    assert run(h, p, 64, 0, p, 0.001, p) == E_ARG and b"must not be" in err()
    assert run(h, p, 48, 0, p, float("inf"), q) == E_ARG and run(h, p, 48, 0, p, float("nan"), q) == E_ARG and b"inv_len" in err()
    assert run(h, p, 48, 0, p, 0.001, q) == E_ARG and b"no sim bound" in err()   # everything else in order: the binding is what is missing
    L.mpc_privobs_destroy(h)
    L.mpc_privobs_destroy(None)


def test_classes_raise_without_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.MpcLibraryError):
        V.PrivilegedObs(4)

    class Few:
        n = 3
    from rl_mpc_locomotion_amd import rl_task as R
    with pytest.raises(ValueError, match="privileged observations hold 3"):
        R.BatchedRLTask([0] * 4, [0] * 4, privileged_obs=Few())           # refused before the device is asked for
