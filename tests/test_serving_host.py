"""CPU tests of the serving path (rlks.serving, rlks_policy_act): the ABI, the argument errors that are
found before any HIP call, the host-side input checks and the fixtures' near-tie cap."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle
import serving_cases as sc
from conftest import ROOT

NEW = ("rlks_policy_act", "rlks_host_alloc", "rlks_host_free")
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def test_new_symbols_declared_exported_and_bound():
    from rlks import _lib

    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rlks.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for s in NEW:
        assert re.search(rf"^int {s}\(", txt, flags=re.M), s
        assert s in _lib.SIGNATURES and hasattr(lib, s)
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s]
    assert len(_lib.SIGNATURES["rlks_policy_act"]) == 16


def _act(desc, params, obs, actions, n=1, mask=None, fstate=None):
    from rlks import _lib

    return _lib.lib().rlks_policy_act(C.byref(desc) if desc is not None else None, params, fstate, obs, mask, n, 0, 0, 0,
                                      0, actions, None, None, None, None, None)


def test_policy_act_argument_errors_before_any_launch():
    """every code below is returned from the host checks: no device is needed (or touched)"""
    from rlks import _lib

    buf = (C.c_ubyte * 256)()
    base = (C.addressof(buf) + 63) // 64 * 64  # a non-null, 64-byte aligned address that is never dereferenced
    p, o, a = base, base + 64, base + 128
    ok = _lib.MlpDesc(6, 256, 2, 0)
    assert _act(None, p, o, a) == ERR_ARG
    assert _act(ok, None, o, a) == ERR_ARG
    assert _act(ok, p, None, a) == ERR_ARG
    assert _act(ok, p, o, None) == ERR_ARG
    assert b"null" in _lib.lib().rlks_last_error()
    assert _act(ok, p, o, a, n=-1) == ERR_ARG
    assert _act(ok, p + 4, o, a) == ERR_ARG          # params: 16-byte aligned fragment loads
    assert _act(ok, p, o + 2, a) == ERR_ARG
    assert _act(ok, p, o, a, mask=base + 4) == ERR_ARG
    for D, Hd, A in [(6, 384, 2), (6, 2048, 2), (0, 256, 2), (193, 256, 2), (6, 256, 0), (6, 256, 65)]:
        assert _act(_lib.MlpDesc(D, Hd, A, 0), p, o, a) == ERR_UNSUPPORTED, (D, Hd, A)
    assert _act(_lib.MlpDesc(6, 256, 65, 0), p, o, a, mask=base) == ERR_UNSUPPORTED
    assert b"64" in _lib.lib().rlks_last_error()
    # n = 0: nothing to do, no launch
    assert _act(ok, p, o, a, n=0) == 0
    assert _act(_lib.MlpDesc(192, 256, 64, 0), p, o, a, n=0, mask=base) == 0
    # the staging allocator's own argument errors
    h, d = C.c_void_p(), C.c_void_p()
    assert _lib.lib().rlks_host_alloc(0, C.byref(h), C.byref(d)) == ERR_ARG
    assert _lib.lib().rlks_host_alloc(64, None, C.byref(d)) == ERR_ARG
    assert _lib.lib().rlks_host_free(None) == 0


def test_input_checks_raise_value_error():
    from rlks.serving import check_inputs, pack_mask

    D, A = 6, 2
    x, bits, single = check_inputs(D, A, 16, False, np.zeros(D))
    assert x.shape == (1, D) and x.dtype == np.float32 and bits is None and single
    x, bits, single = check_inputs(D, A, 16, True, np.zeros((5, D)), np.array([True, False]))
    assert x.shape == (5, D) and not single and bits.dtype == np.uint64 and list(bits) == [1] * 5
    for bad in (np.zeros(D + 1), np.zeros((3, D - 1)), np.zeros((2, 3, D)), np.float32(1.0)):
        with pytest.raises(ValueError, match="obs must be"):
            check_inputs(D, A, 16, False, bad)
    with pytest.raises(ValueError, match="compute_actions"):
        check_inputs(D, A, 16, False, np.zeros((17, D)))
    with pytest.raises(ValueError, match="action_mask"):
        check_inputs(D, A, 16, True, np.zeros((3, D)))  # a masked policy must be given a mask
    for bad in (np.ones(A + 1, bool), np.ones((2, A), bool), np.ones((3, A + 1), bool)):
        with pytest.raises(ValueError, match="action_mask must be"):
            check_inputs(D, A, 16, False, np.zeros((3, D)), bad)
    with pytest.raises(ValueError, match="at most 64"):
        pack_mask(np.ones(65, bool), 1, 65)
    # bit a of row i = mask[i, a], up to bit 63
    m = np.zeros((2, 64), bool)
    m[0, [0, 63]] = True
    m[1, 5] = True
    assert list(pack_mask(m, 2, 64)) == [(1 << 63) | 1, 1 << 5]


def test_policy_server_rejects_a_bad_max_rows_before_allocating():
    from rlks.policy import PolicyParams
    from rlks.serving import PolicyServer

    p = PolicyParams(6, 256, 2, device=None, seed=0)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_rows"):
            PolicyServer(p, max_rows=bad)


def test_fixture_layout_and_biases():
    """serving_cases restates the tensor shapes; adjust() touches the heads and the biases alone"""
    from rlks.policy import PolicyParams

    for D, A in sc.POLICIES:
        p = PolicyParams(D, sc.H, A, device=None, seed=sc.PARAM_SEED)
        assert sc.shapes(D, A) == [tuple(s) for s in p.shapes]
        base = p.flat.numpy()
        flat, off = sc.fixture_flat(D, A)
        for i, shp in enumerate(sc.shapes(D, A)):
            n = int(np.prod(shp))
            a, b = base[off[i]: off[i] + n], flat[off[i]: off[i] + n]
            if i in sc.BIASES:
                assert np.all(a == 0) and np.all(b != 0) and np.abs(b).max() < 0.6  # N(0, 0.1) draws
                assert n < 100 or abs(b.std() - 0.1) < 0.03
            elif i in sc.W_HEADS:
                np.testing.assert_array_equal(b, a * np.float32(sc.HEAD_SCALE))
            else:
                np.testing.assert_array_equal(a, b)


def test_near_tie_cap_holds_for_the_fixtures():
    """test_gpu_serving's agreement test may leave out rows whose f64 top-two gap is below 8 x the row's
    largest band-vs-f64 deviation, at most 1 % of them: from the oracle alone, the 1,024 fixture rows of
    every policy stay far inside that"""
    for D, A in sc.POLICIES:
        flat, off = sc.fixture_flat(D, A)
        obs = sc.observations(sc.AGREE_ROWS, D)
        l64, _ = oracle.mlp_forward(flat, off, D, sc.H, A, obs)
        band, _ = oracle.mlp_forward_fp32_band(flat, off, D, sc.H, A, obs)
        tie = sc.near_ties(l64, band)
        assert tie.mean() <= sc.AGREE_MAX_LEFT_OUT, (D, A, tie.mean())
        top = np.sort(l64, axis=1)
        assert np.median(top[:, -1] - top[:, -2]) > 1e-2  # the scaled heads do give O(1) gaps
