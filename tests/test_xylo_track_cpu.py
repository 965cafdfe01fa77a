"""CPU checks of the Xylo tracking feature: the reference of tests/xylo_track_ref.py satisfies the conditions that keep the GPU tests
honest (ties, moving winners, winners and ties across waves and neuron blocks, non-integer maxima), and the new C-ABI entries are
exported and answer their pure questions and their status codes without a device."""
import ctypes

import numpy as np
import pytest

import xylo_track_ref as R


def _frame_stats(ref, trials, group):
    """Over the frames of `trials`: share with a tie at a positive maximum, distinct winners, share whose tied maxima lie in different
    groups of `group` neurons, share with a winner >= group, share with a non-integer maximum."""
    tie = cross = high = frac = total = 0
    winners = set()
    for b in trials:
        env, idx, peak = ref["env"][b], ref["index"][b], ref["peak_env"][b]
        at_max = env == peak[:, None]
        pos = peak > 0
        tie += int((pos & (at_max.sum(axis=1) > 1)).sum())
        first = idx // group
        last = (env.shape[1] - 1 - np.argmax(at_max[:, ::-1], axis=1)) // group
        cross += int((pos & (last != first)).sum())
        high += int((idx >= group).sum())
        frac += int((peak != np.floor(peak)).sum())
        winners |= set(idx.tolist())
        total += len(idx)
    return dict(tie=tie / total, winners=len(winners), cross=cross / total, high=high / total, frac=frac / total)


@pytest.mark.parametrize("N,T,group,min_high", [(1100, 200, 512, 0.01), (449, 700, 128, 0.10)])
def test_reference_has_ties_and_moving_winners(N, T, group, min_high):
    """The random trials 0 and 2 of the recipe (trial 1 fires every channel), windows (1, 1) and (2, 5)."""
    for w_rise, w_fall in ((1, 1), (2, 5)):
        st = _frame_stats(R.recipe_reference(N, T, w_rise, w_fall), (0, 2), group)
        print(N, T, (w_rise, w_fall), st)
        assert st["tie"] >= 0.5, st
        assert st["winners"] >= 5, st
        assert st["cross"] >= 0.5, st
        assert st["high"] >= min_high, st
        if (w_rise, w_fall) == (2, 5):
            assert st["frac"] >= 0.9, st


def test_reference_envelope_is_the_rule():
    """The helper's host reference is the rule of include/micloc_hip.h, step by step, on one small case."""
    ref = R.recipe_reference(33, 127, 2, 5)
    out, _ = R.recipe_spikes(33, 127)
    a_rise, i_rise, a_fall = 1 - 1 / 2, 1 / 2, 1 - 1 / 5
    e = out[0, 0].astype(np.float64)
    for t in range(1, 127):
        m = out[0, t].astype(np.float64)
        e = np.where(m >= e, a_rise * e + i_rise * m, a_fall * e)
    np.testing.assert_array_equal(e, ref["env_last"][0])
    assert ref["index"][0, -1] == int(np.argmax(e))


# ---- the C-ABI without a device -------------------------------------------------------------------------------------------------
OK, ERR_INVALID, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    from haghighatshoarmuir2024_amd import _lib

    return _lib.load()  # raises if a declared symbol is missing


def test_status_codes_are_the_headers(lib):
    import os
    import re

    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"\b(MICLOC_(?:OK|ERR_INVALID|ERR_SHAPE|ERR_WORKSPACE)) = (-?\d+),", text)}
    assert got == dict(MICLOC_OK=OK, MICLOC_ERR_INVALID=ERR_INVALID, MICLOC_ERR_SHAPE=ERR_SHAPE, MICLOC_ERR_WORKSPACE=ERR_WORKSPACE)
    for name in ("micloc_xylo_track_is_fused", "micloc_xylo_track_workspace_bytes", "micloc_xylo_lif_track_i16"):
        assert name in text and hasattr(lib, name)


def test_is_fused_is_a_pure_function(lib):
    f = lib.micloc_xylo_track_is_fused
    assert f(14, 28, 449, 0, 31) == 1
    assert f(14, 28, 449, -3, 31) == 0   # a recurrent weight
    assert f(0, 28, 449, 0, 31) == 0     # uint8 event counts
    assert f(0, 65, 449, 0, 31) == 0 and f(14, 65, 449, 0, 31) == 0 and f(33, 66, 449, 0, 31) == 0  # more than 64 input channels
    assert f(32, 64, 1100, 0, 1) == 1
    assert f(14, 28, 0, 0, 31) < 0 and f(14, 27, 449, 0, 31) < 0 and f(14, 28, 449, 0, 0) < 0 and f(-1, 28, 449, 0, 31) < 0
    assert f(0, 28, 1025, -3, 31) < 0    # the recurrent kernel holds one workgroup of 1024 neurons


def test_workspace_bytes_is_a_pure_function(lib):
    w = lib.micloc_xylo_track_workspace_bytes
    for N in (1, 449, 512, 513, 1100, 4096):
        for B, T in ((1, 1), (3, 700), (1100, 4799), (1, 240_000)):
            nb = w(14, 28, N, 0, B, T)
            assert 0 < nb <= 16 * B * T * ((N + 511) // 512) + 4096, (N, B, T, nb)
    assert w(14, 28, 449, 0, 1, 240_000) < 240_000 * 449  # nothing of size T x N
    # the two-step route: the raster and the envelope of one trial
    assert 9 * 300 * 100 <= w(0, 28, 100, -3, 5, 300) <= 9 * 300 * 100 + 512
    assert w(0, 28, 100, -3, 5, 300) == w(0, 28, 100, -3, 1, 300)
    # bad arguments
    assert w(14, 28, 449, 0, 0, 700) == 0 and w(14, 28, 449, 0, 3, 0) == 0 and w(14, 28, 0, 0, 3, 700) == 0
    assert w(14, 28, 449, 0, 65535, 65535) == 0  # B T > 2^31 - 1
    assert w(0, 65, 449, 0, 3, 700) == 0 and w(14, 27, 449, 0, 3, 700) == 0


def test_track_entry_returns_its_status_codes_before_touching_the_device(lib):
    """Host buffers only: every call below must return before any launch."""
    f = lib.micloc_xylo_lif_track_i16
    vp = ctypes.c_void_p
    net_bytes = lib.micloc_xylo_workspace_bytes(28, 449)
    ws_bytes = lib.micloc_xylo_track_workspace_bytes(14, 28, 449, 0, 2, 64)
    buf = np.zeros(net_bytes + ws_bytes + 4096, np.uint8)
    base = (buf.ctypes.data + 255) & ~255  # 256-byte aligned host addresses: never dereferenced
    spikes, net, ws = vp(base), vp(base), vp(base + ((net_bytes + 255) & ~255))
    index = vp(base)
    c = (0.5, 0.5, 0.8)

    def call(spikes=spikes, tc=14, B=2, T=64, Cin=28, N=449, w_rec=0, cap=31, index=index, net=net, net_bytes=net_bytes, ws=ws, ws_bytes=ws_bytes):
        return f(spikes, tc, B, T, Cin, N, w_rec, cap, *c, index, None, None, None, net, net_bytes, ws, ws_bytes, None)

    assert call(spikes=None) == ERR_INVALID
    assert call(index=None) == ERR_INVALID
    assert call(B=0) == ERR_INVALID
    assert call(cap=0) == ERR_INVALID
    assert call(T=0) == ERR_SHAPE
    assert call(N=0) == ERR_SHAPE
    assert call(B=65535, T=65535) == ERR_SHAPE
    assert call(Cin=27) == ERR_SHAPE
    assert call(net=None) == ERR_WORKSPACE
    assert call(net_bytes=net_bytes - 1) == ERR_WORKSPACE
    assert call(ws=None) == ERR_WORKSPACE
    assert call(ws=vp(ws.value + 8)) == ERR_WORKSPACE
    assert call(ws_bytes=ws_bytes - 1) == ERR_WORKSPACE
    # the two-step route's minimum is checked the same way
    need = lib.micloc_xylo_track_workspace_bytes(0, 28, 100, -3, 2, 64)
    assert call(tc=0, N=100, w_rec=-3, ws_bytes=need - 1) == ERR_WORKSPACE
