"""The tracked stream (include/micloc_hip.h "streaming, tracking"; csrc/stream_track.hip; streaming.py track=) without a GPU: the premise
of the state hand-off, the ring arithmetic of tracked(), the symbols, the size entries' answer to bad arguments and the host-side refusals."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import csrc_build
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("micloc_stream_track_state_bytes", "micloc_stream_track_workspace_bytes", "micloc_stream_track_reset",
         "micloc_stream_localize_tile_track_f64", "micloc_stream_complex_localize_tile_track_f64")


def test_envelope_split_at_arbitrary_cuts_carrying_the_last_row_is_the_unsplit_envelope():
    """e[t] depends on e[t-1] and |y_t| only: a segment that starts from the carried row (as the oracle's state_0, which it takes from the
    magnitude of its first input row -- the carried row is non-negative) continues the recurrence bit for bit."""
    rng = np.random.RandomState(21)
    T, G = 997, 37
    y = rng.randn(T, G) * np.exp(rng.randn(T, 1))
    y[rng.rand(T, G) < 0.05] = 0.0
    for wf, wr in ((4800, 480), (7, 3), (1, 1)):
        whole = O.envelope(y, wf, wr)
        for trial in range(6):
            cuts = [0] + sorted(set(int(c) for c in rng.randint(1, T, size=rng.randint(1, 40)))) + [T]
            if trial == 0:
                cuts = list(range(T + 1))  # one frame per segment
            out, last = [], None
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                if last is None:
                    seg = O.envelope(y[lo:hi], wf, wr)
                else:
                    seg = O.envelope(np.concatenate([last[None], y[lo:hi]]), wf, wr)[1:]
                out.append(seg)
                last = seg[-1]
            np.testing.assert_array_equal(np.concatenate(out), whole)


def test_ring_rows_against_a_brute_force_ring():
    from haghighatshoarmuir2024_amd.streaming import ring_rows

    for depth in (1, 2, 5, 64):
        ring, items = [None] * depth, []
        assert ring_rows(0, depth) == (0, 0, [])
        for n in range(3 * depth + 3):
            ring[n % depth] = n  # item n goes to row n % depth
            items.append(n)
            first, k, rows = ring_rows(n + 1, depth)
            kept = items[-depth:]
            assert (first, k) == (kept[0], len(kept))
            assert [ring[r] for r in rows] == kept  # ascending, oldest kept item first


def test_header_declares_and_lib_binds_the_symbols():
    from haghighatshoarmuir2024_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "micloc_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert n in _lib.SYMBOLS, n
    assert "streaming, tracking" in open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    assert "stream_track.hip" in csrc_build.built_sources()
    src = open(os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc", "stream_track.hip")).read()
    assert "atomic" not in src.lower() and "hipStreamSynchronize" not in src and "hipDeviceSynchronize" not in src


def test_the_chunk_walk_is_written_once():
    """csrc/track_rows.h holds stages 1 and 2 of the one-shot, the band and the stream kernels, which decide the bits of every y[t][g], once:
    with the comments stripped the fp64 matrix-core product occurs there three times (membrane loop, SNN product, complex product) and the
    complex magnitude once, and neither occurs in a kernel file; both objects are rebuilt when the header changes."""
    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("track_rows.h", "track.hip", "stream_track.hip")}
    code = re.sub(r"//[^\n]*|/\*.*?\*/", "", text["track_rows.h"], flags=re.S)
    for word, times in (("mfma_f64_16x16x4f64", 3), ("hypot(", 1)):
        assert code.count(word) == times, word
        assert word not in text["track.hip"] and word not in text["stream_track.hip"], word
    for f in ("track.hip", "stream_track.hip"):
        assert '#include "track_rows.h"' in text[f], f
    assert {"track.o", "stream_track.o"} <= csrc_build.rebuilt_after_edit("track_rows.h")


def test_size_entries_return_zero_and_entries_refuse_null_before_any_device_work():
    from haghighatshoarmuir2024_amd import _lib

    lib = _lib.load()
    assert lib.micloc_abi_version() == 1
    assert lib.micloc_stream_track_state_bytes(None, 1) == 0
    assert lib.micloc_stream_track_workspace_bytes(None, 1, 4096) == 0
    assert lib.micloc_stream_track_reset(None, 1, None, 0, None) == _lib.MICLOC_ERR_INVALID
    snn = lib.micloc_stream_localize_tile_track_f64(None, None, None, 0, None, 1, 4096, 0, None, None, None, 0, None, 0, 0, 0, 0, None, None, None, None,
                                                    None, 0, 0.9, 0.1, 0.99, 4096, None, None, None, None, None, 0, None)
    cpx = lib.micloc_stream_complex_localize_tile_track_f64(None, None, 0, 1, 100, 0, None, None, None, 0, None, 0, 0, 0, 0, None, None, None, None,
                                                            None, 0, 0.9, 0.1, 0.99, 128, None, None, None, None, None, 0, None)
    assert snn == _lib.MICLOC_ERR_INVALID and cpx == _lib.MICLOC_ERR_INVALID


def test_track_setup_refuses_on_the_host_and_builds_numpy_constants():
    from haghighatshoarmuir2024_amd.streaming import track_setup
    from haghighatshoarmuir2024_amd.utils import Envelope

    env = Envelope(rise_time=10e-3, fall_time=100e-3, fs=48_000)
    a_rise, i_rise, a_fall, R = track_setup(env, 14, 449, False, 16640)
    wl = np.asarray([4800, 480])
    assert (a_rise, i_rise, a_fall) == (float((1 - 1 / wl)[1]), float((1 / wl)[1]), float((1 - 1 / wl)[0]))
    assert R == 66560 and R % 64 == 0 and R >= 4 * 16640  # the default ring of a live source
    assert track_setup(env, 14, 449, False, 12000, total_frames=None)[3] == 48000
    assert track_setup(env, 14, 449, True, 100, total_frames=4799)[3] == 4799
    assert track_setup(env, 14, 449, False, 16640, total_frames=4799)[3] == 16640  # never below what one tile can make final
    assert track_setup(env, 14, 449, False, 16640, max_track=16640)[3] == 16640
    with pytest.raises(ValueError, match="max_track"):
        track_setup(env, 14, 449, False, 16640, max_track=16639)
    with pytest.raises(ValueError, match="16 channels"):
        track_setup(env, 40, 97, False, 16640)  # a 40-channel plan: the two-step route, which has no stream
    with pytest.raises(ValueError, match="512 DoAs"):
        track_setup(env, 14, 1440, False, 16640)
    assert track_setup(env, 14, 1440, True, 100)[3] == 448  # (a complex bf_mat has no such limit)
    with pytest.raises(ValueError, match="at least one sample"):
        track_setup(SimpleNamespace(win_lens=np.asarray([4800, 0])), 14, 449, False, 16640)
