"""CPU-only checks of the complex Beamformer's stream (include/micloc_hip.h "streaming, complex Beamformer"): the header declares the new
entries and _lib binds them with the header's argument counts, every entry refuses a NULL plan before it touches a device, and the carry /
chunk / emission bookkeeping of the device kernels -- restated here in NumPy, shared with tests/test_hip_stream_complex.py -- keeps its
invariants for random tilings."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

from haghighatshoarmuir2024_amd import _lib, utils

NEW = ["micloc_stream_complex_state_bytes", "micloc_stream_complex_workspace_bytes", "micloc_stream_complex_reset",
       "micloc_stream_complex_bandpass_tile_f64", "micloc_stream_complex_localize_tile_f64", "micloc_stream_complex_window_state_bytes",
       "micloc_stream_complex_window_reset", "micloc_stream_complex_localize_tile_windows_f64", "micloc_stream_complex_status"]


def bookkeeping(tiles, CH, window=None, hop=None):
    """The clock of the stream after every tile, as stream_complex_accumulate_kernel / _window_kernel / _slide_kernel keep it: the last
    tile is the final one.  -> list of dict(chunks, frames, carry, pushed, windows) (windows: emitted so far; None without `window`)."""
    T = int(sum(tiles))
    chunks = frames = carry = pushed = 0
    out = []
    for i, n in enumerate(tiles):
        final = i == len(tiles) - 1
        avail = carry + n
        whole = avail // CH
        rows = -(-avail // CH) if final else whole  # the ragged last chunk is contracted on the final tile only
        taken = avail if final else whole * CH
        chunks += rows
        frames += taken
        carry = 0 if final else avail - whole * CH
        pushed += n
        nwin = None
        if window is not None:
            h = window if hop is None else hop
            if final:
                nwin = 1 if T <= window else 1 + -(-(T - window) // h)
            else:
                nwin = 0 if frames < window else (frames - window) // h + 1
        out.append(dict(chunks=chunks, frames=frames, carry=carry, pushed=pushed, windows=nwin))
    return out


def test_header_declares_and_lib_binds_the_new_entries():
    text = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    assert "streaming, complex Beamformer" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(micloc_[A-Za-z0-9_]+)\s*\(", text))
    ctype_of = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/micloc_hip.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.SYMBOLS"
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        res, args = _lib.SYMBOLS[name]
        assert res is ctype_of[m.group(1)], name
        params = [a.strip() for a in m.group(2).split(",")]
        assert len(args) == len(params), name
        for a, p in zip(args, params):  # the scalar kinds line up with the header's
            if "*" in p:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)), (name, p)
            elif p.startswith("size_t"):
                assert a is ctypes.c_size_t, (name, p)
            else:
                assert p.startswith("int ") and a is ctypes.c_int, (name, p)


def test_python_surface():
    import micloc.streaming
    from haghighatshoarmuir2024_amd import streaming
    from haghighatshoarmuir2024_amd.beamformer import Beamformer

    assert micloc.streaming.ComplexStreamingLocalizer is streaming.ComplexStreamingLocalizer
    for name in ("push", "push_replay", "status", "latest_window", "windows", "finish"):
        assert callable(getattr(streaming.ComplexStreamingLocalizer, name))
    assert callable(Beamformer.streaming_localizer)
    x = np.arange(2 * 5 * 3, dtype=np.float64).reshape(2, 5, 3)
    w = streaming.ComplexStreamingLocalizer.wrap_rows(x, 4)  # at least L / 2 frames: the last L / 2
    assert np.array_equal(w, x[:, 3:, :])
    w = streaming.ComplexStreamingLocalizer.wrap_rows(x[:, :1, :], 8)  # shorter: np.roll's rows, zero padded
    assert w.shape == (2, 4, 3) and np.array_equal(w[:, 0], x[:, 0]) and not w[:, 1:].any()


def test_every_entry_refuses_a_null_plan():
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    st4 = (ctypes.c_int * 4)()
    assert lib.micloc_stream_complex_state_bytes(None, 1) == 0
    assert lib.micloc_stream_complex_workspace_bytes(None, 1, 12000) == 0
    assert lib.micloc_stream_complex_window_state_bytes(None, 1, 256, 256, 4) == 0
    assert lib.micloc_stream_complex_reset(None, 1, one, 4096, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_complex_bandpass_tile_f64(None, one, 1, 16, 16, 0, 16, one, 4096, one, 4096, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_complex_localize_tile_f64(None, one, 4096, 1, 16, 0, one, one, one, 4096, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_complex_window_reset(None, 1, one, 4096, 256, 256, 4, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_complex_localize_tile_windows_f64(None, one, 4096, 1, 16, 0, one, one, one, 4096, one, 4096, 256, 256, 4, one, one, one,
                                                               one, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_complex_status(None, st4, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_complex_status(one, None, None) == _lib.MICLOC_ERR_INVALID


def random_tiling(rng, T, longest):
    tiles = []
    while sum(tiles) < T:
        tiles.append(int(min(rng.integers(1, longest + 1), T - sum(tiles))))
    return tiles


def test_bookkeeping_for_random_tilings():
    rng = np.random.default_rng(20240611)
    for CH in (256, 512):
        for case in range(60):
            T = int(rng.integers(1, 9 * CH))
            tiles = random_tiling(rng, T, int(rng.choice([1, 7, CH - 1, CH, 3 * CH + 5])) if T > 40 or case % 2 else 1)
            wch, hch = int(rng.integers(1, 5)), 1
            hch = int(rng.integers(1, wch + 1))
            window, hop = wch * CH, hch * CH
            log = bookkeeping(tiles, CH, window, hop)
            pushed = 0
            for i, (n, s) in enumerate(zip(tiles, log)):
                pushed += n
                final = i == len(tiles) - 1
                assert s["pushed"] == pushed
                assert 0 <= s["carry"] < CH  # the remainder is always less than a chunk
                if final:
                    assert s["carry"] == 0 and s["frames"] == T and s["chunks"] == -(-T // CH)
                else:
                    assert s["frames"] + s["carry"] == pushed  # every frame is contracted or waits in the carry
                    assert s["frames"] == (pushed // CH) * CH and s["chunks"] == pushed // CH
                # the windows emitted are those of the streaming window rule for the frames contracted
                assert s["windows"] == utils.windows_complete(s["frames"], window, hop, T=T if final else None)
                if i:
                    assert s["windows"] >= log[i - 1]["windows"] and s["chunks"] >= log[i - 1]["chunks"]
            assert log[-1]["windows"] == len(utils.window_bounds(T, window, hop)[0])


def test_bookkeeping_hand_written_cases():
    # the header's case: window = 4 CH', hop = CH' with CH' = 256 and T = 1100 has 2 windows, not 5
    log = bookkeeping([300, 300, 300, 200], 256, 1024, 256)
    assert [s["chunks"] for s in log] == [1, 2, 3, 5]
    assert [s["carry"] for s in log] == [44, 88, 132, 0]
    assert [s["windows"] for s in log] == [0, 0, 0, 2]
    # tiles shorter than a chunk throughout: a chunk row appears only when the carry fills up
    log = bookkeeping([100] * 6, 256)
    assert [s["chunks"] for s in log] == [0, 0, 1, 1, 1, 3]  # 100, 200, 300, 400, 500 frames pushed; the final tile takes both that are left
    assert [s["frames"] for s in log] == [0, 0, 256, 256, 256, 600]
    assert [s["carry"] for s in log] == [100, 200, 44, 144, 244, 0]
    # one frame
    assert bookkeeping([1], 256, 256, 256) == [dict(chunks=1, frames=1, carry=0, pushed=1, windows=1)]
