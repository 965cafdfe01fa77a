"""CPU-only checks of the wideband complex stream (include/micloc_hip.h "wideband streaming, complex Beamformer"): the header declares the
new entries and _lib binds them with the header's argument counts and kinds, every entry refuses NULL plans and F outside 1..16 before it
touches a device, the Python surface and the shims exist, and the depth of the bands' window ring -- restated here in NumPy, shared with
tests/test_hip_stream_wideband_complex.py -- bounds the windows one tile completes for random tilings."""
import ctypes
import os
import re

import numpy as np
import pytest

import csrc_build
from conftest import ROOT
from test_stream_complex_cpu import bookkeeping, random_tiling

from haghighatshoarmuir2024_amd import _lib, utils

NEW = ["micloc_stream_complex_bands_state_bytes", "micloc_stream_complex_bands_workspace_bytes", "micloc_stream_complex_bands_reset",
       "micloc_stream_complex_bands_bandpass_tile_f64", "micloc_stream_complex_bands_localize_tile_f64",
       "micloc_stream_complex_bands_window_state_bytes", "micloc_stream_complex_bands_window_reset",
       "micloc_stream_complex_bands_localize_tile_windows_f64", "micloc_stream_complex_bands_status"]

FS = 48_000
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0]]


def ring_depth(max_tile, CH, hop):
    """stream_bands_ring_depth (csrc/stream_bands_complex.hip): a tile contracts at most Ks = ceil((max_tile + CH - 1) / CH) chunk rows,
    r chunk rows complete at most ceil(r / (hop / CH)) windows, and the final tile cuts at most one more at the end of the recording."""
    Ks = (max_tile + 2 * CH - 2) // CH
    return -(-Ks // (hop // CH)) + 1


def test_header_declares_and_lib_binds_the_new_entries():
    raw = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    assert "wideband streaming, complex Beamformer" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define\s+MICLOC_ABI_VERSION\s+1\b", text)  # additive: the ABI version stays
    declared = set(re.findall(r"\b(micloc_[A-Za-z0-9_]+)\s*\(", text))
    ctype_of = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/micloc_hip.h"
        assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.SYMBOLS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        res, args = _lib.SYMBOLS[name]
        assert res is ctype_of[m.group(1)], name
        params = [" ".join(a.split()) for a in m.group(2).split(",")]
        assert len(args) == len(params), name
        for a, p in zip(args, params):  # the kinds line up with the header's
            if "*const *" in p or "* const *" in p:
                assert a == ctypes.POINTER(ctypes.c_void_p), (name, p)
            elif "*" in p:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)), (name, p)
            elif p.startswith("size_t"):
                assert a is ctypes.c_size_t, (name, p)
            else:
                assert p.startswith("int ") and a is ctypes.c_int, (name, p)
    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "stream_bands_complex.hip")).read())
    assert "stream_bands_bandpass_tile_kernel" in code
    assert "atomic" not in code.lower() and "hipStreamSynchronize" not in code and "hipDeviceSynchronize" not in code and "hipMalloc" not in code
    assert "stream_bands_complex.hip" in csrc_build.built_sources()


def test_every_entry_refuses_null_plans_and_a_bad_band_count():
    """MICLOC_ERR_INVALID (0 for the size functions) for plans == NULL, a NULL plan in the array, F = 0 and F = 17 -- before any device call
    (the codes that need a plan are in tests/test_hip_stream_wideband_complex.py)."""
    lib = _lib.load()
    INV = _lib.MICLOC_ERR_INVALID
    one = ctypes.c_void_p(256)
    nulls = (ctypes.c_void_p * 17)(*([None] * 17))
    s6 = (ctypes.c_int * 6)()
    for plans, F in ((None, 2), (nulls, 2), (nulls, 0), (nulls, 17), (nulls, -1)):
        assert lib.micloc_stream_complex_bands_state_bytes(plans, F, 1) == 0
        assert lib.micloc_stream_complex_bands_workspace_bytes(plans, F, 1, 100) == 0
        assert lib.micloc_stream_complex_bands_window_state_bytes(plans, F, 1, 100, 256, 256, 4) == 0
        assert lib.micloc_stream_complex_bands_reset(plans, F, 1, one, 1 << 20, None) == INV
        assert lib.micloc_stream_complex_bands_bandpass_tile_f64(plans, F, one, 1, 16, 16, 0, 16, 0, one, 1 << 20, one, 1 << 20, None) == INV
        assert lib.micloc_stream_complex_bands_localize_tile_f64(plans, F, one, 1 << 20, 1, 16, 0, None, one, one, one, 1 << 20, None) == INV
        assert lib.micloc_stream_complex_bands_window_reset(plans, F, 1, 100, one, 1 << 20, 256, 256, 4, None) == INV
        assert lib.micloc_stream_complex_bands_localize_tile_windows_f64(plans, F, one, 1 << 20, 1, 16, 0, None, one, one, one, 1 << 20, one, 1 << 20, 256,
                                                                         256, 4, one, one, one, one, None) == INV
    # arguments that are refused whatever the plans are
    assert lib.micloc_stream_complex_bands_bandpass_tile_f64(nulls, 2, one, 1, 16, 16, 0, 16, 48, one, 1 << 20, one, 1 << 20, None) == INV
    assert lib.micloc_stream_complex_bands_status(None, None, s6, None) == INV
    assert lib.micloc_stream_complex_bands_status(one, None, None, None) == INV


def _loc(bands, G=33, seed=5):
    from micloc.array_geometry import CenterCircularArray
    from micloc.beamformer import Beamformer
    from micloc.filterbank import ButterworthFilterbank
    from micloc.wideband import WidebandBeamformerLocalizer

    beamfs = [Beamformer(CenterCircularArray(4.5e-2, 7), 10e-3, fr, fs=FS) for fr in bands]
    rng = np.random.RandomState(seed)
    return WidebandBeamformerLocalizer(beamfs, [rng.randn(7, G) + 1j * rng.randn(7, G) for _ in bands], ButterworthFilterbank(freq_bands=bands, order=2, fs=FS))


def test_python_surface_and_shims():
    import micloc.streaming
    import micloc.wideband
    from haghighatshoarmuir2024_amd import streaming, wideband

    cls = streaming.WidebandComplexStreamingLocalizer
    assert micloc.streaming.WidebandComplexStreamingLocalizer is cls
    assert issubclass(cls, streaming._TileStream)
    for name in ("push", "push_replay", "status", "latest_window", "windows", "finish"):
        assert callable(getattr(cls, name))
    assert callable(wideband.WidebandBeamformerLocalizer.streaming_localizer)
    assert micloc.wideband.WidebandBeamformerLocalizer.streaming_localizer is wideband.WidebandBeamformerLocalizer.streaming_localizer
    # (localization_demo.Demo gains no method of its own: tests/test_wideband_complex_cpu.py pins that; Demo.localizer() returns the
    # WidebandBeamformerLocalizer whose streaming_localizer() is the live route)


def test_constructor_refuses_a_wrongly_shaped_wrap_tail():
    """The shape is checked before any plan is built: [bands, batch, L // 2, num_mic]."""
    loc = _loc(BANDS)
    L2 = len(loc.beamfs[0].kernel) // 2
    for shape in ((3, L2, 7), (2, 3, L2 - 1, 7), (3, 2, L2, 7), (2, 3, L2, 6)):
        with pytest.raises(ValueError, match="wrap_tail"):
            loc.streaming_localizer(batch=3, total_frames=4800, wrap_tail=np.zeros(shape))
    with pytest.raises(ValueError, match="give window as well"):
        loc.streaming_localizer(batch=1, hop=256)


def test_ring_depth_bounds_the_windows_one_tile_completes():
    rng = np.random.default_rng(20240618)
    for CH in (256, 512):
        for case in range(150):
            max_tile = int(rng.choice([1, 7, CH - 1, CH, CH + 1, 3 * CH + 5, 12 * CH]))
            T = int(rng.integers(1, 12 * CH))
            wch = int(rng.integers(1, 6))
            hch = int(rng.integers(1, wch + 1))
            window, hop = wch * CH, hch * CH
            tiles = random_tiling(rng, T, max_tile) if case % 3 else [min(max_tile, T - t) for t in range(0, T, max_tile)]  # random, or as long as allowed
            Kb = ring_depth(max_tile, CH, hop)
            log = bookkeeping(tiles, CH, window, hop)
            before = 0
            for i, s in enumerate(log):
                final = i == len(tiles) - 1
                assert s["windows"] == utils.windows_complete(s["frames"], window, hop, T=T if final else None)
                assert s["windows"] - before <= Kb, (CH, max_tile, window, hop, tiles[:5], i)
                before = s["windows"]


def test_ring_depth_hand_written_cases():
    # a tile of 5 chunks, hop = 1 chunk, the recording ends inside a window: 5 complete windows and the cut one in ONE tile
    CH = 256
    log = bookkeeping([CH, 5 * CH + 7], CH, CH, CH)
    assert [s["windows"] for s in log] == [1, 7] and ring_depth(5 * CH + 7, CH, CH) >= 6
    # one-frame tiles: at most one chunk row per tile, two windows at the end (the last complete one and the cut one)
    assert ring_depth(1, CH, CH) == 2
    log = bookkeeping([1] * (CH + 1), CH, CH, CH)
    assert [s["windows"] for s in log[-2:]] == [1, 2]
    # the bound is met, so the "+ 1" of the cut window cannot be dropped: window = hop = 2 chunks, the final tile brings two chunk rows (one
    # ragged) that complete window 1 AND cut window 2
    tiles = [CH, CH, CH, CH + 1]
    log = bookkeeping(tiles, CH, 2 * CH, 2 * CH)
    assert [s["windows"] for s in log] == [0, 1, 1, 3] and ring_depth(CH + 1, CH, 2 * CH) == 2
