"""CPU checks of the streaming windows (include/micloc_hip.h, "streaming windows"): the new C-ABI symbols and their status codes
without a device, the Makefile entry, and utils.windows_complete -- the host's statement of WHEN a window is emitted -- against
utils.window_bounds.  (StreamingLocalizer's constructor needs a device: its ValueError paths are in test_hip_stream_windows.py.)"""
import ctypes
import os

import numpy as np
import pytest

import csrc_build
from conftest import ROOT

from haghighatshoarmuir2024_amd import _lib
from haghighatshoarmuir2024_amd.utils import window_bounds, windows_complete

NAMES = ("micloc_stream_window_state_bytes", "micloc_stream_window_reset", "micloc_stream_localize_tile_windows_f64", "micloc_stream_window_count")


def test_abi_symbols_and_status_codes_without_a_gpu():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(raw, n) and f"{n}(" in header, n
    assert lib.micloc_abi_version() == 1  # additive
    vp = ctypes.c_void_p
    one = vp(256)  # non-null, 256-byte aligned, never dereferenced: validation comes first
    cnt = ctypes.c_int(-7)
    assert lib.micloc_stream_window_state_bytes(None, 1, 1024, 512, 8) == 0
    assert lib.micloc_stream_window_reset(None, 1, one, 1 << 20, 1024, 512, 8, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_localize_tile_windows_f64(None, one, one, 1 << 20, one, 1, 512, 0, None, None, one, 1 << 20, one, 1 << 20, 1024, 512, 8,
                                                       None, one, None, None, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_window_count(None, ctypes.byref(cnt), None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_window_count(one, None, None) == _lib.MICLOC_ERR_INVALID
    assert cnt.value == -7


def test_stream_windows_source_has_no_atomics_and_is_built():
    text = open(os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc", "stream_windows.hip")).read().lower()
    assert "atomic" not in text.replace("no atomics", "")
    assert "stream_window_kernel" in text
    assert "stream_windows.hip" in csrc_build.built_sources()


def test_windows_complete_hand_cases():
    # window = 1024, hop = 256, T = 1100: 2 windows, not the 5 that start before T
    assert len(window_bounds(1100, 1024, 256)[0]) == 2
    assert [windows_complete(f, 1024, 256) for f in (0, 256, 1023, 1024, 1279, 1280)] == [0, 0, 0, 1, 1, 2]
    assert windows_complete(1024, 1024, 256, T=1100) == 1   # the final tile has not been beamformed yet
    assert windows_complete(1100, 1024, 256, T=1100) == 2   # ... now it has: the leftover window of 844 frames, and no more
    # T <= window: nothing until the end, then the one window cut at T
    assert windows_complete(768, 1024, 512) == 0 and windows_complete(768, 1024, 512, T=1000) == 0
    assert windows_complete(1000, 1024, 512, T=1000) == 1 and windows_complete(1024, 1024, 512, T=1024) == 1
    assert windows_complete(4799, 5120, 256, T=4799) == 1 and windows_complete(4608, 5120, 256, T=4799) == 0
    # T = 1024, window = 512, hop = 256: an exact fit, 3 windows, each emitted with its last chunk
    assert [windows_complete(f, 512, 256, T=1024) for f in (0, 256, 512, 768, 1024)] == [0, 0, 1, 2, 3]
    assert windows_complete(1024, 512, 256) == 3
    assert windows_complete(4799, 1024, 512, T=4799) == 9 and windows_complete(4608, 1024, 512, T=4799) == 8
    assert windows_complete(512, 256) == 2  # hop defaults to window
    for bad in ((0, 0, 256), (0, 256, 0), (-1, 256, 256), (0, 256, 512), (0, 256, -256)):
        with pytest.raises(ValueError):
            windows_complete(*bad)
    with pytest.raises(ValueError):
        windows_complete(0, 256, 256, T=0)


def test_windows_complete_random_draws_against_window_bounds():
    rng = np.random.RandomState(0)
    for _ in range(200):
        q = int(rng.choice([256, 512]))
        window = q * int(rng.randint(1, 40))
        hop = q * int(rng.randint(1, window // q + 1))
        T = int(rng.randint(1, 60_000))
        start, stop = window_bounds(T, window, hop)
        assert windows_complete(T, window, hop, T=T) == len(start), (T, window, hop)
        # whole chunks become final one after the other, the ragged last one with the final tile: monotone, never more than the
        # rule holds, and window n is counted exactly from the frame at which its last frame is final
        frames = list(range(0, T, q)) + [T]
        counts = [windows_complete(f, window, hop, T=T) for f in frames]
        assert counts == sorted(counts) and counts[-1] == len(start), (T, window, hop)
        for f, c in zip(frames[:-1], counts[:-1]):
            assert c == int(np.sum(start + window <= f)) == windows_complete(f, window, hop), (T, window, hop, f)
