"""The library calls of ONE pushed tile, per streaming localizer (haghighatshoarmuir2024_amd/streaming.py): which entries of libmicloc_hip
push() goes through, and in which order.  The bit-for-bit tests of the streams would not notice an extra launch in a tile, or a status read
(a stream synchronisation) inside push(); this file pins the sequence.  The cached library handle is replaced by a proxy that forwards every
attribute and records its name; the tables below are written down from the tile protocol (include/micloc_hip.h, "streaming" and the
sections after it), `micloc_` omitted."""
import numpy as np
import pytest

from test_hip_stream_complex import beamformer, random_bf_mat
from test_hip_stream_music import _music
from test_hip_stream_wideband_complex import random_localizer
from test_hip_stream_windows import _beamformer

pytestmark = pytest.mark.gpu

FS = 48_000
B, M, G, T, TILE, WINDOW = 2, 7, 33, 1600, 320, 512
BANDS2 = [[1000.0, 1600.0], [1600.0, 2400.0]]

SNN = ["stream_begin_tile", "stht_f64", "stream_wrap_rows_f64", "stream_encode_tile_f64", "stream_localize_tile_f64"]
COMPLEX = ["stht_f64", "stream_wrap_rows_f64", "stream_complex_bandpass_tile_f64", "stream_complex_localize_tile_f64"]
WIDEBAND_SNN = ["filterbank_tile_f64"] + SNN * len(BANDS2) + ["stream_band_sum_f64"]
WIDEBAND_COMPLEX = ["filterbank_tile_f64", "stht_f64", "stream_wrap_rows_f64", "stream_complex_bands_bandpass_tile_f64",
                    "stream_complex_bands_localize_tile_f64"]
MUSIC = ["stream_music_tile_f64"]


def windowed(calls):
    """The list of a localizer built with window=: every localize entry is its _windows_f64 form, nothing else changes."""
    return [c.replace("localize_tile_f64", "localize_tile_windows_f64") for c in calls]


class _Recorder:
    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        self.log.append(name)
        return getattr(self._lib, name)


@pytest.fixture
def lib(monkeypatch):
    """The library handle every localizer built inside the test will hold: the real one behind a recording proxy."""
    from haghighatshoarmuir2024_amd import _lib

    rec = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "_lib", rec)
    return rec


# micloc_padded_T is integer arithmetic on the host (csrc/api_plan.hip: (T + 7) & ~7): it launches nothing and touches no stream, and the
# STHT front of a tile asks it for the row pitch.  It is the only entry left out of the comparison.
HOST_ARITHMETIC = {"micloc_padded_T"}


def calls_of_one_tile(lib, loc, x):
    lib.log.clear()
    loc.push(x[:, :TILE, :])
    assert not loc.done and loc.t == TILE
    assert all(c.startswith("micloc_") for c in lib.log), lib.log
    return [c[len("micloc_") :] for c in lib.log if c not in HOST_ARITHMETIC]


def _x(seed):
    return np.random.RandomState(seed).randn(B, T, M)


def _window_kw(with_window):
    return dict(window=WINDOW, hop=WINDOW) if with_window else {}


@pytest.mark.parametrize("with_window", [False, True], ids=["running", "windows"])
def test_streaming_localizer(lib, with_window):
    from haghighatshoarmuir2024_amd.streaming import StreamingLocalizer

    W = np.random.RandomState(1).randn(2 * M, G)
    loc = StreamingLocalizer(_beamformer(), W, B, T, max_tile=TILE, **_window_kw(with_window))
    assert calls_of_one_tile(lib, loc, _x(2)) == (windowed(SNN) if with_window else SNN)


@pytest.mark.parametrize("with_window", [False, True], ids=["running", "windows"])
def test_complex_streaming_localizer(lib, with_window):
    W = random_bf_mat(np.random.default_rng(3), M, G)
    loc = beamformer(M).streaming_localizer(W, batch=B, total_frames=T, max_tile=TILE, **_window_kw(with_window))
    assert calls_of_one_tile(lib, loc, _x(4)) == (windowed(COMPLEX) if with_window else COMPLEX)


@pytest.mark.parametrize("with_window", [False, True], ids=["running", "windows"])
def test_wideband_streaming_localizer(lib, with_window):
    from haghighatshoarmuir2024_amd.streaming import WidebandStreamingLocalizer
    from micloc.array_geometry import CenterCircularArray
    from micloc.filterbank import ButterworthFilterbank
    from micloc.snn_beamformer import SNNBeamformer
    from micloc.wideband import WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    beamfs = []
    for fr in BANDS2:
        tau = 1 / (2 * np.pi * np.mean(fr))
        beamfs.append(SNNBeamformer(geo, 10e-3, fr, [tau, tau], bipolar_spikes=True, fs=FS))
    rng = np.random.RandomState(5)
    wide = WidebandSNNLocalizer(beamfs, [rng.randn(2 * M, G) for _ in BANDS2], ButterworthFilterbank(freq_bands=BANDS2, order=1, fs=FS))
    loc = WidebandStreamingLocalizer(wide, B, T, max_tile=TILE, **_window_kw(with_window))
    assert len(loc.bands) == len(BANDS2)
    assert calls_of_one_tile(lib, loc, _x(6)) == (windowed(WIDEBAND_SNN) if with_window else WIDEBAND_SNN)


@pytest.mark.parametrize("with_window", [False, True], ids=["running", "windows"])
def test_wideband_complex_streaming_localizer(lib, with_window):
    loc = random_localizer(M, G, 7, bands=BANDS2).streaming_localizer(batch=B, total_frames=T, max_tile=TILE, **_window_kw(with_window))
    assert calls_of_one_tile(lib, loc, _x(8)) == (windowed(WIDEBAND_COMPLEX) if with_window else WIDEBAND_COMPLEX)


def test_music_streaming_localizer(lib):
    loc = _music(G=G, M=M).streaming_localizer(B, 1, 0.0, 128, total_frames=T, max_tile=TILE)
    assert calls_of_one_tile(lib, loc, _x(9)) == MUSIC
