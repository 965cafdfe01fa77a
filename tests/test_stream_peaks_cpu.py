"""CPU checks of the streaming multi-source read-out (include/micloc_hip.h, "streaming, multi-source"): the C-ABI entries and the count
accessors, their status codes without a device, the Python refusals in front of any device work, the build entries, and the one rule for
the defaults that utils.find_doa_peaks and the streams share (utils.doa_peaks_defaults)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import csrc_build
from conftest import ROOT

from haghighatshoarmuir2024_amd import _lib, streaming, utils

CSRC = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
ENTRIES = {"micloc_stream_peaks_state_bytes": 0, "micloc_stream_peaks_reset": 3, "micloc_stream_peaks_tile_f64": 20, "micloc_stream_peaks_status": 3}
ACCESSORS = ("micloc_stream_bands_window_count_ptr", "micloc_stream_complex_bands_window_count_ptr", "micloc_stream_music_slice_count_ptr")
FS = 48_000


def test_header_declares_the_entries_and_the_accessors():
    header = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert "streaming, multi-source" in header
    for n, nargs in ENTRIES.items():
        assert f"{n}(" in header and n in _lib.SYMBOLS and hasattr(raw, n), n
        assert len(_lib.SYMBOLS[n][1]) == nargs <= 36, n
    for n in ACCESSORS + ("micloc_stream_window_count_ptr",):
        assert f"{n}(" in header and n in _lib.SYMBOLS and hasattr(raw, n), n
        assert _lib.SYMBOLS[n] == (ctypes.c_void_p, [ctypes.c_void_p]), n  # modelled on micloc_stream_window_count_ptr
    assert max(len(args) for _, args in _lib.SYMBOLS.values()) <= 36
    lib = _lib.load()
    assert lib.micloc_abi_version() == 1  # additive
    assert lib.micloc_stream_peaks_state_bytes() == 256
    assert 1 <= _lib.MICLOC_STREAM_PEAKS_SLOTS <= 64
    # the row rule is stated in the section, with the sentence that ties a peak row to the bits of its window row
    section = header.split("streaming, multi-source", 1)[1].split("---- misc", 1)[0]
    assert "is always the rule applied to the bits of row r of window_power" in " ".join(section.split()).replace("* ", "")


def test_accessors_are_plain_address_arithmetic():
    lib = _lib.load()
    base = 1 << 20
    assert lib.micloc_stream_bands_window_count_ptr(ctypes.c_void_p(base)) == base                 # word [0] of micloc_stream_bands_status
    assert lib.micloc_stream_music_slice_count_ptr(ctypes.c_void_p(base)) == base + 4             # word [1] of micloc_stream_music_status
    p = lib.micloc_stream_complex_bands_window_count_ptr(ctypes.c_void_p(base))
    assert base < p < base + 256 and p % 4 == 0                                                    # inside the window state's 256-B head
    assert lib.micloc_stream_music_slice_count_ptr(None) is None and lib.micloc_stream_complex_bands_window_count_ptr(None) is None


def test_tile_entry_status_codes_without_a_gpu():
    lib = _lib.load()
    vp = ctypes.c_void_p
    one = vp(256)  # non-null, 256-byte aligned, never dereferenced: validation comes first

    def tile(power=one, window_power=one, count=one, B=1, G=8, max_windows=4, doa=one, kind=_lib.MICLOC_GRID_LINEAR, K=2, sep=0.1, rel=0.0, st=one,
             nbytes=256, peaks=one, window_peaks=one):
        return lib.micloc_stream_peaks_tile_f64(power, window_power, count, B, G, max_windows, doa, kind, K, sep, rel, st, nbytes, peaks, one,
                                                window_peaks, one, one, one, None)

    INVALID, WORKSPACE = _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_WORKSPACE
    assert tile(doa=None) == INVALID
    assert tile(K=0) == INVALID and tile(K=17) == INVALID
    assert tile(G=0) == INVALID and tile(G=4097) == INVALID
    assert tile(sep=-0.5) == INVALID and tile(sep=float("nan")) == INVALID
    assert tile(rel=-0.5) == INVALID and tile(rel=float("nan")) == INVALID and tile(rel=float("inf")) == INVALID
    assert tile(max_windows=-1) == INVALID
    assert tile(kind=3) == INVALID and tile(kind=-1) == INVALID
    assert tile(B=0) == INVALID
    assert tile(power=None, window_power=None) == INVALID and tile(power=None, max_windows=0) == INVALID  # nothing to read
    assert tile(peaks=None) == INVALID and tile(count=None) == INVALID and tile(window_peaks=None) == INVALID
    # the limits come first: a bad K with a bad state is INVALID, a good call with a short or misaligned state is WORKSPACE
    assert tile(K=17, st=None, nbytes=0) == INVALID
    assert tile(st=None) == WORKSPACE and tile(nbytes=255) == WORKSPACE and tile(st=vp(264)) == WORKSPACE
    assert lib.micloc_stream_peaks_reset(None, 256, None) == INVALID
    assert lib.micloc_stream_peaks_reset(one, 255, None) == WORKSPACE and lib.micloc_stream_peaks_reset(vp(264), 256, None) == WORKSPACE
    st2 = (ctypes.c_int * 2)(-7, -7)
    assert lib.micloc_stream_peaks_status(None, st2, None) == INVALID and lib.micloc_stream_peaks_status(one, None, None) == INVALID
    assert list(st2) == [-7, -7]


def test_the_api_unit_and_the_kernel_are_built():
    assert os.path.exists(os.path.join(CSRC, "api_stream_peaks.hip")) and "__global__" not in open(os.path.join(CSRC, "api_stream_peaks.hip")).read()
    srcs = csrc_build.built_sources()
    assert "api_stream_peaks.hip" in srcs and "stream_peaks.hip" in srcs
    for f in ("peaks_rows.h", "stream_peaks.h", "stream_peaks.hip"):
        assert os.path.exists(os.path.join(CSRC, f)), f
    kernel = open(os.path.join(CSRC, "stream_peaks.hip")).read()
    assert "stream_peaks_kernel" in kernel and '#include "peaks_rows.h"' in kernel
    code = "\n".join(line.split("//")[0] for line in kernel.splitlines()).lower()
    assert "atomic" not in code and "hipstreamsynchronize" not in code and "hipdevicesynchronize" not in code
    # the row rule names its one exception, as readout_rows.h does
    head = open(os.path.join(CSRC, "peaks_rows.h")).read().split("#pragma once", 1)[0]
    assert "THE ONE EXCEPTION" in head and "peaks.hip" in head and "profiles/multisource/RECORD.json" in head


# ---- the Python refusals, in front of any device work --------------------------------------------------------------------------------------
def _no_device(monkeypatch):
    """Any attempt to reach the device from here on fails the test."""
    from haghighatshoarmuir2024_amd import runtime

    def boom(*a, **k):
        raise AssertionError("device work in front of a refusal")

    monkeypatch.setattr(runtime, "require_gpu", boom)
    monkeypatch.setattr(runtime.Plan, "__init__", boom)
    monkeypatch.setattr(runtime, "_as_dev", boom)


def _geo():
    from micloc.array_geometry import CenterCircularArray

    return CenterCircularArray(4.5e-2, 7)


G = 65
DOA = np.linspace(-np.pi, np.pi, G)
BAD = [(dict(num_sources=2), "doa_list"), (dict(num_sources=0, doa_list=DOA), "num_sources"), (dict(num_sources=17, doa_list=DOA), "num_sources"),
       (dict(num_sources=2, doa_list=DOA[:-1]), "doa_list has 64"), (dict(num_sources=2, doa_list=DOA, min_separation=-0.1), "min_separation"),
       (dict(num_sources=2, doa_list=DOA, rel_threshold=-1.0), "rel_threshold"), (dict(min_separation=0.1), "give num_sources")]


@pytest.mark.parametrize("kw,match", BAD, ids=[m for _, m in BAD])
def test_single_band_streams_refuse_before_any_device_work(kw, match, monkeypatch):
    from micloc.beamformer import Beamformer
    from micloc.snn_beamformer import SNNBeamformer

    tau = 1 / (2 * np.pi * 2000)
    snn = SNNBeamformer(_geo(), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)
    cpx = Beamformer(_geo(), 10e-3, [1000.0, 2000.0], fs=FS)
    rng = np.random.RandomState(0)
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match=match):
        snn.streaming_localizer(rng.randn(14, G), batch=2, **kw)
    with pytest.raises(ValueError, match=match):
        cpx.streaming_localizer(rng.randn(7, G) + 1j * rng.randn(7, G), batch=2, **kw)


@pytest.mark.parametrize("kw,match", BAD, ids=[m for _, m in BAD])
def test_wideband_streams_refuse_before_any_device_work(kw, match, monkeypatch):
    from micloc.beamformer import Beamformer
    from micloc.filterbank import ButterworthFilterbank
    from micloc.snn_beamformer import SNNBeamformer
    from micloc.wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

    bands = [[1000.0, 1600.0], [1600.0, 2400.0]]
    rng = np.random.RandomState(1)
    cpx = WidebandBeamformerLocalizer([Beamformer(_geo(), 10e-3, fr, fs=FS) for fr in bands], [rng.randn(7, G) + 1j * rng.randn(7, G) for _ in bands],
                                      ButterworthFilterbank(freq_bands=bands, order=2, fs=FS))
    taus = [1 / (2 * np.pi * np.mean(fr)) for fr in bands]
    snn = WidebandSNNLocalizer([SNNBeamformer(_geo(), 10e-3, fr, np.asarray([t, t]), bipolar_spikes=True, fs=FS) for fr, t in zip(bands, taus)],
                               [rng.randn(14, G) for _ in bands], ButterworthFilterbank(freq_bands=bands, order=1, fs=FS))
    _no_device(monkeypatch)
    for loc in (cpx, snn):
        assert not hasattr(loc, "doa_list")
        with pytest.raises(ValueError, match=match):
            loc.streaming_localizer(batch=2, **kw)
    # the localizer's own grid is the default, as in localize_batch: a grid of the wrong length is still refused
    cpx.doa_list = DOA[:-1]
    with pytest.raises(ValueError, match="doa_list has 64"):
        cpx.streaming_localizer(batch=2, num_sources=2)


def test_music_stream_refuses_before_any_device_work(monkeypatch):
    from micloc.music_beamformer import MUSIC

    m = MUSIC(geometry=_geo(), freq_range=[1000.0, 2000.0], doa_list=np.linspace(-np.pi, np.pi, 33), frame_duration=512 / 8000, fs=8000)
    _no_device(monkeypatch)
    for kw, match in ((dict(num_sources=0), "num_sources"), (dict(num_sources=17), "num_sources"), (dict(num_sources=2, min_separation=-1.0), "min_separation"),
                      (dict(num_sources=2, rel_threshold=float("nan")), "rel_threshold"), (dict(min_separation=0.2), "give num_sources")):
        with pytest.raises(ValueError, match=match):
            m.streaming_localizer(2, 1, 0.0, 128, **kw)
    assert "doa_list" not in inspect.signature(streaming.MusicStreamingLocalizer.__init__).parameters  # the grid is music.doa_list
    with pytest.raises(TypeError):
        m.streaming_localizer(2, 1, 0.0, 128, num_sources=2, doa_list=np.linspace(-np.pi, np.pi, 33))


def test_the_xylo_stream_takes_no_num_sources():
    params = inspect.signature(streaming.XyloStreamingLocalizer.__init__).parameters
    for name in ("num_sources", "doa_list", "min_separation", "rel_threshold"):
        assert name not in params, name
    with pytest.raises(TypeError, match="num_sources"):
        streaming.XyloStreamingLocalizer(None, 1, num_sources=2)
    for cls in (streaming.StreamingLocalizer, streaming.ComplexStreamingLocalizer, streaming.WidebandStreamingLocalizer,
                streaming.WidebandComplexStreamingLocalizer):
        p = inspect.signature(cls.__init__).parameters
        assert all(n in p for n in ("num_sources", "doa_list", "min_separation", "rel_threshold")) and "track" in p, cls.__name__
    for name in ("_set_peaks", "_alloc_peaks", "_peaks_tile", "latest_peaks", "peaks_status"):
        assert callable(getattr(streaming._TileStream, name)), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "XyloStreamingLocalizer takes no num_sources" in design


# ---- one rule for the defaults ---------------------------------------------------------------------------------------------------------------
def _old_defaults(doa_list, num_sources, min_separation=None, grid=None):
    """find_doa_peaks' lines as they stood before the helper, restated."""
    doa = np.asarray(doa_list, dtype=np.float64)
    if doa.ndim != 1:
        raise ValueError("doa_list should be 1-dim!")
    K = int(num_sources)
    if not 1 <= K <= 16:
        raise ValueError("num_sources must be between 1 and 16")
    if grid is None:
        grid = utils.doa_grid_kind(doa)
    if min_separation is None:
        min_separation = 2 * abs(doa[-1] - doa[0]) / (len(doa) - 1) if len(doa) > 1 else 0.0
    return doa, K, grid, min_separation


def test_the_defaults_helper_gives_find_doa_peaks_old_values():
    grids = {"circular_closed": np.linspace(-np.pi, np.pi, 65), "circular": np.arange(64) * (2 * np.pi / 64), "linear": np.linspace(0.0, 1.0, 9)}
    for kind, doa in grids.items():
        for K in (1, 2, 16):
            got, want = utils.doa_peaks_defaults(doa, K), _old_defaults(doa, K)
            assert got[1:3] == want[1:3] == (K, kind)
            assert np.array_equal(got[0], want[0]) and got[0].dtype == np.float64
            assert np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes() == np.float64(2 * abs(doa[-1] - doa[0]) / (len(doa) - 1)).tobytes()
        # what the caller names is kept
        assert utils.doa_peaks_defaults(doa, 3, min_separation=0.25, grid="linear")[2:] == ("linear", 0.25)
        assert utils.doa_peaks_defaults(list(doa), 3)[2] == kind
    assert utils.doa_peaks_defaults([0.5], 1)[2:] == ("linear", 0.0)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="num_sources"):
            utils.doa_peaks_defaults(grids["linear"], bad)
    with pytest.raises(ValueError, match="1-dim"):
        utils.doa_peaks_defaults(np.zeros((3, 3)), 2)
    # find_doa_peaks itself goes through the helper
    assert "doa_peaks_defaults(" in inspect.getsource(utils.find_doa_peaks)
    assert "doa_peaks_defaults(" in inspect.getsource(streaming._TileStream._set_peaks)


def test_sweep_has_the_stream_localizer_and_the_command_line_flag():
    from haghighatshoarmuir2024_amd import sweep

    sig = inspect.signature(sweep.stream_multi_localizer)
    assert list(sig.parameters) == ["beamf", "bf_mat", "doa_list", "tile", "num_sources", "min_separation", "rel_threshold", "max_batch"]
    assert sig.parameters["min_separation"].default is None and sig.parameters["rel_threshold"].default == 0.0 and sig.parameters["max_batch"].default == 1100
    with pytest.raises(ValueError, match="tile"):
        sweep.stream_multi_localizer(None, None, DOA, 0, 2)
    with pytest.raises(SystemExit):
        sweep.main(["--sweep", "noisy", "--stream-tile", "1024"])
    with pytest.raises(SystemExit):
        sweep.main(["--sweep", "multi-noisy", "--method", "music", "--stream-tile", "1024"])
