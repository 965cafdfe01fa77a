"""The host side of the MUSIC stream and of localization_demo_MUSIC.Demo, without a GPU: the slice rule's host mirror against
MUSIC.slice_plan, the ValueErrors, the host estimators against the reference's (tests/golden/make_golden_music_demo.py), the alias, the
argument checks of the four C entries."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN

from haghighatshoarmuir2024_amd import _lib
from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
from haghighatshoarmuir2024_amd.localization_demo_MUSIC import Demo
from haghighatshoarmuir2024_amd.music_beamformer import MUSIC
from haghighatshoarmuir2024_amd.streaming import MusicStreamingLocalizer, _TileStream

FS = 48_000


def _geo():
    return CenterCircularArray(radius=4.5e-2, num_mic=7)


def _demo(k=20, **kw):
    return Demo(geometry=_geo(), freq_range=np.asarray([1200, 2000]), num_active_freq=k, doa_list=np.linspace(-np.pi, np.pi, 225), **kw)


@pytest.mark.parametrize("L,hop", [(8, 8), (8, 3), (8, 1), (9, 4), (12, 7), (10, 5)])
def test_host_mirror_of_the_slice_rule_agrees_with_slice_plan(L, hop):
    fs = 1024  # (a power of two: fs * duration is exact)
    m = MUSIC(geometry=_geo(), freq_range=[100.0, 200.0], doa_list=np.linspace(-np.pi, np.pi, 9), frame_duration=L / fs, fs=fs)
    for T in range(1, 4 * L + 1):
        starts, lens, L_, hop_ = m.slice_plan(T, (L - hop) / fs)
        assert (L_, hop_) == (L, hop)
        full, left = MusicStreamingLocalizer.slices_of(T, L, hop)
        exp = [(s * hop, L) for s in range(full)] + ([left] if left is not None else [])
        assert exp == list(zip(starts.tolist(), lens.tolist())), (T, exp, starts, lens)
        assert left is None or (left[0] == full * hop and left[0] + left[1] == T and left[1] < L)
        assert MusicStreamingLocalizer.slice_count(T, L, hop) == len(starts)


def test_the_constructor_raises_localize_batchs_value_errors_without_a_device():
    m = MUSIC(geometry=_geo(), freq_range=[1200.0, 2000.0], doa_list=np.linspace(-np.pi, np.pi, 33), frame_duration=0.25, fs=FS)
    with pytest.raises(ValueError, match="number of frequencies is quite large"):
        m.streaming_localizer(1, 100, 0.0, 2048)  # the reference's run_demo defaults: 34 are allowed
    with pytest.raises(ValueError, match="num_active_freq must be >= 0"):
        m.streaming_localizer(1, -1, 0.0, 2048)
    with pytest.raises(ValueError, match="duration of overlap window is larger"):
        m.streaming_localizer(1, 20, 0.25, 2048)
    with pytest.raises(ValueError, match="shorter than the FFT length"):
        m.streaming_localizer(1, 20, 0.0, 16384)  # N > L
    with pytest.raises(ValueError, match="a signal slice of 7000 samples is shorter than the FFT length 8192"):
        m.streaming_localizer(1, 20, 0.0, 8192, total_frames=12_000 + 7000)  # the leftover slice, known in advance
    with pytest.raises(ValueError, match="max_windows must be at least 1"):
        m.streaming_localizer(1, 20, 0.0, 2048, max_slices=0)
    empty = MUSIC(geometry=_geo(), freq_range=[1200.0, 1201.0], doa_list=np.linspace(-np.pi, np.pi, 33), frame_duration=0.25, fs=FS)
    with pytest.raises(ValueError, match="no FFT bin lies in the frequency range"):
        empty.streaming_localizer(1, 0, 0.0, 2048)
    assert issubclass(MusicStreamingLocalizer, _TileStream) and MusicStreamingLocalizer.TILE_MULTIPLE == 1
    for name in ("push", "push_replay", "status", "latest_window", "windows", "finish"):
        assert callable(getattr(MusicStreamingLocalizer, name))


def test_demo_has_the_reference_attributes_and_fails_like_it_on_its_own_defaults():
    d = _demo()
    assert isinstance(d.music, MUSIC) and d.music.frame_duration == 0.25
    assert (d.num_active_freq, d.recording_duration, d.num_fft_bin, d.fs) == (20, 0.25, 2048, 48_000)
    assert len(d.doa_list) == 225
    for name in ("estimate_doa", "process_frame", "process_frames", "run", "streaming_localizer"):
        assert callable(getattr(Demo, name))
    # the reference's run_demo(): 100 active frequencies in 1200-2000 Hz at N = 2048 -- beamforming's check fails on the first frame,
    # here as there; nothing is clamped
    ref_defaults = _demo(k=100)
    pack = np.zeros((12_000, 8), dtype=np.int32)
    pack[:, :7] = 1 << 24
    with pytest.raises(ValueError, match="number of frequencies is quite large"):
        ref_defaults.process_frame(pack)
    with pytest.raises(ValueError, match="number of frequencies is quite large"):
        ref_defaults.process_frames(pack[None])
    with pytest.raises(ValueError, match="number of frequencies is quite large"):
        ref_defaults.streaming_localizer()
    # a silent pack never reaches the device
    assert np.isnan(d.process_frame(np.zeros((12_000, 8), dtype=np.int32)))
    assert np.isnan(d.process_frames(np.zeros((2, 12_000, 8), dtype=np.int32))).all()
    with pytest.raises(ValueError, match="only the following estimation methods are supported"):
        d.estimate_doa(np.ones(225), "median")


def test_estimate_doa_reproduces_the_reference():
    z = np.load(os.path.join(GOLDEN, "music_demo.npz"))
    d = _demo(k=int(z["k"]))
    methods = [str(m) for m in z["methods"]]
    assert methods == ["peak", "periodic_ml", "trimmed_periodic_ml"]
    raised = 0
    for specs, doas, errs in ((z["ang_pow_spec"], z["doa"], z["doa_index_error"]), (z["syn_spectrum"], z["syn_doa"], z["syn_index_error"])):
        for spec, doa, err in zip(specs, doas, errs):
            for i, m in enumerate(methods):
                if err[i]:
                    raised += 1
                    with pytest.raises(IndexError):
                        d.estimate_doa(spec, m)
                else:
                    assert d.estimate_doa(spec, m) == doa[i], (m, d.estimate_doa(spec, m), doa[i])  # the same NumPy expressions: the same bits
    assert raised == 1 and z["syn_index_error"][1, 2] == 1


def test_alias_imports():
    import micloc.localization_demo_MUSIC

    import haghighatshoarmuir2024_amd

    assert micloc.localization_demo_MUSIC.Demo is Demo
    assert "localization_demo_MUSIC" in haghighatshoarmuir2024_amd.__all__


def test_the_entries_check_their_arguments_before_the_device():
    lib = _lib.load()
    for name in ("micloc_stream_music_state_bytes", "micloc_stream_music_reset", "micloc_stream_music_tile_f64", "micloc_stream_music_status"):
        assert name in _lib.SYMBOLS
    good = dict(B=2, M=7, L=512, hop=128, N=128, nbin=17, G=33, k=3, max_slices=4)
    size = lib.micloc_stream_music_state_bytes(*good.values())
    assert size > 0 and size % 256 == 0
    # K = ceil(L / hop) + 1 = 5 slots: the state grows with the slots, not with max_slices
    assert lib.micloc_stream_music_state_bytes(*{**good, "max_slices": 400}.values()) == size
    assert lib.micloc_stream_music_state_bytes(*{**good, "hop": 512}.values()) < size
    bad = [("hop", 0, _lib.MICLOC_ERR_INVALID), ("hop", 513, _lib.MICLOC_ERR_SHAPE), ("N", 513, _lib.MICLOC_ERR_SHAPE), ("k", 18, _lib.MICLOC_ERR_SHAPE),
           ("k", -1, _lib.MICLOC_ERR_INVALID), ("B", 0, _lib.MICLOC_ERR_INVALID), ("max_slices", 0, _lib.MICLOC_ERR_INVALID),
           ("nbin", 129, _lib.MICLOC_ERR_SHAPE), ("G", 0, _lib.MICLOC_ERR_INVALID)]
    buf = (ctypes.c_char * 4096)()
    addr = (ctypes.addressof(buf) + 255) & ~255  # an aligned host address: no entry may reach the device with these arguments
    ba = np.array([1.0, 0.5]), np.array([1.0, 0.25])
    bp, ap = (a.ctypes.data_as(_lib.c_double_p) for a in ba)

    def tile(state=addr, nbytes=size, x=addr, n=16, ncoef=2, W=addr, sre=addr, sim=addr, **kw):
        g = {**good, **kw}
        return lib.micloc_stream_music_tile_f64(state, nbytes, x, g["B"], n, g["M"], 0, bp, ap, ncoef, g["L"], g["hop"], g["N"], W, g["nbin"], sre, sim,
                                                g["G"], g["k"], g["max_slices"], None, None, None, None, None, None, None, None)

    for key, value, code in bad:
        args = {**good, key: value}
        assert lib.micloc_stream_music_state_bytes(*args.values()) == 0, key
        assert lib.micloc_stream_music_reset(addr, size, *args.values(), None) == code, key
        assert tile(**{key: value}) == code, key
    assert lib.micloc_stream_music_reset(None, size, *good.values(), None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_music_reset(addr, size - 1, *good.values(), None) == _lib.MICLOC_ERR_WORKSPACE
    assert lib.micloc_stream_music_reset(addr + 8, size, *good.values(), None) == _lib.MICLOC_ERR_WORKSPACE
    for kw in (dict(state=None), dict(x=None), dict(W=None), dict(sre=None), dict(sim=None), dict(n=0), dict(ncoef=0), dict(ncoef=10)):
        assert tile(**kw) == _lib.MICLOC_ERR_INVALID, kw
    assert tile(nbytes=size - 256) == _lib.MICLOC_ERR_WORKSPACE
    st4 = (ctypes.c_int * 4)()
    assert lib.micloc_stream_music_status(None, st4, None) == _lib.MICLOC_ERR_INVALID
    assert lib.micloc_stream_music_status(addr, None, None) == _lib.MICLOC_ERR_INVALID
