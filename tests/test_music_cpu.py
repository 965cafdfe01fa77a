"""MUSIC host surface without a GPU: the drop-in alias, the constructor and its checks, array_response, the band-pass design and
the slice plan of apply_to_signal, against the reference's goldens (tests/golden/make_golden_music.py)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

from haghighatshoarmuir2024_amd.array_geometry import ArrayGeometry, CenterCircularArray

FS = 48_000


def _geo(z, pre):
    return ArrayGeometry(z[pre + "r_vec"], z[pre + "theta_vec"])


def test_alias_imports_the_implementation():
    import micloc.music_beamformer as alias

    from haghighatshoarmuir2024_amd import music_beamformer

    assert alias.MUSIC is music_beamformer.MUSIC


def test_constructor_attributes_without_a_device():
    from micloc.music_beamformer import MUSIC

    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    doa = np.linspace(-np.pi, np.pi, 57)
    m = MUSIC(geometry=geo, freq_range=[1600, 2400], doa_list=doa)
    assert m.frame_duration == 0.25 and m.fs == 48_000 and m.geometry is geo
    assert np.array_equal(m.freq_range, [1600, 2400]) and np.array_equal(m.doa_list, doa)
    assert len(m.filterbank) == 1
    with pytest.raises(ValueError):
        MUSIC(geometry=geo, freq_range=[2400, 1600], doa_list=doa)
    with pytest.raises(ValueError):
        MUSIC(geometry=geo, freq_range=[1600, 2000, 2400], doa_list=doa)


def test_host_checks_raise_before_any_device_work():
    from micloc.music_beamformer import MUSIC

    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    m = MUSIC(geometry=geo, freq_range=[1600, 2400], doa_list=np.linspace(-np.pi, np.pi, 57), frame_duration=0.05)
    x = np.zeros((4096, 7))
    with pytest.raises(ValueError, match="quite large"):
        m.beamforming(x, num_active_freq=35, num_fft_bin=2048)  # max_num_freq = int(800 / 23.4375) = 34
    with pytest.raises(ValueError, match="T x num_mic"):
        m.beamforming(np.zeros((4096, 6)), num_active_freq=1, num_fft_bin=2048)
    with pytest.raises(ValueError):
        m.beamforming(np.zeros((1000, 7)), num_active_freq=1, num_fft_bin=2048)  # T < N: the reference's broadcast ValueError
    with pytest.raises(ValueError, match="no FFT bin"):
        MUSIC(geometry=geo, freq_range=[1600, 1601], doa_list=[0.0]).beamforming(x, num_active_freq=0, num_fft_bin=64)
    with pytest.raises(ValueError, match="overlap"):
        m.apply_to_signal(x, num_active_freq=1, duration_overlap=0.05, num_fft_bin=512)
    with pytest.raises(ValueError, match="microphones"):
        m.apply_to_signal(np.zeros((4096, 5)), num_active_freq=1, duration_overlap=0.0, num_fft_bin=512)
    with pytest.raises(ValueError):
        m.apply_to_template(([0.0, 1.0], [0.0, 1.0]), num_active_freq=1, duration_overlap=0.0, num_fft_bin=512, snr_db=0.0)
    # no slice at all: the reference's empty result, without touching the device
    assert m.apply_to_signal(np.zeros((1000, 7)), num_active_freq=1, duration_overlap=0.0, num_fft_bin=512).shape == (0,)


def test_array_response_and_filter_match_the_reference():
    from micloc.music_beamformer import MUSIC

    z = np.load(os.path.join(GOLDEN, "music_beamforming.npz"))
    for i in range(int(z["num_cases"])):
        pre = f"c{i}_"
        m = MUSIC(geometry=_geo(z, pre), freq_range=list(z[pre + "band"]), doa_list=np.linspace(-np.pi, np.pi, int(z[pre + "G"])))
        b, a = m.filterbank.ba_list[0]
        assert np.array_equal(b, z[pre + "b"]) and np.array_equal(a, z[pre + "a"])
        if i == 0:
            assert np.array_equal(m.array_response(z["ar_freqs"]), z["array_response"])
        # the selected bins lie in the band of linspace(0, fs, N) (labels k fs / (N - 1))
        assert set(z[pre + "sel"]) <= set(m.in_band_bins(int(z[pre + "N"])))
        if int(z[pre + "k"]) in (0, len(m.in_band_bins(int(z[pre + "N"])))):
            assert sorted(z[pre + "sel"]) == list(m.in_band_bins(int(z[pre + "N"])))


def test_slice_plan_matches_the_reference():
    from micloc.music_beamformer import MUSIC

    z = np.load(os.path.join(GOLDEN, "music_apply_signal.npz"))
    geo = CenterCircularArray(radius=4.5e-2, num_mic=7)
    for i in range(int(z["num_cases"])):
        pre = f"c{i}_"
        m = MUSIC(geometry=geo, freq_range=[1000.0, 4000.0], doa_list=np.linspace(-np.pi, np.pi, 121), frame_duration=float(z[pre + "frame_duration"]))
        starts, lens, L, hop = m.slice_plan(int(z[pre + "T"]), float(z[pre + "overlap"]))
        assert np.array_equal(starts, z[pre + "starts"]) and np.array_equal(lens, z[pre + "lens"])
        assert np.array_equal(lens // int(z[pre + "N"]), z[pre + "F"])
        assert z[pre + "spectrum"].shape[0] == len(starts)
    # the scripts' shape: the resampled 1 s template (47 999 samples) is one leftover slice of 23 frames
    m = MUSIC(geometry=geo, freq_range=[1600, 2400], doa_list=np.linspace(-np.pi, np.pi, 57), frame_duration=1.0)
    starts, lens, L, hop = m.slice_plan(47_999, 0.0)
    assert list(starts) == [0] and list(lens) == [47_999] and lens[0] // 2048 == 23 and len(m.in_band_bins(2048)) == 34


def test_sweep_cli_offers_the_music_sweeps():
    from haghighatshoarmuir2024_amd import sweep

    with pytest.raises(SystemExit):
        sweep.main(["--sweep", "music-speech"])  # needs --flac or --pcm-npz: refused before any work
    assert callable(sweep.music_noisy_sweep) and callable(sweep.music_speech_sweep)
