#!/usr/bin/env python3
"""Generate tests/golden/multi_targets.npz by running the *real* reference: its classes (`micloc.snn_beamformer.SNNBeamformer`,
`micloc.beamformer.Beamformer`, `micloc.music_beamformer.MUSIC`) and the `signal_multiple_targets` of its multi-target scripts
(paper_plots/multiple_targets_snn.py, multiple_targets_beamformer.py, multiple_targets_music.py), with the scripts' parameters.

Run in the build container only (the reference must be importable, with PYTHONPATH pointing at it):

    python tests/golden/make_golden_multitarget.py

Only numbers are written.  Per case (prefix `<method>_<scenario>_<freq>_`): the reference's `bf_mat` (SNN [14, 225] real, Beamformer
[7, 225] complex; MUSIC has none), the unnormalised `power_bf = np.mean(np.abs(sig_bf) ** 2, axis=0)` (the scripts divide it by its
maximum for the plot), and `peaks`: the two indices the multi-source rule (include/micloc_hip.h, restated in tests/multisource_ref.py)
picks on that power with its default separation of two grid steps.  Scenarios:
  sin       x(t) = sin(2 pi f t), 0.4 s, f = 1 and 2 kHz, targets at -60 and +60 deg with gains (1, 1), 225-point closed grid
  wideband  (SNN, 2 kHz centre) the script's band-passed white noise (butter(2, [1.5, 2.5] kHz) on randn(T)); the script draws it
            from the unseeded global stream -- here after np.random.seed(WIDEBAND_SEED), recorded as `wideband_seed`
Each script synthesises with its own copy of `signal_multiple_targets`; the MUSIC script's copy delays with `time - delays`, the other
two with `time + delays`, and each case is generated with its script's copy.
The coherent targets do not always show as two peaks: the file records what the reference produces.
"""
import importlib.util
import os
import sys

REF = os.environ.get("MICLOC_REFERENCE", "/root/reference")
if not os.path.isdir(REF):
    sys.exit("reference not present: golden vectors can only be regenerated in the build container")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(os.path.join(HERE, "..", ".."))]

import numpy as np  # noqa: E402
from scipy.signal import butter, lfilter  # noqa: E402

import micloc  # noqa: E402

assert os.path.abspath(list(micloc.__path__)[0]).startswith(os.path.abspath(REF)), micloc

from micloc.array_geometry import CenterCircularArray  # noqa: E402
from micloc.beamformer import Beamformer  # noqa: E402
from micloc.music_beamformer import MUSIC  # noqa: E402
from micloc.snn_beamformer import SNNBeamformer  # noqa: E402

sys.path.insert(0, os.path.join(HERE, ".."))
import multisource_ref as R  # noqa: E402

FS = 48_000
DURATION = 0.4
FREQS = (1000, 2000)
DOA_TARGETS = np.asarray([-np.pi / 3, np.pi / 3])
POWER_TARGETS = np.asarray([1, 1])
WIDEBAND_SEED = 20240
WIDEBAND_CENTER = 2000
BANDWIDTH = 1000


def _script_fn(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "paper_plots", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.signal_multiple_targets


def _targets(fn, geometry, time_temp, sig_temp):
    T = len(sig_temp)
    return fn(geometry=geometry, time_temp=time_temp, sig_temp=sig_temp, doa_timeseries_targets=np.ones((T, 1)) * DOA_TARGETS.reshape(1, -1),
              power_timeseries_targets=np.ones((T, 1)) * POWER_TARGETS.reshape(1, -1))


def main():
    geometry = CenterCircularArray(radius=4.5e-2, num_mic=7)
    doa_list = np.linspace(-np.pi, np.pi, 32 * 7 + 1)
    time_temp = np.arange(0, DURATION, step=1 / FS)
    out = dict(doa_list=doa_list, doa_targets=DOA_TARGETS, power_targets=POWER_TARGETS.astype(np.float64), fs=FS, duration=DURATION,
               freqs=np.asarray(FREQS), r_vec=geometry.r_vec, theta_vec=geometry.theta_vec, wideband_seed=WIDEBAND_SEED,
               wideband_center=WIDEBAND_CENTER, bandwidth=BANDWIDTH)

    def record(pre, power, bf_mat=None):
        out[pre + "power_bf"] = power
        out[pre + "peaks"] = R.peaks(power, doa_list, 2)[0][0]
        if bf_mat is not None:
            out[pre + "bf_mat"] = bf_mat
        print(pre, "peaks", out[pre + "peaks"], np.rad2deg(doa_list[out[pre + "peaks"]]))

    snn_sig, bf_sig, mu_sig = (_script_fn(n) for n in ("multiple_targets_snn", "multiple_targets_beamformer", "multiple_targets_music"))
    for f in FREQS:
        sig_temp = np.sin(2 * np.pi * f * time_temp)
        # multiple_targets_snn.py:snn_multiple_targets_sin
        tau = 1 / (2 * np.pi * f)
        beamf = SNNBeamformer(geometry=geometry, kernel_duration=10e-3, freq_range=np.array([f / 2, 2 * f]), tau_vec=np.asarray([tau, tau]),
                              bipolar_spikes=True, fs=FS)
        bf_mat = beamf.design_from_template(template=(time_temp, sig_temp), doa_list=doa_list)
        sig_in = _targets(snn_sig, geometry, time_temp, sig_temp)
        sig_bf = beamf.apply_to_signal(bf_mat=bf_mat, sig_in_vec=(time_temp, sig_in))
        record(f"snn_sin_{f}_", np.mean(np.abs(sig_bf) ** 2, axis=0), bf_mat)
        # multiple_targets_beamformer.py:beamformer_multiple_targets_sin
        cbf = Beamformer(geometry=geometry, kernel_duration=10e-3, freq_range=[f / 2, 2 * f], fs=FS)
        bf_mat, _ = cbf.design_from_template(template=(time_temp, sig_temp), doa_list=doa_list)
        sig_in = _targets(bf_sig, geometry, time_temp, sig_temp)
        sig_bf = cbf.apply_to_signal(bf_mat=bf_mat, sig_in=sig_in)
        record(f"beamformer_sin_{f}_", np.mean(np.abs(sig_bf) ** 2, axis=0), bf_mat)
        # multiple_targets_music.py:music_multiple_targets_sin
        music = MUSIC(geometry=geometry, freq_range=np.asarray([f / 2, 2 * f]), doa_list=doa_list, frame_duration=DURATION, fs=FS)
        sig_in = _targets(mu_sig, geometry, time_temp, sig_temp)
        sig_bf = music.apply_to_signal(sig_in=sig_in, num_active_freq=1, duration_overlap=0.0, num_fft_bin=2048)
        record(f"music_sin_{f}_", np.mean(np.abs(sig_bf) ** 2, axis=0))

    # multiple_targets_snn.py:snn_multiple_targets_wideband at the 2 kHz centre, seeded
    c = WIDEBAND_CENTER
    tau = 1 / (2 * np.pi * c)
    freq_range = np.asarray([c - BANDWIDTH / 2, c + BANDWIDTH / 2])
    b, a = butter(2, freq_range, btype="pass", analog=False, output="ba", fs=FS)
    np.random.seed(WIDEBAND_SEED)
    sig_temp = lfilter(b, a, np.random.randn(len(time_temp)))
    beamf = SNNBeamformer(geometry=geometry, kernel_duration=10e-3, freq_range=freq_range, tau_vec=np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)
    bf_mat = beamf.design_from_template(template=(time_temp, sig_temp), doa_list=doa_list)
    sig_in = _targets(snn_sig, geometry, time_temp, sig_temp)
    sig_bf = beamf.apply_to_signal(bf_mat=bf_mat, sig_in_vec=(time_temp, sig_in))
    record(f"snn_wideband_{c}_", np.mean(np.abs(sig_bf) ** 2, axis=0), bf_mat)

    path = os.path.join(HERE, "multi_targets.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
