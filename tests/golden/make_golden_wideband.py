#!/usr/bin/env python3
"""Generate tests/golden/wideband_packs.npz by running the *real* reference (build container only, like make_golden.py):

    python tests/golden/make_golden_wideband.py

The wideband form of the live demo's loop (micloc/localization_demo_snn.py:125-193; the band sum is :166-190): an order-1 Butterworth
filterbank, per band the SNNBeamformer designed for it, the angular power patterns added, one arg-max -- restated from the
reference's own ButterworthFilterbank and SNNBeamformer as gen_live_demo_frame (make_golden.py) does, because the module itself
needs the sound card's recorder.  Three bands with different filters, neuron kernels and matrices, three synthetic packs.
Only data is written: the packs, the reference's matrices and the reference's results.
"""
import contextlib
import io
import os
import sys

REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("reference not present: golden vectors can only be regenerated in the build container")
sys.path.insert(0, REF)
# make sure the in-repo drop-in `micloc` shim does not shadow the reference package
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))]

import numpy as np  # noqa: E402

import micloc  # noqa: E402

assert os.path.abspath(micloc.__file__ if micloc.__file__ else list(micloc.__path__)[0]).startswith(REF), micloc

from micloc.array_geometry import CenterCircularArray  # noqa: E402
from micloc.filterbank import ButterworthFilterbank  # noqa: E402
from micloc.snn_beamformer import SNNBeamformer  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
FS, NUM_MIC, REC = 48_000, 7, 0.1
FREQ_BANDS = [[1000, 1600], [1600, 2400], [2400, 3400]]
TONES = [1300.0, 2000.0, 2900.0]
# per pack: the direction of every band's tone (packs 0 and 1: one direction; pack 2: a different one per band)
PACK_DOAS = [[2.1, 2.1, 2.1], [-0.8, -0.8, -0.8], [0.6, -2.0, 2.7]]
NOISE, SEED = 0.4, 33


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def main():
    geometry = CenterCircularArray(radius=4.5e-2, num_mic=NUM_MIC)
    doa_list = np.linspace(-np.pi, np.pi, 16 * NUM_MIC)
    beamfs, bf_mats = [], []
    t = np.arange(0, REC, step=1 / FS)
    for fr in FREQ_BANDS:
        fm = np.mean(fr)
        tau = 1 / (2 * np.pi * fm)
        bfm = SNNBeamformer(geometry=geometry, kernel_duration=10e-3, freq_range=fr, tau_vec=[tau, tau], bipolar_spikes=True, fs=FS)
        bf_mats.append(quiet(bfm.design_from_template, template=(t, np.sin(2 * np.pi * fm * t)), doa_list=doa_list))
        beamfs.append(bfm)
    fb = ButterworthFilterbank(freq_bands=FREQ_BANDS, order=1, fs=FS)
    T = int(REC * FS)
    tt = np.arange(T) / FS
    rng = np.random.RandomState(SEED)
    packs16 = np.zeros((len(PACK_DOAS), T, NUM_MIC + 1), dtype=np.int16)  # the devkit's format: the last channel unused
    band_power = np.zeros((len(PACK_DOAS), len(FREQ_BANDS), len(doa_list)))
    power_grid = np.zeros((len(PACK_DOAS), len(doa_list)))
    for p, doas in enumerate(PACK_DOAS):
        sig = NOISE * rng.randn(T, NUM_MIC)
        for f0, doa in zip(TONES, doas):
            d = geometry.delays(doa, normalized=True)
            sig = sig + np.sin(2 * np.pi * f0 * (tt.reshape(-1, 1) - d.reshape(1, -1)))
        q = np.rint(sig * 4096)
        assert np.abs(q).max() < 32768
        packs16[p, :, :NUM_MIC] = q.astype(np.int16)
        pack = packs16[p].astype(np.int32) << 8  # what the tests restore
        data = np.asarray(pack[:, :-1], dtype=np.float64)
        assert np.sqrt(np.mean(data**2)) > 1e-4 * np.iinfo(np.int32).max
        data_filt = fb.evolve(sig_in=data)
        total = 0
        for f, (filt, W, bfm) in enumerate(zip(data_filt, bf_mats, beamfs)):
            y = bfm.apply_to_signal(bf_mat=W, sig_in_vec=(tt, filt))
            band_power[p, f] = np.mean(np.abs(y) ** 2, axis=0)
            total = total + band_power[p, f]  # ((p_0 + p_1) + p_2): localization_demo_snn.py:166-190
        power_grid[p] = total
        top = np.sort(total)[-2:]
        # the arg-max must not be a rounding matter: change PACK_DOAS or SEED until this holds
        assert (top[1] - top[0]) > 1e-6 * top[1], (p, top)
    doa_index = np.argmax(power_grid, axis=1).astype(np.int64)
    path = os.path.join(OUT, "wideband_packs.npz")
    np.savez_compressed(path, packs16=packs16, shift=np.int64(8), freq_bands=np.asarray(FREQ_BANDS, dtype=np.float64), doa_list=doa_list,
                        bf_mats=np.stack(bf_mats), band_power=band_power, power_grid=power_grid, doa_index=doa_index,
                        pack_doas=np.asarray(PACK_DOAS), tones=np.asarray(TONES), noise=np.float64(NOISE), seed=np.int64(SEED),
                        recording_duration=np.float64(REC), kernel_duration=np.float64(10e-3), fs=np.int64(FS))
    print(f"wrote wideband_packs.npz  ({os.path.getsize(path) / 1024:.0f} KiB)  doa_index {doa_index}")
    assert os.path.getsize(path) < 500_000


if __name__ == "__main__":
    main()
