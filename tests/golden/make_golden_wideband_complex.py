#!/usr/bin/env python3
"""Generate tests/golden/wideband_complex_packs.npz by running the *real* reference (build container only, like make_golden.py):

    MICLOC_REFERENCE=<checkout of the reference> python tests/golden/make_golden_wideband_complex.py

The wideband form of the complex Beamformer's live loop (micloc/localization_demo.py:43-89,158-182): an order-2 Butterworth
filterbank, per band the Beamformer designed on a sine at the band's centre, mean |y|^2 per band, the patterns added, one arg-max --
restated from the reference's own ButterworthFilterbank and Beamformer, because the module itself needs the sound card's recorder.
The packs are the three of wideband_packs.npz (make_golden_wideband.py) and are NOT stored again: only the reference's matrices and
the reference's results are written.
"""
import contextlib
import io
import os
import sys

REF = os.environ.get("MICLOC_REFERENCE", "")
if not REF or not os.path.isdir(REF):
    sys.exit("reference not present (MICLOC_REFERENCE): golden vectors can only be regenerated in the build container")
REF = os.path.abspath(REF)
sys.path.insert(0, REF)
# make sure the in-repo drop-in `micloc` shim does not shadow the reference package
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))]

import numpy as np  # noqa: E402

import micloc  # noqa: E402

assert os.path.abspath(micloc.__file__ if micloc.__file__ else list(micloc.__path__)[0]).startswith(REF), micloc

from micloc.array_geometry import CenterCircularArray  # noqa: E402
from micloc.beamformer import Beamformer  # noqa: E402
from micloc.filterbank import ButterworthFilterbank  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ORDER = 2  # micloc/localization_demo.py:80


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


def main():
    z = np.load(os.path.join(OUT, "wideband_packs.npz"))
    fs, rec, kd = int(z["fs"]), float(z["recording_duration"]), float(z["kernel_duration"])
    freq_bands, doa_list = z["freq_bands"], z["doa_list"]
    num_mic = z["packs16"].shape[2] - 1
    geometry = CenterCircularArray(radius=4.5e-2, num_mic=num_mic)
    beamfs, bf_mats = [], []
    t = np.arange(0, rec, step=1 / fs)
    for fr in freq_bands:
        fm = np.mean(fr)
        bfm = Beamformer(geometry=geometry, kernel_duration=kd, freq_range=fr, fs=fs)
        bf_vecs, _ = quiet(bfm.design_from_template, template=(t, np.sin(2 * np.pi * fm * t)), doa_list=doa_list)
        bf_mats.append(np.asarray(bf_vecs, dtype=np.complex128))
        beamfs.append(bfm)
    fb = ButterworthFilterbank(freq_bands=freq_bands, order=ORDER, fs=fs)
    packs = z["packs16"].astype(np.int32) << int(z["shift"])
    band_power = np.zeros((len(packs), len(freq_bands), len(doa_list)))
    power_grid = np.zeros((len(packs), len(doa_list)))
    for p, pack in enumerate(packs):
        data = np.asarray(pack[:, :-1], dtype=np.float64)
        data_filt = fb.evolve(sig_in=data)
        total = 0
        for f, (filt, W, bfm) in enumerate(zip(data_filt, bf_mats, beamfs)):
            y = bfm.apply_to_signal(bf_mat=W, sig_in=filt)
            band_power[p, f] = np.mean(np.abs(y) ** 2, axis=0)
            total = total + band_power[p, f]  # ((p_0 + p_1) + p_2): localization_demo.py:164-178
        power_grid[p] = total
        top = np.sort(total)[-2:]
        # the arg-max must not be a rounding matter
        assert (top[1] - top[0]) > 1e-6 * top[1], (p, top)
        print(f"pack {p}: relative gap of the two largest sums {(top[1] - top[0]) / top[1]:.2e}, per-band arg-max {np.argmax(band_power[p], axis=1)}")
    doa_index = np.argmax(power_grid, axis=1).astype(np.int64)
    path = os.path.join(OUT, "wideband_complex_packs.npz")
    np.savez_compressed(path, bf_mats=np.stack(bf_mats), band_power=band_power, power_grid=power_grid, doa_index=doa_index,
                        filterbank_order=np.int64(ORDER))
    print(f"wrote wideband_complex_packs.npz  ({os.path.getsize(path) / 1024:.0f} KiB)  doa_index {doa_index}")
    assert os.path.getsize(path) < 100_000


if __name__ == "__main__":
    main()
