#!/usr/bin/env python3
"""Generate tests/golden/windows.npz -- windowed power and arg-max -- by running the *real* reference beamformers.

Run in the build container only (the reference must be importable, with PYTHONPATH pointing at it):

    python tests/golden/make_golden_windows.py

Only numeric data is written: the reference's `apply_to_signal` output y [T, G], reduced per window of the rule in
include/micloc_hip.h to `mean(|y[s:e]|**2, axis=0)` and its arg-max.  The inputs are existing fixtures and are not stored again.

Cases
  a_*  the three config-2 noisy trials of trials_cfg2.npz through SNNBeamformer.apply_to_signal, window 1024, hop 512
       (9 windows, the last one 703 frames long)
  b_*  the moving-DoA trial of moving_target.npz (0.5 s, its quantised recording), window 2048, hop 1024: the arg-max moves
  c_*  the noisy trial of beamformer_c128_g449.npz through the complex Beamformer.apply_to_signal, window 1024, hop 512

The generator asserts that in every stored window the top-two relative margin of the reference's power exceeds 1e-9, so the
tests compare every arg-max without exclusions.
"""
import os
import sys

REF = os.environ.get("MICLOC_REFERENCE", "/root/reference")
if not os.path.isdir(REF):
    sys.exit("reference not present: golden vectors can only be regenerated in the build container")
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(os.path.join(HERE, "..", ".."))]

import numpy as np  # noqa: E402

import micloc  # noqa: E402

assert os.path.abspath(list(micloc.__path__)[0]).startswith(os.path.abspath(REF)), micloc

from micloc.array_geometry import CenterCircularArray  # noqa: E402
from micloc.beamformer import Beamformer  # noqa: E402
from micloc.snn_beamformer import SNNBeamformer  # noqa: E402

FS = 48_000
MARGIN = 1e-9


def bounds(T, window, hop):
    """The window rule (restated by utils.window_bounds in the package)."""
    nW = 1 if T <= window else 1 + -(-(T - window) // hop)
    start = np.arange(nW) * hop
    return start, np.minimum(start + window, T)


def windows(y, window, hop, what):
    start, stop = bounds(len(y), window, hop)
    p = np.stack([np.mean(np.abs(y[s:e]) ** 2, axis=0) for s, e in zip(start, stop)])
    top = np.sort(p, axis=1)[:, -2:]
    margin = (top[:, 1] - top[:, 0]) / top[:, 1]
    assert margin.min() > MARGIN, f"{what}: top-two margin {margin.min():.3g} in window {int(np.argmin(margin))}: choose another window"
    return p, np.argmax(p, axis=1), start, stop


def main():
    geometry = CenterCircularArray(radius=4.5e-2, num_mic=7)
    tau = 1.0 / (2 * np.pi * 2000)
    snn = SNNBeamformer(geometry=geometry, kernel_duration=10.0e-3, tau_vec=np.asarray([tau, tau]), freq_range=[1000.0, 2000.0], fs=FS,
                        bipolar_spikes=True)
    bf = np.load(os.path.join(HERE, "bf_mat_chirp449_bipolar.npz"))["bf_mat"]
    out = {}

    z = np.load(os.path.join(HERE, "trials_cfg2.npz"))
    pa, ia = [], []
    for i in range(3):
        y = snn.apply_to_signal(bf_mat=bf, sig_in_vec=(z["time0"], z["sig_in"][i]))
        np.testing.assert_allclose(np.mean(y**2, axis=0), z["power"][i], rtol=1e-12)  # the trial the fixture holds
        p, a, start, stop = windows(y, 1024, 512, f"a{i}")
        pa.append(p)
        ia.append(a)
    assert len(start) == 9 and stop[-1] - start[-1] == 703
    out.update(a_window=np.int64(1024), a_hop=np.int64(512), a_power=np.stack(pa), a_argmax=np.stack(ia), a_start=start, a_stop=stop)

    m = np.load(os.path.join(HERE, "moving_target.npz"))
    sig = m["trial_sig_q"].astype(np.float64) / 4096.0
    y = snn.apply_to_signal(bf_mat=bf, sig_in_vec=(m["trial_time"], sig))
    np.testing.assert_allclose(y[m["trial_rows"]], m["trial_y_rows"], rtol=0, atol=1e-13)
    p, a, start, stop = windows(y, 2048, 1024, "b")
    assert len(np.unique(a)) > 3, "the arg-max should move"
    out.update(b_window=np.int64(2048), b_hop=np.int64(1024), b_power=p, b_argmax=a, b_start=start, b_stop=stop)

    c = np.load(os.path.join(HERE, "beamformer_c128_g449.npz"))
    cbf = Beamformer(geometry=geometry, kernel_duration=10.0e-3, freq_range=[1000.0, 2000.0], fs=FS)
    y = cbf.apply_to_signal(bf_mat=c["bf_mat"], sig_in=c["sig_in"])
    np.testing.assert_allclose(np.mean(np.abs(y) ** 2, axis=0), c["power"], rtol=1e-12)
    p, a, start, stop = windows(y, 1024, 512, "c")
    out.update(c_window=np.int64(1024), c_hop=np.int64(512), c_power=p, c_argmax=a, c_start=start, c_stop=stop)

    path = os.path.join(HERE, "windows.npz")
    np.savez_compressed(path, **out)
    print(f"wrote windows.npz ({os.path.getsize(path) / 1024:.0f} KiB); b arg-max: {out['b_argmax']}")


if __name__ == "__main__":
    main()
