"""Time the MUSIC kernels at the two sweep shapes of paper_plots/target_localization_MUSIC.py.

python tools/music_time.py [noisy|speech|both] -- average time of one MUSIC.localize_batch launch chain over 10 launches (HIP events on
the launch stream), and the band-limited DFT's algorithmic fp64 rate (2 x rows x N x 2 nbin flop) over the whole chain.  Per-kernel
times (music_filter_kernel, music_dft_kernel, music_select_kernel, music_steer_kernel, music_readout_kernel): run this under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/music_time.py`; the DFT's share of the 78.6 TFLOP/s fp64 matrix peak is
its flop count (printed here) over its kernel time.
  noisy:  1100 trials x 47 999 samples, 7 mics, 1 slice of 23 frames, N = 2048, 34 bins, 57 DoAs, k = 1
  speech:  100 trials x 332 159 samples, 7 mics, 7 slices (6 x 23 + 1 x 21 frames), N = 2048, 34 bins, 449 DoAs, k = 1
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray  # noqa: E402
from haghighatshoarmuir2024_amd.music_beamformer import MUSIC  # noqa: E402

SHAPES = {"noisy": (1100, 47_999, 57), "speech": (100, 332_159, 449)}


def run(name):
    B, T, G = SHAPES[name]
    N, fs = 2048, 48_000
    m = MUSIC(CenterCircularArray(4.5e-2, 7), [1600.0, 2400.0], np.linspace(-np.pi, np.pi, G), frame_duration=1.0, fs=fs)
    starts, lens, L, hop = m.slice_plan(T, 0.0)
    x = torch.randn((B, T, 7), dtype=torch.float64, device="cuda")
    for _ in range(3):
        out = m.localize_batch(x, 1, 0.0, N, want_spectrum=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 10
    e0.record()
    for _ in range(n):
        out = m.localize_batch(x, 1, 0.0, N, want_spectrum=False)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    nbin = len(m.in_band_bins(N))
    rows = B * len(starts) * 7 * int(lens.max() // N)
    flop = 2.0 * rows * N * 2 * nbin
    print(f"music {name}: B={B} T={T} S={len(starts)} F={list(lens // N)} nbin={nbin} G={G}: {ms:.3f} ms per localize_batch "
          f"({ms / B * 1e3:.2f} us per trial); DFT {flop / 1e9:.1f} GFLOP, {B * T * 7 * 8 / 1e9:.2f} GB input; "
          f"DFT flop over the whole chain {flop / ms / 1e9:.2f} TFLOP/s = {flop / ms / 1e9 / 78.6:.3f} of 78.6; argmax[0]={int(out['argmax'][0])}")


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    for name in (["noisy", "speech"] if which == "both" else [which]):
        run(name)
