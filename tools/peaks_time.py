"""Time the multi-source read-out (micloc_doa_peaks_f64, `doa_peaks_kernel`) at the noisy sweep's shape.

python tools/peaks_time.py [B] [G] [K] -- average time of one runtime.doa_peaks launch over 20 launches (HIP events on the launch stream)
for B rows of G DoAs (default 1100 x 449, the 11 SNRs x 100 trials of one sweep step), K peaks (default 2), the closed grid
np.linspace(-pi, pi, G), two grid steps of separation.  Per-kernel time: run this under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/peaks_time.py`.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from haghighatshoarmuir2024_amd import runtime  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 1100
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 449
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    doa = np.linspace(-np.pi, np.pi, G)
    # a profile of two bumps plus noise per row: a few dozen local maxima, as a noisy beamformer power has
    rng = np.random.RandomState(0)
    x = np.arange(G)
    c = rng.randint(0, G, size=(B, 2))
    p = np.exp(-0.5 * ((x[None] - c[:, :1]) / 10.0) ** 2) + np.exp(-0.5 * ((x[None] - c[:, 1:]) / 10.0) ** 2) + 0.05 * rng.rand(B, G)
    power = torch.from_numpy(p).cuda()
    d = torch.from_numpy(doa).cuda()
    sep = 2 * (2 * np.pi / (G - 1))
    idx = torch.empty((B, K), dtype=torch.int32, device="cuda")
    val = torch.empty((B, K), dtype=torch.float64, device="cuda")
    for _ in range(3):
        runtime.doa_peaks(power, d, "circular_closed", K, sep, index_out=idx, value_out=val)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    e0.record()
    for _ in range(n):
        runtime.doa_peaks(power, d, "circular_closed", K, sep, index_out=idx, value_out=val)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    print(f"doa_peaks: B={B} G={G} K={K}: {ms * 1e3:.1f} us per launch (events, includes launch gaps); index[0]={idx[0].tolist()}")


if __name__ == "__main__":
    main()
