"""Time the time-resolved read-out (micloc_lif_beamform_windows_f64: `window_power_kernel` of csrc/windows.hip) beside the one-shot
reduction it extends.

python tools/windows_time.py [B] [T] [G] [window] [hop] [plain|windows] -- average time of one Plan.lif_beamform call over 20 calls
(HIP events on the launch stream) for B trials of T frames and G DoAs on the 7-microphone plan of the sweeps (14 channels, random
ternary spikes at 6 % density, random unit-norm bf_mat): `windows` (default) asks for power and arg-max per window AND the ordinary
whole-recording ones in the same call, `plain` is today's call without `window`.  Defaults: the headline shape 1100 x 4799 x 360,
window = hop = 1024; the speech shape is `125 332157 449 4096 2048`.  Per-kernel times: run each mode under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <name> -- python tools/windows_time.py ...`; the beamforming
kernel is the same launch in both modes, `power_argmax_kernel` / `power_columns_kernel` + `argmax_rows_kernel` are the one-shot
reduction, `window_power_kernel` is the new read-out.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from haghighatshoarmuir2024_amd.runtime import Plan  # noqa: E402
from haghighatshoarmuir2024_amd.snn_beamformer import neuron_impulse_response  # noqa: E402


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    B, T, G, window, hop = arg(1, 1100), arg(2, 4799), arg(3, 360), arg(4, 1024), arg(5, 1024)
    mode = sys.argv[6] if len(sys.argv) > 6 else "windows"
    if mode not in ("plain", "windows"):
        sys.exit("mode must be 'plain' or 'windows'")
    from scipy.signal import butter, hilbert

    fs, M = 48_000, 7
    impulse = np.zeros(480)
    impulse[0] = 1
    b, a = butter(2, [1000.0, 2000.0], btype="bandpass", analog=False, output="ba", fs=fs)
    plan = Plan(M, np.fft.fftshift(np.imag(hilbert(impulse))), b, a, 12, True)
    tau = 1.0 / (2 * np.pi * 2000)
    plan.set_neuron_kernel(neuron_impulse_response(np.arange(T) / fs, [tau, tau]))
    rng = np.random.RandomState(0)
    W = rng.randn(2 * M, G)
    plan.set_bf_mat(W / np.linalg.norm(W, axis=0, keepdims=True))
    gen = torch.Generator(device="cuda").manual_seed(0)
    spikes = torch.empty((B, T, 2 * M), dtype=torch.int8, device="cuda")
    for s in range(0, B, 64):  # (in slabs: the uniform draws of the speech shape would be 2.3 GB at once)
        u = torch.rand(spikes[s : s + 64].shape, device="cuda", generator=gen)
        spikes[s : s + 64] = (u < 0.03).to(torch.int8) - (u > 0.97).to(torch.int8)
    kw = dict(window=window, hop=hop) if mode == "windows" else {}
    for _ in range(3):
        out = plan.lif_beamform(spikes, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    e0.record()
    for _ in range(n):
        out = plan.lif_beamform(spikes, **kw)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    q = plan.window_quantum()
    shape = tuple(out["window_power"].shape) if mode == "windows" else tuple(out["power"].shape)
    print(f"lif_beamform [{mode}]: B={B} T={T} G={G} quantum={q} window={window} hop={hop}: {ms * 1e3:.1f} us per call (events, includes "
          f"launch gaps and the output allocation); result {shape}; argmax[0]={int(out['argmax'][0])}")


if __name__ == "__main__":
    main()
