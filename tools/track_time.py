"""Time the fused moving-target read-out (micloc_lif_beamform_track_f64: `track_ws_kernel` + `track_combine_kernel` of csrc/track.hip)
beside the two-step route it replaces (beamforming with y stored, `envelope_kernel`, `rows_argmax_kernel`).

python tools/track_time.py [B] [T] [G] [fused|twostep|complex] [launches] -- per-launch times (HIP events on the launch stream, one pair per
launch) of one call for B trials of T frames and G DoAs on the 7-microphone plan of the sweeps (14 channels, random ternary spikes at
6 % density, random unit-norm bf_mat, the script's 10 ms / 100 ms envelope): median, minimum and maximum over `launches` (default 11)
after 2 warm-up calls, and the median per trial.  `twostep` is Plan.lif_beamform(want_y=True) + runtime.envelope_track on B trials
(2 x 8 T G bytes of device memory per trial: choose a B that fits).  `complex` is the fused call of the complex Beamformer on the same plan
(micloc_beamform_c128_track_f64: `track_wsc_kernel<3, 2>`): random planar band-passed rows [B, 14, Ts], a random complex bf_mat of unit
columns, the same shapes and reporting as `fused`.  Shapes of DESIGN.md 4.12: `1100 4799 449` and `2 239999 449`.
Prints one JSON line.  Per-kernel times: run a mode under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <name> -- python tools/track_time.py ...` (a run of its own, without
counter collection).
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from haghighatshoarmuir2024_amd import runtime  # noqa: E402
from haghighatshoarmuir2024_amd.runtime import Plan  # noqa: E402
from haghighatshoarmuir2024_amd.snn_beamformer import neuron_impulse_response  # noqa: E402


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    B, T, G = arg(1, 1100), arg(2, 4799), arg(3, 449)
    mode = sys.argv[4] if len(sys.argv) > 4 else "fused"
    n = arg(5, 11)
    if mode not in ("fused", "twostep", "complex"):
        sys.exit("mode must be 'fused', 'twostep' or 'complex'")
    from scipy.signal import butter, hilbert

    fs, M = 48_000, 7
    impulse = np.zeros(480)
    impulse[0] = 1
    b, a = butter(2, [1000.0, 2000.0], btype="bandpass", analog=False, output="ba", fs=fs)
    plan = Plan(M, np.fft.fftshift(np.imag(hilbert(impulse))), b, a, 12, True)
    tau = 1.0 / (2 * np.pi * 2000)
    plan.set_neuron_kernel(neuron_impulse_response(np.arange(T) / fs, [tau, tau]))
    rng = np.random.RandomState(0)
    W = rng.randn(2 * M, G) if mode != "complex" else rng.randn(M, G) + 1j * rng.randn(M, G)
    plan.set_bf_mat(W / np.linalg.norm(W, axis=0, keepdims=True))
    gen = torch.Generator(device="cuda").manual_seed(0)
    if mode == "complex":
        pre = torch.randn((B, 2 * M, plan.padded_T(T)), dtype=torch.float64, device="cuda", generator=gen)
    else:
        spikes = torch.empty((B, T, 2 * M), dtype=torch.int8, device="cuda")
        for s in range(0, B, 64):
            u = torch.rand(spikes[s : s + 64].shape, device="cuda", generator=gen)
            spikes[s : s + 64] = (u < 0.03).to(torch.int8) - (u > 0.97).to(torch.int8)
    wf, wr = int(fs * 100e-3), int(fs * 10e-3)
    env_buf = torch.empty((B, T, G), dtype=torch.float64, device="cuda") if mode == "twostep" else None

    def call():
        if mode == "fused":
            return plan.track(spikes, wf, wr, kind="spikes")["index"]
        if mode == "complex":
            return plan.track(pre, wf, wr, kind="planar", T=T)["index"]
        y = plan.lif_beamform(spikes, want_y=True, want_power=False)["y"]
        return runtime.envelope_track(y, wf, wr, want_index=True, env_out=env_buf)[1]

    for _ in range(2):
        idx = call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        idx = call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.asarray(ms)
    print(json.dumps(dict(mode=mode, B=B, T=T, G=G, launches=n, fused_kernels=bool(plan.track_is_fused()), median_ms=float(np.median(ms)),
                          min_ms=float(ms.min()), max_ms=float(ms.max()), median_ms_per_trial=float(np.median(ms) / B),
                          peak_alloc_mb=torch.cuda.max_memory_allocated() / 1e6, index_sum=int(idx.long().sum()))))


if __name__ == "__main__":
    main()
