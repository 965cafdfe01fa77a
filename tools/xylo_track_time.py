"""Time the fused Xylo tracking call (micloc_xylo_lif_track_i16: `xylo_lif_track_kernel` of csrc/xylo.hip) beside the two-step route it
replaces (`xylo_lif_pk_kernel` with the raster stored, `envelope_kernel`, `rows_argmax_kernel`) and beside the counts-only packed kernel
at the same shape, which gives the price of the read-out.

python tools/xylo_track_time.py [B] [T] [N] [fused|twostep|counts|alternate] [launches] -- per-launch times (HIP events on the launch
stream, one pair per launch) of one call for B trials of T frames on the sweep's network shape (14 ternary channels = 28 input channels,
N neurons quantised by xylo_specification from a random unit-norm bf_mat, random ternary raster at 6 % density, the sweep's 1 ms / 10 ms
envelope): median, minimum and maximum over `launches` (default 11) after 2 warm-up calls.  `twostep` is XyloNetwork.run(want_spikes=True)
+ runtime.envelope_track on B trials (9 T N bytes of device memory per trial: choose a B that fits); `counts` is
XyloNetwork.run(queued=False), one workgroup per trial like the tracking form; `alternate` times fused and twostep in turns in one
process.  Shapes of DESIGN.md 4.23: `1100 4799 449 fused`, `1100 4799 449 counts` and `64 4799 449 alternate`.
Prints one JSON line.  Per-kernel times: run a mode under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o <name> -- python tools/xylo_track_time.py ...` (a run of its own,
without counter collection).
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from haghighatshoarmuir2024_amd import runtime  # noqa: E402
from haghighatshoarmuir2024_amd.utils import Envelope  # noqa: E402
from haghighatshoarmuir2024_amd.xylo_snn_localization import XyloNetwork, xylo_specification  # noqa: E402

MODES = ("fused", "twostep", "counts", "alternate")


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
    B, T, N = arg(1, 1100), arg(2, 4799), arg(3, 449)
    mode = sys.argv[4] if len(sys.argv) > 4 else "fused"
    n = arg(5, 11)
    if mode not in MODES:
        sys.exit(f"mode must be one of {MODES}")
    fs, C = 48_000, 14
    rng = np.random.RandomState(0)
    W = rng.randn(C, N)
    tau = 1.0 / (2 * np.pi * 1500)
    spec = xylo_specification([W / np.linalg.norm(W, axis=0, keepdims=True)], [[tau, tau]], fs=fs, target_dt=1e-3, bipolar_spikes=True)
    net = XyloNetwork(spec)
    gen = torch.Generator(device="cuda").manual_seed(0)
    raster = torch.empty((B, T, C), dtype=torch.int8, device="cuda")
    for s in range(0, B, 64):
        u = torch.rand(raster[s : s + 64].shape, device="cuda", generator=gen)
        raster[s : s + 64] = (u < 0.03).to(torch.int8) - (u > 0.97).to(torch.int8)
    env = Envelope(rise_time=1e-3, fall_time=10e-3, fs=fs)
    env_buf = torch.empty((B, T, N), dtype=torch.float64, device="cuda") if mode in ("twostep", "alternate") else None

    def fused():
        return net.track(raster, env, ternary=True, want_rate=True)["index"]

    def twostep():
        out, _ = net.run(raster, ternary=True, want_spikes=True)
        return runtime.envelope_track(out, env.win_lens[0], env.win_lens[1], want_index=True, env_out=env_buf)[1]

    def counts():
        return net.run(raster, ternary=True, queued=False)[1]

    calls = dict(fused=[fused], twostep=[twostep], counts=[counts], alternate=[fused, twostep])[mode]
    for _ in range(2):
        for c in calls:
            res = c()
    torch.cuda.synchronize()
    ms = {c.__name__: [] for c in calls}
    for _ in range(n):
        for c in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = c()
            e1.record()
            torch.cuda.synchronize()
            ms[c.__name__].append(e0.elapsed_time(e1))
    out = dict(mode=mode, B=B, T=T, N=N, Cin=2 * C, launches=n, fused_kernel=bool(net.track_is_fused(True)),
               peak_alloc_mb=torch.cuda.max_memory_allocated() / 1e6, result_sum=int(res.long().sum()))
    for name, v in ms.items():
        v = np.asarray(v)
        out[name] = dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()), spread_ms=float(v.max() - v.min()),
                         median_ms_per_trial=float(np.median(v) / B))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
