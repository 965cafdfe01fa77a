"""Time the packed Xylo LIF kernel alone on the sweep's shape (1100 trials x 48000 steps, 14 -> 28 channels, 360 neurons);
MICLOC_DEV_LIB selects a variant build.

    python tools/dev/xylo_lif_bench.py                                   the packed kernel: ticket queue and one workgroup per trial
    python tools/dev/xylo_lif_bench.py general|recurrent [B] [T] [Cin]   the general kernel (xylo_lif_kernel of csrc/xylo.hip) on uint8 events
                                                                         (ternary=False), `recurrent` with w_rec = -1: the counts call
                                                                         (run) and the windowed call (run_windows, window = hop = 1024),
                                                                         each as the median of 11 calls after 2 warm-ups, twice
"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from haghighatshoarmuir2024_amd import _lib
if os.environ.get("MICLOC_DEV_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["MICLOC_DEV_LIB"])
from haghighatshoarmuir2024_amd.xylo_snn_localization import XyloNetwork

rng = np.random.RandomState(0)
mode = sys.argv[1] if len(sys.argv) > 1 else "packed"
if mode not in ("packed", "general", "recurrent"):
    sys.exit("mode must be 'packed', 'general' or 'recurrent'")
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
C, N, B, T = arg(4, 28) // 2, 360, arg(2, 1100 if mode == "packed" else 256), arg(3, 48000)
spec = dict(W_in=rng.randint(-127, 128, size=(2 * C, N)).astype(np.int8), w_rec=-1 if mode == "recurrent" else 0, dash_syn=rng.randint(1, 4, size=N).astype(np.uint8),
            dash_mem=rng.randint(1, 4, size=N).astype(np.uint8), threshold=rng.randint(3000, 6000, size=N).astype(np.int16))
net = XyloNetwork(spec)
if mode != "packed":
    events = (torch.rand(B, T, 2 * C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)) < 0.02).to(torch.uint8)
    arms = {"counts": lambda: net.run(events, ternary=False)[1], "windows": lambda: net.run_windows(events, 1024, 1024, ternary=False)["counts"]}
    for name in ("counts", "windows", "counts", "windows"):
        ms = []
        for i in range(13):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c = arms[name]()
            e1.record(); torch.cuda.synchronize()
            if i >= 2: ms.append(e0.elapsed_time(e1))
        print(os.environ.get("MICLOC_DEV_LIB", "default"), mode, name, "B %d T %d Cin %d" % (B, T, 2 * C), "xylo LIF median %.4f ms (%.4f - %.4f)" % (float(np.median(ms)), min(ms), max(ms)),
              "spikes", int(c.sum()), flush=True)
    sys.exit(0)
raster = (torch.rand(B, T, C, device="cuda") < 0.02).to(torch.int8) * (torch.randint(0, 2, (B, T, C), device="cuda", dtype=torch.int8) * 2 - 1)
for queued in (True, False, True, False):
    def run():
        return net.run(raster, ternary=True, queued=queued)[1]
    for _ in range(2): run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5): c = run()
    e1.record(); torch.cuda.synchronize()
    print(os.environ.get("MICLOC_DEV_LIB", "default"), "ticket queue" if queued else "one workgroup per trial", "xylo LIF %.2f ms" % (e0.elapsed_time(e1) / 5), "spikes", int(c.sum()), flush=True)
