#!/usr/bin/env python3
"""Times the time-resolved Xylo read-out for batches against the counts of the whole recording, HIP events around whole calls:

  demo   Demo.windows_batch (encoder, the chunk-count LIF launch, the window sums, rate and peak per window, rate and peak of the
         recording)   vs   Demo.counts_batch(queued=False), the same launch shape without the chunk rows (one workgroup per trial)   vs
         Demo.counts_batch(), the ticket queue.  window = 12 288 frames with hop = 12 288 and with hop = 3072.
  lif    the same three on a raster that is already encoded -- XyloNetwork.run_windows vs run(queued=False) vs run() -- so that the
         encoder, which all arms share, does not hide the difference.

7 microphones, 449 DoAs, one band (1-2 kHz), T = 48 000 frames (the sweep's 1 s), B = 1, 64 and 1100 trials.  Each figure is the median
(min - max) of 20 calls after 3 warm-ups; the arms alternate call by call in one process.  PARITY UNPINNED for the LIF.
--out FILE writes the figures, the command, the device and the source hashes as JSON.

    python tools/xylo_windows_time.py [--batches 1,64,1100] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.wideband_time import timed  # noqa: E402

FS, T, M, G, WINDOW, HOPS, WIN_SIZE = 48_000, 48_000, 7, 449, 12_288, (12_288, 3072), 15
SOURCES = ["haghighatshoarmuir2024_amd/csrc/xylo.hip", "haghighatshoarmuir2024_amd/csrc/xylo_rows.h", "haghighatshoarmuir2024_amd/csrc/xylo_windows.h",
           "haghighatshoarmuir2024_amd/csrc/sweep.hip", "haghighatshoarmuir2024_amd/csrc/api_track.hip", "haghighatshoarmuir2024_amd/xylo_snn_localization.py",
           "tools/wideband_time.py", "tools/xylo_windows_time.py"]


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.xylo_snn_localization import Demo

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64,1100")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    demo = Demo(CenterCircularArray(radius=4.5e-2, num_mic=M), [[1000, 2000]], np.linspace(-np.pi, np.pi, G), recording_duration=0.05, fs=FS)
    net = demo.network()
    t = torch.arange(T, dtype=torch.float64, device="cuda") / FS
    rows = []
    for B in [int(v) for v in args.batches.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(B)
        x = torch.sin(2 * np.pi * 1500 * t)[None, :, None] + 0.3 * torch.randn((B, T, M), dtype=torch.float64, device="cuda", generator=gen)
        raster = demo.raster_device(x)
        fns = {"demo_counts_queued": lambda: demo.counts_batch(x), "demo_counts_unqueued": lambda: demo.counts_batch(x, queued=False),
               "lif_counts_queued": lambda: net.run(raster, ternary=True), "lif_counts_unqueued": lambda: net.run(raster, ternary=True, queued=False)}
        for hop in HOPS:
            fns[f"demo_windows_hop{hop}"] = lambda hop=hop: demo.windows_batch(x, WINDOW, hop, win_size=WIN_SIZE)
            fns[f"lif_windows_hop{hop}"] = lambda hop=hop: net.run_windows(raster, WINDOW, hop, ternary=True)
        arms = timed(fns, calls=20, warmup=3)
        # the arms computed the same thing
        counts = net.run(raster, ternary=True, queued=False)[1]
        assert torch.equal(counts, demo.counts_batch(x)) and int(counts.sum()) > 0
        net.check()
        for hop in HOPS:
            w = demo.windows_batch(x, WINDOW, hop, win_size=WIN_SIZE)
            assert torch.equal(w["counts"], counts) and (hop != WINDOW or torch.equal(w["window_counts"].sum(dim=1), counts))
        row = dict(B=B, T=T, G=G, M=M, bands=1, window=WINDOW, hops=list(HOPS), quantised_w_rec_of_the_design=int(demo.spec["w_rec"]),
                   chunk_row_bytes=B * ((T + 255) // 256) * G * 4, **arms)
        for hop in HOPS:
            row[f"lif_windows_hop{hop}_over_unqueued"] = arms[f"lif_windows_hop{hop}"]["median_ms"] / arms["lif_counts_unqueued"]["median_ms"]
            row[f"demo_windows_hop{hop}_over_unqueued"] = arms[f"demo_windows_hop{hop}"]["median_ms"] / arms["demo_counts_unqueued"]["median_ms"]
        print(json.dumps(row))
        rows.append(row)
        del x, raster, fns
        torch.cuda.empty_cache()
    record = dict(command="python tools/xylo_windows_time.py " + " ".join(sys.argv[1:] if argv is None else argv), device=torch.cuda.get_device_name(0),
                  method="HIP events around whole calls; median (min - max) of 20 calls after 3 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
