#!/usr/bin/env python3
"""Times the wideband localizer against the routes it replaces, HIP events around whole calls:

  batched   WidebandSNNLocalizer.localize_batch(x [B, T, M])         vs  Demo.power_grid pack by pack (the parent route)
  filterbank  one micloc_filterbank_f64 launch for F bands             vs  the F runtime.lfilter calls it replaces

at B = 1 and B = 64 packs of 12 000 frames, F = 3 bands, G = 112 DoAs, M = 7.  Each figure is the median (min - max) of 11 calls after
2 warm-ups; the two arms of a comparison alternate call by call in one process.  The matrices are random unit columns (timing does
not depend on their values).  --out FILE writes the figures, the command and the source hashes as JSON (profiles/wideband/RECORD.json).

    python tools/wideband_time.py [--batches 1,64] [--frames 12000] [--out profiles/wideband/RECORD.json]
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

FS, M, G = 48_000, 7, 112
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]
SOURCES = ["haghighatshoarmuir2024_amd/csrc/filterbank.hip", "haghighatshoarmuir2024_amd/csrc/api_bands.hip", "haghighatshoarmuir2024_amd/csrc/api_plan.hip", "haghighatshoarmuir2024_amd/csrc/api_internal.h", "haghighatshoarmuir2024_amd/csrc/rzcc.hip",
           "haghighatshoarmuir2024_amd/csrc/beamform.hip", "haghighatshoarmuir2024_amd/csrc/stht.hip", "haghighatshoarmuir2024_amd/wideband.py",
           "haghighatshoarmuir2024_amd/runtime.py", "haghighatshoarmuir2024_amd/localization_demo_snn.py", "tools/wideband_time.py"]


def build():
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.filterbank import ButterworthFilterbank
    from haghighatshoarmuir2024_amd.localization_demo_snn import Demo
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer

    geo = CenterCircularArray(4.5e-2, M)
    rng = np.random.RandomState(0)
    demo = Demo.__new__(Demo)
    demo.beamfs, demo.bf_mats = [], []
    for fr in BANDS:
        tau = 1 / (2 * np.pi * np.mean(fr))
        demo.beamfs.append(SNNBeamformer(geometry=geo, kernel_duration=10e-3, freq_range=fr, tau_vec=[tau, tau], bipolar_spikes=True, fs=FS))
        W = rng.randn(2 * M, G)
        demo.bf_mats.append(W / np.linalg.norm(W, axis=0, keepdims=True))
    demo.filterbank = ButterworthFilterbank(freq_bands=BANDS, order=1, fs=FS)
    demo.doa_list, demo.fs = np.linspace(-np.pi, np.pi, G), FS
    return demo, demo.localizer()


def timed(arms, calls=11, warmup=2):
    """arms: name -> callable.  Alternating, HIP events around every call.  Returns name -> dict(median_ms, min_ms, max_ms)."""
    import torch

    ms = {k: [] for k in arms}
    for i in range(warmup + calls):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), calls=len(v)) for k, v in ms.items()}


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd import runtime

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--frames", type=int, default=12_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    demo, loc = build()
    T = args.frames
    t = np.arange(T) / FS
    rng = np.random.RandomState(1)
    results = []
    for B in [int(v) for v in args.batches.split(",")]:
        x_host = (np.sin(2 * np.pi * 2000 * t)[None, :, None] + 0.4 * rng.randn(B, T, M)) * 2.0**20
        x = torch.from_numpy(x_host).cuda()
        packs = [np.ascontiguousarray(x_host[i]) for i in range(B)]
        xf = torch.empty((len(BANDS), B, T, M), dtype=torch.float64, device=x.device)
        ba = demo.filterbank.ba_list

        def lfilters():
            for f, (b, a) in enumerate(ba):
                runtime.lfilter(b, a, x, out=xf[f])

        # both arms go from host packs to a host power pattern, as Demo.power_grid does
        whole = timed({"localize_batch": lambda: loc.localize_batch(x_host)["power"].cpu(), "power_grid_per_pack": lambda: [demo.power_grid(p) for p in packs]})
        fb = timed({"filterbank_launch": lambda: runtime.filterbank(ba, x, out=xf), "lfilter_calls": lfilters})
        row = dict(B=B, T=T, F=len(BANDS), G=G, M=M, **whole, **fb)
        results.append(row)
        print(json.dumps(row))
    record = dict(command="python tools/wideband_time.py " + " ".join(sys.argv[1:] if argv is None else argv), device=torch.cuda.get_device_name(0),
                  method="HIP events around whole calls; median (min - max) of 11 calls after 2 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
