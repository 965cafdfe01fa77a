#!/usr/bin/env python3
"""Times the complex Beamformer's stream against the routes the parent commit has, HIP events around whole calls:

  tile      one ComplexStreamingLocalizer.push_replay of a 12 000-frame pack (ONE graph launch: STHT, wrap rows, band-pass tile,
            contraction, accumulate, slide; the pack is already on the device)   vs  Beamformer.localize_batch on the same pack (the
            restart route: the parent's only live form)
  bandpass  stream_bandpass_tile_kernel (micloc_stream_complex_bandpass_tile_f64) vs  the one-shot band-pass launch
            (micloc_bandpass_rzcc_f64 with `pre` only) on the same planar rows

at B = 1 and B = 64, M = 7, G = 449.  Each figure is the median (min - max) of 11 calls after 2 warm-ups; the two arms of a comparison
alternate call by call in one process.  bf_mat is random (timing does not depend on its values).
--out FILE writes the figures, the command, the device and the source hashes as JSON (profiles/streaming/COMPLEX_RECORD.json).

    python tools/stream_complex_time.py [--batches 1,64] [--frames 12000] [--out profiles/streaming/COMPLEX_RECORD.json]
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

FS, M, G = 48_000, 7, 449
SOURCES = ["haghighatshoarmuir2024_amd/csrc/stream_complex.hip", "haghighatshoarmuir2024_amd/csrc/api_stream.hip", "haghighatshoarmuir2024_amd/csrc/api_plan.hip", "haghighatshoarmuir2024_amd/csrc/api_internal.h", "haghighatshoarmuir2024_amd/csrc/rzcc.hip",
           "haghighatshoarmuir2024_amd/csrc/beamform.hip", "haghighatshoarmuir2024_amd/csrc/stht.hip", "haghighatshoarmuir2024_amd/streaming.py",
           "haghighatshoarmuir2024_amd/runtime.py", "haghighatshoarmuir2024_amd/beamformer.py", "tools/wideband_time.py", "tools/stream_complex_time.py"]


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.beamformer import Beamformer

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--frames", type=int, default=12_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    T = args.frames
    bf = Beamformer(CenterCircularArray(radius=4.5e-2, num_mic=M), kernel_duration=10.0e-3, freq_range=[1000.0, 2000.0], fs=FS)
    rng = np.random.RandomState(1)
    W = rng.randn(M, G) + 1j * rng.randn(M, G)
    t = np.arange(T) / FS
    rows = []
    for B in [int(v) for v in args.batches.split(",")]:
        x = torch.from_numpy(np.sin(2 * np.pi * 1500 * t)[None, :, None] + 0.4 * rng.randn(B, T, M)).cuda()
        stream = bf.streaming_localizer(W, batch=B, max_tile=T)
        stream.push(x)         # eager: the first tile of this length
        stream.push_replay(x)  # captured
        tile = timed({"push_replay_tile": lambda: stream.push_replay(x), "localize_batch_restart": lambda: bf.localize_batch(W, x)})
        s = stream.status()
        status = dict(frames_pushed=stream.t, frames_contracted=s["frames"], carry=s["carry"])  # (recorded with the figures: the work that was timed)
        # the band-pass stage alone, on the planar rows of the pack
        plan = stream.plan
        lib = plan.lib
        h = plan.stht(x)
        Ts = h.shape[2]
        st = runtime._stream(x.device)

        def bp_tile():
            _lib.check(lib.micloc_stream_complex_bandpass_tile_f64(plan.handle, runtime._ptr(h), B, T, Ts, 0, stream.max_tile, runtime._ptr(stream.state),
                                                                   stream.nstate, runtime._ptr(stream.ws), stream.nws, st), "stream_complex_bandpass_tile")

        pre = torch.empty_like(h)

        def bp_one_shot():
            _lib.check(lib.micloc_bandpass_rzcc_f64(plan.handle, runtime._ptr(h), B, T, Ts, runtime._ptr(pre), None, None, 0, st), "bandpass_rzcc")

        bp = timed({"bandpass_tile": bp_tile, "bandpass_one_shot": bp_one_shot})
        row = dict(B=B, T=T, G=G, M=M, pack_seconds=T / FS, stream_status=status, **tile, **bp)
        print(json.dumps(row))
        rows.append(row)
    record = dict(command="python tools/stream_complex_time.py " + " ".join(sys.argv[1:] if argv is None else argv), device=torch.cuda.get_device_name(0),
                  method="HIP events around whole calls; median (min - max) of 11 calls after 2 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
