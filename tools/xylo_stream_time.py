#!/usr/bin/env python3
"""Times the Xylo stream against the one-shot call at the live demo's shape, HIP events around whole calls:

  tile      one XyloStreamingLocalizer.push_replay of a 12 000-frame tile, 0.25 s of audio (ONE graph launch: the STHT of [history | tile],
            the band's clock / slide, encoder tile, horizon, resumable LIF, commit, tick, and the read-out; the tile is copied into the
            graph's input buffer first)   vs   Demo.counts_batch on the same 12 000 frames (the one-shot chain from zero state: fused
            STHT + band-pass + RZCC pipeline, then the LIF's ticket queue).  The audio is on the device in both.

  tracked    the same tile through a second stream built with track= (the tracking LIF in place of the counting one: a DoA
            index and a peak envelope per frame)   vs   Demo.track_batch on the same 12 000 frames.  --arms plain leaves these two out:
            the two arms above alone, as the tool ran before the tracked stream existed (the comparison with an older library).

7 microphones, 449 DoAs, one band (1-2 kHz), 1 trial and 64 trials.  Each figure is the median (min - max) of 20 calls after 3 warm-ups; the
two arms alternate call by call in one process.  The real-time factor is 0.25 s over the tile time.  PARITY UNPINNED for the LIF.
--out FILE writes the figures, the command, the device and the source hashes as JSON.

    python tools/xylo_stream_time.py [--batches 1,64] [--arms all|plain] [--out FILE]
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

FS, T, M, G = 48_000, 12_000, 7, 449
SOURCES = ["haghighatshoarmuir2024_amd/csrc/stream_xylo.hip", "haghighatshoarmuir2024_amd/csrc/api_xylo_stream.hip", "haghighatshoarmuir2024_amd/csrc/xylo.hip",
           "haghighatshoarmuir2024_amd/csrc/xylo_rows.h", "haghighatshoarmuir2024_amd/csrc/rzcc.hip", "haghighatshoarmuir2024_amd/streaming.py", "haghighatshoarmuir2024_amd/xylo_snn_localization.py",
           "tools/wideband_time.py", "tools/xylo_stream_time.py"]


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.xylo_snn_localization import Demo, xylo_specification

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--arms", default="all", choices=("all", "plain"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    demo = Demo(CenterCircularArray(radius=4.5e-2, num_mic=M), [[1000, 2000]], np.linspace(-np.pi, np.pi, G), recording_duration=0.05, fs=FS)
    w_rec = int(demo.spec["w_rec"])
    if w_rec != 0:  # (the stream's precondition; at 449 DoAs the paper's -0.1 / N quantises to 0 by itself)
        demo.spec = xylo_specification(demo.bf_mats, demo.tau_vecs, demo.fs, 1e-3, True, w_rec_coef=0.0)
    rng = np.random.RandomState(1)
    t = np.arange(T) / FS
    rows = []
    for B in [int(v) for v in args.batches.split(",")]:
        x = torch.from_numpy(np.sin(2 * np.pi * 1500 * t)[None, :, None] + 0.3 * rng.randn(B, T, M)).cuda()
        stream = demo.streaming_localizer(batch=B, max_tile=T)
        stream.push(x)         # eager: the first tile of this length
        stream.push_replay(x)  # captured
        fns = {"push_replay_tile": lambda: stream.push_replay(x), "one_shot_counts_batch": lambda: demo.counts_batch(x)}
        if args.arms == "all":
            from haghighatshoarmuir2024_amd.utils import Envelope

            env = Envelope(rise_time=1e-3, fall_time=10e-3, fs=FS)
            tracked = demo.streaming_localizer(batch=B, max_tile=T, track=env)
            tracked.push(x)
            tracked.push_replay(x)
            fns["tracked_push_replay_tile"] = lambda: tracked.push_replay(x)
            fns["one_shot_track_batch"] = lambda: demo.track_batch(x, env)
        arms = timed(fns, calls=20, warmup=3)
        st = stream.status()
        assert st["lag_failures"] == 0 and st["overflow"] == 0, st
        assert int(stream.counts.sum()) > 0 and list(stream._graphs) == [T]
        tile_ms = arms["push_replay_tile"]["median_ms"]
        row = dict(B=B, T=T, G=G, M=M, bands=1, tile_seconds=T / FS, quantised_w_rec_of_the_design=w_rec, real_time_factor=T / FS / (tile_ms * 1e-3), **arms)
        if args.arms == "all":
            st = tracked.status()
            assert st["lag_failures"] == 0 and st["overflow"] == 0 and list(tracked._graphs) == [T], st
            w = tracked.tracked()
            assert w["count"] == st["frames"] > 0 and torch.equal(tracked.counts, stream.counts) and float(w["peak_envelope"].max()) > 0.0
            tr_ms = arms["tracked_push_replay_tile"]["median_ms"]
            row.update(tracked_over_plain_tile=tr_ms / tile_ms, tracked_real_time_factor=T / FS / (tr_ms * 1e-3))
        print(json.dumps(row))
        rows.append(row)
    record = dict(command="python tools/xylo_stream_time.py " + " ".join(sys.argv[1:] if argv is None else argv), device=torch.cuda.get_device_name(0),
                  method="HIP events around whole calls; median (min - max) of 20 calls after 3 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
