#!/usr/bin/env python3
"""Times the tracked stream at the live demo's shape, HIP events around whole calls:

  tracked   one StreamingLocalizer(track=).push_replay of a 12 000-frame tile, 0.25 s of audio (ONE graph launch: clock / slide, the STHT
            of [history | tile], encoder tile, horizon, LIF + beamforming, accumulation, the tracking launch and its combine, commit,
            tick; the tile is copied into the graph's input buffer first)
  plain     the same stream without track=: the launches the streams had before the tracked read-out existed
  one_shot  SNNBeamformer.track_batch on the same 12 000 frames (the one-shot chain from zero state).

7 microphones, 449 DoAs, 1 trial and 64 trials; the audio is on the device in all three.  Each figure is the median (min - max) of 20
calls after 3 warm-ups; the arms alternate call by call in one process.  The real-time factor is 0.25 s over the tile time.
--out FILE writes the figures, the command, the box and the source hashes as JSON (profiles/stream_track/RECORD.json).

    python tools/stream_track_time.py [--batches 1,64] [--out profiles/stream_track/RECORD.json]
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
SOURCES = ["haghighatshoarmuir2024_amd/csrc/stream_track.hip", "haghighatshoarmuir2024_amd/csrc/stream_track.h", "haghighatshoarmuir2024_amd/csrc/track_rows.h",
           "haghighatshoarmuir2024_amd/csrc/track.hip", "haghighatshoarmuir2024_amd/csrc/api_stream.hip", "haghighatshoarmuir2024_amd/csrc/rzcc.hip",
           "haghighatshoarmuir2024_amd/csrc/beamform.hip", "haghighatshoarmuir2024_amd/streaming.py", "tools/wideband_time.py", "tools/stream_track_time.py"]


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.utils import Envelope

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    tau = 1 / (2 * np.pi * 2000)
    bf = SNNBeamformer(CenterCircularArray(4.5e-2, M), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)
    env = Envelope(rise_time=10e-3, fall_time=100e-3, fs=FS)
    rng = np.random.RandomState(0)
    W = rng.randn(2 * M, G)  # random unit columns: the timing does not depend on their values
    W /= np.linalg.norm(W, axis=0, keepdims=True)
    t = np.arange(T) / FS
    rows = []
    for B in [int(v) for v in args.batches.split(",")]:
        x = torch.from_numpy(np.sin(2 * np.pi * 1500 * t)[None, :, None] + 0.3 * rng.randn(B, T, M)).cuda()
        tracked = bf.streaming_localizer(W, batch=B, max_tile=T, track=env)
        plain = bf.streaming_localizer(W, batch=B, max_tile=T)
        for s in (tracked, plain):
            s.push(x)         # eager: the first tile of this length
            s.push_replay(x)  # captured
        arms = timed({"tracked_push_replay_tile": lambda: tracked.push_replay(x), "plain_push_replay_tile": lambda: plain.push_replay(x),
                      "one_shot_track_batch": lambda: bf.track_batch(W, x, env)}, calls=20, warmup=3)
        for s in (tracked, plain):
            st = s.status()
            assert st["lag_failures"] == 0 and st["overflow"] == 0 and list(s._graphs) == [T], st
        assert tracked.tracked()["count"] == tracked.status()["frames"] > 20 * T
        tile_ms, plain_ms = arms["tracked_push_replay_tile"]["median_ms"], arms["plain_push_replay_tile"]["median_ms"]
        row = dict(B=B, T=T, G=G, M=M, tile_seconds=T / FS, max_track=tracked.max_track, tracking_adds_ms=tile_ms - plain_ms,
                   real_time_factor=T / FS / (tile_ms * 1e-3), **arms)
        print(json.dumps(row))
        rows.append(row)
    prop = torch.cuda.get_device_properties(0)
    record = dict(command="python tools/stream_track_time.py " + " ".join(sys.argv[1:] if argv is None else argv),
                  box=dict(device=torch.cuda.get_device_name(0), gcn_arch=getattr(prop, "gcnArchName", ""), compute_units=prop.multi_processor_count,
                           hip=torch.version.hip),
                  method="HIP events around whole calls; median (min - max) of 20 calls after 3 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
