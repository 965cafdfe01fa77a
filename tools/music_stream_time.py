#!/usr/bin/env python3
"""Times the MUSIC stream against the one-shot call at the live demo's shape, HIP events around whole calls:

  pack      one MusicStreamingLocalizer.push_replay of a 12 000-sample pack (ONE graph launch: filter tile, DFT of the completed frames,
            slice, read-out; the pack is copied into the graph's input buffer first)   vs  the one-shot MUSIC.beamforming's device work on
            the same pack (micloc_music_f64 on B packs of one slice each: filter, DFT, select, steer).  The pack is on the device in both.
  last      the time from a pack's last sample to its DoA: the pack arrives in tiles of --last samples (240: 5 ms of audio), every tile
            but the last is pushed (push_replay) and waited for, then the last one is timed; the one-shot call cannot start before the last
            sample, so its `pack` figure is its latency.

1 trial and 64 trials, 7 microphones, N = 2048, 225 DoAs, band 1200-2000 Hz, 20 active frequencies, no overlap.  Each figure is the median
(min - max) of 11 calls after 2 warm-ups; the arms of a comparison alternate call by call in one process.
--out FILE writes the figures, the command, the device and the source hashes as JSON.

    python tools/music_stream_time.py [--batches 1,64] [--last 240] [--out profiles/music/STREAM_RECORD.json]
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

FS, T, M, G, N, K = 48_000, 12_000, 7, 225, 2048, 20
SOURCES = ["haghighatshoarmuir2024_amd/csrc/stream_music.hip", "haghighatshoarmuir2024_amd/csrc/music.hip", "haghighatshoarmuir2024_amd/csrc/music_rows.h",
           "haghighatshoarmuir2024_amd/csrc/api_stream.hip", "haghighatshoarmuir2024_amd/csrc/api_ops.hip", "haghighatshoarmuir2024_amd/streaming.py",
           "haghighatshoarmuir2024_amd/music_beamformer.py", "tools/wideband_time.py", "tools/music_stream_time.py"]


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.localization_demo_MUSIC import Demo

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--last", type=int, default=240)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if T % args.last:
        ap.error("--last must divide 12000")
    demo = Demo(CenterCircularArray(radius=4.5e-2, num_mic=M), np.asarray([1200, 2000]), K, np.linspace(-np.pi, np.pi, G), recording_duration=T / FS,
                num_fft_bin=N, fs=FS)
    music = demo.music
    rng = np.random.RandomState(1)
    t = np.arange(T) / FS
    rows = []
    for B in [int(v) for v in args.batches.split(",")]:
        x = torch.from_numpy(np.sin(2 * np.pi * 1500 * t)[None, :, None] + 0.4 * rng.randn(B, T, M)).cuda()
        stream = demo.streaming_localizer(batch=B, max_tile=T)
        stream.push(x)         # eager: the first tile of this length
        stream.push_replay(x)  # captured

        def one_shot():
            return music._run(x, T, T, 1, K, N)["spectrum"]

        pack = timed({"push_replay_pack": lambda: stream.push_replay(x), "one_shot_beamforming": one_shot})
        assert torch.equal(stream.latest_window()[0], one_shot()[:, 0])  # the work that was timed: the same spectrum
        # the last tile of a pack that arrives in small tiles
        n, tiles = args.last, T // args.last
        small = demo.streaming_localizer(batch=B, max_tile=n)
        last = []
        for rep in range(13):
            for i in range(tiles - 1):
                small.push_replay(x[:, i * n : (i + 1) * n])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            small.push_replay(x[:, T - n :])
            e1.record()
            e1.synchronize()
            if rep >= 2:
                last.append(e0.elapsed_time(e1))
        assert torch.equal(small.latest_window()[0], one_shot()[:, 0])
        row = dict(B=B, T=T, G=G, M=M, N=N, k=K, pack_seconds=T / FS, last_tile=n, slices=stream.status()["slices"], **pack,
                   last_tile_to_doa=dict(median_ms=float(np.median(last)), min_ms=float(np.min(last)), max_ms=float(np.max(last)), calls=len(last)))
        print(json.dumps(row))
        rows.append(row)
    record = dict(command="python tools/music_stream_time.py " + " ".join(sys.argv[1:] if argv is None else argv), device=torch.cuda.get_device_name(0),
                  method="HIP events around whole calls; median (min - max) of 11 calls after 2 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
