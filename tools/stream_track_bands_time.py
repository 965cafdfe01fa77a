#!/usr/bin/env python3
"""Times the tracked wideband streams at the live demos' shape, HIP events around whole calls:

  tracked   one push_replay of a 12 000-frame tile (0.25 s of audio at 48 kHz: the demos' pack) through the wideband stream with track= --
            ONE graph launch: the filterbank tile, every band's tile, the band sum and the tracking launches (SNN: frontier, band kernel,
            combine; complex: band kernel and combine in front of the slide); the tile is copied into the graph's input buffer first
  plain     the same stream without track=: the launches the wideband streams had before the tracked read-out existed
  one_shot  the wideband localizer's track_batch on a recording of 20 such tiles, for scale (3 calls).

Both kinds (WidebandStreamingLocalizer over SNN bands, WidebandComplexStreamingLocalizer), 3 bands, 7 microphones, 449 DoAs, 1 trial and
64 trials; the audio is on the device.  Each stream figure is the median (min - max) of 11 calls after 2 warm-ups; the arms alternate call
by call in one process; every run is recorded.  The real-time factor is 0.25 s over the tracked tile time.  Not measured here: hardware
counters and kernel traces.
--out FILE writes every run, the command, the commit, the box and the source hashes as JSON (profiles/stream_track_bands/RECORD.json).

    python tools/stream_track_bands_time.py [--batches 1,64] [--kinds snn,complex] [--out profiles/stream_track_bands/RECORD.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS, T, M, G, F, TILES = 48_000, 12_000, 7, 449, 3, 20
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]
SOURCES = ["haghighatshoarmuir2024_amd/csrc/stream_track_bands.hip", "haghighatshoarmuir2024_amd/csrc/stream_track_bands.h",
           "haghighatshoarmuir2024_amd/csrc/stream_track_rows.h", "haghighatshoarmuir2024_amd/csrc/track_bands_rows.h",
           "haghighatshoarmuir2024_amd/csrc/track_rows.h", "haghighatshoarmuir2024_amd/csrc/track.hip", "haghighatshoarmuir2024_amd/csrc/api_stream.hip",
           "haghighatshoarmuir2024_amd/streaming.py", "tools/stream_track_bands_time.py"]


def localizer(kind):
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.filterbank import ButterworthFilterbank
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    rng = np.random.RandomState(0)  # random unit columns: the timing does not depend on their values
    if kind == "snn":
        beamfs = [SNNBeamformer(geo, 10e-3, fr, np.asarray([1 / (2 * np.pi * np.mean(fr))] * 2), bipolar_spikes=True, fs=FS) for fr in BANDS]
        Ws = []
        for _ in BANDS:
            W = rng.randn(2 * M, G)
            Ws.append(W / np.linalg.norm(W, axis=0, keepdims=True))
        return WidebandSNNLocalizer(beamfs, Ws, ButterworthFilterbank(freq_bands=np.asarray(BANDS), order=1, fs=FS))
    beamfs = [Beamformer(geo, 10e-3, fr, fs=FS) for fr in BANDS]
    Ws = [(rng.randn(M, G) + 1j * rng.randn(M, G)) / np.sqrt(2 * M) for _ in BANDS]
    return WidebandBeamformerLocalizer(beamfs, Ws, ButterworthFilterbank(freq_bands=np.asarray(BANDS), order=2, fs=FS))


def timed(arms, calls, warmup):
    """arms: name -> callable.  Alternating call by call, HIP events around every call -> name -> dict(median_ms, min_ms, max_ms, runs_ms)."""
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
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), runs_ms=[float(u) for u in v]) for k, v in ms.items()}


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd.streaming import WidebandComplexStreamingLocalizer, WidebandStreamingLocalizer
    from haghighatshoarmuir2024_amd.utils import Envelope

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--kinds", default="snn,complex")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit of the tree, where the tool runs from an export without a repository")
    args = ap.parse_args(argv)
    env = Envelope(rise_time=10e-3, fall_time=100e-3, fs=FS)
    t = np.arange(T) / FS
    rows = []
    for kind in args.kinds.split(","):
        loc = localizer(kind)
        cls = WidebandStreamingLocalizer if kind == "snn" else WidebandComplexStreamingLocalizer
        for B in [int(v) for v in args.batches.split(",")]:
            rng = np.random.RandomState(1)
            tone = sum(np.sin(2 * np.pi * np.mean(fr) * t) for fr in BANDS)
            x = torch.from_numpy(tone[None, :, None] + 0.3 * rng.randn(B, T, M)).cuda()
            tracked, plain = cls(loc, B, max_tile=T, track=env), cls(loc, B, max_tile=T)
            for s in (tracked, plain):
                s.push(x)         # eager: the first tile of this length
                s.push_replay(x)  # captured
            arms = timed({"tracked_push_replay_tile": lambda: tracked.push_replay(x), "plain_push_replay_tile": lambda: plain.push_replay(x)}, 11, 2)
            for s in (tracked, plain):
                st = s.status()
                assert st.get("lag_failures", 0) == 0 and st.get("overflow", 0) == 0 and list(s._graphs) == [T], st
            assert tracked.status()["tracked"] > 10 * T and tracked.tracked()["count"] == tracked.status()["tracked"]
            long = x.repeat(1, TILES, 1)
            arms.update(timed({"one_shot_track_batch_20_tiles": lambda: loc.track_batch(long, env)}, 3, 1))
            del long
            tile_ms, plain_ms = arms["tracked_push_replay_tile"]["median_ms"], arms["plain_push_replay_tile"]["median_ms"]
            row = dict(kind=kind, F=F, B=B, T=T, G=G, M=M, tile_seconds=T / FS, max_track=tracked.max_track, tracking_adds_ms=tile_ms - plain_ms,
                       real_time_factor=T / FS / (tile_ms * 1e-3), **arms)
            print(json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "runs_ms"}) for k, v in row.items()}), flush=True)
            rows.append(row)
            del tracked, plain, x
            torch.cuda.empty_cache()
    prop = torch.cuda.get_device_properties(0)
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    record = dict(command="python tools/stream_track_bands_time.py " + " ".join(sys.argv[1:] if argv is None else argv),
                  commit=commit, commit_note="the parent commit when run on a working tree: the source hashes identify the code that ran",
                  box=dict(device=torch.cuda.get_device_name(0), gcn_arch=getattr(prop, "gcnArchName", ""), compute_units=prop.multi_processor_count,
                           hip=torch.version.hip),
                  method="HIP events around whole calls; streams: median (min - max) of 11 calls after 2 warm-ups, arms alternating call by call in one "
                         "process; track_batch on 20 tiles: 3 calls after 1 warm-up",
                  not_measured=["hardware counters", "kernel traces"],
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
