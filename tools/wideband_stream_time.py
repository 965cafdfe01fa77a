#!/usr/bin/env python3
"""Times the wideband stream against the routes the parent commit has, HIP events around whole calls:

  tile        one WidebandStreamingLocalizer.push_replay of a 12 000-frame pack (ONE graph launch: filterbank tile, three band chains,
              band sum; the pack is already on the device)          vs  Demo.process_frame on the same pack (the restart route: host
              pack in, DoA out -- the parent's only live form)
  filterbank  filterbank_tile_kernel (micloc_filterbank_tile_f64)    vs  the one-shot micloc_filterbank_f64 on the same pack

at B = 1, F = 3 bands, G = 112 DoAs, M = 7.  Each figure is the median (min - max) of 11 calls after 2 warm-ups; the two arms of a
comparison alternate call by call in one process.  The matrices are random unit columns (timing does not depend on their values).
--out FILE writes the figures, the command and the source hashes as JSON (profiles/wideband/STREAM_RECORD.json).

    python tools/wideband_stream_time.py [--frames 12000] [--out profiles/wideband/STREAM_RECORD.json]
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

from tools.wideband_time import BANDS, FS, G, M, build, timed  # noqa: E402

SOURCES = ["haghighatshoarmuir2024_amd/csrc/filterbank.hip", "haghighatshoarmuir2024_amd/csrc/stream_bands.hip", "haghighatshoarmuir2024_amd/csrc/stream_windows.hip",
           "haghighatshoarmuir2024_amd/csrc/api_stream.hip", "haghighatshoarmuir2024_amd/csrc/api_bands.hip", "haghighatshoarmuir2024_amd/csrc/api_plan.hip", "haghighatshoarmuir2024_amd/csrc/api_internal.h", "haghighatshoarmuir2024_amd/csrc/rzcc.hip", "haghighatshoarmuir2024_amd/csrc/beamform.hip",
           "haghighatshoarmuir2024_amd/csrc/stht.hip", "haghighatshoarmuir2024_amd/streaming.py", "haghighatshoarmuir2024_amd/runtime.py",
           "haghighatshoarmuir2024_amd/localization_demo_snn.py", "tools/wideband_time.py", "tools/wideband_stream_time.py"]


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=12_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    demo, _ = build()
    T, B, F = args.frames, 1, len(BANDS)
    t = np.arange(T) / FS
    rng = np.random.RandomState(1)
    pack = ((np.sin(2 * np.pi * 2000 * t)[:, None] + 0.4 * rng.randn(T, M + 1)) * 2.0**12).astype(np.int16)  # a recorded pack: M + 1 channels
    x = torch.from_numpy(np.ascontiguousarray(pack[None, :, :-1], dtype=np.float64)).cuda()
    stream = demo.streaming_localizer(batch=B, max_tile=T)
    stream.push(x)         # eager: the first tile of this length
    stream.push_replay(x)  # captured
    tile = timed({"push_replay_tile": lambda: stream.push_replay(x), "process_frame_restart": lambda: demo.process_frame(pack)})
    s = stream.status()
    status = dict(frames_pushed=stream.t, frames_beamformed=s["frames"], overflow=s["overflow"], lag_failures=s["lag_failures"],
                  band_sum_failures=s["band_sum_failures"])  # (a stream that lost frames would have timed less work: recorded with the figures)
    lib = _lib.load()
    ba = demo.filterbank.ba_list
    bb, aa, n = runtime.pad_ba_list(ba)
    nfb = lib.micloc_filterbank_stream_state_bytes(F, n, B, M)
    state = torch.zeros(nfb, dtype=torch.uint8, device=x.device)
    xf = torch.empty((F, B, T, M), dtype=torch.float64, device=x.device)
    st = runtime._stream(x.device)

    def fb_tile():
        _lib.check(lib.micloc_filterbank_tile_f64(runtime._dptr(bb), runtime._dptr(aa), F, n, runtime._ptr(x), B, T, M, runtime._ptr(state), nfb,
                                                  runtime._ptr(xf), st), "filterbank_tile")

    fb = timed({"filterbank_tile": fb_tile, "filterbank_one_shot": lambda: runtime.filterbank(ba, x, out=xf)})
    row = dict(B=B, T=T, F=F, G=G, M=M, pack_seconds=T / FS, stream_status=status, **tile, **fb)
    print(json.dumps(row))
    record = dict(command="python tools/wideband_stream_time.py " + " ".join(sys.argv[1:] if argv is None else argv), device=torch.cuda.get_device_name(0),
                  method="HIP events around whole calls; median (min - max) of 11 calls after 2 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=[row])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
