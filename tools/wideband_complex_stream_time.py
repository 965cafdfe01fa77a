#!/usr/bin/env python3
"""Times the wideband complex stream against the composition it replaces, HIP events around whole calls:

  tile      one WidebandComplexStreamingLocalizer.push_replay of a 12 000-frame pack (ONE graph launch: filterbank tile, one STHT, wrap
            rows, ONE band-pass tile launch for all bands, F contractions, accumulate, slide, band sum)   vs  the composition from the same
            tree, captured as one graph as well: the filterbank tile, F x ComplexStreamingLocalizer's tile launches on the bands' slices
            (each its own STHT, wrap rows, band-pass tile, contraction, accumulate, slide), micloc_stream_band_sum_f64.  Both arms copy the
            pack into their graph's input buffer first; the pack is already on the device.
  bandpass  stream_bands_bandpass_tile_kernel, one launch for the F * B * 2M chains (micloc_stream_complex_bands_bandpass_tile_f64, the
            launcher's choice of chains per workgroup)   vs  F launches of stream_bandpass_tile_kernel
            (micloc_stream_complex_bandpass_tile_f64 per band) on the same planar rows; at B = 64 also the one launch with 16, 32 and 64
            chains per workgroup forced

at B = 1 and B = 64, M = 7, F = 3, G = 112.  Each figure is the median (min - max) of 11 calls after 2 warm-ups; the arms of a comparison
alternate call by call in one process.  The matrices are random (timing does not depend on their values).
--out FILE writes the figures, the command, the device and the source hashes as JSON (profiles/wideband/COMPLEX_STREAM_RECORD.json).

    python tools/wideband_complex_stream_time.py [--batches 1,64] [--frames 12000] [--out profiles/wideband/COMPLEX_STREAM_RECORD.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.wideband_complex_time import BANDS, FS, G, M, build  # noqa: E402
from tools.wideband_time import timed  # noqa: E402

SOURCES = ["haghighatshoarmuir2024_amd/csrc/stream_bands_complex.hip", "haghighatshoarmuir2024_amd/csrc/stream_complex.hip",
           "haghighatshoarmuir2024_amd/csrc/stream_bands.hip", "haghighatshoarmuir2024_amd/csrc/filterbank.hip", "haghighatshoarmuir2024_amd/csrc/api_stream.hip", "haghighatshoarmuir2024_amd/csrc/api_bands.hip", "haghighatshoarmuir2024_amd/csrc/api_plan.hip", "haghighatshoarmuir2024_amd/csrc/api_internal.h",
           "haghighatshoarmuir2024_amd/csrc/beamform.hip", "haghighatshoarmuir2024_amd/csrc/stht.hip", "haghighatshoarmuir2024_amd/streaming.py",
           "haghighatshoarmuir2024_amd/runtime.py", "tools/wideband_time.py", "tools/wideband_complex_time.py", "tools/wideband_complex_stream_time.py"]


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime
    from haghighatshoarmuir2024_amd.runtime import _dptr, _ptr, _stream
    from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--frames", type=int, default=12_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    T, F = args.frames, len(BANDS)
    loc = build()
    lib = _lib.load()
    rng = np.random.RandomState(1)
    t = np.arange(T) / FS
    rows = []
    for B in [int(v) for v in args.batches.split(",")]:
        stream = loc.streaming_localizer(batch=B, max_tile=T)
        dev = stream.device
        st = _stream(dev)
        x = torch.from_numpy(np.sin(2 * np.pi * 1500 * t)[None, :, None] + 0.4 * rng.randn(B, T, M)).to(dev)
        stream.push(x)         # eager: the first tile of this length
        stream.push_replay(x)  # captured
        # the composition: the filterbank tile, one complex stream per band, the band sum -- as one graph
        singles = [ComplexStreamingLocalizer(beamf, W, B, max_tile=T) for beamf, W in zip(loc.beamfs, loc.bf_mats)]
        nfb = int(lib.micloc_filterbank_stream_state_bytes(F, stream.ncoef, B, M))
        fb_state = torch.empty(nfb, dtype=torch.uint8, device=dev)
        nbs = int(lib.micloc_stream_bands_state_bytes())
        bands_state = torch.empty(nbs, dtype=torch.uint8, device=dev)
        _lib.check(lib.micloc_filterbank_stream_reset(_ptr(fb_state), nfb, st), "filterbank_stream_reset")
        _lib.check(lib.micloc_stream_bands_reset(_ptr(bands_state), nbs, st), "stream_bands_reset")
        xf = torch.empty((F, B, T, M), dtype=torch.float64, device=dev)
        power = torch.empty((B, G), dtype=torch.float64, device=dev)
        argmax = torch.empty((B,), dtype=torch.int32, device=dev)
        p_power = (ctypes.c_void_p * F)(*[s.power.data_ptr() for s in singles])

        def composition_tile(x_in):
            _lib.check(lib.micloc_filterbank_tile_f64(_dptr(stream.bb), _dptr(stream.aa), F, stream.ncoef, _ptr(x_in), B, T, M, _ptr(fb_state), nfb,
                                                      _ptr(xf), st_now()), "filterbank_tile")
            for f, s in enumerate(singles):
                s._tile(xf[f], T, False)
            _lib.check(lib.micloc_stream_band_sum_f64(F, B, G, p_power, 0, 0, 0, None, None, _ptr(bands_state), nbs, _ptr(power), _ptr(argmax), None, None,
                                                      None, None, st_now()), "stream_band_sum")

        st_now = lambda: _stream(dev)  # noqa: E731  (the capture runs on a side stream)
        composition_tile(x)  # eager: lazy kernel set-up must not happen inside a capture
        x_in = torch.empty_like(x)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            composition_tile(x_in)
        torch.cuda.current_stream(dev).wait_stream(side)

        def composition_replay():
            x_in.copy_(x)
            graph.replay()

        tile = timed({"push_replay_tile": lambda: stream.push_replay(x), "composition_graph": composition_replay})
        s = stream.status()
        status = dict(frames_pushed=stream.t, frames_contracted=s["frames"], carry=s["carry"])  # (recorded with the figures: the work that was timed)
        # the band-pass stage alone, on the planar rows of the pack's filterbank output
        plan = stream.plan
        h = plan.stht(xf.view(F * B, T, M))
        Ts = h.shape[2]

        def bp_one(chains):
            def run():
                _lib.check(lib.micloc_stream_complex_bands_bandpass_tile_f64(stream.handles, F, _ptr(h), B, T, Ts, 0, stream.max_tile, chains,
                                                                             _ptr(stream.state), stream.nstate, _ptr(stream.ws), stream.nws, st), "bands_bandpass_tile")
            return run

        def bp_per_band():
            for f, sg in enumerate(singles):
                _lib.check(lib.micloc_stream_complex_bandpass_tile_f64(sg.plan.handle, _ptr(h[f * B : (f + 1) * B]), B, T, Ts, 0, sg.max_tile, _ptr(sg.state),
                                                                       sg.nstate, _ptr(sg.ws), sg.nws, st), "stream_complex_bandpass_tile")

        arms = {"bandpass_one_launch": bp_one(0), "bandpass_per_band": bp_per_band}
        if B >= 64:
            arms.update({f"bandpass_one_launch_ch{c}": bp_one(c) for c in (16, 32, 64)})
        bp = timed(arms)
        row = dict(B=B, T=T, G=G, M=M, F=F, chains=F * B * 2 * M, pack_seconds=T / FS, stream_status=status, **tile, **bp)
        print(json.dumps(row))
        rows.append(row)
    record = dict(command="python tools/wideband_complex_stream_time.py " + " ".join(sys.argv[1:] if argv is None else argv),
                  device=torch.cuda.get_device_name(0),
                  method="HIP events around whole calls; median (min - max) of 11 calls after 2 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
