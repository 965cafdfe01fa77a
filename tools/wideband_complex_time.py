#!/usr/bin/env python3
"""Times the wideband complex Beamformer's entry against the composition it replaces, HIP events around whole calls:

  entry     micloc_beamformer_pipeline_bands_f64 (filterbank, ONE STHT launch, ONE band-pass launch, F contractions, one time
            reduction, band sum: 5 + F launches)   vs  the composition: micloc_filterbank_f64, F x micloc_beamformer_pipeline_f64 on the
            bands' slices, micloc_band_sum_f64 (2 + 4 F launches) -- both arms as C calls into buffers allocated beforehand
  bandpass  bands_bandpass_kernel, one launch for the F * B * 2M chains (micloc_beamformer_bands_bandpass_f64, STHT rows given)
            vs  the F one-shot band-pass launches on the same rows (the same entry with one_launch = 0)

at B = 1 and B = 64 packs of 12 000 frames, M = 7, F = 3, G = 112.  Each figure is the median (min - max) of 11 calls after 2 warm-ups;
the two arms of a comparison alternate call by call in one process.  The matrices are random (timing does not depend on their values).
--out FILE writes the figures, the command, the device and the source hashes as JSON (profiles/wideband/COMPLEX_RECORD.json).

    python tools/wideband_complex_time.py [--batches 1,64] [--frames 12000] [--out profiles/wideband/COMPLEX_RECORD.json]
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

from tools.wideband_time import timed  # noqa: E402

FS, M, G = 48_000, 7, 112
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]
SOURCES = ["haghighatshoarmuir2024_amd/csrc/bands_complex.hip", "haghighatshoarmuir2024_amd/csrc/filterbank.hip", "haghighatshoarmuir2024_amd/csrc/api_bands.hip", "haghighatshoarmuir2024_amd/csrc/api_plan.hip", "haghighatshoarmuir2024_amd/csrc/api_internal.h",
           "haghighatshoarmuir2024_amd/csrc/rzcc.hip", "haghighatshoarmuir2024_amd/csrc/beamform.hip", "haghighatshoarmuir2024_amd/csrc/stht.hip",
           "haghighatshoarmuir2024_amd/wideband.py", "haghighatshoarmuir2024_amd/runtime.py", "tools/wideband_time.py", "tools/wideband_complex_time.py"]


def build():
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.filterbank import ButterworthFilterbank
    from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    rng = np.random.RandomState(0)
    mats = [rng.randn(M, G) + 1j * rng.randn(M, G) for _ in BANDS]
    return WidebandBeamformerLocalizer([Beamformer(geo, 10e-3, fr, fs=FS) for fr in BANDS], mats, ButterworthFilterbank(freq_bands=BANDS, order=2, fs=FS))


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd import _lib, runtime
    from haghighatshoarmuir2024_amd.runtime import _dptr, _ptr, _stream

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--frames", type=int, default=12_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    T, F = args.frames, len(BANDS)
    loc = build()
    plans = loc.plans()
    lib = _lib.load()
    dev = plans[0].device
    st = _stream(dev)
    handles = (ctypes.c_void_p * F)(*[p.handle.value for p in plans])
    bb, aa, n = runtime.pad_ba_list(loc.filterbank.ba_list)
    rng = np.random.RandomState(1)
    t = np.arange(T) / FS
    rows = []
    for B in [int(v) for v in args.batches.split(",")]:
        x = torch.from_numpy(np.sin(2 * np.pi * 1500 * t)[None, :, None] + 0.4 * rng.randn(B, T, M)).to(dev)
        out = {k: (torch.empty((B, G), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)) for k in ("entry", "comp")}
        nbytes = lib.micloc_beamformer_bands_workspace_bytes(handles, F, B, T, 0, 0)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        xf = torch.empty((F, B, T, M), dtype=torch.float64, device=dev)
        bp = torch.empty((F, B, G), dtype=torch.float64, device=dev)
        nb1 = max(lib.micloc_workspace_bytes(p.handle, B, T) for p in plans)
        ws1 = torch.empty(nb1, dtype=torch.uint8, device=dev)

        def entry():
            _lib.check(lib.micloc_beamformer_pipeline_bands_f64(handles, F, _dptr(bb), _dptr(aa), n, _ptr(x), B, T, 0, 0, None, _ptr(out["entry"][0]),
                                                                _ptr(out["entry"][1]), _ptr(ws), nbytes, st), "beamformer_pipeline_bands")

        def composition():
            _lib.check(lib.micloc_filterbank_f64(_dptr(bb), _dptr(aa), F, n, _ptr(x), B, T, M, _ptr(xf), st), "filterbank")
            for f, p in enumerate(plans):
                _lib.check(lib.micloc_beamformer_pipeline_f64(p.handle, _ptr(xf[f]), B, T, None, _ptr(bp[f]), None, _ptr(ws1), nb1, st), "beamformer_pipeline")
            _lib.check(lib.micloc_band_sum_f64(_ptr(bp), F, B, G, _ptr(out["comp"][0]), _ptr(out["comp"][1]), st), "band_sum")

        whole = timed({"entry": entry, "composition": composition})
        torch.cuda.synchronize()
        same = bool(torch.equal(out["entry"][0], out["comp"][0]) and torch.equal(out["entry"][1], out["comp"][1]))  # (recorded with the figures)
        # the band-pass stage alone, on the STHT rows of the pack's filterbank output
        h, pre = runtime.beamformer_bands_bandpass(plans, xf)
        pre2 = torch.empty_like(pre)
        stage = timed({"bandpass_one_launch": lambda: runtime.beamformer_bands_bandpass(plans, xf, one_launch=True, pre=pre, h=h),
                       "bandpass_per_band": lambda: runtime.beamformer_bands_bandpass(plans, xf, one_launch=False, pre=pre2, h=h)})
        torch.cuda.synchronize()
        same_rows = bool(torch.equal(pre[..., :T], pre2[..., :T]))
        row = dict(B=B, T=T, G=G, M=M, F=F, chains=F * B * 2 * M, pack_seconds=T / FS, results_equal=same, bandpass_rows_equal=same_rows, **whole, **stage)
        print(json.dumps(row))
        rows.append(row)
    record = dict(command="python tools/wideband_complex_time.py " + " ".join(sys.argv[1:] if argv is None else argv), device=torch.cuda.get_device_name(0),
                  method="HIP events around whole calls; median (min - max) of 11 calls after 2 warm-ups; arms alternate call by call",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
