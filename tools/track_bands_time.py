#!/usr/bin/env python3
"""Times wideband moving-target tracking, HIP events around whole calls, F = 3 bands, 7 microphones, 449 DoAs:

  fused     WidebandSNNLocalizer.track_batch / WidebandBeamformerLocalizer.track_batch: ONE library call -- the filterbank, every band's
            front end, track_bands_ws_kernel / track_bands_wsc_kernel (csrc/track.hip) and the combine
  composed  what a user had before that call existed (it runs on the parent commit as well): the filterbank, per band the pipeline with y
            stored (apply_to_signal(to_host=False) for a batch), the device sum of the magnitudes, Envelope.track -- in sub-batches of
            --chunk trials, so that the F + 2 arrays of 8 T G bytes per trial fit

at the sweep's shape (B = 1100, T = 4799) and at the script's recording (B = 2, T = 239 999).  Each figure is the median (min - max) of 11
calls after 2 warm-ups; the arms alternate call by call in one process.  The peak allocation of an arm is the rise of
torch.cuda.max_memory_allocated across one call of its own, taken before the timed calls.  --out FILE writes the figures, the command, the
commit, the box and the source hashes as JSON (profiles/track_bands/RECORD.json).

    python tools/track_bands_time.py [--methods snn,beamformer] [--shapes 1100x4799,2x239999] [--chunk 64] [--commit SHA]
                                       [--out profiles/track_bands/RECORD.json]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.wideband_time import timed  # noqa: E402

FS, M, G = 48_000, 7, 449
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0], [2400.0, 3400.0]]
SOURCES = ["haghighatshoarmuir2024_amd/csrc/track.hip", "haghighatshoarmuir2024_amd/csrc/track_rows.h", "haghighatshoarmuir2024_amd/csrc/track_bands.h",
           "haghighatshoarmuir2024_amd/csrc/api_bands.hip", "haghighatshoarmuir2024_amd/csrc/filterbank.hip", "haghighatshoarmuir2024_amd/csrc/rzcc.hip",
           "haghighatshoarmuir2024_amd/csrc/beamform.hip", "haghighatshoarmuir2024_amd/csrc/sweep.hip", "haghighatshoarmuir2024_amd/wideband.py",
           "haghighatshoarmuir2024_amd/runtime.py", "tools/wideband_time.py", "tools/track_bands_time.py"]


def build(method):
    """A three-band localizer with random matrices (the timing does not depend on their values)."""
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.filterbank import ButterworthFilterbank
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    rng = np.random.RandomState(0)
    if method == "snn":
        beamfs = [SNNBeamformer(geo, 10e-3, fr, np.asarray([1 / (2 * np.pi * np.mean(fr))] * 2), bipolar_spikes=True, fs=FS) for fr in BANDS]
        Ws = [rng.randn(2 * M, G) for _ in BANDS]
        return WidebandSNNLocalizer(beamfs, [W / np.linalg.norm(W, axis=0, keepdims=True) for W in Ws],
                                    ButterworthFilterbank(freq_bands=np.asarray(BANDS), order=1, fs=FS))
    beamfs = [Beamformer(geo, 10e-3, fr, fs=FS) for fr in BANDS]
    return WidebandBeamformerLocalizer(beamfs, [(rng.randn(M, G) + 1j * rng.randn(M, G)) / np.sqrt(2 * M) for _ in BANDS],
                                       ButterworthFilterbank(freq_bands=np.asarray(BANDS), order=2, fs=FS))


def composed(loc, env, x, chunk):
    """index [B, T] by the calls that exist without the band entries, `chunk` trials at a time."""
    import torch

    from haghighatshoarmuir2024_amd import runtime

    snn = hasattr(loc.beamfs[0], "tau_vec")
    B, T, _ = x.shape
    plans = loc.plans(np.arange(T) / FS) if snn else loc.plans()
    out = []
    for lo in range(0, B, chunk):
        xf = runtime.filterbank(loc.filterbank.ba_list, x[lo : lo + chunk])
        m = None
        for f, p in enumerate(plans):
            y = (p.snn_pipeline(xf[f], want_y=True, want_power=False) if snn else p.beamformer_pipeline(xf[f], want_y=True, want_power=False))["y"]
            a = y.abs()
            m = a if m is None else m.add_(a)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out.append(env.track(m))
    return torch.cat(out)


def peak_rise(fn, plans):
    """The rise of the peak allocation across one call that starts without the plans' cached workspaces."""
    import torch

    torch.cuda.synchronize()
    for p in plans:
        p.ws.buf = None
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def main(argv=None):
    import torch

    from haghighatshoarmuir2024_amd import runtime
    from haghighatshoarmuir2024_amd.utils import Envelope

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--methods", default="snn,beamformer")
    ap.add_argument("--shapes", default="1100x4799,2x239999")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--commit", default=None, help="the commit the working tree stands on, where git cannot be asked (recorded as given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    env = Envelope(rise_time=10e-3, fall_time=100e-3, fs=FS)  # the script's envelope
    rows = []
    for method in args.methods.split(","):
        loc = build(method)
        for shape in args.shapes.split(","):
            B, T = (int(v) for v in shape.split("x"))
            gen = torch.Generator(device="cuda").manual_seed(0)
            t = torch.arange(T, device="cuda", dtype=torch.float64) / FS
            x = torch.empty((B, T, M), dtype=torch.float64, device="cuda")
            for lo in range(0, B, 64):  # a tone in every band plus noise
                n = min(64, B - lo)
                x[lo : lo + n] = 0.3 * torch.randn((n, T, M), dtype=torch.float64, device="cuda", generator=gen)
                x[lo : lo + n] += sum(torch.sin(2 * np.pi * np.mean(fr) * t) for fr in BANDS)[None, :, None]
            arms = {"fused_track_batch": lambda: loc.track_batch(x, env)["index"], "composed_two_step": lambda: composed(loc, env, x, args.chunk)}
            same = bool(torch.equal(arms["fused_track_batch"](), arms["composed_two_step"]().to(torch.int32))) if method == "snn" else None
            plans = loc.plans(np.arange(T) / FS) if method == "snn" else loc.plans()
            peaks = {k: peak_rise(fn, plans) for k, fn in arms.items()}
            res = timed(arms, calls=11, warmup=2)
            row = dict(method=method, F=len(BANDS), B=B, T=T, G=G, M=M, chunk=args.chunk, fused_kernel=runtime.bands_track_is_fused(plans, method != "snn"),
                       index_equal=same, peak_alloc_bytes=peaks, **res)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del x
            torch.cuda.empty_cache()
    prop = torch.cuda.get_device_properties(0)
    git = lambda *a: subprocess.run(["git", "-C", ROOT, *a], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()  # noqa: E731
    head = git("rev-parse", "HEAD")
    record = dict(command="python tools/track_bands_time.py " + " ".join(sys.argv[1:] if argv is None else argv),
                  commit=args.commit or head or None, uncommitted=bool(git("status", "--porcelain")) if head else None,  # (None: no git to ask; the hashes say)
                  box=dict(device=torch.cuda.get_device_name(0), gcn_arch=getattr(prop, "gcnArchName", ""), compute_units=prop.multi_processor_count,
                           hip=torch.version.hip),
                  method="HIP events around whole calls; median (min - max) of 11 calls after 2 warm-ups; arms alternate call by call; peak "
                         "allocation: rise of max_memory_allocated across one call of the arm",
                  sources_sha256={rel: hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() for rel in SOURCES}, results=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
