"""Time one tile of the live loop (StreamingLocalizer.push_replay: one hipGraph launch per tile) with and without the multi-source read-out.

python tools/stream_peaks_time.py [--batch B] [--doas G] [--tile N] [--tiles K] [--warmup W] [--window N] [--hop N] [--sources K] [--out FILE] VARIANT...

VARIANT is `none` (no `window`: the running estimate only), `windows` (window= / hop=, one arg-max per window: the tile as it stood before
the read-out existed) or `peaks` (the same stream built with num_sources=K: micloc_stream_peaks_tile_f64 as the last launches of the tile's
graph).  One localizer per variant, all fed the same tiles of N frames (default 12 000: the demo's 0.25 s at 48 kHz) of band noise on the
7-microphone plan of the sweeps with a random unit-norm bf_mat of G columns (default 360, the headline shape) over np.linspace(-pi, pi, G);
window 1024, hop 512, K = 2 by default; a live source (no total_frames).  The variants take their tiles IN TURN -- tile k of every variant
before tile k + 1 of any -- so that they see the same box at the same time.  Every push_replay is timed by its own pair of HIP events on
the launch stream (the copy of the tile into the graph's input buffer included); the first W tiles of each variant (default 6: the eager
first push, the capture, the first replays) are left out.  Prints one JSON line per variant: median, min and max per tile in microseconds,
the windows emitted and, for `peaks`, the read-out's two counters.

`none` and `windows` run on any commit that has the streaming windows, so the same file times the parent commit's tile from a checkout
of it.  The kernel's own time per tile comes from a run of this file (variant `peaks` alone) under `rocprofv3 --kernel-trace --stats`,
the program behind `--`: stream_peaks_kernel and stream_peaks_commit_kernel, one launch each per tile.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from haghighatshoarmuir2024_amd.streaming import StreamingLocalizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--doas", type=int, default=360)
    ap.add_argument("--tile", type=int, default=12_000)
    ap.add_argument("--tiles", type=int, default=46)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("variants", nargs="+", choices=["none", "windows", "peaks"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs the GPU: a time taken anywhere else says nothing")
    if a.tiles <= a.warmup or a.warmup < 2:
        sys.exit("tiles must exceed warmup >= 2 (the first push is eager, the second is the capture)")
    from micloc.array_geometry import CenterCircularArray
    from micloc.snn_beamformer import SNNBeamformer

    fs, M, B, G, n = 48_000, 7, a.batch, a.doas, a.tile
    tau = 1 / (2 * np.pi * 2000)
    bf = SNNBeamformer(CenterCircularArray(4.5e-2, M), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=fs)
    rng = np.random.RandomState(0)
    W = rng.randn(2 * M, G)
    W /= np.linalg.norm(W, axis=0, keepdims=True)
    doa_list = np.linspace(-np.pi, np.pi, G)
    gen = torch.Generator(device="cuda").manual_seed(0)
    t = torch.arange(4 * n, device="cuda", dtype=torch.float64) / fs
    pool = torch.sin(2 * np.pi * 1500.0 * t)[None, :, None] + 0.5 * torch.randn((B, 4 * n, M), device="cuda", dtype=torch.float64, generator=gen)
    locs = []
    for v in a.variants:
        kw = {}
        if v != "none":
            kw = dict(window=a.window, hop=a.hop)
        if v == "peaks":
            kw.update(num_sources=a.sources, doa_list=doa_list)
        locs.append(StreamingLocalizer(bf, W, B, max_tile=n, **kw))
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.tiles)] for _ in locs]
    for k in range(a.tiles):
        x = pool[:, (k % 4) * n : (k % 4 + 1) * n, :]
        for i, s in enumerate(locs):
            ev[i][k][0].record()
            s.push_replay(x)
            ev[i][k][1].record()
    torch.cuda.synchronize()
    lines = []
    for v, s, e in zip(a.variants, locs, ev):
        us = np.asarray([e0.elapsed_time(e1) * 1e3 for e0, e1 in e[a.warmup :]])
        st = s.status()
        assert len(s._graphs) == 1 and st["lag_failures"] == 0 and st["overflow"] == 0, (v, st)
        r = dict(variant=v, B=B, G=G, tile=n, timed_tiles=len(us), median_us=round(float(np.median(us)), 1), min_us=round(float(us.min()), 1),
                 max_us=round(float(us.max()), 1), frames_beamformed=st["frames"], argmax0=int(s.argmax[0]))
        if v != "none":
            r.update(window=a.window, hop=a.hop, windows_emitted=s.windows()["count"])
        if v == "peaks":
            read, skipped = s.peaks_status()
            assert (read, skipped) == (r["windows_emitted"], 0), (read, skipped, r)
            r.update(sources=a.sources, windows_read=read, windows_skipped=skipped, peaks0=[int(i) for i in s.latest_peaks()[0][0].cpu()])
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
