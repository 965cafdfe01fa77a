"""CPU checks of the time-resolved Xylo read-out for batches (include/micloc_hip.h "time-resolved DoA, Xylo"): the four
C-ABI symbols, the pure functions, every refusal in front of any launch (the pointers are dummies: a launch would fault), the window
count against utils.window_bounds, the command line's routing, and the premise of the GPU tests' reference on the oracle's raster."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from haghighatshoarmuir2024_amd import _lib
from haghighatshoarmuir2024_amd.utils import window_bounds
from oracle import oracle as O

INVALID, SHAPE, WORKSPACE = _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_SHAPE, _lib.MICLOC_ERR_WORKSPACE
NAMES = ("micloc_xylo_window_quantum", "micloc_xylo_windows_workspace_bytes", "micloc_xylo_lif_windows_i16", "micloc_xylo_window_readout")
# (T, window, hop) of the GPU tests
CASES = [(T, w, h) for T in (1, 255, 256, 257, 1100, 4799) for (w, h) in ((256, 256), (512, 256), (768, 256), (1024, 256), (1024, 1024), (8192, 256))]


def test_symbols_are_exported_bound_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    assert "time-resolved DoA, Xylo" in header
    for n in NAMES:
        assert n in _lib.SYMBOLS and hasattr(lib, n) and f"{n}(" in header, n
    assert lib.micloc_abi_version() == 1
    assert lib.micloc_xylo_window_quantum() == 256


def test_workspace_bytes_is_a_pure_function():
    lib = _lib.load()
    ws = lib.micloc_xylo_windows_workspace_bytes
    for bad in ((0, 100, 33), (-1, 100, 33), (65536, 100, 33), (1, 0, 33), (1, -5, 33), (1, 100, 0), (1, 100, -1)):
        assert ws(*bad) == 0, bad
    assert ws(3, 1100, 33) == ws(3, 1100, 33) > 0
    assert ws(1, 1, 1) == 256                                  # one chunk row of one neuron, padded to the alignment
    assert ws(1, 240_000, 449) == (938 * 449 * 4 + 255) // 256 * 256  # the footprint of DESIGN 4.25: 1.7 MB, not T x N
    for N in (33, 449, 513):
        prev = 0
        for B in (1, 2, 3, 64, 1100, 65535):
            assert ws(B, 4799, N) >= prev
            prev = ws(B, 4799, N)
        prev = 0
        for T in (1, 255, 256, 257, 1100, 4799, 48_000, 240_000):
            assert ws(3, T, N) >= prev and ws(3, T, N) >= 3 * -(-T // 256) * N * 4
            prev = ws(3, T, N)


def _lif(lib, **kw):
    a = dict(spikes=256, tc=14, B=2, T=1100, Cin=28, N=33, w_rec=0, max_spikes=31, window=1024, hop=256, wc=256, counts=None, net=256,
             net_bytes=1 << 20, ws=256, ws_bytes=1 << 20)
    a.update(kw)
    vp = ctypes.c_void_p
    return lib.micloc_xylo_lif_windows_i16(vp(a["spikes"]), a["tc"], a["B"], a["T"], a["Cin"], a["N"], a["w_rec"], a["max_spikes"], a["window"], a["hop"],
                                           vp(a["wc"]), vp(a["counts"]), vp(a["net"]), a["net_bytes"], vp(a["ws"]), a["ws_bytes"], None)


def _readout(lib, **kw):
    a = dict(wc=256, B=2, T=1100, window=1024, hop=256, G=33, bands=1, fs=48_000.0, win=1, rate=256, peak=256)
    a.update(kw)
    vp = ctypes.c_void_p
    return lib.micloc_xylo_window_readout(vp(a["wc"]), a["B"], a["T"], a["window"], a["hop"], a["G"], a["bands"], a["fs"], a["win"], vp(a["rate"]),
                                          vp(a["peak"]), None)


def test_every_refusal_comes_before_any_launch():
    """The pointers are dummies (address 256): had a check let the call through to a launch, the process would not return a status."""
    lib = _lib.load()
    # MICLOC_ERR_SHAPE: the window rule ...
    for kw in (dict(window=1000), dict(hop=100), dict(window=1024, hop=255), dict(window=0), dict(hop=0), dict(window=-256),
               dict(window=256, hop=512),                       # hop > window
               dict(B=65535, T=2**31 - 1, window=256, hop=256)):  # B nW > 2^31 - 1
        assert _lif(lib, **kw) == SHAPE, kw
        assert _readout(lib, **kw) == SHAPE, kw
    # ... and the shapes micloc_xylo_lif_resident_i16 refuses
    for kw in (dict(Cin=65, tc=0), dict(w_rec=-1, N=1025), dict(tc=-1), dict(tc=13), dict(tc=14, Cin=30)):
        assert _lif(lib, **kw) == SHAPE, kw
    # MICLOC_ERR_INVALID: NULL or out-of-range arguments
    for kw in (dict(spikes=None), dict(wc=None), dict(B=0), dict(B=65536), dict(T=0), dict(Cin=0), dict(N=0), dict(max_spikes=0)):
        assert _lif(lib, **kw) == INVALID, kw
    for kw in (dict(wc=None), dict(B=0), dict(B=65536), dict(T=0), dict(G=0), dict(bands=0), dict(fs=0.0), dict(fs=float("nan")),
               dict(rate=None, peak=None),                      # both outputs NULL
               dict(win=0), dict(win=2), dict(win=17), dict(win=-1), dict(G=16385, win=1)):  # what micloc_peak_location_i32 refuses
        assert _readout(lib, **kw) == INVALID, kw
    # MICLOC_ERR_WORKSPACE: a missing, short or misaligned buffer
    need_net, need_ws = lib.micloc_xylo_workspace_bytes(28, 33), lib.micloc_xylo_windows_workspace_bytes(2, 1100, 33)
    assert need_net > 0 and need_ws > 0
    for kw in (dict(net=None), dict(net_bytes=need_net - 1), dict(net=264), dict(ws=None), dict(ws_bytes=5 * 33 * 4 * 2 - 1), dict(ws=384 + 8)):
        assert _lif(lib, **kw) == WORKSPACE, kw


def test_window_count_agrees_with_window_bounds():
    lib = _lib.load()
    q = lib.micloc_xylo_window_quantum()
    for T, w, h in CASES:
        start, stop = window_bounds(T, w, h)
        assert lib.micloc_window_count(T, w, h, q) == len(start), (T, w, h)
        assert (stop > start).all() and stop[-1] == T          # every window holds frames, the last one ends the recording
    assert len(window_bounds(1100, 1024, 256)[0]) == 2 and window_bounds(1100, 1024, 256)[1][1] - 256 == 844
    assert len(window_bounds(1100, 768, 256)[0]) == 3
    assert len(window_bounds(4799, 8192, 256)[0]) == 1


def test_method_xylo_still_refuses_the_other_sweeps(capsys):
    from haghighatshoarmuir2024_amd import sweep

    for name in ("noisy", "speech", "xylo", "multi-noisy", "music-noisy", "wideband-speech"):
        with pytest.raises(SystemExit):
            sweep.main(["--sweep", name, "--method", "xylo"])
        assert "--method xylo" in capsys.readouterr().err
    with pytest.raises(SystemExit):  # the windowed sweep needs its window
        sweep.main(["--sweep", "windowed-noisy", "--method", "xylo"])
    assert "--window-frames" in capsys.readouterr().err


def test_cli_routes_windowed_noisy_xylo_to_the_xylo_sweep(monkeypatch, capsys):
    from haghighatshoarmuir2024_amd import sweep, xylo_snn_localization

    seen = {}

    class FakeDemo:
        def __init__(self, **kw):
            seen["demo"] = kw

    def fake_sweep(demo, window, hop=None, **kw):
        seen["call"] = (demo, window, hop, kw)
        return dict(snr_db_vec=np.zeros(1), mae_deg=np.zeros(1), window_mae_deg=np.zeros((1, 2)), window_start=np.array([0, 512]))

    def never(*a, **kw):
        raise AssertionError("the SNN windowed sweep ran")

    monkeypatch.setattr(xylo_snn_localization, "Demo", FakeDemo)
    monkeypatch.setattr(sweep, "xylo_windowed_target_sweep", fake_sweep)
    monkeypatch.setattr(sweep, "windowed_target_sweep", never)
    sweep.main(["--sweep", "windowed-noisy", "--method", "xylo", "--window-frames", "1024", "--hop-frames", "512", "--num-sim", "3", "--seed", "7",
                "--grid", "57", "--mode", "throughput"])
    demo, window, hop, kw = seen["call"]
    assert isinstance(demo, FakeDemo) and (window, hop) == (1024, 512)
    assert kw == dict(num_sim=3, seed=7, mode="throughput", rank=0, world_size=1)
    assert len(seen["demo"]["doa_list"]) == 57 and seen["demo"]["bipolar_spikes"] is True and seen["demo"]["fs"] == 48_000
    assert "Window starts" in capsys.readouterr().out
    # the hop defaults to the window inside the sweep
    sweep.main(["--sweep", "windowed-noisy", "--method", "xylo", "--window-frames", "2048"])
    assert seen["call"][1:3] == (2048, None) and seen["call"][3]["num_sim"] == 100


def test_the_general_walk_is_written_once():
    """csrc/xylo.hip defines the general walk once: xylo_lif_kernel<REC, NQ, CHUNKS>, whose chunk-count form is the lines marked CHUNKS under
    `if constexpr (CHUNKS)` and whose raster lines stand under `if constexpr (!CHUNKS)`; there is no second kernel to keep in step.  The
    packed form shares its walk (XpLif) and its flush (xp_chunk_done of xylo_rows.h, which the stream's tracking kernel calls too); no
    window kernel uses an atomic."""
    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    text = open(os.path.join(csrc, "xylo.hip")).read()
    assert len(re.findall(r"\bvoid xylo_lif_kernel\(", text)) == 1 and "xylo_lif_chunks_kernel" not in text
    assert re.search(r"template <bool REC, int NQ, bool CHUNKS = false>\s*__global__ [^\n]*void xylo_lif_kernel\(", text)
    at = text.index("void xylo_lif_kernel(")
    start = text.index("\n{\n", at) + 3
    body = text[start : text.index("\n}\n", start)].split("\n")
    raster = [i for i, ln in enumerate(body) if re.search(r"\bob\b", ln) and "ob = nullptr" not in ln]
    assert len(raster) == 2 and "spikes_out" in body[raster[0]] and "ob[" in body[raster[1]], raster
    for i in raster:  # each raster line is the statement of an `if constexpr (!CHUNKS)`
        assert "if constexpr (!CHUNKS)" in body[i] or body[i - 1].strip() == "if constexpr (!CHUNKS)", body[i]
    marked = [i for i, ln in enumerate(body) if "// CHUNKS" in ln]
    assert len(marked) == 3 and any("chunk_counts[" in body[i] for i in marked)
    # the count of the open chunk is a declaration; the flush, two adjacent lines, is the block of an `if constexpr (CHUNKS)`
    assert "int chunk_total = 0;" in body[marked[0]] and marked[2] == marked[1] + 1
    assert body[marked[1] - 1].strip() == "if constexpr (CHUNKS) {" and body[marked[2] + 1].strip() == "}"
    rows = open(os.path.join(csrc, "xylo_rows.h")).read()
    stream = open(os.path.join(csrc, "stream_xylo.hip")).read()
    assert "void xp_chunk_done(" in rows and "xp_chunk_done(lif" in text and "xp_chunk_done(lif" in stream and "sx_chunk_done" not in stream
    sweep = open(os.path.join(csrc, "sweep.hip")).read()
    for src, kernel in ((text, "xylo_window_kernel"), (sweep, "xylo_window_readout_kernel")):
        at = src.index(f"void {kernel}(")
        assert "atomic" not in src[at : src.index("\n}\n", at)].lower(), kernel
    # one statement of rate and peak: the one-shot kernels and the windowed read-out call the same device functions
    def kernel(name):
        at = sweep.index(f"void {name}(")
        return sweep[at : sweep.index("\n}\n", at)]

    assert "rate_from_counts_row(" in kernel("rate_from_counts_kernel") and "rate_from_counts_row(" in kernel("xylo_window_readout_kernel")
    assert "peak_location_row(" in kernel("peak_location_kernel") and "peak_location_row<true>(" in kernel("xylo_window_readout_kernel")


def test_oracle_premise_window_sums_add_up_to_the_counts():
    """The GPU tests' reference is O.xylo_lif's raster, window-summed in NumPy.  Its premise: the oracle's counts are the time sum of its
    raster, so with hop == window the windows add up to the counts and one window >= T is the counts -- with and without a recurrent
    weight, for uint8 event counts above 1, and with steps that emit two spikes and more."""
    rng = np.random.RandomState(5)
    T, Cin, N = 1100, 28, 33
    W = rng.randint(-127, 128, size=(Cin, N)).astype(np.int8)
    ds, dm = rng.randint(0, 7, size=N).astype(np.uint8), rng.randint(0, 7, size=N).astype(np.uint8)
    thr = rng.randint(50, 4001, size=N).astype(np.int16)
    events = (rng.rand(T, Cin) < 0.07).astype(np.uint8)
    events[100] = 3  # a row of event counts above 1
    for w_rec in (0, -1):
        out, counts = O.xylo_lif(events, W, w_rec, ds, dm, thr, 31)
        out = np.asarray(out).astype(np.int64)
        assert out.shape == (T, N) and int(out.max()) >= 2
        np.testing.assert_array_equal(out.sum(axis=0), np.asarray(counts))
        for window in (256, 1024):
            start, stop = window_bounds(T, window, window)
            rows = np.stack([out[a:b].sum(axis=0) for a, b in zip(start, stop)])
            np.testing.assert_array_equal(rows.sum(axis=0), np.asarray(counts))
        start, stop = window_bounds(T, 8192, 256)
        assert len(start) == 1
        np.testing.assert_array_equal(out[start[0] : stop[0]].sum(axis=0), np.asarray(counts))
