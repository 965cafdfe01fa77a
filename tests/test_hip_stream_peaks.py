"""The streaming multi-source read-out on the MI355X (csrc/stream_peaks.hip behind micloc_stream_peaks_tile_f64; num_sources= of the
streaming localizers; include/micloc_hip.h "streaming, multi-source").

There is no tolerance anywhere: both sides of every comparison apply a deterministic rule to identical bits, so indices are compared with
== and values as raw 64-bit patterns, NaN slots included.

1. the entry alone on a synthetic ring the test owns, against tests/multisource_ref.py, through a sequence of counts;
2. the two spellings of the row rule (csrc/peaks.hip and csrc/peaks_rows.h) against each other;
3. every stream class end to end against the one-shot call, for three tilings, mid-stream and at the end;
4. push_replay against push, and num_sources= together with track=;
5. multi_target_sweep read out by the stream."""
import ctypes

import numpy as np
import pytest

import multisource_ref as R

pytestmark = pytest.mark.gpu

FS = 48_000
G65 = 65
DOA65 = np.linspace(-np.pi, np.pi, G65)  # a closed grid
POISON_I = -7
POISON_V = np.uint64(0x7FF8DEAD0000BEEF)  # a marked NaN


@pytest.fixture(scope="module")
def torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=np.float64).view(np.uint64)


def same(got, want, what=""):
    """Indices with ==, values as raw 64-bit patterns."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    if got.dtype.kind == "f" or want.dtype.kind == "f":
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)
    else:
        np.testing.assert_array_equal(got.astype(np.int64), want.astype(np.int64), err_msg=what)


# ---- 1. stage level, synthetic ring ------------------------------------------------------------------------------------------------------
def _grid(kind, G):
    if kind == R.LINEAR:
        return np.linspace(0.0, 1.0, G) if G > 1 else np.zeros(1)
    if kind == R.CIRCULAR:
        return np.arange(G) * (2 * np.pi / G)
    return np.linspace(-np.pi, np.pi, G)


PATTERNS = ("random", "plateaus", "ties", "one_nan", "all_nan", "seam_low", "seam_high")


def make_row(rng, G, pattern):
    p = rng.standard_normal(G)
    if pattern == "plateaus":
        p = rng.integers(0, 4, G).astype(np.float64)  # runs of equal neighbours
    elif pattern == "ties":
        p = np.zeros(G)
        p[rng.integers(0, G, max(1, min(G, 5)))] = 2.5  # equal maxima: the lower reported index goes first
    elif pattern == "one_nan":
        p[rng.integers(0, G)] = np.nan
    elif pattern == "all_nan":
        p[:] = np.nan
    elif pattern == "seam_low":  # the row's maximum sits on the seam, at G - 1: p[0] < p[G - 1]
        p[G - 1] = np.abs(p).max() + 2.0
        p[0] = p[G - 1] - 1.0
    elif pattern == "seam_high":  # p[0] >= p[G - 1]
        p[0] = np.abs(p).max() + 2.0
        p[G - 1] = p[0] if rng.integers(0, 2) else p[0] - 1.0
    return p


def _ref_row(p, doa, K, sep, rel, kind):
    idx, val = R.peaks_row(p, doa, K, sep, rel, kind)
    return idx.astype(np.int32), val.astype(np.float64).view(np.uint64)


class Ring:
    """window_power, power and the count word as the test owns them, the entry's outputs filled with poison, and a host model of what the
    rule says they hold."""

    def __init__(self, torch, rng, B, G, max_windows, K, kind, sep, rel):
        from haghighatshoarmuir2024_amd import _lib, runtime

        self.torch, self.rng, self.lib, self.runtime = torch, rng, _lib.load(), runtime
        self.B, self.G, self.mw, self.K, self.kind, self.rel = B, G, max_windows, K, kind, float(rel)
        self.doa = _grid(kind, G)
        self.sep = R.default_separation(self.doa) if sep == "default" else float(sep)
        dev = self.dev = torch.device("cuda", torch.cuda.current_device())
        self.h_power = np.zeros((B, G))
        self.h_ring = np.full((B, max_windows, G), 123.0)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.d_doa = torch.from_numpy(self.doa).to(dev)
        self.state = torch.full((256,), 0xA5, dtype=torch.uint8, device=dev)
        _lib.check(self.lib.micloc_stream_peaks_reset(runtime._ptr(self.state), 256, runtime._stream(dev)), "reset")
        shapes = dict(peaks=(B, K), window_peaks=(B, max_windows, K), latest_peaks=(B, K))
        self.want_i = {n: np.full(s, POISON_I, dtype=np.int32) for n, s in shapes.items()}
        self.want_v = {n: np.full(s, POISON_V, dtype=np.uint64) for n, s in shapes.items()}
        self.out_i = {n: torch.from_numpy(v.copy()).to(dev) for n, v in self.want_i.items()}
        self.out_v = {n: torch.from_numpy(v.copy().view(np.float64)).to(dev) for n, v in self.want_v.items()}
        self.c = self.r = self.skipped = 0
        self.row_no = 0

    def _row(self):
        self.row_no += 1
        return make_row(self.rng, self.G, PATTERNS[self.row_no % len(PATTERNS)])

    def call(self, c, running=True, windows=True):
        """Emit the windows [self.c, c) into the ring as a stream would, rewrite the running rows, run the entry, advance the model."""
        torch, rt = self.torch, self.runtime
        for n in range(max(self.c, c - self.mw), c):  # (older ones would be overwritten anyway)
            for b in range(self.B):
                self.h_ring[b, n % self.mw] = self._row()
        for b in range(self.B):
            self.h_power[b] = self._row()
        self.c = c
        d_power = torch.from_numpy(self.h_power).to(self.dev)
        d_ring = torch.from_numpy(self.h_ring).to(self.dev)
        self.count.fill_(c)
        o_i, o_v = self.out_i, self.out_v
        rc = self.lib.micloc_stream_peaks_tile_f64(
            rt._ptr(d_power) if running else None, rt._ptr(d_ring) if windows else None, rt._ptr(self.count), self.B, self.G, self.mw, rt._ptr(self.d_doa),
            self.kind, self.K, self.sep, self.rel, rt._ptr(self.state), 256, rt._ptr(o_i["peaks"]), rt._ptr(o_v["peaks"]), rt._ptr(o_i["window_peaks"]),
            rt._ptr(o_v["window_peaks"]), rt._ptr(o_i["latest_peaks"]), rt._ptr(o_v["latest_peaks"]), rt._stream(self.dev))
        assert rc == 0, rc
        # ---- the model ----
        ref = lambda p: _ref_row(p, self.doa, self.K, self.sep, self.rel, self.kind)  # noqa: E731
        if running:
            for b in range(self.B):
                self.want_i["peaks"][b], self.want_v["peaks"][b] = ref(self.h_power[b])
        if windows:
            for n in range(max(self.r, c - self.mw), c):
                for b in range(self.B):
                    self.want_i["window_peaks"][b, n % self.mw], self.want_v["window_peaks"][b, n % self.mw] = ref(self.h_ring[b, n % self.mw])
            if c > self.r:
                self.want_i["latest_peaks"][:] = self.want_i["window_peaks"][:, (c - 1) % self.mw]
                self.want_v["latest_peaks"][:] = self.want_v["window_peaks"][:, (c - 1) % self.mw]
            self.skipped += max(0, c - self.mw - self.r)
            self.r = c

    def check(self, what):
        st2 = (ctypes.c_int * 2)()
        assert self.lib.micloc_stream_peaks_status(self.runtime._ptr(self.state), st2, self.runtime._stream(self.dev)) == 0
        assert (int(st2[0]), int(st2[1])) == (self.r, self.skipped), (what, list(st2), self.r, self.skipped)
        for n in self.want_i:  # every row the rule writes holds the rule's bits, every other one the poison
            np.testing.assert_array_equal(_np(self.out_i[n]), self.want_i[n], err_msg=f"{what}: {n} (index)")
            np.testing.assert_array_equal(_bits(self.out_v[n]), self.want_v[n], err_msg=f"{what}: {n} (value)")


GS = [1, 2, 3, 64, 65, 449, 4096]
MWS = [1, 3, 8]
KS = [1, 2, 16]
SEPS = [0.0, "default", np.pi]
CASES = []
for _i, _G in enumerate(GS):
    for _j, _mw in enumerate(MWS):
        _n = 3 * _i + _j
        # B, K, kind, separation and threshold cycle with different periods, so every value meets every G and every ring depth
        CASES.append(pytest.param(_G, _mw, (1, 5)[(_i + _j) % 2], KS[(_i + _j) % 3], (_i + 2 * _j) % 3, SEPS[(2 * _i + _j) % 3], (0.0, 0.5)[(_n // 2) % 2],
                                  id=f"G{_G}-ring{_mw}"))


@pytest.mark.parametrize("G,max_windows,B,K,kind,sep,rel", CASES)
def test_entry_follows_the_count_on_a_synthetic_ring(torch, G, max_windows, B, K, kind, sep, rel):
    from haghighatshoarmuir2024_amd import _lib

    S = _lib.MICLOC_STREAM_PEAKS_SLOTS
    if G == 4096 and max_windows > 1:
        B = 1  # (the NumPy restatement walks every ring point in Python; B = 5 meets G = 4096 at the ring of one row)
    ring = Ring(torch, np.random.default_rng(1000 * G + max_windows), B, G, max_windows, K, kind, sep, rel)
    # none, none, one, none, several, more than the slots, more than the ring holds, none
    counts = [0, 0, 1, 1, 4, 4 + S + 3, 4 + S + 3 + max_windows + 5, 4 + S + 3 + max_windows + 5]
    before = 0
    for step, c in enumerate(counts):
        held = {n: (_np(ring.out_i[n]).copy(), _bits(ring.out_v[n]).copy()) for n in ("window_peaks", "latest_peaks")}
        ring.call(c)
        ring.check(f"step {step}: count {before} -> {c}")
        if c == before:  # the count did not move: nothing but the running rows changes
            for n, (i, v) in held.items():
                np.testing.assert_array_equal(_np(ring.out_i[n]), i, err_msg=f"step {step}: {n}")
                np.testing.assert_array_equal(_bits(ring.out_v[n]), v, err_msg=f"step {step}: {n}")
        before = c
    # the windows whose rows were overwritten before a call read them, from the counts alone
    assert ring.skipped == sum(max(0, c - max_windows - r) for r, c in zip([0] + counts, counts)) >= 5
    # the running read-out alone (window_power NULL, and max_windows 0), and the windows alone (power NULL): the other part is untouched
    ring.call(ring.c, windows=False)
    ring.check("running rows only")
    ring.call(ring.c + 2, running=False)
    ring.check("windows only")


def test_all_grid_kinds_thresholds_and_separations_meet(torch):
    """The axes the case list above cycles through, crossed in full at two small grids (a few rows each)."""
    for G in (3, 65):
        for kind in (R.LINEAR, R.CIRCULAR, R.CIRCULAR_CLOSED):
            for rel in (0.0, 0.5):
                for sep in SEPS:
                    for K in KS:
                        ring = Ring(torch, np.random.default_rng(G + 7 * kind + K), 2, G, 3, K, kind, sep, rel)
                        for c in (2, 7):
                            ring.call(c)
                        ring.check(f"G {G} kind {kind} rel {rel} sep {sep} K {K}")


# ---- 2. the two spellings ------------------------------------------------------------------------------------------------------------------
def test_the_two_spellings_of_the_row_rule_agree_bit_for_bit(torch):
    from haghighatshoarmuir2024_amd import _lib, runtime

    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = runtime._stream(dev)
    rng = np.random.default_rng(20241021)
    state = torch.empty(256, dtype=torch.uint8, device=dev)
    for case in range(200):
        G, mw, B, K = int(rng.choice(GS)), int(rng.choice(MWS)), int(rng.choice([1, 5])), int(rng.choice(KS))
        kind, rel = int(rng.integers(0, 3)), float(rng.choice([0.0, 0.5]))
        doa = _grid(kind, G)
        sep = [0.0, R.default_separation(doa), np.pi][int(rng.integers(0, 3))]
        rows = np.stack([make_row(rng, G, PATTERNS[(case + i) % len(PATTERNS)]) for i in range(B * mw)]).reshape(B, mw, G)
        d_rows, d_doa = torch.from_numpy(rows).to(dev), torch.from_numpy(doa).to(dev)
        i1 = torch.full((B * mw, K), POISON_I, dtype=torch.int32, device=dev)
        v1 = torch.zeros((B * mw, K), dtype=torch.float64, device=dev)
        _lib.check(lib.micloc_doa_peaks_f64(runtime._ptr(d_rows), B * mw, G, runtime._ptr(d_doa), kind, K, sep, rel, runtime._ptr(i1), runtime._ptr(v1), st),
                   "doa_peaks")
        i2 = torch.full((B, mw, K), POISON_I, dtype=torch.int32, device=dev)
        v2 = torch.zeros((B, mw, K), dtype=torch.float64, device=dev)
        li, lv = torch.full((B, K), POISON_I, dtype=torch.int32, device=dev), torch.zeros((B, K), dtype=torch.float64, device=dev)
        ri, rv = torch.full((B, K), POISON_I, dtype=torch.int32, device=dev), torch.zeros((B, K), dtype=torch.float64, device=dev)
        count = torch.full((1,), mw, dtype=torch.int32, device=dev)  # count 0 -> every row of the ring
        _lib.check(lib.micloc_stream_peaks_reset(runtime._ptr(state), 256, st), "reset")
        _lib.check(lib.micloc_stream_peaks_tile_f64(runtime._ptr(d_rows[:, 0].contiguous()), runtime._ptr(d_rows), runtime._ptr(count), B, G, mw,
                                                    runtime._ptr(d_doa), kind, K, sep, rel, runtime._ptr(state), 256, runtime._ptr(ri), runtime._ptr(rv),
                                                    runtime._ptr(i2), runtime._ptr(v2), runtime._ptr(li), runtime._ptr(lv), st), "stream_peaks_tile")
        what = f"case {case}: G {G} ring {mw} B {B} K {K} kind {kind} rel {rel} sep {sep}"
        same(i2.reshape(B * mw, K), i1, what)
        same(v2.reshape(B * mw, K), v1, what)
        same(li, i1.reshape(B, mw, K)[:, mw - 1], what + " (latest)")
        same(lv, v1.reshape(B, mw, K)[:, mw - 1], what + " (latest)")
        same(ri, i1.reshape(B, mw, K)[:, 0], what + " (running)")
        same(rv, v1.reshape(B, mw, K)[:, 0], what + " (running)")


# ---- 3. end to end, per class ------------------------------------------------------------------------------------------------------------------
T, WINDOW, HOP, K2, BATCH = 4000, 512, 256, 2, 3
T_GRAPH = 4096  # eight equal tiles of 512
BANDS = [[1000.0, 1600.0], [1600.0, 2400.0]]
MUSIC_FS, MUSIC_L, MUSIC_N, MUSIC_OV = 8000, 512, 128, 128
MUSIC_T, MUSIC_T_GRAPH = 3 * MUSIC_L + 300, 8 * 256
KEYS = ("peaks", "peak_power", "window_peaks", "window_peak_power")


def _geo():
    from micloc.array_geometry import CenterCircularArray

    return CenterCircularArray(4.5e-2, 7)


def _recording(fs, frames, freq, seed):
    """BATCH trials of two targets 90 degrees apart (sweep.synthesize_targets), a little noise on top: [BATCH, frames, 7]."""
    from haghighatshoarmuir2024_amd import sweep

    rng = np.random.RandomState(seed)
    t = np.arange(frames + 8) / fs
    out = []
    for b in range(BATCH):
        d = -2.0 + 0.9 * b
        _, sig = sweep.synthesize_targets(_geo(), fs, t, np.sin(2 * np.pi * freq * t), [d, d + np.pi / 2], [1.0, 0.8])
        out.append(sig[:frames] + 0.05 * rng.randn(frames, sig.shape[1]))
    return np.ascontiguousarray(np.stack(out))


def _host(d):
    out = {k: _np(v) for k, v in d.items() if k in KEYS + ("slice_peaks", "slice_peak_power", "track_index", "window_count", "slice_count")}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


class _Case:
    """One stream class at the test's shapes: the recording, the one-shot reference (computed once per length, read-only) and the stream."""

    multiple = 1  # tiles other than the last are multiples of this
    ring_kw = "max_windows"

    def __init__(self):
        self.x = _recording(FS, T_GRAPH, 1500.0, 3)
        self._one = {}

    def frames(self, graph):
        return T_GRAPH if graph else T

    def one(self, graph=False):
        if graph not in self._one:
            self._one[graph] = _host(self.one_shot(np.ascontiguousarray(self.x[:, : self.frames(graph)])))
        return self._one[graph]

    def tilings(self):
        n = self.frames(False)
        ragged = [16, 240, 1024, 48, 1600, 528] if self.multiple == 16 else [1, 255, 700, 1, 1333, 17]
        return {"one": [n], "256s": [256] * (n // 256) + ([n % 256] if n % 256 else []), "ragged": ragged + [n - sum(ragged)]}

    def merged(self, with_windows, without):
        out = dict(with_windows)
        out.update({k: without[k] for k in ("peaks", "peak_power")})
        return out

    def envelope(self):
        from haghighatshoarmuir2024_amd.utils import Envelope

        return Envelope(rise_time=1e-3, fall_time=10e-3, fs=FS)


class _Snn(_Case):
    multiple = 16

    def __init__(self):
        from micloc.snn_beamformer import SNNBeamformer

        super().__init__()
        tau = 1 / (2 * np.pi * 2000)
        self.bf = SNNBeamformer(_geo(), 10e-3, [1000.0, 2000.0], np.asarray([tau, tau]), bipolar_spikes=True, fs=FS)
        W = np.random.RandomState(11).randn(14, G65)
        self.W = W / np.linalg.norm(W, axis=0, keepdims=True)

    def one_shot(self, x):
        kw = dict(num_sources=K2, doa_list=DOA65)
        return self.merged(self.bf.localize_batch(self.W, x, window=WINDOW, hop=HOP, **kw), self.bf.localize_batch(self.W, x, **kw))

    def stream(self, x, max_tile, **kw):
        from haghighatshoarmuir2024_amd.streaming import ComplexStreamingLocalizer

        kw.setdefault("window", WINDOW), kw.setdefault("hop", HOP if kw["window"] else None)
        if kw.get("num_sources") is not None:
            kw.setdefault("doa_list", DOA65)
        return self.bf.streaming_localizer(self.W, batch=x.shape[0], total_frames=x.shape[1], max_tile=max_tile,
                                           wrap_tail=ComplexStreamingLocalizer.wrap_rows(x, len(self.bf.kernel)), **kw)


class _Complex(_Snn):
    multiple = 1

    def __init__(self):
        from micloc.beamformer import Beamformer

        _Case.__init__(self)
        self.bf = Beamformer(_geo(), 10e-3, [1000.0, 2000.0], fs=FS)
        rng = np.random.RandomState(12)
        self.W = rng.randn(7, G65) + 1j * rng.randn(7, G65)


class _WideSnn(_Case):
    multiple = 16

    def __init__(self):
        from micloc.filterbank import ButterworthFilterbank
        from micloc.snn_beamformer import SNNBeamformer
        from micloc.wideband import WidebandSNNLocalizer

        super().__init__()
        rng = np.random.RandomState(13)
        taus = [1 / (2 * np.pi * np.mean(fr)) for fr in BANDS]
        mats = [rng.randn(14, G65) for _ in BANDS]
        self.loc = WidebandSNNLocalizer([SNNBeamformer(_geo(), 10e-3, fr, np.asarray([t, t]), bipolar_spikes=True, fs=FS) for fr, t in zip(BANDS, taus)],
                                        [W / np.linalg.norm(W, axis=0, keepdims=True) for W in mats], ButterworthFilterbank(freq_bands=BANDS, order=1, fs=FS))

    def one_shot(self, x):
        kw = dict(num_sources=K2, doa_list=DOA65)
        return self.merged(self.loc.localize_batch(x, window=WINDOW, hop=HOP, **kw), self.loc.localize_batch(x, **kw))

    def stream(self, x, max_tile, **kw):
        kw.setdefault("window", WINDOW), kw.setdefault("hop", HOP if kw["window"] else None)
        kw.setdefault("doa_list", DOA65)
        L2 = len(self.loc.beamfs[0].kernel) // 2
        tail = self.loc.filterbank.evolve_batch(np.ascontiguousarray(x))[:, :, -L2:, :].contiguous()
        return self.loc.streaming_localizer(batch=x.shape[0], total_frames=x.shape[1], max_tile=max_tile, wrap_tail=tail, **kw)


class _WideComplex(_WideSnn):
    multiple = 1

    def __init__(self):
        from micloc.beamformer import Beamformer
        from micloc.filterbank import ButterworthFilterbank
        from micloc.wideband import WidebandBeamformerLocalizer

        _Case.__init__(self)
        rng = np.random.RandomState(14)
        self.loc = WidebandBeamformerLocalizer([Beamformer(_geo(), 10e-3, fr, fs=FS) for fr in BANDS], [rng.randn(7, G65) + 1j * rng.randn(7, G65) for _ in BANDS],
                                               ButterworthFilterbank(freq_bands=BANDS, order=2, fs=FS))


class _Music(_Case):
    ring_kw = "max_slices"

    def __init__(self):
        from micloc.music_beamformer import MUSIC

        self.m = MUSIC(geometry=_geo(), freq_range=[1000.0, 2000.0], doa_list=np.linspace(-np.pi, np.pi, 33), frame_duration=MUSIC_L / MUSIC_FS, fs=MUSIC_FS)
        self.x = _recording(MUSIC_FS, MUSIC_T_GRAPH, 1300.0, 5)
        self._one = {}

    def frames(self, graph):
        return MUSIC_T_GRAPH if graph else MUSIC_T

    def tilings(self):
        n = MUSIC_T
        ragged = [1, 300, 511, 7]
        return {"one": [n], "256s": [256] * (n // 256) + [n % 256], "ragged": ragged + [n - sum(ragged)]}

    def one_shot(self, x):
        from haghighatshoarmuir2024_amd.utils import find_doa_peaks

        out = dict(self.m.localize_batch(x, 1, MUSIC_OV / MUSIC_FS, MUSIC_N, num_sources=K2))
        B, S, G = out["spectrum"].shape
        i, v = find_doa_peaks(out["spectrum"].reshape(B * S, G), self.m.doa_list, K2)
        out.update(window_peaks=i.reshape(B, S, K2), window_peak_power=v.reshape(B, S, K2))
        out.update(slice_peaks=out["window_peaks"], slice_peak_power=out["window_peak_power"])
        return out

    def stream(self, x, max_tile, **kw):
        kw.pop("window", None), kw.pop("hop", None)
        return self.m.streaming_localizer(x.shape[0], 1, MUSIC_OV / MUSIC_FS, MUSIC_N, total_frames=x.shape[1], max_tile=max_tile, **kw)


CLASSES = {"snn": _Snn, "complex": _Complex, "wideband_snn": _WideSnn, "wideband_complex": _WideComplex, "music": _Music}
_CASES = {}


@pytest.fixture(params=list(CLASSES))
def case(request, torch):
    if request.param not in _CASES:
        _CASES[request.param] = CLASSES[request.param]()
    return _CASES[request.param]


def _keys(case):
    return KEYS + (("slice_peaks", "slice_peak_power") if isinstance(case, _Music) else ())


@pytest.mark.parametrize("tiling", ["one", "256s", "ragged"])
def test_stream_gives_the_one_shot_peaks_for_any_tiling(case, tiling):
    n = case.frames(False)
    x = np.ascontiguousarray(case.x[:, :n])
    one = case.one()
    nW = one["window_peaks"].shape[1]
    assert one["peaks"].shape == (BATCH, K2) and one["window_peaks"].shape == (BATCH, nW, K2) and nW >= 4
    assert (one["peaks"][:, 0] >= 0).all()
    tiles = case.tilings()[tiling]
    assert sum(tiles) == n and all(t % case.multiple == 0 for t in tiles[:-1]) and (tiling != "ragged" or 1 in tiles or case.multiple == 16)
    s = case.stream(x, max(tiles), num_sources=K2)
    t = 0
    for k in tiles:
        s.push(x[:, t : t + k, :])
        t += k
        w = s.windows()
        what = f"{tiling}: after {t} frames, {w['count']} windows"
        assert s.peaks_status() == (w["count"], 0), what
        same(w["window_peaks"], one["window_peaks"][:, w["first"] : w["count"]], what)
        same(w["window_peak_power"], one["window_peak_power"][:, w["first"] : w["count"]], what)
        latest = s.latest_peaks()
        assert len(latest) == 4
        if w["count"]:
            same(latest[2], one["window_peaks"][:, w["count"] - 1], what + " (latest)")
            same(latest[3], one["window_peak_power"][:, w["count"] - 1], what + " (latest)")
        else:
            assert (_np(latest[2]) == -1).all() and np.isnan(_np(latest[3])).all()
    out = s.finish()
    for key in _keys(case):
        same(out[key], one[key], f"{tiling}: {key}")
    same(s.latest_peaks()[0], one["peaks"], "running peaks")
    assert s.peaks_status() == (nW, 0)


def test_a_ring_of_two_windows_is_never_overrun(case):
    n = case.frames(False)
    x = np.ascontiguousarray(case.x[:, :n])
    one = case.one()
    nW = one["window_peaks"].shape[1]
    tiles = case.tilings()["256s"]
    s = case.stream(x, max(tiles), num_sources=K2, **{case.ring_kw: 2})
    t = 0
    for k in tiles:
        s.push(x[:, t : t + k, :])
        t += k
    w = s.windows()
    assert (w["count"], w["first"]) == (nW, nW - 2) and s.peaks_status() == (nW, 0)
    same(w["window_peaks"], one["window_peaks"][:, nW - 2 :], "the two newest rows")
    same(w["window_peak_power"], one["window_peak_power"][:, nW - 2 :], "the two newest rows")
    same(s.latest_peaks()[0], one["peaks"], "running peaks")
    same(s.latest_peaks()[1], one["peak_power"], "running peaks")


NOT_MUSIC = [n for n in CLASSES if n != "music"]


@pytest.mark.parametrize("case", NOT_MUSIC, indirect=True)  # (MUSIC's slices are its windows: there is no stream without them)
def test_without_windows_the_running_peaks_alone(case):
    n = case.frames(False)
    x = np.ascontiguousarray(case.x[:, :n])
    s = case.stream(x, n, num_sources=K2, window=None)
    s.push(x)
    out = s.finish()
    assert "window_peaks" not in out and len(s.latest_peaks()) == 2
    same(out["peaks"], case.one()["peaks"], "peaks")
    same(out["peak_power"], case.one()["peak_power"], "peak_power")
    assert s.peaks_status() == (0, 0)
    plain = case.stream(x, n, window=None)
    with pytest.raises(ValueError, match="num_sources"):
        plain.latest_peaks()
    plain.push(x)
    assert "peaks" not in plain.finish()


# ---- 4. the graph, and track= beside num_sources= -----------------------------------------------------------------------------------------
def _run(case, x, replay, **kw):
    n = x.shape[1]
    tile = n // 8
    s = case.stream(x, tile, **kw)
    for t in range(0, n, tile):
        (s.push_replay if replay else s.push)(x[:, t : t + tile, :])
    if replay:
        assert list(s._graphs) == [tile]  # captured on the length's second occurrence, replayed from then on
    latest = [_np(v) for v in s.latest_peaks()] if kw.get("num_sources") else None
    return _host(s.finish()), latest, s


def test_push_replay_gives_the_bits_of_push(case):
    x = np.ascontiguousarray(case.x[:, : case.frames(True)])
    one = case.one(graph=True)
    eager, eager_latest, _ = _run(case, x, False, num_sources=K2)
    graph, graph_latest, s = _run(case, x, True, num_sources=K2)
    nW = one["window_peaks"].shape[1]
    for key in _keys(case):
        same(graph[key], eager[key], f"replay against push: {key}")
        same(graph[key], one[key], f"replay against the one-shot call: {key}")
    for a, b in zip(graph_latest, eager_latest):
        same(a, b, "latest_peaks")
    assert s.peaks_status() == (nW, 0)


@pytest.mark.parametrize("case", NOT_MUSIC, indirect=True)  # (the MUSIC stream has no tracked read-out)
def test_num_sources_and_track_together(case):
    x =np.ascontiguousarray(case.x[:, : case.frames(True)])
    env = case.envelope()
    both, _, _ = _run(case, x, True, num_sources=K2, track=env)
    track_only, _, _ = _run(case, x, True, track=env)
    peaks_only, _, _ = _run(case, x, False, num_sources=K2)
    same(both["track_index"], track_only["track_index"], "track_index")
    assert "peaks" not in track_only
    for key in KEYS:
        same(both[key], peaks_only[key], key)
        same(both[key], case.one(graph=True)[key], key)


# ---- 5. the sweep ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["snn", "complex"])
def test_multi_target_sweep_read_out_by_the_stream(torch, method):
    from haghighatshoarmuir2024_amd import sweep

    if method not in _CASES:
        _CASES[method] = CLASSES[method]()
    c = _CASES[method]
    kw = dict(num_targets=2, num_sim=3, snr_db_vec=[0, 10], mode="parity", seed=0)
    peak_separation = (np.pi / 4) / 2  # multi_target_sweep's default: min_separation / 2
    ref = sweep.multi_target_sweep(c.bf, c.W, DOA65, **kw)
    got = sweep.multi_target_sweep(c.bf, c.W, DOA65, localizer=sweep.stream_multi_localizer(c.bf, c.W, DOA65, tile=1024, num_sources=2,
                                                                                           min_separation=peak_separation), **kw)
    for key in ("peaks", "peak_power", "err", "mae_deg", "resolved_rate"):
        same(got[key], ref[key], key)
    assert ref["peaks"].shape == (2, 3, 2)
