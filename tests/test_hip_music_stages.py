"""MUSIC on the MI355X stage by stage (csrc/music.hip, csrc/stream_music.hip, csrc/music_rows.h) against tests/music_ref.py, through the
two C entries micloc_music_f64 and micloc_stream_music_tile_f64 with tables of the tests' own:

  exact tier     integer data, filters, DFT and steering tables: sel, spectrum, power and arg-max equal the integer reference BIT FOR BIT,
                 at every filter length the entries dispatch (n = 1 .. 9) and at the shape edges of the kernels; the stream equals the
                 one-shot call bit for bit for every tiling.  Exact ties of bin power and of the read-out, the all-zero recording.
  rounding tier  real data against the long-double chain, every stage within the first-order bound music_ref derives from the count
                 of roundings on its path; a stage is isolated by the probe tables (filter_probe, delta_steering).
  non-finite     a NaN or +Inf sample: the rank rule is total, so sel stays a list of distinct in-band bins, the call returns, and
                 every other slice and trial keeps its bits.

Figures of the first run on the MI355X (the device's worst deviation beside what it is held to; the tests print them):
  plan W against long-double cos / -sin     5.59, 7.44, 11.29 x 2^-53 at N = 64, 100, 333 (allowed 20 x 2^-53)
  DFT probe, N = 100                        |sqrt P - |X|| <= 1.62e-14, at most 0.0127 of its bound
  steering probe                            k = 0: 0.0066 of the bound (1.7e-16 of the maximum, the bound 2.7e-14), power 0.0037 of its bound;
                                            k = 3: 0.0095 (1.5e-16, 1.7e-14), power 0.0073
  filter probe, Butterworth order 1 .. 4    e_host 2.67e-16, 7.95e-16, 1.99e-15, 8.34e-15; device 1.85e-16, 4.70e-16, 1.61e-15, 5.16e-15
                                            (allowed 8 e_host = 2.14e-15, 6.36e-15, 1.59e-14, 6.67e-14): below the host route at every order
  whole chain                               spectrum 4.6e-16 of the maximum (bound 2.2e-13, 0.0021 of it; the fixed limit 1e-12), power 7.2e-16
The bounds are worst-case counts and the device sits at about a hundredth of them; a relative slip of 1e-12 is outside every one.
"""
import functools

import numpy as np
import pytest

import music_ref as R

from haghighatshoarmuir2024_amd import _lib, runtime
from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray

pytestmark = pytest.mark.gpu

U = R.U


# ---- the two C entries -------------------------------------------------------------------------------------------------------------
class Tables:
    """Device tables of one call: W [N, 2 nbin] (padded here to [Np, Cp]), steer_re / steer_im [nbin, M, G]."""

    def __init__(self, N, W, sre, sim):
        import torch

        self.N, self.nbin, self.M, self.G = N, W.shape[1] // 2, sre.shape[1], sre.shape[2]
        assert W.shape == (N, 2 * self.nbin) and sre.shape == sim.shape == (self.nbin, self.M, self.G)
        self.host = (np.asarray(W), np.asarray(sre), np.asarray(sim))
        self.W, self.sre, self.sim = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).cuda() for t in (R.pad_W(W, N), sre, sim))


def _results(B, S, ksel, G):
    """Result buffers filled with what no kernel writes: an entry that stays is seen."""
    import torch

    return dict(sel=torch.full((B, S, ksel), -1, dtype=torch.int32, device="cuda"),
                spectrum=torch.full((B, S, G), -7.0, dtype=torch.float64, device="cuda"),
                power=torch.full((B, G), -7.0, dtype=torch.float64, device="cuda"),
                argmax=torch.full((B,), -1, dtype=torch.int32, device="cuda"))


def one_shot(x, ba, L, hop, tab, k):
    """micloc_music_f64 on x [B, T, M] -> dict(rc, sel, spectrum, power, argmax) on the host."""
    import torch

    lib = _lib.load()
    x = np.asarray(x, dtype=np.float64)
    B, T, M = x.shape
    S = len(R.slices(T, L, hop))
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    bb, aa, n = runtime.pad_ba(*ba)
    out = _results(B, S, R.ksel_of(k, tab.nbin), tab.G)
    nbytes = lib.micloc_music_workspace_bytes(B, T, M, L, hop, S, tab.N, tab.nbin, tab.G, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p = runtime._ptr
    rc = lib.micloc_music_f64(p(xd), B, T, M, runtime._dptr(bb), runtime._dptr(aa), n, L, hop, S, tab.N, p(tab.W), tab.nbin, p(tab.sre), p(tab.sim),
                              tab.G, k, p(out["sel"]), p(out["spectrum"]), p(out["power"]), p(out["argmax"]), p(ws), nbytes, runtime._stream(xd.device))
    torch.cuda.synchronize()
    return dict({key: v.cpu().numpy() for key, v in out.items()}, rc=rc)


def stream(x, ba, L, hop, tab, k, tiles):
    """micloc_stream_music_tile_f64 on x [B, T, M] cut into `tiles` -> as one_shot, plus slice_argmax [B, S] and the newest slice."""
    import ctypes

    import torch

    lib = _lib.load()
    x = np.asarray(x, dtype=np.float64)
    B, T, M = x.shape
    assert sum(tiles) == T and min(tiles) >= 1
    S = len(R.slices(T, L, hop))
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    bb, aa, n = runtime.pad_ba(*ba)
    ksel = R.ksel_of(k, tab.nbin)
    out = _results(B, S, ksel, tab.G)
    out["slice_argmax"] = torch.full((B, S), -1, dtype=torch.int32, device="cuda")
    out["latest_spec"] = torch.full((B, tab.G), -7.0, dtype=torch.float64, device="cuda")
    out["latest_argmax"] = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    kk = min(k, tab.nbin)  # (the stream's rule: 0 or 1 .. nbin)
    dims = (B, M, L, hop, tab.N, tab.nbin, tab.G, kk, S)
    nstate = lib.micloc_stream_music_state_bytes(*dims)
    assert nstate > 0
    state = torch.empty(nstate, dtype=torch.uint8, device="cuda")
    p, st = runtime._ptr, runtime._stream(xd.device)
    assert lib.micloc_stream_music_reset(p(state), nstate, *dims, st) == _lib.MICLOC_OK
    t, rc = 0, _lib.MICLOC_OK
    for i, nt in enumerate(tiles):
        xt = xd[:, t : t + nt, :].contiguous()
        rc = lib.micloc_stream_music_tile_f64(p(state), nstate, p(xt), B, nt, M, int(i == len(tiles) - 1), runtime._dptr(bb), runtime._dptr(aa), n, L,
                                              hop, tab.N, p(tab.W), tab.nbin, p(tab.sre), p(tab.sim), tab.G, kk, S, p(out["power"]), p(out["argmax"]),
                                              p(out["latest_spec"]), p(out["latest_argmax"]), p(out["spectrum"]), p(out["sel"]), p(out["slice_argmax"]), st)
        if rc != _lib.MICLOC_OK:
            break
        t += nt
    st4 = (ctypes.c_int * 4)()
    assert lib.micloc_stream_music_status(p(state), st4, st) == _lib.MICLOC_OK
    torch.cuda.synchronize()
    assert rc != _lib.MICLOC_OK or list(st4) == [T, S, 0, 0], list(st4)
    return dict({key: v.cpu().numpy() for key, v in out.items()}, rc=rc)


def cut(T, n):
    return [n] * (T // n) + ([T % n] if T % n else [])


def assert_stream_equals_one_shot(got, one, what):
    assert got["rc"] == _lib.MICLOC_OK, what
    for key in ("sel", "spectrum", "power", "argmax"):
        assert np.array_equal(got[key], one[key], equal_nan=key in ("spectrum", "power")), f"{what}: {key} differs"
    finite = ~np.isnan(one["spectrum"]).any(axis=2)
    assert np.array_equal(got["slice_argmax"][finite], np.argmax(one["spectrum"], axis=2)[finite]), f"{what}: slice_argmax differs"
    assert np.array_equal(got["latest_spec"], one["spectrum"][:, -1], equal_nan=True), f"{what}: the newest slice differs"
    if finite[:, -1].all():
        assert np.array_equal(got["latest_argmax"], np.argmax(one["spectrum"][:, -1], axis=1)), what


# ---- the exact tier ----------------------------------------------------------------------------------------------------------------
def _sparse(rng, shape, per_column, axis0):
    """Integers in {-1, 0, 1}: `per_column` entries of +-1 along axis 0 (length axis0) for every index of the other axes; the first of
    them walks through every index of axis 0, so every row is read somewhere."""
    out = np.zeros(shape, dtype=np.int64).reshape(axis0, -1)
    cols = np.arange(out.shape[1])
    rows = np.concatenate([(cols % axis0)[None, :], rng.randint(0, axis0, (per_column - 1, len(cols)))])
    out[rows, cols[None, :]] = rng.choice([-1, 1], size=rows.shape)
    return out.reshape(shape)


# name -> the shape, the filter, the tilings of the stream.  Which edge a case is there for:
#   N = 64: no padding of the frame rows; 33, 65, 96, 300: padding to Np = 64, 128, 128, 320
#   nbin = 260 > 256 threads of the select kernel and of the stream's slice kernel; Cp = 528: five column blocks, the last of one tile
#   nbin = 70: Cp = 144, nine column tiles in two blocks, the second with 16 columns; nbin = 1: one column tile, 14 of its columns padding
#   B S M = 75 lanes of the filter kernel: two workgroups, the second partial; 75 frame rows: no multiple of 64
#   a leftover slice with fewer frames than a full one (cases "one", "wide", "frames3")
#   G = 1, 129 (a second steering block of 128), 257 (a third one, and a second pass of the read-out's loop over 256 threads)
#   k = 0, 1 (the ties below), nbin, > nbin, and in between
SHAPES = {
    "one": dict(B=1, T=198, M=1, L=128, hop=128, N=64, nbin=1, G=1, k=0, filt="n3", xmax=3, wn=3, sn=1, tilings=([198], cut(198, 1), cut(198, 37))),
    "lanes75": dict(B=5, T=288, M=5, L=96, hop=96, N=96, nbin=70, G=129, k=3, filt="n5", xmax=1, wn=2, sn=2, tilings=([288], cut(288, 37))),
    "wide": dict(B=1, T=950, M=2, L=600, hop=600, N=300, nbin=260, G=257, k=260, filt="n1", xmax=2, wn=2, sn=1, tilings=([950], cut(950, 97))),
    "wide, k > nbin": dict(B=1, T=950, M=2, L=600, hop=600, N=300, nbin=260, G=257, k=300, filt="n1", xmax=2, wn=2, sn=1, tilings=([950],),
                           like="wide"),  # the same recording and tables: k > nbin takes every bin, as k = nbin does
    "overlap": dict(B=2, T=170, M=2, L=130, hop=17, N=65, nbin=5, G=9, k=4, filt="n4", xmax=2, wn=3, sn=1, tilings=([170], cut(170, 1), cut(170, 50))),
    # divisions that round: F = 3 (every full slice), S = 3
    "frames3": dict(B=3, T=420, M=2, L=205, hop=100, N=65, nbin=5, G=7, k=2, filt="n3", xmax=2, wn=3, sn=1, tilings=([420], cut(420, 37))),
    "slices3": dict(B=1, T=132, M=2, L=66, hop=33, N=33, nbin=4, G=129, k=0, filt="n2", xmax=2, wn=3, sn=1, tilings=([132], cut(132, 37))),
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    c = SHAPES[name]
    if "like" in c:
        o = SHAPES[c["like"]]
        assert R.ksel_of(c["k"], c["nbin"]) == R.ksel_of(o["k"], o["nbin"]) and all(c[key] == o[key] for key in c if key not in ("k", "tilings", "like"))
        return shape_case(c["like"])
    rng = np.random.RandomState(len(name) + c["N"])
    x = rng.randint(-c["xmax"], c["xmax"] + 1, size=(c["B"], c["T"], c["M"]))
    W = _sparse(rng, (c["N"], 2 * c["nbin"]), c["wn"], c["N"])
    sre = np.moveaxis(_sparse(rng, (c["M"], c["nbin"], c["G"]), c["sn"], c["M"]), 0, 1)
    sim = np.moveaxis(_sparse(rng, (c["M"], c["nbin"], c["G"]), c["sn"], c["M"]), 0, 1)
    ba = R.INTEGER_FILTERS[c["filt"]]
    ref = R.exact_music(x, *ba, c["L"], c["hop"], c["N"], W, sre, sim, c["k"])
    return x, ba, Tables(c["N"], W, sre, sim), ref


def assert_exact(got, ref, what, spec_ulp=0, power_ulp=0):
    assert got["rc"] == _lib.MICLOC_OK, what
    assert np.array_equal(got["sel"], ref["sel"]), f"{what}: sel differs"
    if spec_ulp == 0:
        assert np.array_equal(got["spectrum"], ref["spectrum"]), f"{what}: spectrum differs"
    else:
        assert np.all(np.abs(got["spectrum"] - ref["spectrum"]) <= spec_ulp * np.spacing(ref["spectrum"])), f"{what}: spectrum differs"
    if power_ulp == 0:
        assert np.array_equal(got["power"], ref["power"]), f"{what}: power differs"
        assert np.array_equal(got["argmax"], ref["argmax"]), f"{what}: argmax differs"
    else:
        assert np.all(np.abs(got["power"] - ref["power"]) <= power_ulp * np.spacing(ref["power"])), f"{what}: power differs"
        assert np.array_equal(got["argmax"], np.argmax(got["power"], axis=1)), f"{what}: argmax is not the first maximum of power"


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_edges_equal_the_integer_reference_bit_for_bit(name):
    c = SHAPES[name]
    x, ba, tab, ref = shape_case(name)
    sl = R.slices(c["T"], c["L"], c["hop"])
    assert ref["S"] == len(sl)
    if name in ("one", "wide", "frames3"):
        assert sl[-1][1] // c["N"] < c["L"] // c["N"]  # the leftover slice has fewer frames
    if name == "lanes75":
        assert c["B"] * len(sl) * c["M"] == 75 and (c["B"] * len(sl) * c["M"] * (c["L"] // c["N"])) % 64
    # one rounding per division by 3 and per addition behind it: the spectrum within 1 ulp; P^2 then carries 2 ulp and the S sums one each
    ulps = dict(frames3=(1, 6 + len(sl)), slices3=(0, 1)).get(name, (0, 0))
    got = one_shot(x, ba, c["L"], c["hop"], tab, c["k"])
    assert_exact(got, ref, name, *ulps)
    for tiles in c["tilings"]:
        assert_stream_equals_one_shot(stream(x, ba, c["L"], c["hop"], tab, c["k"], tiles), got, f"{name}, tiles of {tiles[0]}")


# ---- every filter length, through the filter probe ---------------------------------------------------------------------------------
PROBE = dict(B=2, T=161, M=2, L=71, hop=40, N=33)  # F = 2; three full slices and a leftover one of 41 samples, F = 1


@functools.lru_cache(maxsize=None)
def probe_tables():
    N, M = PROBE["N"], PROBE["M"]
    return Tables(N, R.filter_probe(N, np.arange(N)), *R.delta_steering(N, M))


@pytest.mark.parametrize("name", list(R.INTEGER_FILTERS))
def test_every_filter_length_equals_the_integer_reference_bit_for_bit(name):
    """P[j M + m] = mean_f y_m[f N + j]^2: every filtered sample of every frame, squared, with nothing else added to it."""
    c = PROBE
    ba = R.INTEGER_FILTERS[name]
    rng = np.random.RandomState(len(ba[1]))
    x = rng.randint(-8, 9, size=(c["B"], c["T"], c["M"]))
    tab = probe_tables()
    ref = R.exact_music(x, *ba, c["L"], c["hop"], c["N"], *tab.host, 0)
    assert ref["S"] == 4 and np.count_nonzero(ref["spectrum"]) > 0.8 * ref["spectrum"].size
    # (the probe reads what the definition says: the difference equation's samples)
    y = R.exact_lfilter(*ba, x[0, 40 : 40 + 66])
    assert np.array_equal(ref["spectrum"][0, 1].reshape(c["N"], c["M"]), (y[:33].astype(float) ** 2 + y[33:].astype(float) ** 2) / 2)
    got = one_shot(x, ba, c["L"], c["hop"], tab, 0)
    assert_exact(got, ref, name)
    for tiles in ([c["T"]], cut(c["T"], 1), cut(c["T"], 37)):  # 37: cuts inside a chunk of 32 samples and inside a frame of 33
        assert_stream_equals_one_shot(stream(x, ba, c["L"], c["hop"], tab, 0, tiles), got, f"{name}, tiles of {tiles[0]}")


# ---- exact ties --------------------------------------------------------------------------------------------------------------------
TIE = dict(B=2, T=300, M=2, L=128, hop=64, N=64, nbin=6, G=257)
TIE_TILINGS = ([300], cut(300, 37))


def _tie_tables(rng):
    c = TIE
    W = _sparse(rng, (c["N"], 2 * c["nbin"]), 1, c["N"])
    sre = np.moveaxis(_sparse(rng, (c["M"], c["nbin"], c["G"]), 1, c["M"]), 0, 1)
    sim = np.moveaxis(_sparse(rng, (c["M"], c["nbin"], c["G"]), 1, c["M"]), 0, 1)
    return W, sre, sim


def test_equal_bin_powers_the_later_bin_sorts_later():
    c = TIE
    rng = np.random.RandomState(11)
    W, sre, sim = _tie_tables(rng)
    j1, j2 = 1, 4
    W[:, 2 * j1 : 2 * j1 + 2] = 2 * _sparse(rng, (c["N"], 2), 6, c["N"])  # the strongest bin by far ...
    W[:, 2 * j2 : 2 * j2 + 2] = W[:, 2 * j1 : 2 * j1 + 2]  # ... twice
    x = rng.randint(-3, 4, size=(c["B"], c["T"], c["M"]))
    ba = R.INTEGER_FILTERS["n3"]
    tab = Tables(c["N"], W, sre, sim)
    for k, want in ((1, [j2]), (2, [j1, j2]), (3, None)):
        ref = R.exact_music(x, *ba, c["L"], c["hop"], c["N"], W, sre, sim, k)
        pw = ref["pw"]
        assert np.array_equal(pw[..., j1], pw[..., j2]) and np.all(pw[..., j1] > np.delete(pw, [j1, j2], axis=-1).max(axis=-1))
        if want is not None:
            assert np.all(ref["sel"] == np.asarray(want))
        got = one_shot(x, ba, c["L"], c["hop"], tab, k)
        assert np.all(got["sel"][..., -2:] == np.asarray([j1, j2])[-min(k, 2) :])
        assert_exact(got, ref, f"k = {k}")
        for tiles in TIE_TILINGS:
            assert_stream_equals_one_shot(stream(x, ba, c["L"], c["hop"], tab, k, tiles), got, f"k = {k}, tiles of {tiles[0]}")


def test_equal_maxima_of_the_read_out_the_first_one_wins():
    c = TIE
    rng = np.random.RandomState(12)
    W, sre, sim = _tie_tables(rng)
    x = rng.randint(-3, 4, size=(1, c["T"], c["M"]))
    ba = R.INTEGER_FILTERS["n3"]
    first = int(R.exact_music(x, *ba, c["L"], c["hop"], c["N"], W, sre, sim, 2)["argmax"][0])
    g1, g2 = (first, c["G"] - 1) if first < c["G"] - 1 else (0, first)  # g2 = 256: the second pass of thread 0 over the directions
    src = first
    for t in (sre, sim):
        t[:, :, g1] = t[:, :, src]
        t[:, :, g2] = t[:, :, src]
    ref = R.exact_music(x, *ba, c["L"], c["hop"], c["N"], W, sre, sim, 2)
    assert g1 < g2 and ref["power"][0, g1] == ref["power"][0, g2] == ref["power"][0].max() and ref["argmax"][0] == g1
    assert np.array_equal(ref["spectrum"][0, :, g1], ref["spectrum"][0, :, g2])
    tab = Tables(c["N"], W, sre, sim)
    got = one_shot(x, ba, c["L"], c["hop"], tab, 2)
    assert got["argmax"][0] == g1
    assert_exact(got, ref, "two equal maxima")
    for tiles in TIE_TILINGS:
        s = stream(x, ba, c["L"], c["hop"], tab, 2, tiles)
        assert s["argmax"][0] == g1
        assert_stream_equals_one_shot(s, got, f"two equal maxima, tiles of {tiles[0]}")  # (slice_argmax: the first maximum of every slice)


@pytest.mark.parametrize("name,k", [("wide", 5), ("wide", 260), ("overlap", 0), ("lanes75", 3), ("one", 0)])
def test_all_zero_recording_ties_everything(name, k):
    c = SHAPES[name]
    x, ba, tab, _ = shape_case(name)
    x = np.zeros_like(x)
    ksel = R.ksel_of(k, c["nbin"])
    got = one_shot(x, ba, c["L"], c["hop"], tab, k)
    assert got["rc"] == _lib.MICLOC_OK
    assert np.all(got["sel"] == np.arange(c["nbin"] - ksel, c["nbin"]))  # the last ksel bins, ascending
    assert np.all(got["spectrum"] == 0) and np.all(got["power"] == 0) and np.all(got["argmax"] == 0)
    for tiles in c["tilings"][:1] + c["tilings"][-1:]:
        s = stream(x, ba, c["L"], c["hop"], tab, k, tiles)
        assert_stream_equals_one_shot(s, got, f"{name}, tiles of {tiles[0]}")
        assert np.all(s["slice_argmax"] == 0) and np.all(s["latest_argmax"] == 0)


# ---- the rounding tier -------------------------------------------------------------------------------------------------------------
FS = 8000
BAND = (1000.0, 2000.0)


def _music(M=7, G=33, band=BAND, frame_duration=0.025):
    from micloc.music_beamformer import MUSIC

    return MUSIC(geometry=CenterCircularArray(radius=4.5e-2, num_mic=M), freq_range=list(band), doa_list=np.linspace(-np.pi, np.pi, G),
                 frame_duration=frame_duration, fs=FS)


def _real_signal(rng, T, M, B=1):
    t = np.arange(T) / FS
    x = 0.3 * rng.randn(B, T, M)
    for f, amp in ((1300.0, 1.0), (1700.0, 0.5)):
        x += amp * np.sin(2 * np.pi * f * t[None, :, None] + rng.uniform(0, 2 * np.pi, (B, 1, M)))
    return x


IDENTITY = ([1.0], [1.0])


@pytest.mark.parametrize("N", [64, 100, 333])
def test_plan_dft_table_against_long_double(N):
    """cos / -sin of 2 pi ((k n) mod N) / N: three roundings of an angle up to 2 pi (2 pi, the product, the quotient: 3 x 2^-53 x 2 pi
    < 19 x 2^-53) and one ulp of the function."""
    pl = _music().plan(N)
    W = pl.W.cpu().numpy()
    nb = pl.nbin
    assert W.shape == ((N + 63) // 64 * 64, (2 * nb + 15) // 16 * 16) and nb >= 8
    ref = R.ld_dft_table(N, pl.bins)
    err = np.abs(W[:N, : 2 * nb].astype(R.LD) - ref)
    print(f"plan W, N = {N}: worst deviation {float(err.max()) / U:.2f} x 2^-53 (allowed 20)")
    assert err.max() <= 20 * U
    assert np.all(np.sign(W[1, 1 : 2 * nb : 2]) == -1)  # -sin: the angle of bin k at n = 1 is below pi for every in-band bin here
    assert not W[N:].any() and not W[:, 2 * nb :].any()


def test_dft_probe_one_dot_product_against_long_double():
    """The identity filter, the plan's own W with only the real or only the imaginary column of a bin kept, one frame, the delta steering:
    P = fl(X^2), the square of ONE dot product of the DFT.  sqrt(P) against the long-double product within dft_bound, plus the square's
    and the root's rounding (2 x 2 x 2^-53 |X|)."""
    N, M, B = 100, 3, 2
    pl = _music().plan(N)
    nb = pl.nbin
    Wp = pl.W.cpu().numpy()[:N, : 2 * nb]
    W = np.zeros((N, 4 * nb))
    W[:, 0::4] = Wp[:, 0::2]  # bin 2 j: (Re column of the plan's bin j, 0)
    W[:, 3::4] = Wp[:, 1::2]  # bin 2 j + 1: (0, Im column)
    tab = Tables(N, W, *R.delta_steering(2 * nb, M))
    x = _real_signal(np.random.RandomState(21), N, M, B)
    got = one_shot(x, IDENTITY, N, N, tab, 0)
    assert got["rc"] == _lib.MICLOC_OK
    fr = np.moveaxis(x, 1, 2).astype(R.LD)  # [B, M, N]
    Wl = W.astype(R.LD)
    X = fr @ Wl  # [B, M, 4 nb]
    col = X[..., 0::4], X[..., 3::4]
    ref = np.stack(col, axis=-1).reshape(B, M, 2 * nb)  # the non-zero column of bin j'
    bound = np.stack((R.dft_bound(np.abs(fr), Wl, 128)[..., 0::4], R.dft_bound(np.abs(fr), Wl, 128)[..., 3::4]), axis=-1).reshape(B, M, 2 * nb)
    bound = bound + 4 * U * np.abs(ref)
    dev = np.sqrt(got["spectrum"][:, 0].reshape(B, 2 * nb, M)).astype(R.LD)
    err = np.abs(dev - np.abs(np.moveaxis(ref, 1, 2)))
    ratio = err / np.moveaxis(bound, 1, 2)
    print(f"DFT probe, N = {N}, {2 * nb} columns x {B * M} rows: worst |sqrt P - |X|| = {float(err.max()):.3e}, worst deviation / bound = "
          f"{float(ratio.max()):.4f}, smallest bound {float(bound.min()):.3e}")
    assert np.all(err <= np.moveaxis(bound, 1, 2)) and err.max() > 0


@pytest.mark.parametrize("k", [0, 3])
def test_steering_probe_against_long_double(k):
    """The identity filter and a W of unit vectors: X[m, f, bin j] = x[f N + 2 j] + 1j x[f N + 2 j + 1] exactly; the plan's own steering
    table of the 7-microphone circular array.  Only music_steer_sum and the read-out remain."""
    N, M, G = 100, 7, 33
    pl = _music(M=M, G=G).plan(N)
    nb = pl.nbin
    W = np.zeros((N, 2 * nb))
    W[np.arange(2 * nb), np.arange(2 * nb)] = 1.0
    sre, sim = pl.sre.cpu().numpy(), pl.sim.cpu().numpy()
    tab = Tables(N, W, sre, sim)
    L, T = 2 * N, 2 * N + 150  # a full slice of two frames and a leftover one of one
    x = _real_signal(np.random.RandomState(22), T, M)
    got = one_shot(x, IDENTITY, L, L, tab, k)
    assert got["rc"] == _lib.MICLOC_OK
    specs, bounds = [], []
    for s, (start, length) in enumerate(R.slices(T, L, L)):
        F = length // N
        fr = x[0, start : start + F * N].T.reshape(M, F, N).astype(R.LD)
        re, im = fr[..., 0 : 2 * nb : 2], fr[..., 1 : 2 * nb : 2]
        pw = np.sum(re * re + im * im, axis=(0, 1)) / (M * F)
        order = np.argsort(pw.astype(float), kind="stable")
        sel = order[nb - R.ksel_of(k, nb) :]
        srt = pw[order]
        assert np.min(np.diff(srt) / srt[1:]) > 1e-9  # no near-tie: the order is not a matter of rounding
        assert np.array_equal(got["sel"][0, s], sel)
        P, dP = R.ld_steer(re, im, sre, sim, sel)
        specs.append(P), bounds.append(dP)
    specs, bounds = np.asarray(specs), np.asarray(bounds)
    assert len(specs) == 2
    err = np.abs(got["spectrum"][0] - specs)
    power, dpower = R.power_bound(specs, bounds)
    perr = np.abs(got["power"][0] - power)
    print(f"steering probe, k = {k}: worst spectrum deviation / bound = {float((err / bounds).max()):.4f} (deviation {float(err.max() / specs.max()):.2e}, "
          f"bound {float((bounds / specs.max()).max()):.2e} of the maximum); power deviation / bound = {float((perr / dpower).max()):.4f}")
    assert np.all(err <= bounds) and np.all(perr <= dpower) and err.max() > 0
    assert got["argmax"][0] == np.argmax(power.astype(float))


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_filter_probe_butterworth_band_passes_against_long_double(order):
    """n = 3, 5, 7, 9 on real data: P = fl(y^2) of every sample of one frame of 256.  The recurrence has no closed bound, so the yardstick
    is measured: e_host, the largest deviation of float64 scipy.signal.lfilter from the long-double recurrence on the same data.  The
    device is held to 8 e_host (the margin the design tests give a device route over its host route), and to not less than
    4 x 2^-53 max |y|."""
    from scipy.signal import butter, lfilter

    N, M = 256, 2
    b, a = butter(order, BAND, btype="bandpass", fs=FS)
    assert len(a) == 2 * order + 1
    x = _real_signal(np.random.RandomState(30 + order), N, M)
    y, _ = R.ld_lfilter(b, a, x[0])  # [N, M]
    e_host = float(np.max(np.abs(lfilter(b, a, x[0], axis=0) - y)))
    tol = max(8 * e_host, 4 * U * float(np.abs(y).max()))
    tab = Tables(N, R.filter_probe(N, np.arange(N)), *R.delta_steering(N, M))
    got = one_shot(x, (b, a), N, N, tab, 0)
    assert got["rc"] == _lib.MICLOC_OK
    dev = float(np.max(np.abs(np.sqrt(got["spectrum"][0, 0].reshape(N, M)).astype(R.LD) - np.abs(y))))
    print(f"filter probe, order {order} (n = {len(a)}): e_host = {e_host:.3e}, device deviation = {dev:.3e}, allowed {tol:.3e}, max |y| = {float(np.abs(y).max()):.3f}")
    assert dev <= tol
    s = stream(x, (b, a), N, N, tab, 0, cut(N, 37))
    assert np.array_equal(s["spectrum"], got["spectrum"])


def test_whole_chain_small_against_long_double():
    """M = 3, N = 64, two slices of three frames, five in-band bins, G = 7, the two strongest bins: the plan's tables and its order-1
    band-pass, end to end within music_ref's bound and within 1e-12 of the spectrum's maximum."""
    M, N, G, k = 3, 64, 7, 2
    m = _music(M=M, G=G, band=(1000.0, 1600.0))
    pl = m.plan(N)
    assert pl.nbin == 5
    L, T = 200, 400
    assert int(FS * m.frame_duration) == L
    x = _real_signal(np.random.RandomState(23), T, M)
    W = pl.W.cpu().numpy()[:N, : 2 * pl.nbin]
    sre, sim = pl.sre.cpu().numpy(), pl.sim.cpu().numpy()
    ba = m.filterbank.ba_list[0]
    ref = R.ld_music(x[0], *ba, L, L, N, W, sre, sim, k)
    assert ref["S"] == 2 and min(ref["gap"]) > 1e-6
    got = one_shot(x, ba, L, L, Tables(N, W, sre, sim), k)
    assert got["rc"] == _lib.MICLOC_OK and np.array_equal(got["sel"][0], ref["sel"])
    top = float(ref["spectrum"].max())
    err, bound = np.abs(got["spectrum"][0] - ref["spectrum"]), ref["spectrum_bound"]
    perr = np.abs(got["power"][0] - ref["power"])
    print(f"whole chain: worst spectrum deviation {float(err.max()) / top:.3e} of the maximum, worst bound {float(bound.max()) / top:.3e}, "
          f"worst deviation / bound {float((err / bound).max()):.4f}; power deviation / bound {float((perr / ref['power_bound']).max()):.4f}, "
          f"power deviation {float(perr.max() / ref['power'].max()):.3e} of the maximum")
    assert np.all(err <= bound) and np.all(perr <= ref["power_bound"])
    assert err.max() <= 1e-12 * top and perr.max() <= 1e-12 * float(ref["power"].max())
    assert got["argmax"][0] == np.argmax(ref["power"].astype(float))
    # the package's own call on the same recording runs the same kernels on the same tables
    out = m.localize_batch(x, k, 0.0, N, want_sel=True)
    assert np.array_equal(out["spectrum"].cpu().numpy(), got["spectrum"]) and np.array_equal(out["sel"].cpu().numpy(), got["sel"])


# ---- non-finite samples ------------------------------------------------------------------------------------------------------------
NF = dict(B=2, M=2, L=66, hop=66, N=33, nbin=6, G=9, T=198)  # three slices of two frames, back to back


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_nonfinite_sample_stays_in_its_slice(bad, k):
    """Trial 0 has one non-finite sample inside slice 1 of 3 (the band-pass carries it on, and 0 x NaN = NaN takes it into every bin of
    the slice: all its bin powers are NaN); trial 1 is clean."""
    c = NF
    rng = np.random.RandomState(40)
    W = _sparse(rng, (c["N"], 2 * c["nbin"]), 3, c["N"])
    sre = np.moveaxis(_sparse(rng, (c["M"], c["nbin"], c["G"]), 1, c["M"]), 0, 1)
    sim = np.moveaxis(_sparse(rng, (c["M"], c["nbin"], c["G"]), 1, c["M"]), 0, 1)
    ba = R.INTEGER_FILTERS["n3"]
    clean = rng.randint(-3, 4, size=(c["B"], c["T"], c["M"]))
    ref = R.exact_music(clean, *ba, c["L"], c["hop"], c["N"], W, sre, sim, k)
    assert ref["S"] == 3
    ksel = R.ksel_of(k, c["nbin"])
    x = clean.astype(np.float64)
    x[0, c["hop"] + 5, 1] = bad
    tab = Tables(c["N"], W, sre, sim)
    got = one_shot(x, ba, c["L"], c["hop"], tab, k)
    assert got["rc"] == _lib.MICLOC_OK
    sel = got["sel"]
    assert np.all((0 <= sel) & (sel < c["nbin"])) and all(len(set(row)) == ksel for row in sel.reshape(-1, ksel))
    want = ref["sel"].copy()
    want[0, 1] = R.select([float("nan")] * c["nbin"], ksel)  # the rule on a slice of NaN powers: the last ksel bins, ascending
    assert np.array_equal(want[0, 1], np.arange(c["nbin"] - ksel, c["nbin"])) and np.array_equal(sel, want)
    # trial 1: the bits of a run of trial 1 alone (and the clean reference's)
    alone = one_shot(x[1:], ba, c["L"], c["hop"], tab, k)
    for key in ("sel", "spectrum", "power", "argmax"):
        assert np.array_equal(got[key][1], alone[key][0]), key
        assert np.array_equal(got[key][1], ref[key][1]), key
    # trial 0: the untouched slices keep the clean run's bits; the read-out is NaN and its arg-max a direction
    assert np.array_equal(got["spectrum"][0, [0, 2]], ref["spectrum"][0, [0, 2]])
    assert np.isnan(got["spectrum"][0, 1]).all() and np.isnan(got["power"][0]).all()
    assert 0 <= got["argmax"][0] < c["G"]
    for tiles in ([c["T"]], cut(c["T"], 37)):
        s = stream(x, ba, c["L"], c["hop"], tab, k, tiles)
        assert_stream_equals_one_shot(s, got, f"tiles of {tiles[0]}")
        assert np.all((0 <= s["slice_argmax"]) & (s["slice_argmax"] < c["G"]))
