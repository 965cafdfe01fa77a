"""CPU-only checks of the tracked Xylo stream (include/micloc_hip.h "streaming, Xylo tracking"): the envelope recurrence
may be cut anywhere when only e[t-1] per neuron and the LIF state are carried, the frame-0 rule is observable, the ring arithmetic, the
new entries' pure answers and status codes, the host refusals, the header as plain C and the recurrence's single text.  The reference is
tests/xylo_track_ref.py (the oracle's integer LIF, Envelope.evolve, np.argmax).  PARITY UNPINNED for the LIF itself, as everywhere."""
import ctypes
import os
import types

import numpy as np
import pytest

import xylo_track_ref as R
from conftest import ROOT

from haghighatshoarmuir2024_amd import _lib

OK, INVALID, SHAPE, WORKSPACE = _lib.MICLOC_OK, _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_SHAPE, _lib.MICLOC_ERR_WORKSPACE
BIG = 1 << 30


# ---- the recurrence cut at launch borders ---------------------------------------------------------------------------------------
def _constants(w_rise, w_fall):
    wl = np.asarray([w_fall, w_rise])
    inv = 1 / wl
    a = 1 - inv
    return float(a[1]), float(inv[1]), float(a[0])


def _walk(counts, cuts, w_rise, w_fall, restart_at=(0,)):
    """The rule of the header over the ranges between `cuts`, carrying e[t-1] per neuron alone: counts [T, N] (the step counts: the LIF
    state is carried by whoever made them) -> (index [T], peak [T], env_last [N]).  e = m is taken at the absolute frames `restart_at`."""
    a_rise, i_rise, a_fall = _constants(w_rise, w_fall)
    T, N = counts.shape
    e = np.zeros(N)  # the reset state
    index, peak = np.zeros(T, np.int64), np.zeros(T)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for t in range(lo, hi):
            m = counts[t].astype(np.float64)
            e = m.copy() if t in restart_at else np.where(m >= e, a_rise * e + i_rise * m, a_fall * e)
            index[t] = int(np.argmax(e))
            peak[t] = e[index[t]]
    return index, peak, e


def _cut_sets(T, rng):
    k = sorted(set(rng.randint(1, T, size=9).tolist()))
    return [[0, T], list(range(0, T, 16)) + [T], [0] + k + [T], [0, T - 1, T]]


@pytest.mark.parametrize("w_rise,w_fall", [(1, 1), (2, 5), (48, 480)])
def test_the_recurrence_may_be_cut_anywhere(w_rise, w_fall):
    N, T = 33, 300
    out, _ = R.recipe_spikes(N, T)
    ref = R.recipe_reference(N, T, w_rise, w_fall)
    rng = np.random.RandomState(7)
    for b in range(out.shape[0]):
        for cuts in _cut_sets(T, rng):
            index, peak, e = _walk(out[b], cuts, w_rise, w_fall)
            np.testing.assert_array_equal(index, ref["index"][b])
            np.testing.assert_array_equal(peak.view(np.int64), ref["peak_env"][b].view(np.int64))
            np.testing.assert_array_equal(e.view(np.int64), ref["env_last"][b].view(np.int64))


@pytest.mark.parametrize("w_rise,w_fall", [(2, 5), (48, 480)])
def test_a_restart_anywhere_but_frame_0_is_observable(w_rise, w_fall):
    """A stream whose tap took e = m at position 0 of a raster window that has slid (or of every range) does not give the one-shot rows: on
    the recipe at N = 33, T = 300 every trial shows it at the tile and chunk borders 128 and 256, and the trial that fires every channel
    (the random trials are still silent there) at the first group border, 16."""
    N, T = 33, 300
    out, _ = R.recipe_spikes(N, T)
    ref = R.recipe_reference(N, T, w_rise, w_fall)
    for b in range(out.shape[0]):
        for at in (16, 128, 256) if b == 1 else (128, 256):
            index, peak, e = _walk(out[b], [0, at, T], w_rise, w_fall, restart_at=(0, at))
            assert not np.array_equal(peak.view(np.int64), ref["peak_env"][b].view(np.int64)), (b, at)
            np.testing.assert_array_equal(peak[:at].view(np.int64), ref["peak_env"][b, :at].view(np.int64))  # (the frames in front are the rule's)
    # and never taking it -- e[-1] = 0 from the reset, the recurrence at frame 0 -- is wrong at frame 0 whenever w_rise > 1
    index, peak, _ = _walk(out[1], [0, T], w_rise, w_fall, restart_at=())
    assert peak[0] != ref["peak_env"][1, 0]


# ---- ring arithmetic ------------------------------------------------------------------------------------------------------------
def test_ring_rows_and_ring_depth():
    from haghighatshoarmuir2024_amd.streaming import ring_rows, track_ring, track_setup

    assert ring_rows(0, 8) == (0, 0, [])
    assert ring_rows(5, 8) == (0, 5, [0, 1, 2, 3, 4])
    assert ring_rows(8, 8) == (0, 8, list(range(8)))
    assert ring_rows(19, 8) == (11, 8, [3, 4, 5, 6, 7, 0, 1, 2])
    env = R.envelope(48, 480)
    a_rise, i_rise, a_fall = _constants(48, 480)
    assert track_ring(env, 768) == (a_rise, i_rise, a_fall, 3072)            # the smallest multiple of 64 >= 4 x most
    assert track_ring(env, 800)[3] == 3200 and track_ring(env, 801)[3] == 3264
    assert track_ring(env, 768, total_frames=100)[3] == 768                  # never below most
    assert track_ring(env, 768, total_frames=6000)[3] == 6000
    assert track_ring(env, 768, total_frames=6000, max_track=768)[3] == 768
    with pytest.raises(ValueError, match="max_track"):
        track_ring(env, 768, max_track=767)
    with pytest.raises(ValueError, match="one sample"):
        track_ring(R.envelope(0, 5), 768)
    # track_setup is track_ring behind the fused route's refusal, which the Xylo stream does not share
    assert track_setup(env, 14, 33, False, 768, 6000, None) == track_ring(env, 768, 6000, None)
    with pytest.raises(ValueError, match="fused"):
        track_setup(env, 28, 33, False, 768)
    with pytest.raises(ValueError, match="fused"):
        track_setup(env, 14, 513, False, 768)


# ---- the C-ABI without a device ---------------------------------------------------------------------------------------------------
def test_symbols_and_size_functions():
    lib = _lib.load()  # raises if a declared symbol is missing
    text = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    assert "streaming, Xylo tracking" in text
    for name in ("micloc_xylo_stream_track_state_bytes", "micloc_xylo_stream_track_workspace_bytes", "micloc_xylo_stream_track_reset",
                 "micloc_xylo_lif_track_resume_i16", "micloc_stream_xylo_tile_track_i16"):
        assert name in text and name in _lib.SYMBOLS and hasattr(lib, name), name
    st, ws = lib.micloc_xylo_stream_track_state_bytes, lib.micloc_xylo_stream_track_workspace_bytes
    # [B][N rounded up to 512 / 2] lane pairs of two doubles; the LIF state's layout and size are unchanged
    assert st(3, 449) == 3 * 256 * 16 and st(1, 513) == 512 * 16 and st(2, 1100) == 2 * 768 * 16
    assert lib.micloc_xylo_stream_state_bytes(3, 449) == 3 * 256 * 16
    for bad in ((0, 449), (3, 0), (70000, 449), (-1, 449)):
        assert st(*bad) == 0, bad
    # one neuron block: the workgroup writes the ring itself; never 0 for valid arguments
    for N in (1, 33, 449, 512):
        assert ws(3, N, 16640) == 256 and ws(1, N, 1) == 256
    for N, blocks in ((513, 2), (1100, 3)):
        nb = ws(3, N, 16640)
        assert 12 * 3 * 16640 * blocks <= nb <= 12 * 3 * 16640 * blocks + 512 and nb % 256 == 0
    assert ws(1, 449, 240_000) < 240_000 * 449  # nothing of size T x N
    for bad in ((0, 449, 768), (3, 0, 768), (3, 449, 0), (3, 449, -5), (70000, 449, 768)):
        assert ws(*bad) == 0, bad


def test_track_resume_entry_validates_before_any_launch():
    lib = _lib.load()
    vp = ctypes.c_void_p
    one = vp(256)  # a non-null, 256-byte aligned dummy: validation must fail before it is ever dereferenced
    f = lib.micloc_xylo_lif_track_resume_i16
    good = dict(raster=one, tc=14, stride=700, B=3, t0=16, n=100, Cin=28, N=449, ms=31, state=one, sb=BIG, ts=one, tb=BIG, R=128, index=one, peak=one,
                lidx=one, lpeak=one, env_last=one, counts=one, ws=one, wb=BIG, tws=one, twb=BIG)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["raster"], a["tc"], a["stride"], a["B"], a["t0"], a["n"], a["Cin"], a["N"], a["ms"], a["state"], a["sb"], a["ts"], a["tb"], 0.5, 0.5,
                 0.8, a["R"], a["index"], a["peak"], a["lidx"], a["lpeak"], a["env_last"], a["counts"], a["ws"], a["wb"], a["tws"], a["twb"], None)

    for name in ("raster", "counts", "state", "ws", "ts", "index", "peak", "lidx", "lpeak", "env_last", "tws"):
        assert call(**{name: None}) == INVALID, name
    for kw in (dict(B=0), dict(stride=0), dict(t0=-16), dict(n=-1), dict(N=0), dict(ms=0), dict(tc=0), dict(R=0)):
        assert call(**kw) == INVALID, kw
    assert call(t0=8) == SHAPE                      # t0 % 16
    assert call(Cin=27) == SHAPE                    # Cin != 2 x ternary channels
    assert call(tc=33, Cin=66) == SHAPE             # Cin > 64
    assert call(t0=688, n=100) == SHAPE             # past the trial stride
    assert call(raster=vp(264)) == SHAPE            # raster not 16-byte aligned
    assert call(R=99) == SHAPE                      # a ring below what the call makes final
    assert call(sb=3 * 256 * 16 - 1) == WORKSPACE   # short LIF state
    assert call(tb=3 * 256 * 16 - 1) == WORKSPACE   # short envelope state
    assert call(ts=vp(264)) == WORKSPACE            # misaligned envelope state
    assert call(wb=100) == WORKSPACE                # short network workspace
    assert call(twb=255) == WORKSPACE               # short scratch (one neuron block: 256)
    assert call(N=1100, sb=BIG, tb=BIG, twb=lib.micloc_xylo_stream_track_workspace_bytes(3, 1100, 100) - 1) == WORKSPACE
    assert call(tws=vp(264)) == WORKSPACE
    r = lib.micloc_xylo_stream_track_reset
    assert r(None, BIG, 3, 449, None) == INVALID and r(one, BIG, 0, 449, None) == INVALID and r(one, BIG, 3, 0, None) == INVALID
    assert r(one, 3 * 256 * 16 - 1, 3, 449, None) == WORKSPACE and r(vp(264), BIG, 3, 449, None) == WORKSPACE


def test_tile_track_entry_refuses_without_a_plan():
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    f = lib.micloc_stream_xylo_tile_track_i16
    tail = (one, BIG, 0.5, 0.5, 0.8, 768, one, one, one, one, one, one, BIG, None)
    # the entries of a band's stream take the band's plan: without one they refuse (a plan needs a device)
    assert f(None, one, one, BIG, one, 1, 768, 0, 33, 31, one, one, BIG, one, BIG, None, 0, None, 0, 0, 0, 0, *tail) == INVALID
    assert f(None, one, one, BIG, one, 1, 768, 0, 33, 31, one, one, BIG, one, BIG, one, BIG, one, BIG, 1024, 512, 4, *tail) == INVALID
    # windows without the chunk-count scratch
    assert f(None, one, one, BIG, one, 1, 768, 0, 33, 31, one, one, BIG, one, BIG, None, 0, one, BIG, 1024, 512, 4, *tail) == INVALID


# ---- the host refusals --------------------------------------------------------------------------------------------------------------
def _standin(F=1, M=7, G=33):
    """What XyloStreamingLocalizer reads of a Demo before it touches the device."""
    C = 2 * M
    spec = dict(W_in=np.zeros((2 * F * C, F * G), np.int8), w_rec=0, dash_syn=np.zeros(F * G, np.uint8), dash_mem=np.zeros(F * G, np.uint8),
                threshold=np.ones(F * G, np.int16))
    beamf = types.SimpleNamespace(geometry=[0] * M)
    return types.SimpleNamespace(spec=spec, bipolar_spikes=True, beamfs=[beamf] * F, doa_list=np.linspace(-np.pi, np.pi, G), fs=48_000)


def test_localizer_refuses_before_any_device_work():
    from haghighatshoarmuir2024_amd.streaming import XyloStreamingLocalizer

    env = R.envelope(48, 480)
    with pytest.raises(ValueError, match="one band"):
        XyloStreamingLocalizer(_standin(F=2), 2, track=env)
    with pytest.raises(ValueError, match="one sample"):
        XyloStreamingLocalizer(_standin(), 2, track=R.envelope(0, 480))
    with pytest.raises(ValueError, match="give track as well"):
        XyloStreamingLocalizer(_standin(), 2, max_track=100_000)
    # cap = max_tile + lag_frames + two chunks, rounded up to a chunk: 1600 + 4096 + 512 -> 6400
    with pytest.raises(ValueError, match="6400"):
        XyloStreamingLocalizer(_standin(), 2, max_tile=1600, track=env, max_track=6399)
    with pytest.raises(ValueError, match="bipolar"):  # (the refusals without tracking are still in front)
        XyloStreamingLocalizer(types.SimpleNamespace(**dict(vars(_standin()), bipolar_spikes=False)), 2, track=env)


def test_track_resume_refuses_before_any_device_call():
    import torch

    from haghighatshoarmuir2024_amd.xylo_snn_localization import XyloNetwork

    net = XyloNetwork.__new__(XyloNetwork)  # (the constructor uploads the network: no device here)
    net.Cin, net.N, net.w_rec = 28, 33, -1
    raster = torch.zeros((2, 64, 14), dtype=torch.int8)
    env = R.envelope(2, 5)
    with pytest.raises(ValueError, match="w_rec"):
        net.new_track_state(2)
    with pytest.raises(ValueError, match="w_rec"):
        net.track_resume(raster, 0, 16, None, None, env)
    net.w_rec = 0
    with pytest.raises(ValueError, match="int8"):
        net.track_resume(raster.to(torch.uint8), 0, 16, None, None, env)
    with pytest.raises(ValueError, match="multiple of 16"):
        net.track_resume(raster, 8, 16, None, None, env)
    with pytest.raises(ValueError, match="channels"):
        net.track_resume(raster[:, :, :13].contiguous(), 0, 16, None, None, env)
    st = dict(B=2)
    with pytest.raises(ValueError, match="does not fit"):
        net.track_resume(raster, 48, 17, st, st, env)
    with pytest.raises(ValueError, match="does not fit"):
        net.track_resume(raster, 0, 16, st, dict(B=3), env)
    with pytest.raises(ValueError, match="one sample"):
        net.track_resume(raster, 0, 16, st, st, R.envelope(0, 5))
    with pytest.raises(ValueError, match="ring"):
        net.track_resume(raster, 0, 16, st, st, env, out=dict(index=torch.zeros((2, 8), dtype=torch.int32)))


# ---- the header and the source ----------------------------------------------------------------------------------------------------
def test_header_with_the_xylo_tracking_section_is_plain_c(tmp_path):
    import shutil
    import subprocess

    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this host")
    src = tmp_path / "xylo_stream_track_c.c"
    src.write_text(
        '#include "micloc_hip.h"\n#include <stdio.h>\n'
        "int main(void) {\n"
        '    printf("%zu %zu %d\\n", micloc_xylo_stream_track_state_bytes(3, 449), micloc_xylo_stream_track_workspace_bytes(3, 449, 768),\n'
        "           micloc_xylo_lif_track_resume_i16(NULL, 14, 700, 3, 0, 16, 28, 449, 31, NULL, 0, NULL, 0, 0.5, 0.5, 0.8, 64, NULL, NULL, NULL, NULL,\n"
        "                                            NULL, NULL, NULL, 0, NULL, 0, NULL));\n"
        "    if (micloc_xylo_stream_track_reset(NULL, 0, 3, 449, NULL) != MICLOC_ERR_INVALID) return 1;\n"
        "    return micloc_stream_xylo_tile_track_i16(NULL, NULL, NULL, 0, NULL, 1, 768, 0, 33, 31, NULL, NULL, 0, NULL, 0, NULL, 0, NULL, 0, 0, 0, 0,\n"
        "                                             NULL, 0, 0.5, 0.5, 0.8, 768, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL) == MICLOC_ERR_INVALID ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, "-fsyntax-only", str(src)])
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "xylo_stream_track_c"
    import torch

    rpaths = [libdir, os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib"]
    r = subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lmicloc_hip", "-Wl,--allow-shlib-undefined"]
                       + [f"-Wl,-rpath,{p}" for p in rpaths], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert out.stdout.decode().split() == [str(3 * 256 * 16), "256", str(INVALID)]


def test_the_envelope_recurrence_is_written_once():
    """The stream kernel wraps the one-shot tap: the recurrence, the per-frame combine over the waves and the block combine stand once in
    csrc/ -- in xylo_track_rows.h, which the one-shot kernel (xylo.hip) and the stream kernel (stream_xylo.hip) include; the C-ABI unit
    holds no kernel.  The names are counted over every source and header of csrc/, the rounded products over the Xylo files (the
    float-beamformer trackers of track_rows.h and sweep.hip keep a recurrence of their own on other state)."""
    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    files = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    text = "\n".join(files.values())
    xylo = "\n".join(t for f, t in files.items() if "xylo" in f)
    assert len([f for f in files if "xylo" in f]) >= 8 and "__dmul_rn(a_fall" in files["xylo_track_rows.h"]
    assert xylo.count("__dmul_rn(a_fall") == 1
    assert xylo.count("__dmul_rn(") == 3  # two rounded products going up, one going down
    assert text.count("struct XpTrackStreamTap : XpTrackTap") == 1
    assert text.count("xp_track_rows(") == 3 and text.count("xylo_track_combine_row(") == 3  # the definition and its two callers
    for name in ("xp_track_rows(", "xylo_track_combine_row("):  # defined in the header, called once by each form
        assert [files[f].count(name) for f in ("xylo_track_rows.h", "xylo.hip", "stream_xylo.hip")] == [1, 1, 1], name
    assert "xylo_lif_track_kernel" in files["xylo.hip"] and "xylo_track_combine_kernel" in files["xylo.hip"]
    text = files["stream_xylo.hip"]
    for kernel in ("xylo_lif_track_stream_kernel", "xylo_track_stream_combine_kernel"):
        assert kernel in text, kernel
    assert "__global__" not in open(os.path.join(csrc, "api_xylo_stream.hip")).read()
    rows = open(os.path.join(csrc, "xylo_rows.h")).read()
    assert "begin(off, first)" in rows and "XpTrackStreamTap" not in rows  # the tap protocol is unchanged; the stream's tap is a wrapper
