"""CPU-only checks of the streaming Xylo surface (include/micloc_hip.h "streaming, Xylo"; streaming.XyloStreamingLocalizer): the
new entries validate their arguments before any launch, the Python classes refuse what they cannot serve before any device work, and the
premise of the stream -- the bands of the block-diagonal network may be integrated independently -- holds in the oracle.
PARITY UNPINNED for the LIF itself (rockpool is absent): the oracle restates the published Xylo update rule."""
import ctypes
import os
import types

import numpy as np
import pytest

import csrc_build
from conftest import ROOT
from oracle import oracle as O

from haghighatshoarmuir2024_amd import _lib

OK, INVALID, SHAPE, WORKSPACE = _lib.MICLOC_OK, _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_SHAPE, _lib.MICLOC_ERR_WORKSPACE
BIG = 1 << 30


def test_size_functions():
    lib = _lib.load()
    assert lib.micloc_xylo_stream_state_bytes(0, 449) == 0 and lib.micloc_xylo_stream_state_bytes(3, 0) == 0
    assert lib.micloc_xylo_stream_state_bytes(70000, 449) == 0
    # [B][N rounded up to 512 / 2] lane pairs of 16 bytes
    assert lib.micloc_xylo_stream_state_bytes(3, 449) == 3 * 256 * 16 and lib.micloc_xylo_stream_state_bytes(1, 513) == 512 * 16
    assert lib.micloc_stream_xylo_state_bytes() >= 80 and lib.micloc_stream_xylo_state_bytes() % 256 == 0
    assert lib.micloc_stream_xylo_readout_state_bytes() >= 16
    assert lib.micloc_stream_xylo_workspace_bytes(2, 33, 768) >= 2 * 3 * 33 * 4
    for bad in ((0, 33, 768), (2, 0, 768), (2, 33, 0), (2, 33, 700)):
        assert lib.micloc_stream_xylo_workspace_bytes(*bad) == 0, bad
    assert lib.micloc_stream_xylo_window_state_bytes(2, 33, 1024, 512, 4) >= 256 + 2 * (2 + 4) * 33 * 4
    for bad in ((0, 33, 1024, 512, 4), (2, 0, 1024, 512, 4), (2, 33, 1000, 512, 4), (2, 33, 1024, 500, 4), (2, 33, 512, 1024, 4), (2, 33, 1024, 512, 0),
                (2, 33, 0, 0, 4)):
        assert lib.micloc_stream_xylo_window_state_bytes(*bad) == 0, bad


def test_resume_entry_validates_before_any_launch():
    lib = _lib.load()
    vp = ctypes.c_void_p
    one = vp(256)  # a non-null, 256-byte aligned dummy: validation must fail before it is ever dereferenced
    f = lib.micloc_xylo_lif_resume_i16
    good = dict(raster=one, tc=14, stride=700, B=3, t0=16, n=100, Cin=28, N=449, ms=31, out=None, T_out=0, counts=one, state=one, sb=BIG, ws=one, wb=BIG)

    def call(**kw):
        a = dict(good, **kw)
        return f(a["raster"], a["tc"], a["stride"], a["B"], a["t0"], a["n"], a["Cin"], a["N"], a["ms"], a["out"], a["T_out"], a["counts"], a["state"],
                 a["sb"], a["ws"], a["wb"], None)

    for name in ("raster", "counts", "state", "ws"):
        assert call(**{name: None}) == INVALID, name
    for kw in (dict(B=0), dict(stride=0), dict(t0=-16), dict(n=-1), dict(N=0), dict(ms=0), dict(tc=0)):
        assert call(**kw) == INVALID, kw
    assert call(t0=8) == SHAPE                      # t0 % 16
    assert call(Cin=27) == SHAPE                    # Cin != 2 x ternary channels
    assert call(tc=33, Cin=66) == SHAPE             # Cin > 64
    assert call(t0=688, n=100) == SHAPE             # past the trial stride
    assert call(out=one, T_out=50) == SHAPE         # past the output rows
    assert call(raster=vp(264)) == SHAPE            # raster not 16-byte aligned
    assert call(sb=3 * 256 * 16 - 1) == WORKSPACE   # short state
    assert call(state=vp(264)) == WORKSPACE         # misaligned state
    assert call(wb=100) == WORKSPACE                # short network workspace
    assert lib.micloc_xylo_stream_reset(None, 256, None) == INVALID
    assert lib.micloc_xylo_stream_reset(one, 0, None) == INVALID
    assert lib.micloc_xylo_stream_reset(vp(264), 4096, None) == WORKSPACE


def test_stream_entries_validate_before_any_launch():
    lib = _lib.load()
    vp = ctypes.c_void_p
    one, two = vp(256), vp(512)
    # the entries of a band's stream take the band's plan: without one they refuse (a plan needs a device)
    assert lib.micloc_stream_xylo_reset(None, 1, one, BIG, one, BIG, one, 768, 33, one, BIG, one, None) == INVALID
    assert lib.micloc_stream_xylo_begin_tile(None, one, one, two, 1, 16, 768, None) == INVALID
    assert lib.micloc_stream_xylo_tile_i16(None, one, one, BIG, one, 1, 768, 0, 33, 31, one, one, BIG, one, BIG, None) == INVALID
    assert lib.micloc_stream_xylo_tile_windows_i16(None, one, one, BIG, one, 1, 768, 0, 33, 31, one, one, BIG, one, BIG, one, BIG, one, BIG, 1024, 512, 4,
                                                   None) == INVALID
    assert lib.micloc_stream_xylo_status(None, None, None) == INVALID
    st4 = (ctypes.c_int * 4)()
    assert lib.micloc_stream_xylo_status(None, st4, None) == INVALID
    # the window state
    assert lib.micloc_stream_xylo_window_reset(None, BIG, 2, 33, 1024, 512, 4, None) == INVALID
    assert lib.micloc_stream_xylo_window_reset(one, BIG, 0, 33, 1024, 512, 4, None) == INVALID
    assert lib.micloc_stream_xylo_window_reset(one, BIG, 2, 33, 1024, 512, 0, None) == INVALID
    assert lib.micloc_stream_xylo_window_reset(one, BIG, 2, 33, 1000, 512, 4, None) == SHAPE
    assert lib.micloc_stream_xylo_window_reset(one, BIG, 2, 33, 512, 1024, 4, None) == SHAPE
    assert lib.micloc_stream_xylo_window_reset(one, 100, 2, 33, 1024, 512, 4, None) == WORKSPACE
    # the read-out over the bands
    assert lib.micloc_stream_xylo_readout_reset(None, 256, None) == INVALID
    assert lib.micloc_stream_xylo_readout_reset(one, 8, None) == WORKSPACE
    ptrs = (vp * 2)(256, 512)
    ro = lib.micloc_stream_xylo_readout

    def readout(F=2, B=2, G=33, fs=48000.0, win=1, bc=ptrs, bl=ptrs, window=0, hop=0, Kb=0, maxw=0, bw=None, state=one, nb=256, counts=one, rate=one,
                peak=one, wc=None, wr=None, wp=None):
        return ro(F, B, G, fs, win, bc, bl, window, hop, Kb, maxw, bw, state, nb, counts, rate, peak, wc, wr, wp, None, None, None, None)

    assert readout(bc=None) == INVALID and readout(bl=None) == INVALID and readout(state=None) == INVALID
    assert readout(counts=None) == INVALID and readout(rate=None) == INVALID and readout(peak=None) == INVALID
    assert readout(F=0) == INVALID and readout(F=_lib.MICLOC_MAX_BANDS + 1) == INVALID and readout(B=0) == INVALID and readout(fs=0.0) == INVALID
    assert readout(win=2) == INVALID and readout(win=17) == INVALID          # micloc_peak_location_i32's rule: odd, at most G / 2
    assert readout(bc=(vp * 2)(256, None)) == INVALID                        # a band without counts
    assert readout(window=1024, hop=512, Kb=4, maxw=8) == INVALID            # windows without the bands' window states and the tables
    assert readout(window=1000, hop=512, Kb=4, maxw=8, bw=ptrs, wc=one, wr=one, wp=one) == SHAPE
    assert readout(window=1024, hop=512, Kb=4, maxw=0, bw=ptrs, wc=one, wr=one, wp=one) == INVALID
    assert readout(G=5000) == SHAPE                                          # the band sums of the read-out live in LDS
    assert readout(nb=16) == WORKSPACE
    assert lib.micloc_stream_xylo_readout_status(None, None, None) == INVALID


def _standin(F=1, M=7, G=33, w_rec=0, bipolar=True):
    """What XyloStreamingLocalizer reads of a Demo before it touches the device."""
    C = 2 * M
    spec = dict(W_in=np.zeros((2 * F * C, F * G), np.int8), w_rec=w_rec, dash_syn=np.zeros(F * G, np.uint8), dash_mem=np.zeros(F * G, np.uint8),
                threshold=np.ones(F * G, np.int16))
    beamf = types.SimpleNamespace(geometry=[0] * M)
    return types.SimpleNamespace(spec=spec, bipolar_spikes=bipolar, beamfs=[beamf] * F, doa_list=np.linspace(-np.pi, np.pi, G), fs=48_000)


def test_localizer_refuses_before_any_device_work():
    from haghighatshoarmuir2024_amd.streaming import XyloStreamingLocalizer

    with pytest.raises(ValueError, match="quantises to 0"):
        XyloStreamingLocalizer(_standin(w_rec=-1), 2)
    with pytest.raises(ValueError, match="bipolar"):
        XyloStreamingLocalizer(_standin(bipolar=False), 2)
    with pytest.raises(ValueError, match="16 microphones"):
        XyloStreamingLocalizer(_standin(M=17), 2)
    with pytest.raises(ValueError, match="bands"):
        XyloStreamingLocalizer(_standin(F=_lib.MICLOC_MAX_BANDS + 1), 2)
    for kw in (dict(window=1000), dict(window=1024, hop=100), dict(window=0), dict(window=512, hop=0)):
        with pytest.raises(ValueError, match="256"):
            XyloStreamingLocalizer(_standin(), 2, **kw)
    with pytest.raises(ValueError, match="hop <= window"):
        XyloStreamingLocalizer(_standin(), 2, window=512, hop=1024)
    with pytest.raises(ValueError):
        XyloStreamingLocalizer(_standin(), 2, hop=256)  # hop without window
    with pytest.raises(ValueError, match="win_size"):
        XyloStreamingLocalizer(_standin(), 2, win_size=4)


def test_run_resume_refuses_before_any_device_call():
    import torch

    from haghighatshoarmuir2024_amd.xylo_snn_localization import XyloNetwork

    net = XyloNetwork.__new__(XyloNetwork)  # (the constructor uploads the network: no device here)
    net.Cin, net.N, net.w_rec = 28, 33, -1
    raster = torch.zeros((2, 64, 14), dtype=torch.int8)
    with pytest.raises(ValueError, match="w_rec"):
        net.new_state(2)
    with pytest.raises(ValueError, match="w_rec"):
        net.run_resume(raster, 0, 16, None)
    net.w_rec = 0
    with pytest.raises(ValueError, match="int8"):
        net.run_resume(raster.to(torch.uint8), 0, 16, None)
    with pytest.raises(ValueError, match="multiple of 16"):
        net.run_resume(raster, 8, 16, None)


def test_bands_of_the_block_diagonal_network_integrate_independently():
    """Pure oracle: the quantised specification of a two-band network, sliced into band blocks AFTER the global quantisation
    (XyloStreamingLocalizer.band_spec), gives per band the counts and the spikes of the whole network's neurons of that band."""
    from haghighatshoarmuir2024_amd.streaming import XyloStreamingLocalizer
    from haghighatshoarmuir2024_amd.xylo_snn_localization import xylo_specification

    rng = np.random.RandomState(11)
    F, C, G, T = 2, 14, 33, 900
    bf_mats = [rng.randn(C, G) / np.sqrt(C) * (1.0 + f) for f in range(F)]  # bands of different scale: one global quantisation
    taus = [[1 / (2 * np.pi * 1300), 1 / (2 * np.pi * 1300)], [1 / (2 * np.pi * 2000), 1 / (2 * np.pi * 2000)]]
    spec = xylo_specification(bf_mats, taus, fs=48_000, target_dt=1e-3, bipolar_spikes=True, threshold=0.2)
    assert spec["w_rec"] == 0 and spec["W_in"].shape == (2 * F * C, F * G)
    raster = rng.choice([-1, 0, 1], size=(T, F * C), p=[0.035, 0.93, 0.035]).astype(np.int8)
    events = np.concatenate([raster > 0, raster < 0], axis=1).astype(np.uint8)
    out, rate = O.xylo_lif(events, spec["W_in"], 0, spec["dash_syn"], spec["dash_mem"], spec["threshold"], 31)
    assert int(rate.sum()) > 0
    for f in range(F):
        bs = XyloStreamingLocalizer.band_spec(spec, f, F, C, G)
        assert bs["W_in"].shape == (2 * C, G)
        rb = raster[:, f * C : (f + 1) * C]
        eb = np.concatenate([rb > 0, rb < 0], axis=1).astype(np.uint8)
        out_b, rate_b = O.xylo_lif(eb, bs["W_in"], 0, bs["dash_syn"], bs["dash_mem"], bs["threshold"], 31)
        assert int(rate_b.sum()) > 0, f
        np.testing.assert_array_equal(rate_b, rate[f * G : (f + 1) * G])
        np.testing.assert_array_equal(out_b, out[:, f * G : (f + 1) * G])


def test_the_packed_step_is_written_once():
    """csrc/xylo_rows.h holds the packed LIF of the one-shot and of the stream kernel: the saturating subtraction of the first spike and
    the int8 matrix-core product occur there and in neither kernel file, and both objects are rebuilt when the header changes."""
    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("xylo_rows.h", "xylo.hip", "stream_xylo.hip")}
    for word in ("__builtin_elementwise_sub_sat", "mfma_i32_16x16x32_i8"):
        assert word in text["xylo_rows.h"], word
        assert word not in text["xylo.hip"] and word not in text["stream_xylo.hip"], word
    for f in ("xylo.hip", "stream_xylo.hip"):
        assert '#include "xylo_rows.h"' in text[f], f
    assert {"xylo.o", "stream_xylo.o"} <= csrc_build.rebuilt_after_edit("xylo_rows.h")


def test_header_with_the_xylo_stream_section_is_plain_c(tmp_path):
    import shutil
    import subprocess

    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this host")
    src = tmp_path / "xylo_stream_c.c"
    src.write_text(
        '#include "micloc_hip.h"\n#include <stdio.h>\n'
        "int main(void) {\n"
        '    printf("%zu %zu %zu %d\\n", micloc_xylo_stream_state_bytes(3, 449), micloc_stream_xylo_state_bytes(),\n'
        "           micloc_stream_xylo_window_state_bytes(2, 33, 1024, 512, 4),\n"
        "           micloc_xylo_lif_resume_i16(NULL, 14, 700, 3, 0, 16, 28, 449, 31, NULL, 0, NULL, NULL, 0, NULL, 0, NULL));\n"
        "    return micloc_stream_xylo_status(NULL, NULL, NULL) == MICLOC_ERR_INVALID ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, "-fsyntax-only", str(src)])
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = tmp_path / "xylo_stream_c"
    import torch

    rpaths = [libdir, os.path.join(os.path.dirname(torch.__file__), "lib"), "/opt/rocm/lib"]
    r = subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lmicloc_hip", "-Wl,--allow-shlib-undefined"]
                       + [f"-Wl,-rpath,{p}" for p in rpaths], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    fields = out.stdout.decode().split()
    assert fields == [str(3 * 256 * 16), "256", fields[2], str(INVALID)] and int(fields[2]) > 0
