"""The tracked wideband streams (include/micloc_hip.h "wideband streaming, tracking"; csrc/stream_track_bands.hip; streaming.py track= of the
two wideband classes) without a GPU: the symbols and the header as plain C, the refusals that read no plan, the host-side refusals of the
stream classes, the frontier rule of the SNN bands against a brute-force simulation, and the source contract of the new kernel file.
tests/test_hip_stream_track_bands.py has the device side."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import csrc_build
from conftest import ROOT

FS = 48_000
CSRC = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
NAMES = ("micloc_stream_bands_track_state_bytes", "micloc_stream_bands_track_workspace_bytes", "micloc_stream_bands_track_reset",
         "micloc_stream_bands_track_tile_f64", "micloc_stream_complex_bands_localize_tile_track_f64", "micloc_stream_bands_track_status")


def test_header_declares_and_lib_binds_the_symbols():
    from haghighatshoarmuir2024_amd import _lib

    header = open(os.path.join(ROOT, "include", "micloc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", text), f"{n} is not declared in the header"
        assert n in _lib.SYMBOLS and hasattr(raw, n), n
    assert "wideband streaming, tracking" in header and "MICLOC_ABI_VERSION 1" in header
    assert _lib.load().micloc_abi_version() == 1


def test_header_section_compiles_as_plain_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this host")
    src = tmp_path / "stream_bands_track_c.c"
    src.write_text(
        '#include "micloc_hip.h"\n'
        "int main(void) {\n"
        "    const micloc_plan *plans[MICLOC_MAX_BANDS] = {0};\n"
        "    const void *loc_states[MICLOC_MAX_BANDS] = {0};\n"
        "    const int8_t *windows[MICLOC_MAX_BANDS] = {0};\n"
        "    int frontier = 0;\n"
        "    int (*tile)(const micloc_plan *const *, int, const void *const *, const int8_t *const *, int, int, void *, size_t, double, double,\n"
        "                double, int, int32_t *, double *, int32_t *, double *, void *, size_t, void *) = micloc_stream_bands_track_tile_f64;\n"
        "    int rc = tile(plans, 0, loc_states, windows, 1, 256, 0, 0, 0.9, 0.1, 0.99, 256, 0, 0, 0, 0, 0, 0, 0);\n"
        "    (void)micloc_stream_complex_bands_localize_tile_track_f64;\n"
        "    rc += micloc_stream_bands_track_reset(plans, 0, 1, 0, 0, 0) + micloc_stream_bands_track_status(0, &frontier, 0);\n"
        "    return rc + (int)micloc_stream_bands_track_state_bytes(plans, 0, 1) + (int)micloc_stream_bands_track_workspace_bytes(plans, 0, 1, 256);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_size_entries_return_zero_and_entries_refuse_null_or_dummy_pointers_before_any_device_work():
    from haghighatshoarmuir2024_amd import _lib

    lib = _lib.load()
    INV = _lib.MICLOC_ERR_INVALID
    one = ctypes.c_void_p(256)  # non-null, 256-byte aligned, never dereferenced: every refusal below comes first
    c = (0.9, 0.1, 0.99)

    def ptrs(n, hole=None):
        return (ctypes.c_void_p * max(n, 1))(*[None if i == hole else 256 for i in range(max(n, 1))])

    state, ws = lib.micloc_stream_bands_track_state_bytes, lib.micloc_stream_bands_track_workspace_bytes
    assert state(None, 1, 1) == 0 and state(ptrs(1), 0, 1) == 0 and state(ptrs(17), 17, 1) == 0 and state(ptrs(2, hole=1), 2, 1) == 0
    assert state(ptrs(1), 1, 0) == 0 and state(ptrs(1), 1, 65536) == 0
    assert ws(None, 1, 1, 4096) == 0 and ws(ptrs(1), 0, 1, 4096) == 0 and ws(ptrs(2, hole=0), 2, 1, 4096) == 0 and ws(ptrs(1), 1, 0, 4096) == 0
    assert ws(ptrs(1), 1, 1, 0) == 0
    reset = lib.micloc_stream_bands_track_reset
    assert reset(None, 1, 1, one, 4096, None) == INV and reset(ptrs(1), 1, 1, None, 4096, None) == INV
    assert reset(ptrs(1), 0, 1, one, 4096, None) == INV and reset(ptrs(2, hole=1), 2, 1, one, 4096, None) == INV and reset(ptrs(1), 1, 0, one, 4096, None) == INV
    assert lib.micloc_stream_bands_track_status(None, None, None) == INV and lib.micloc_stream_bands_track_status(one, None, None) == INV

    def snn(plans=ptrs(1), F=1, loc=ptrs(1), win=ptrs(1), B=1, frames=4096, state=one, R=4096, index=one, peak=one, li=one, lp=one):
        return lib.micloc_stream_bands_track_tile_f64(plans, F, loc, win, B, frames, state, 4096, *c, R, index, peak, li, lp, one, 4096, None)

    assert snn(plans=None) == INV and snn(F=0) == INV and snn(plans=ptrs(17), F=17) == INV and snn(plans=ptrs(2, hole=1), F=2, loc=ptrs(2), win=ptrs(2)) == INV
    assert snn(loc=None) == INV and snn(win=None) == INV and snn(loc=ptrs(1, hole=0)) == INV and snn(win=ptrs(1, hole=0)) == INV
    assert snn(B=0) == INV and snn(frames=0) == INV and snn(state=None) == INV and snn(R=0) == INV
    assert snn(index=None) == INV and snn(peak=None) == INV and snn(li=None) == INV and snn(lp=None) == INV

    def cpx(plans=ptrs(1), F=1, st=one, B=1, max_tile=100, ws_=one, win_state=None, wargmax=None, state=one, R=128, index=one):
        return lib.micloc_stream_complex_bands_localize_tile_track_f64(plans, F, st, 4096, B, max_tile, 0, None, one, one, ws_, 4096, win_state, 0, 0, 0, 0,
                                                                       None, wargmax, None, None, state, 4096, *c, R, index, one, one, one, one, 4096, None)

    assert cpx(plans=None) == INV and cpx(F=0) == INV and cpx(plans=ptrs(2, hole=0), F=2) == INV and cpx(st=None) == INV and cpx(ws_=None) == INV
    assert cpx(B=0) == INV and cpx(max_tile=0) == INV and cpx(state=None) == INV and cpx(R=0) == INV and cpx(index=None) == INV
    assert cpx(win_state=one, wargmax=None) == INV


def _localizers(M=7, G=33):
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.filterbank import ButterworthFilterbank
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, M)
    bands = [[1000.0, 1600.0], [1600.0, 2400.0]]
    rng = np.random.RandomState(0)
    snn = [SNNBeamformer(geo, 10e-3, fr, np.asarray([1 / (2 * np.pi * np.mean(fr))] * 2), bipolar_spikes=True, fs=FS) for fr in bands]
    cpx = [Beamformer(geo, 10e-3, fr, fs=FS) for fr in bands]
    yield WidebandSNNLocalizer(snn, [rng.randn(2 * M, G) for _ in bands], ButterworthFilterbank(freq_bands=np.asarray(bands), order=1, fs=FS))
    yield WidebandBeamformerLocalizer(cpx, [rng.randn(M, G) + 1j * rng.randn(M, G) for _ in bands],
                                      ButterworthFilterbank(freq_bands=np.asarray(bands), order=2, fs=FS))


def _stream_class(loc):
    from haghighatshoarmuir2024_amd.streaming import WidebandComplexStreamingLocalizer, WidebandStreamingLocalizer

    return WidebandStreamingLocalizer if hasattr(loc.beamfs[0], "tau_vec") else WidebandComplexStreamingLocalizer


def test_both_stream_classes_take_track_and_refuse_on_the_host():
    """track_setup's refusals are ValueErrors in front of any device work (on a box without a device making a plan raises MiclocError,
    which is not a ValueError): more than 16 channels, max_track without track, an envelope window below one sample."""
    import inspect

    from haghighatshoarmuir2024_amd.utils import Envelope

    env = Envelope(rise_time=1e-3, fall_time=10e-3, fs=FS)
    short = Envelope(rise_time=1e-6, fall_time=10e-3, fs=FS)  # int(fs * rise_time) == 0
    assert short.win_lens[1] == 0
    n = 0
    for loc in _localizers():
        cls = _stream_class(loc)
        assert {"track", "max_track"} <= set(inspect.signature(cls.__init__).parameters)
        with pytest.raises(ValueError, match="max_track belongs to the tracked read-out"):
            cls(loc, 1, 4800, max_track=4800)
        with pytest.raises(ValueError, match="at least one sample"):
            cls(loc, 1, 4800, track=short)
        n += 1
    for loc in _localizers(M=20):
        with pytest.raises(ValueError, match="track_batch"):
            _stream_class(loc)(loc, 1, 4800, track=env)
        n += 1
    assert n == 4
    from haghighatshoarmuir2024_amd.streaming import WidebandStreamingLocalizer

    assert "time_vec" in inspect.signature(WidebandStreamingLocalizer.__init__).parameters


def _simulate(rng, F, CH, T, stall=None):
    """Random tiles and random per-band chunk counts `done` (non-decreasing, done_f CH <= frames pushed, every chunk on the final tile) ->
    per push (t_end, done [F]).  stall = (band, push): that band's count stops growing there (a lag failure)."""
    pushes, t, done, k = [], 0, [0] * F, 0
    while t < T:
        n = min(16 * int(rng.randint(1, 40)), T - t)
        t += n
        final = t == T
        for f in range(F):
            if stall is not None and f == stall[0] and k >= stall[1]:
                continue
            top = -(-T // CH) if final else t // CH
            done[f] = top if final else int(rng.randint(done[f], top + 1))
        pushes.append((t, list(done)))
        k += 1
    return pushes


@pytest.mark.parametrize("F", [1, 2, 3, 16])
def test_the_frontier_rule_against_a_brute_force_simulation(F):
    from haghighatshoarmuir2024_amd.streaming import bands_track_span

    rng = np.random.RandomState(40 + F)
    for trial in range(20):
        CH = int(rng.choice([64, 256, 512]))
        T = int(rng.randint(1, 12 * CH))
        T += T % CH == 0  # a ragged last chunk
        final_flags = np.zeros(T, dtype=bool)  # brute force: which frames every band has beamformed
        prev, covered = 0, 0
        for t_end, done in _simulate(rng, F, CH, T):
            beamformed = [min(d * CH, t_end) for d in done]  # frames band f has beamformed (the last chunk of the recording is ragged)
            now = np.zeros(T, dtype=bool)
            now[: min(beamformed)] = True
            want_first, want_last = int(final_flags.sum()), int(now.sum())
            first, last = bands_track_span(prev, done, CH, t_end)
            assert (first, last) == (want_first, want_last) and first == covered, (trial, t_end, done)
            assert all(last <= b for b in beamformed)  # no span passes any band's beamformed frames
            final_flags |= now
            covered, prev = last, last
        assert covered == T and T % CH != 0  # the spans tile [0, T): no gap, no overlap, and the final tile ends at T


def test_a_band_that_stalls_stalls_the_frontier():
    from haghighatshoarmuir2024_amd.streaming import bands_track_span

    rng = np.random.RandomState(9)
    F, CH, T = 3, 256, 20 * 256 + 7
    pushes = _simulate(rng, F, CH, T, stall=(1, 3))
    stuck = pushes[3][1][1] if len(pushes) > 3 else pushes[-1][1][1]
    prev = 0
    for k, (t_end, done) in enumerate(pushes):
        first, last = bands_track_span(prev, done, CH, t_end)
        assert first == prev <= last
        if k >= 3:
            assert done[1] == stuck and last <= stuck * CH
        prev = last
    assert prev == min(stuck * CH, T) < T  # the other bands went on to T; the frontier did not
    assert bands_track_span(512, [1, 5, 5], 256, 4096) == (512, 512)  # the frontier never moves back


def test_sources_keep_the_contract():
    assert "stream_track_bands.hip" in csrc_build.built_sources()
    assert "stream_track_bands.o" in csrc_build.rebuilt_after_edit("track_rows.h")
    src = open(os.path.join(CSRC, "stream_track_bands.hip")).read()
    assert '#include "track_rows.h"' in src
    for name in ("track_bands_ws_stream_kernel", "track_bands_wsc_stream_kernel", "track_bands_ws_walk", "track_bands_wsc_walk"):
        assert name in src, name
    walks = open(os.path.join(CSRC, "track_bands_rows.h")).read()
    for text in (src, walks, open(os.path.join(CSRC, "stream_track_rows.h")).read()):
        for word in ("mfma_f64_16x16x4f64", "hypot(", "hipMalloc", "Synchronize"):
            assert word not in text, word
    # one walk over the bands for the one-shot kernels and the stream kernels: defined in the shared header, called from both files
    trk = open(os.path.join(CSRC, "track.hip")).read()
    for walk in ("track_bands_ws_walk(", "track_bands_wsc_walk<KM, KV>("):
        assert walk in trk and walk in src, walk
    assert walks.count("void track_bands_ws_walk(") == 1 and walks.count("void track_bands_wsc_walk(") == 1
    assert "void track_bands_ws_walk(" not in trk and "void track_bands_wsc_walk(" not in trk
    for api in ("api_bands.hip", "api_track.hip", "api_stream.hip"):
        assert "__global__" not in open(os.path.join(CSRC, api)).read(), api
