"""CPU checks of wideband moving-target tracking (tests/test_hip_track_bands.py has the device side): the C symbols and the ABI version,
the header as plain C, the refusals that read no plan -- from the entries called with dummy pointers -- and track_batch's own argument
errors in front of any device work.  The refusals that compare plans (device, M, G, the kind of bf_mat, a missing table, the workspace)
need plans, which only exist on a device: they stand in the device file, still in front of any launch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FS = 48_000
NAMES = ("micloc_snn_bands_track_workspace_bytes", "micloc_beamformer_bands_track_workspace_bytes", "micloc_snn_bands_track_is_fused",
         "micloc_beamformer_bands_track_is_fused", "micloc_lif_beamform_bands_track_f64", "micloc_beamform_c128_bands_track_f64",
         "micloc_snn_pipeline_bands_track_f64", "micloc_beamformer_pipeline_bands_track_f64")


def test_symbols_load_and_the_abi_version_is_one():
    from haghighatshoarmuir2024_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "micloc_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", text), f"{n} is not declared in the header"
        assert n in _lib.SYMBOLS and hasattr(raw, n), n
    assert _lib.load().micloc_abi_version() == 1
    assert "MICLOC_ABI_VERSION 1" in open(os.path.join(ROOT, "include", "micloc_hip.h")).read()


def test_header_section_compiles_as_plain_c(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this host")
    src = tmp_path / "bands_track_c.c"
    src.write_text(
        '#include "micloc_hip.h"\n'
        "int main(void) {\n"
        "    const micloc_plan *plans[MICLOC_MAX_BANDS] = {0};\n"
        "    int (*pipe)(const micloc_plan *const *, int, const double *, const double *, int, const double *, int, int, double, double, double,\n"
        "                int32_t *, double *, double *, void *, size_t, void *) = micloc_snn_pipeline_bands_track_f64;\n"
        "    int (*stage)(const micloc_plan *const *, int, const int8_t *, int, int, double, double, double, int32_t *, double *, double *,\n"
        "                 void *, size_t, void *) = micloc_lif_beamform_bands_track_f64;\n"
        "    pipe = micloc_beamformer_pipeline_bands_track_f64;\n"
        "    (void)pipe; (void)stage; (void)micloc_beamform_c128_bands_track_f64;\n"
        "    return (int)micloc_snn_bands_track_workspace_bytes(plans, 0, 1, 1) + (int)micloc_beamformer_bands_track_workspace_bytes(plans, 0, 1, 1)\n"
        "           + (micloc_snn_bands_track_is_fused(plans, 0) == MICLOC_ERR_INVALID ? 0 : 1)\n"
        "           + (micloc_beamformer_bands_track_is_fused(plans, 0) == MICLOC_ERR_INVALID ? 0 : 1);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_refusals_that_read_no_plan_come_back_from_dummy_pointers():
    from haghighatshoarmuir2024_amd import _lib

    lib = _lib.load()
    INV, SHAPE = _lib.MICLOC_ERR_INVALID, _lib.MICLOC_ERR_SHAPE
    one = ctypes.c_void_p(256)  # non-null, 256-byte aligned, never dereferenced: every refusal below comes first
    c = (0.9, 0.1, 0.99)
    tail = (one, None, None, one, 1 << 20, None)
    ba = np.asarray([[1.0, 0.0]]), np.asarray([[1.0, 0.0]])
    bp, ap = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for a in ba)

    def plans(n, hole=None):
        return (ctypes.c_void_p * max(n, 1))(*[None if i == hole else 256 for i in range(max(n, 1))])

    stage_snn = lambda pl, F, src, B, T, idx=one: lib.micloc_lif_beamform_bands_track_f64(pl, F, src, B, T, *c, idx, *tail[1:])  # noqa: E731
    stage_cpx = lambda pl, F, src, B, T, idx=one: lib.micloc_beamform_c128_bands_track_f64(pl, F, src, B, T, 16, *c, idx, *tail[1:])  # noqa: E731
    for stage in (stage_snn, stage_cpx):
        assert stage(None, 1, one, 1, 10) == INV            # no plans
        assert stage(plans(1), 1, None, 1, 10) == INV       # no input
        assert stage(plans(1), 1, one, 1, 10, None) == INV  # no index
        assert stage(plans(1), 0, one, 1, 10) == INV and stage(plans(17), 17, one, 1, 10) == INV  # F outside 1 .. MICLOC_MAX_BANDS
        assert stage(plans(3, hole=1), 3, one, 1, 10) == INV  # a NULL plan
        assert stage(plans(1), 1, one, 0, 10) == INV and stage(plans(1), 1, one, 65536, 10) == INV
        assert stage(plans(2), 2, one, 40000, 10) == INV    # F * B trials map to one grid dimension
        assert stage(plans(1), 1, one, 1, 0) == SHAPE
        assert stage(plans(1), 1, one, 65535, 40000) == SHAPE  # B * T > 2^31 - 1
    for name in ("snn", "beamformer"):
        pipe = getattr(lib, f"micloc_{name}_pipeline_bands_track_f64")
        assert pipe(None, 1, bp, ap, 2, one, 1, 10, *c, *tail) == INV
        assert pipe(plans(1), 1, bp, ap, 2, None, 1, 10, *c, *tail) == INV
        assert pipe(plans(1), 1, bp, ap, 2, one, 1, 10, *c, None, *tail[1:]) == INV
        assert pipe(plans(1), 1, None, ap, 2, one, 1, 10, *c, *tail) == INV
        assert pipe(plans(1), 0, bp, ap, 2, one, 1, 10, *c, *tail) == INV and pipe(plans(17), 17, bp, ap, 2, one, 1, 10, *c, *tail) == INV
        assert pipe(plans(1), 1, bp, ap, 0, one, 1, 10, *c, *tail) == INV  # fb_n outside 1 .. MICLOC_MAX_IIR
        zero = np.zeros((1, 2)).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert pipe(plans(1), 1, bp, zero, 2, one, 1, 10, *c, *tail) == INV  # a_f[0] == 0
        assert pipe(plans(1, hole=0), 1, bp, ap, 2, one, 1, 10, *c, *tail) == INV
        assert pipe(plans(1), 1, bp, ap, 2, one, 0, 10, *c, *tail) == INV
        assert pipe(plans(1), 1, bp, ap, 2, one, 1, 0, *c, *tail) == SHAPE
        assert pipe(plans(1), 1, bp, ap, 2, one, 65535, 40000, *c, *tail) == SHAPE
        size = getattr(lib, f"micloc_{name}_bands_track_workspace_bytes")
        fused = getattr(lib, f"micloc_{name}_bands_track_is_fused")
        assert size(None, 1, 1, 10) == 0 and size(plans(1), 0, 1, 10) == 0 and size(plans(1, hole=0), 1, 1, 10) == 0
        assert size(plans(1), 1, 65535, 40000) == 0 and size(plans(1), 1, 1, 0) == 0
        assert fused(None, 1) == INV and fused(plans(1), 0) == INV and fused(plans(17), 17) == INV and fused(plans(2, hole=1), 2) == INV


def test_sources_keep_the_contract():
    csrc = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
    trk = open(os.path.join(csrc, "track.hip")).read()
    assert "track_bands_ws_kernel" in trk and "track_bands_wsc_kernel" in trk
    assert "hipStreamSynchronize" not in trk and "hipDeviceSynchronize" not in trk and "hipMalloc" not in trk
    api = open(os.path.join(csrc, "api_bands.hip")).read()
    assert "__global__" not in api and "hipMalloc" not in api and "Synchronize" not in api
    run = open(os.path.join(csrc, "api_track.hip")).read()  # the unit that calls launch_track_bands_fused: the run of a set (api_sets.h)
    assert "launch_track_bands_fused(" in run and "launch_track_bands_fused(" not in api
    assert "__global__" not in run and "hipMalloc" not in run and "Synchronize" not in run
    assert '#include "track_bands.h"' in trk and '#include "track_bands.h"' in run


def _localizers():
    from haghighatshoarmuir2024_amd.array_geometry import CenterCircularArray
    from haghighatshoarmuir2024_amd.beamformer import Beamformer
    from haghighatshoarmuir2024_amd.filterbank import ButterworthFilterbank
    from haghighatshoarmuir2024_amd.snn_beamformer import SNNBeamformer
    from haghighatshoarmuir2024_amd.wideband import WidebandBeamformerLocalizer, WidebandSNNLocalizer

    geo = CenterCircularArray(4.5e-2, 7)
    bands = [[1000.0, 1600.0], [1600.0, 2400.0]]
    rng = np.random.RandomState(0)
    snn = [SNNBeamformer(geo, 10e-3, fr, np.asarray([1 / (2 * np.pi * np.mean(fr))] * 2), bipolar_spikes=True, fs=FS) for fr in bands]
    cpx = [Beamformer(geo, 10e-3, fr, fs=FS) for fr in bands]
    yield WidebandSNNLocalizer(snn, [rng.randn(14, 33) for _ in bands], ButterworthFilterbank(freq_bands=np.asarray(bands), order=1, fs=FS))
    yield WidebandBeamformerLocalizer(cpx, [rng.randn(7, 33) + 1j * rng.randn(7, 33) for _ in bands],
                                      ButterworthFilterbank(freq_bands=np.asarray(bands), order=2, fs=FS))


def test_track_batch_raises_before_any_device_work():
    """A wrong microphone count and envelope windows below one sample are ValueErrors of the host layer: no plan is made (on a box
    without a device making one raises MiclocError, which is not a ValueError)."""
    from haghighatshoarmuir2024_amd.utils import Envelope

    env = Envelope(rise_time=1e-3, fall_time=10e-3, fs=FS)
    short = Envelope(rise_time=1e-6, fall_time=10e-3, fs=FS)  # int(fs * rise_time) == 0
    assert short.win_lens[1] == 0
    n = 0
    for loc in _localizers():
        assert hasattr(loc, "track_batch")
        with pytest.raises(ValueError, match="microphones"):
            loc.track_batch(np.zeros((2, 100, 6)), env)
        with pytest.raises(ValueError, match="at least one sample"):
            loc.track_batch(np.zeros((2, 100, 7)), short)
        n += 1
    assert n == 2


def test_cli_knows_the_sweep_and_refuses_other_methods(capsys):
    from haghighatshoarmuir2024_amd import sweep

    for method in ("music", "xylo"):
        with pytest.raises(SystemExit):
            sweep.main(["--sweep", "moving-wideband", "--method", method, "--num-sim", "1"])
    assert "moving-wideband" in capsys.readouterr().err
    assert callable(sweep.wideband_moving_target_sweep) and callable(sweep.wideband_track_localizer)
