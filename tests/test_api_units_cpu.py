"""CPU checks of the C-ABI's host sources, one translation unit per surface (csrc/api_*.hip, what they share in csrc/api_internal.h):
every unit is built, none holds a kernel, and the sweep encoder's measurement record (profiles/encoder_slots/RECORD.json, whose source
hashes tests/test_ring_depth_cpu.py checks against the tree) pins the units the headline step calls into and not the wideband, streaming
and tracking ones, which other features edit."""
import glob
import json
import os

import csrc_build
from conftest import ROOT

CSRC = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
UNITS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "api_*.hip")))


def test_every_api_unit_is_in_the_makefile_and_api_hip_is_gone():
    srcs = csrc_build.built_sources()
    assert len(UNITS) >= 2 and not os.path.exists(os.path.join(CSRC, "api.hip"))
    for unit in UNITS:
        assert unit in srcs, unit
    assert "api.hip" not in srcs


def test_no_api_unit_holds_a_kernel():
    for unit in UNITS:
        assert "__global__" not in open(os.path.join(CSRC, unit)).read(), unit


def test_encoder_record_pins_the_sweeps_api_units_only():
    rec = json.load(open(os.path.join(ROOT, "profiles", "encoder_slots", "RECORD.json")))
    pinned = {os.path.basename(rel) for rel in rec["sources_sha256"]}
    assert pinned & set(UNITS), "the record pins no api_*.hip"
    assert not pinned & {"api.hip", "api_bands.hip", "api_stream.hip", "api_track.hip"}
