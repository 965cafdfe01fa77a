"""Candidate-ring demand of the sweep encoder (csrc/rzcc_sweep.hip) on the CPU (tools/dev/ring_demand.py): the 32-entry ring of the
three-slot form holds the headline's streams at the lowest SNR of the sweep, and the closed-form model agrees with a step-by-step
walk of the kernel's protocol.  Both are CPU implementations of the same reading of the kernel; the check of the model against the
DEVICE's fallback count is tests/test_hip_encoder_slots.py.  Also here, because rzcc_sweep.hip is not among the sources the round
profiles pin: its emitted ISA passes the LDS-read hazard check, and profiles/encoder_slots/RECORD.json was taken on its text."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("ring_demand", os.path.join(ROOT, "tools", "dev", "ring_demand.py"))
ring_demand = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ring_demand)

RING = 32


def test_headline_streams_fit_the_32_entry_ring(cfg2):
    """2002 streams (143 trials x 7 in-phase + 7 quadrature channels through the plan's Hilbert kernel, the golden 48 kHz one),
    2 kHz tone in noise at -10 dB minus the bandwidth gain, seed 0.  Measured: exact-check demand at most 14 of 32 (11 entries
    outstanding; 4004 streams: 15 and 12), with the detect wave reading the older publication of the select waves."""
    demand, outstanding = ring_demand.headline_demand(trials=143, seed=0, kernel=cfg2["kernel"])
    assert len(demand) >= 2000
    assert demand.max() <= RING, f"exact-check demand {demand.max()} of {RING} (outstanding entries: max {outstanding.max()})"
    assert demand.max() >= outstanding.max() + 3  # (the three unconditional stores are part of every tile's demand)
    print(f"ring demand on {len(demand)} headline-like streams: max {demand.max()} of {RING}, outstanding max {outstanding.max()}")


def _walk(c, w, ring, exact, select_lag):
    """The kernel's protocol step by step for one bipolar stream -> (overflowed, largest n - oldest seen by the detect wave)."""
    T = len(c)
    NM = (T + 15) // 16
    pos, pol = [], []            # the candidate list (never wrapped here: the check is what is modelled)
    n, live, direction, left, worst = 0, True, 0, 0, 0
    sel = [dict(i_next=-1, s_open=-1, l_last=0) for _ in range(2)]
    pubs = [[0, 0]]              # oldest per polarity as published at the end of each step (before the first: 0)
    n_pub = [0]                  # n as published by the detect wave at the end of each step
    over = False
    for k in range(NM + 2):
        mine = list(pubs[-1])
        if k >= 2:               # select waves: what the detect wave published before the last barrier
            seen = n_pub[-1]
            for q in (0, 1):
                s = sel[q]
                if s["i_next"] < 0 and seen > 0:
                    s["i_next"] = pol[0] ^ q
                while 0 <= s["i_next"] < seen:
                    i = s["i_next"]
                    if s["s_open"] >= 0 and pos[i] - s["l_last"] >= w:
                        s["s_open"] = -1
                    if s["s_open"] < 0:
                        s["s_open"] = i
                    s["l_last"] = pos[i]
                    s["i_next"] = i + 2
                mine[q] = s["s_open"] if s["s_open"] >= 0 else max(s["i_next"], 0)
        if 1 <= k <= NM:         # detect wave: tile k - 1
            old = min(pubs[-1] if select_lag == 2 else mine)
            ev = []
            for t in range(16 * (k - 1), min(16 * k, T)):
                if t == 0 or c[t] == c[t - 1]:
                    continue
                d = 1 if c[t] > c[t - 1] else 2
                if direction and d != direction:
                    ev.append(((left + t - 1) >> 1, 0 if d == 2 else 1))
                direction, left = d, t
            worst = max(worst, n - old)
            if live and ((n + max(len(ev), 3) - old > ring) if exact else (n + 16 - old > ring - 1)):
                live, over = False, True
            if live:
                for p_, q_ in ev:
                    pos.append(p_)
                    pol.append(q_)
                n += len(ev)
        pubs.append(mine)
        n_pub.append(n)
    return over, worst


@pytest.mark.parametrize("w", [28, 36, 48])
def test_model_agrees_with_a_walk_of_the_protocol(w):
    """Band-passed white noise, 1 - 2 kHz (the device test's inputs for w = 28 and 36; its w = 48 case sits behind a 2 - 4 kHz
    band, here w = 48 stays in the sweep's band, where every stream overflows as well): overflow predicted in closed form ==
    overflow taken by the walk, per stream, for the exact check at both ends of the detect wave's race and for the whole-tile check."""
    from scipy.signal import butter

    b, a = butter(2, [1000.0, 2000.0], btype="bandpass", fs=48_000)
    sums = ring_demand.running_sums(np.random.RandomState(7).randn(2, 1000, 7), b, a, ring_demand.stht_kernel())
    taken = {}
    for lag in (2, 1):
        for exact in (True, False):
            want = [ring_demand.overflows(c, w, RING, True, exact, lag) for c in sums]
            got = [_walk(c, w, RING, exact, lag)[0] for c in sums]
            assert got == want, f"w={w} lag={lag} exact={exact}"
            taken[lag, exact] = sum(got)
    if w == 28:  # up to 19 entries outstanding: the whole-tile check flags streams, the exact one none
        assert taken[2, True] == 0 and taken[2, False] > 0
        assert max(_walk(c, w, 1 << 20, True, 2)[1] for c in sums) == max(ring_demand.ring_demand(c, w)["outstanding"] for c in sums)
    if w == 48:
        assert taken[2, True] == taken[1, True] == len(sums)


def test_sweep_encoder_isa_has_no_read_of_an_lds_destination_in_flight():
    """tests/test_isa_hazards_cpu.py looks at rzcc.hip; the hand-issued ds_read_b64 / s_waitcnt sequences of rzcc_sweep.hip's loader
    and filter waves get the same check (tools/check_isa_hazards.py; hipcc cross-compiles, the assembly is cached under build_dev/)."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa_hazards as H

    findings, seen, with_asm = H.check_file(H.emit("rzcc_sweep.hip"))
    assert seen >= 3 and with_asm >= 1, (seen, with_asm)
    assert findings == [], findings[:5]


def test_encoder_slots_record_belongs_to_the_sources_in_the_tree():
    """profiles/encoder_slots/RECORD.json: the step times and resource counts quoted in DESIGN.md 4.2 were taken on these sources."""
    import hashlib
    import json

    rec = json.load(open(os.path.join(ROOT, "profiles", "encoder_slots", "RECORD.json")))
    assert "haghighatshoarmuir2024_amd/csrc/rzcc_sweep.hip" in rec["sources_sha256"]
    for rel, h in rec["sources_sha256"].items():
        assert hashlib.sha256(open(os.path.join(ROOT, rel), "rb").read()).hexdigest() == h, rel
    assert rec["box"]["gcn_arch"].startswith("gfx950")
