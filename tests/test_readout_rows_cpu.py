"""csrc/readout_rows.h states the read-out rules once: text pins that no kernel file restates them, and that every object
whose source includes the header is rebuilt when it changes."""
import os
import re

import csrc_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "haghighatshoarmuir2024_amd", "csrc")
HEADER = "readout_rows.h"
# the one named exception: its hash is pinned by profiles/r6/MANIFEST.json, so its three copies of the tree fold in with the next round
EXCEPTION = "beamform.hip"
# pk_better of the multi-source read-out: the same comparison between candidates of a greedy selection; the file's text is pinned by the
# kernel profile of profiles/multisource/RECORD.json (tests/test_multitarget_golden_cpu.py), so it stays until that profile is taken again
PINNED_BY_PROFILE = "peaks.hip"

# an operand: a name, a subscripted name, or a name with an expression in the subscript such as sv[col + s]
_OP = r"[A-Za-z_]\w*(?:\[[^\]]*\])?"
# "the larger value, or an equal value with the lower index": <ov> > <mv> || (<ov> == <mv> && <oi> < <mi>), the LDS form (sv[col],
# si[col]) and the register form of the butterfly.  (The rank counts of the stable sorts in design.hip and music_rows.h compare the same
# way but reduce nothing; they parenthesise the first comparison and are not meant.)
TIE_BREAK = re.compile(rf"({_OP})\s*>\s*({_OP})\s*\|\|\s*\(\s*\1\s*==\s*\2\s*&&\s*{_OP}\s*<\s*{_OP}\s*\)")
# windows complete after `done` chunks: (done - wchunks) / hchunks + 1, whatever the operands are called
EMITTED = re.compile(r"\(\s*\w+\s*-\s*wchunks\s*\)\s*/\s*hchunks\s*\+\s*1")


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}


def _code(text):
    """The text without // comments (a comment may quote a rule; only code can restate it)."""
    return "\n".join(line.split("//")[0] for line in text.splitlines())


def test_the_patterns_find_the_spellings_the_kernels_had():
    for old in ("if (ov > sv[col] || (ov == sv[col] && oi < si[col])) {", "if (ov > best || (ov == best && oi < bi)) {",
                "if (ov > bestv[threadIdx.x] || (ov == bestv[threadIdx.x] && oi < besti[threadIdx.x])) {", "ov > sv[col] || (ov == sv[col] && oi < mi))) {",
                "return va > vb || (va == vb && ia < ib);"):
        assert TIE_BREAK.search(old), old
    for old in ("done < wchunks ? 0 : (done - wchunks) / hchunks + 1;", "(ready - wchunks) / hchunks + 1"):
        assert EMITTED.search(old), old


def test_the_tie_break_is_written_once():
    src = _sources()
    assert TIE_BREAK.search(_code(src[HEADER]))
    assert TIE_BREAK.search(_code(src[EXCEPTION])) and TIE_BREAK.search(_code(src[PINNED_BY_PROFILE]))  # (still there: not stale)
    for f, text in src.items():
        if f in (HEADER, EXCEPTION, PINNED_BY_PROFILE):
            continue
        m = TIE_BREAK.search(_code(text))
        assert m is None, f"{f}: {m.group(0)}"
        if "__shfl_xor" in text and "first_max" not in text:
            # a butterfly that is no arg-max (a plain sum or maximum) carries no index
            assert not re.search(r"__shfl_xor\(\s*\w*i\b", _code(text)), f


def test_the_emitted_window_count_is_written_once():
    src = _sources()
    assert EMITTED.search(_code(src[HEADER]))
    for f, text in src.items():
        if f != HEADER:
            m = EMITTED.search(text)  # (comments included: they point to the header)
            assert m is None, f"{f}: {m.group(0)}"
    for f in ("stream_windows.hip", "stream_xylo.hip"):
        assert "StreamWindowWalk" in src[f], f
    assert "window_count64" in src["windows.hip"]
    assert "(window + hop - 1) / hop" not in src["stream_xylo.hip"] and "stream_window_slots(" in src["stream_xylo.hip"]


def test_makefile_names_the_header_for_exactly_the_objects_that_include_it():
    users = csrc_build.including_objects(HEADER)
    assert {"windows.o", "stream_windows.o", "stream_xylo.o", "track.o", "stream_track.o"} <= users
    named = csrc_build.rebuilt_after_edit(HEADER)
    assert named == users, (sorted(named - users), sorted(users - named))
