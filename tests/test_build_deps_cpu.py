"""csrc/Makefile names no header: the compiler writes every object's prerequisites beside it (-MMD).  Held against the include closure
read from the sources: an edit of a header rebuilds exactly the objects whose sources include it, whichever header it is."""
import os

import csrc_build
import pytest

HEADERS = sorted(f for f in os.listdir(csrc_build.CSRC) if f.endswith(".h")) + [csrc_build.PUBLIC_HEADER]


@pytest.mark.parametrize("header", HEADERS, ids=[os.path.basename(h) for h in HEADERS])
def test_an_edit_of_a_header_rebuilds_exactly_the_objects_that_include_it(header):
    users = csrc_build.including_objects(header)
    assert users, f"no source includes {header}"
    rebuilt = csrc_build.rebuilt_after_edit(header)
    assert rebuilt == users, (sorted(rebuilt - users), sorted(users - rebuilt))


def test_every_source_of_the_directory_is_built():
    assert csrc_build.built_sources() == {f for f in os.listdir(csrc_build.CSRC) if f.endswith(".hip")}
