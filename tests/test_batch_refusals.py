"""The four doors of the batch sketcher answer what they answered before their parameter checks moved into one place
(finch_rs_amd/csrc/fh_batch_plan.h): tests/golden/batch_refusals.json holds fh_last_error() of every case of a grid, verbatim,
recorded by tests/golden/make_batch_refusals.py (which defines the grid) on the build before that change.  ACCEPTED means the
parameters pass: a handle where there is a GPU, exactly the "no usable HIP device" message elsewhere.  Where there is a GPU only
the dozen accepted cases the generator lists under CONSTRUCT (at most 4 files, 1 MiB) are asked at all -- the others would pin
gigabytes each."""
import importlib.util
import json
import os

import pytest

from finch_rs_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_batch_refusals", os.path.join(HERE, "golden", "make_batch_refusals.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)
GOLD = json.load(open(os.path.join(HERE, "golden", "batch_refusals.json")))
CASES = GEN.cases()
WANT = [GOLD["messages"][a] for a in GOLD["answers"]]
DOORS = GEN.DOORS + ("fh_batch_new_counts",)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as G
    G.build()
    return _lib.load()


def test_the_golden_file_covers_the_grid():
    assert len(WANT) == len(CASES) > 5000
    accepted = [c for c, w in zip(CASES, WANT) if w == "ACCEPTED"]
    assert len(GEN.CONSTRUCT) == 12 and all(c in accepted and c[6] <= 4 and c[7] == 1 << 20 for c in GEN.CONSTRUCT)
    assert {c[0] for c in GEN.CONSTRUCT} == set(DOORS) and {c[0] for c in accepted} == set(DOORS)
    assert GEN.NO_DEVICE not in GOLD["messages"] and "" not in GOLD["messages"]
    assert sorted(set(GOLD["answers"])) == list(range(len(GOLD["messages"])))  # every message is some case's answer


@pytest.mark.parametrize("door", DOORS)
def test_every_case_answers_as_recorded(L, door):
    have_gpu = L.fh_device_count() > 0
    asked = 0
    for case, want in zip(CASES, WANT):
        if case[0] != door or (have_gpu and want == "ACCEPTED" and case not in GEN.CONSTRUCT):
            continue
        h, msg = GEN.ask(L, case)
        if h:
            L.fh_batch_free(h)
        asked += 1
        if want != "ACCEPTED":
            assert not h and msg == want, (case, msg, want)
        elif have_gpu:
            assert h, (case, msg)
        else:
            assert not h and msg == GEN.NO_DEVICE, (case, msg)
    assert asked > 100
    L.fh_release_cached()
