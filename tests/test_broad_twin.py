"""The pure-Python twin of broad mode (tests/twin_broad.py) against the fixtures made from the reference's own functions: both of
its forms -- the reference's steps, and the decomposition the library makes -- on every case, bit for bit, with the branches the
case table must take."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import broad_cases as BC  # noqa: E402
import twin_broad as T  # noqa: E402

GOLD = os.path.join(HERE, "golden", "broad")
MERGE, ROWS, PARENTS = BC.merge_cases(), BC.rows_cases(), BC.parents_cases()


def golden(file, name):
    with np.load(os.path.join(GOLD, file)) as z:
        return BC.unpack(z[name])


@pytest.mark.parametrize("form", ["steps", "device"])
@pytest.mark.parametrize("case", MERGE, ids=lambda c: c["name"])
def test_merge_twin_equals_the_reference(case, form):
    got = T.merge(form=form, **case["kw"])
    assert BC.differences(BC.canon(got), golden("broad_merge.npz", case["name"])) == []


@pytest.mark.parametrize("form", ["steps", "device"])
@pytest.mark.parametrize("case", ROWS, ids=lambda c: c["name"])
def test_rows_twin_equals_the_reference(case, form):
    with np.errstate(invalid="ignore"):
        got = T.rows(form=form, **case["kw"])
    assert BC.differences(BC.canon(got), golden("broad_rows.npz", case["name"])) == []


@pytest.mark.parametrize("case", ROWS, ids=lambda c: c["name"])
def test_host_pieces_of_the_twin(case):
    kw = case["kw"]
    pr = T.coordinate_runs(kw["parentSolution"], kw["intervals"], kw["ends"])
    cr = T.coordinate_runs(kw["childSolution"], kw["intervals"], kw["ends"])
    assert BC.differences(BC.canon((pr, cr)), golden("broad_host.npz", f"runs/{case['name']}")) == []
    got = [T.blocks(a, b, cr, kw["intervals"], kw["ends"]) for a, b in pr]
    assert BC.differences(BC.canon(got), golden("broad_host.npz", f"blocks/{case['name']}")) == []


@pytest.mark.parametrize("form", ["steps", "device"])
@pytest.mark.parametrize("case", PARENTS, ids=lambda c: c["name"])
def test_parents_twin_equals_the_reference(case, form):
    """The envelope, the support runs, the fallback and the bridging: peaks.py:6884-6932 around the reference's own functions"""
    got = T.parents(form=form, **case["kw"])
    mask = got.pop("mask")
    want = golden("broad_parents.npz", case["name"])
    assert BC.differences(BC.canon(got), want) == []
    filled = np.zeros(mask.size, np.uint8)
    for a, b in zip(got["starts"], got["ends"]):
        filled[a:b + 1] = 1
    assert np.array_equal(mask, filled)


def test_the_support_run_cases_take_every_branch():
    T.reset_branches()
    for case in PARENTS:
        T.parents(form="device", **case["kw"])
    assert [k for k in BC.NEEDED_PARENTS if not T.BRANCHES.get(k)] == [], T.BRANCHES


def test_the_case_table_takes_every_branch():
    T.reset_branches()
    hosts = {}
    for case in MERGE:
        T.merge(form="device", **case["kw"])
    for case in ROWS:
        before = T.BRANCHES.get("decided_on_host", 0)
        with np.errstate(invalid="ignore"):
            T.rows(form="device", **case["kw"])
        hosts[case["name"]] = T.BRANCHES.get("decided_on_host", 0) - before
    lacking = [k for k in BC.NEEDED if not T.BRANCHES.get(k)]
    assert lacking == [], T.BRANCHES
    assert {k for k, v in hosts.items() if v} == set(BC.HOST_DECIDED)
