"""What the clean-up tests share: every case of tests/cleanup_cases.py through a set of entry points (the twin's forms, the
package's drop-ins on the device or on the CPU stand-in), against the fixtures of tests/golden/cleanup."""
import os

import numpy as np

import cleanup_cases as CC
import twin_cleanup as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cleanup")
_CACHE = {}


def golden(kind, name):
    if kind not in _CACHE:
        with np.load(os.path.join(GOLD, f"cleanup_{kind}.npz")) as z:
            _CACHE[kind] = {k: z[k] for k in z.files}
    return {k[len(name) + 1:]: v for k, v in _CACHE[kind].items() if k.startswith(name + "/")}


def force_ids():
    return [c["name"] for c in CC.FORCE]


def check_force(force, name):
    case = next(c for c in CC.FORCE if c["name"] == name)
    for k, kw in enumerate(CC.force_inputs(case)):
        got = force(**kw)
        assert type(got) is tuple and len(got) == 2 and type(got[0]) is list and type(got[1]) is dict
        want = golden("force", f"{name}/{k}")
        assert want, name
        assert T.same_flat(T.flatten_force(got), want) == [], (name, k)


def check_splits(split):
    for case in CC.SPLITS:
        got = split(**{k: v for k, v in case.items() if k != "name"})
        assert T.same_flat(T.flatten_split(got), golden("split", case["name"])) == [], case["name"]


def check_contracts(contract):
    for case in CC.CONTRACTS:
        got = contract(**{k: v for k, v in case.items() if k != "name"})
        assert T.same_flat(T.flatten_contract(got), golden("contract", case["name"])) == [], case["name"]


def row_ids():
    return [c["name"] for c in CC.ROWS]


def check_rows(rows, name):
    case = next(c for c in CC.ROWS if c["name"] == name)
    got = rows(**CC.row_inputs(case))
    assert type(got) is tuple and len(got) == 3
    want = golden("rows", name)
    assert want, name
    assert T.same_flat(T.flatten_rows(got), want) == [], name
    return got
