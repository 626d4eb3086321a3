"""CPU: the oracle's delete-block calibration natives (oracle/consenrich_oracle.c
`cor_total_information`, `cor_fold_mask_information`) against golden vectors captured from the compiled reference
(cuncertainty.pyx:97-157, 160-305) -- bit for bit -- and live against it where it exists (else against its
recorded outputs); argument validation."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import live_cases  # noqa: E402
import unc_cases  # noqa: E402

from oracle import oracle as orc  # noqa: E402
from oracle import ref_loader  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
CASES = {c["name"]: c for c in unc_cases.cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_golden(name):
    got = unc_cases.run(orc, CASES[name])
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert set(got) == set(gold.files)
    for k in gold.files:
        assert np.array_equal(got[k], gold[k], equal_nan=True), k


def test_oracle_matches_live_reference_and_fold_spec():
    """Bit for bit: against what the reference returned (recorded, tests/golden/live_reference.json) and, where its build
    exists, against the reference itself."""
    case = live_cases.UNC_CASE
    b = unc_cases.run(orc, case)
    live_cases.check("uncertainty", "live", b)
    spec = unc_cases.fold_spec(*live_cases.FOLD_SPEC_ARGS)
    live_cases.check("uncertainty", "fold_spec", {str(i): np.asarray(x) for i, x in enumerate(spec)})
    if ref_loader.load() is None:
        return
    from consenrich import cuncertainty as ref

    a = unc_cases.run(ref, case)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert all(np.array_equal(x, y) for x, y in zip(spec, ref.cmakeFoldSpec(*live_cases.FOLD_SPEC_ARGS)))


def test_validation_messages():
    case = CASES["unc_m4_n20"]
    munc, act, lam, (bf, rc, rb) = unc_cases.inputs(case)
    tot = orc.cobservationTotalInformation(munc, act, lam, False, 1e-4, 0.0)
    args = lambda **kw: dict(dict(m=4, n=20, blockLen=5, fold=0, blockFold=bf, repsByBlockCount=rc, repsByBlock=rb,     # noqa: E731
                                  matrixMunc=munc, activeMask=act, totalInfo=tot, lambdaExp=lam, useLambda=False, pad=1e-4), **kw)
    with pytest.raises(ValueError, match="fold must be nonnegative"):
        orc.cmakeFoldMaskAndInformation(**args(fold=-1))
    with pytest.raises(ValueError, match="inconsistent block count"):
        orc.cmakeFoldMaskAndInformation(**args(blockFold=bf[:-1]))
    bad = rb.copy(); bad[0, 1] = bad[0, 0]
    with pytest.raises(ValueError, match="duplicate replicate"):
        orc.cmakeFoldMaskAndInformation(**args(repsByBlock=bad))
    with pytest.raises(ValueError, match="rho must be in"):
        orc.cmakeFoldMaskAndInformation(**args(), replicateDependenceRho=1.0)
    with pytest.raises(ValueError, match="activeMask must match"):
        orc.cobservationTotalInformation(munc, act[:, :-1], lam, False, 1e-4)
