"""TEST INFRASTRUCTURE ONLY -- the yardstick of the background solve: how far is a float64 solution from THE solution?

The system is  A x = r,  A = diag(w) + lamF * sum_i (x[i+1] - x[i])^2 + lam * sum_i (x[i] - 2 x[i+1] + x[i+2])^2  read as a
quadratic form.  `solve_truth` assembles A from that definition, one difference term at a time --
no stencil table of the reference, of the oracle or of the device (`bg_pen_diag`, `bg_off1`) is consulted, so the n = 2, 3, 4 and
boundary rows are checked independently too -- and solves it by a banded LDL' in `numpy.longdouble` (x87: 64-bit significand)
with NO pivot floor: a pivot that is not positive raises.  Zero-centring follows the Lagrange form x - (sum x / sum u) u,
u = A^-1 1, with long-double sums.  The result is rounded to float64 once, at the end.

How good is it?  A banded LDL' of an SPD matrix is backward stable: the long-double solution is within a few 2^-64 cond2(A) of
the exact one relative to max|x| -- 2^-12 of the float64 gates built on it (tests/test_gpu_bg_edges.py: 4 * 2^-52 cond2(A)).
tests/test_bg_truth.py pins that against a 256-bit solve.

`cond2` is the 2-norm condition number of A in float64 (its own relative error is about 2^-52 cond2, negligible for a gate).
Never imported by ``consenrich_amd``.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
DENSE_MAX = 1200


def assemble_bands(w, lam_first, lam, dtype=LD):
    """(a0, a1, a2): main, first and second superdiagonal of A, accumulated term by term in `dtype`."""
    w = np.asarray(w, np.float64).reshape(-1)
    n = w.shape[0]
    a0 = [dtype(float(v)) for v in w]
    a1 = [dtype(0.0)] * max(n - 1, 0)
    a2 = [dtype(0.0)] * max(n - 2, 0)
    lf, l2 = dtype(float(lam_first)), dtype(float(lam))
    for i in range(n - 1):                     # lamF (x[i+1] - x[i])^2  =  lamF c c',  c = (-1, 1) at (i, i+1)
        a0[i] += lf
        a0[i + 1] += lf
        a1[i] -= lf
    for i in range(n - 2):                     # lam (x[i] - 2 x[i+1] + x[i+2])^2  =  lam c c',  c = (1, -2, 1) at (i, i+1, i+2)
        a0[i] += l2
        a0[i + 1] += dtype(4.0) * l2
        a0[i + 2] += l2
        a1[i] -= dtype(2.0) * l2
        a1[i + 1] -= dtype(2.0) * l2
        a2[i] += l2
    return a0, a1, a2


def _ldl_solve(a0, a1, a2, cols):
    """banded LDL' (bandwidth 2), forward and back substitution of every column of `cols`; scalars of the bands' type"""
    n = len(a0)
    zero = a0[0] * 0
    d, l1, l2 = [zero] * n, [zero] * n, [zero] * n          # L[i, i-1], L[i, i-2]
    for i in range(n):
        di = a0[i]
        if i >= 2:
            l2[i] = a2[i - 2] / d[i - 2]
            di -= l2[i] * l2[i] * d[i - 2]
        if i >= 1:
            e = a1[i - 1]
            if i >= 2:
                e -= l2[i] * d[i - 2] * l1[i - 1]
            l1[i] = e / d[i - 1]
            di -= l1[i] * l1[i] * d[i - 1]
        if not di > 0:
            raise np.linalg.LinAlgError(f"pivot {i} is not positive ({float(di):.6g}): the system is not positive definite")
        d[i] = di
    outs = []
    for c in cols:
        y = list(c)
        for i in range(n):
            if i >= 1:
                y[i] -= l1[i] * y[i - 1]
            if i >= 2:
                y[i] -= l2[i] * y[i - 2]
        x = [y[i] / d[i] for i in range(n)]
        for i in range(n - 1, -1, -1):
            if i + 1 < n:
                x[i] -= l1[i + 1] * x[i + 1]
            if i + 2 < n:
                x[i] -= l2[i + 2] * x[i + 2]
        outs.append(x)
    return outs


def solve_longdouble(w, r, lam_first, lam, centred=True):
    """(plain, zero-centred or None) as long-double arrays, before the rounding to float64"""
    w = np.asarray(w, np.float64).reshape(-1)
    r = np.asarray(r, np.float64).reshape(-1)
    n = w.shape[0]
    if r.shape[0] != n:
        raise ValueError("w and r must have the same length")
    if n == 0:
        return np.zeros(0, LD), (np.zeros(0, LD) if centred else None)
    a0, a1, a2 = assemble_bands(w, lam_first, lam)
    cols = [[LD(float(v)) for v in r]]
    if centred:
        cols.append([LD(1.0)] * n)
    sol = _ldl_solve(a0, a1, a2, cols)
    x = sol[0]
    if not centred:
        return np.asarray(x, LD), None
    u = sol[1]
    sx, su = LD(0.0), LD(0.0)
    for i in range(n):
        sx += x[i]
        su += u[i]
    mu = sx / su
    return np.asarray(x, LD), np.asarray([x[i] - mu * u[i] for i in range(n)], LD)


def solve_truth(w, r, lam_first, lam, zero_center):
    """the solution of A x = r (zero_center: minus its Lagrange correction), correct to a few 2^-64 cond2(A) of max|x|, float64"""
    return solve_longdouble(w, r, lam_first, lam, bool(zero_center))[1 if zero_center else 0].astype(np.float64)


def solve_truth_pair(w, r, lam_first, lam):
    """(plain, zero-centred) from one factorisation: the same numbers as two calls of `solve_truth`"""
    x, z = solve_longdouble(w, r, lam_first, lam, True)
    return x.astype(np.float64), z.astype(np.float64)


def cond2(w, lam_first, lam):
    """lambda_max / lambda_min of A: dense `eigvalsh` up to n = 1200, the two extreme eigenvalues of the band above that"""
    a0, a1, a2 = (np.asarray(b, np.float64) for b in assemble_bands(w, lam_first, lam, dtype=np.float64))
    n = a0.shape[0]
    if n == 0:
        return 1.0
    if n <= DENSE_MAX:
        A = np.diag(a0)
        if n > 1:
            A += np.diag(a1, 1) + np.diag(a1, -1)
        if n > 2:
            A += np.diag(a2, 2) + np.diag(a2, -2)
        ev = np.linalg.eigvalsh(A)
        lo, hi = float(ev[0]), float(ev[-1])
    else:
        from scipy.linalg import eigvals_banded

        ab = np.zeros((3, n))                   # lower form: row k holds the k-th subdiagonal
        ab[0], ab[1, :n - 1], ab[2, :n - 2] = a0, a1, a2
        lo = float(eigvals_banded(ab, lower=True, select="i", select_range=(0, 0))[0])
        hi = float(eigvals_banded(ab, lower=True, select="i", select_range=(n - 1, n - 1))[0])
    if not lo > 0.0:
        raise np.linalg.LinAlgError(f"smallest eigenvalue {lo:.6g} is not positive")
    return hi / lo
