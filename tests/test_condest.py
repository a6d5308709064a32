"""sf_chol_plan_condest / sf_lu_plan_condest (CholPlan.condest, LUPlan.condest): Hager / Higham's estimate of |A^-1|_1 with the
resident factor against the exact value from a dense inverse, and against the same estimator (tests/condest_ref.py, pinned on
the CPU in tests/test_lu_trans_ref.py) run over the device's own solves."""
import numpy as np
import pytest

from util import sf
from condest_ref import condest_ref, condest_cases, analyze_case, dense_permuted

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", condest_cases(), ids=lambda c: c[0])
def test_condest_against_dense_inverse(case):
    name, method, n, Cp, Ci, Cx, perm, tol = case
    S = analyze_case(case)
    if method == "lu":
        plan = sf.LUPlan(S)
        plan.set_values(S.Lx, S.Ux)
        if tol > 0:
            plan.set_pivoting(tol)
    else:
        plan = sf.CholPlan(S)
        plan.set_values(S.Lx)
    plan.factorize()
    A = dense_permuted(S)
    exact = np.abs(np.linalg.inv(A)).sum(axis=0).max()
    anorm_want = np.abs(A).sum(axis=0).max()
    kappa = anorm_want * exact
    anorm, est = plan.condest(return_parts=True)
    solves = int(plan.stat("last_condest_solves"))
    print(name, "exact", exact, "estimate", est, "solves", solves, "kappa_1", kappa, "ms", plan.stat("last_condest_ms"))
    assert abs(anorm - anorm_want) <= 1e-14 * anorm_want
    upper = exact * (1 + 100 * n * 2.0 ** -53 * kappa)         # the forward error of the solves, not a tuned number
    assert exact / 3 <= est <= upper, (name, est, exact)
    assert 1 <= solves <= 11
    assert plan.stat("last_condest_ms") > 0 and plan.stat("bytes_condest") > 0
    assert plan.condest() == pytest.approx(anorm * est, rel=1e-12)
    # the same estimator over the device's own solves
    solve_t = (lambda v: plan.solve(v, trans=True)) if method == "lu" else plan.solve
    ref, ref_solves = condest_ref(plan.solve, solve_t, n)
    print(name, "condest_ref over the device solves", ref, ref_solves)
    assert abs(est - ref) <= 1e-8 * ref or exact / 3 <= ref <= upper
    # a second call gives the same bits (fixed-order reductions; the sweeps' atomics only matter where the signs are close calls)
    bytes_before = plan.stat("bytes_device")
    anorm2, est2 = plan.condest(return_parts=True)
    assert anorm2 == anorm and exact / 3 <= est2 <= upper
    assert plan.stat("bytes_device") == bytes_before
    # new values, the same plan: |A|_1 follows the values
    if method == "lu":
        plan.set_values(S.Lx * 2.0, S.Ux * 2.0)
    else:
        plan.set_values(S.Lx * 2.0)
    plan.factorize()
    anorm3, est3 = plan.condest(return_parts=True)
    assert abs(anorm3 - 2 * anorm_want) <= 2e-14 * anorm_want
    assert exact / 6 <= est3 <= upper / 2
    plan.close()


def test_one_by_one():
    S = sf.analyze(1, np.array([0, 1]), np.array([0]), np.array([4.0]), None, 1 << 30)
    plan = sf.CholPlan(S)
    plan.set_values(S.Lx)
    plan.factorize()
    assert plan.condest(return_parts=True) == (4.0, 0.25)
    assert plan.stat("last_condest_solves") == 1
    plan.close()
