"""The life-cycle of a plan's factor (csrc/sf_factor_state.h) through the public API: a Cholesky and an LU plan of the
6 x 6 x 6 seven-point grid (n = 216) walk through values, factorizations (whole, unsynchronised, by phase, as a hipGraph), the
selected inverse, an update, a downdate that fails.  After every step: the stats factor_generation, factor_usable and selinv_valid,
and whether a solve, a solve_device, a selinv_diag, a logdet_grad_values and an update are accepted or refused.  The accepted
update of a step is itself a replacement of the factor, so it comes last and the stats are read again behind it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import updown_ref as ur
from util import sf

pytestmark = pytest.mark.gpu

N = 6
OK, ARG, NOT_POSDEF = "SF_OK", "SF_ERR_ARG", "SF_ERR_NOT_POSDEF"


def code(call):
    try:
        call()
    except sf.SparseFrameError as e:
        return str(e).rsplit(": ", 1)[1]
    return OK


class Walk:
    """a plan, the generation its factor must have, the dense matrix that factor belongs to (Cholesky) and the probes"""

    def __init__(self, lu):
        import torch
        n, Cp, Ci, Cx = sf.gen.laplacian_lower(N, N, N)
        perm = sf.grid_nd_perm(N, N, N)
        self.lu = lu
        self.sym = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", True) if lu else sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30)
        assert self.sym.n == 216 and self.sym.nsuper > 4
        self.plan = (sf.LUPlan if lu else sf.CholPlan)(self.sym)
        self.gen = 0
        self.A0 = None if lu else ur.dense_matrix(self.sym)
        self.A = None
        self.b = 1.0 + np.arange(n) / n
        self.B = torch.tensor(self.b, device="cuda:0")
        self.bump = np.zeros(n)
        self.bump[n // 3] = 0.25

    def stats(self):
        return tuple(int(self.plan.stat(k)) for k in ("factor_generation", "factor_usable", "selinv_valid"))

    def set_values(self):
        self.plan.set_values(self.sym.Lx)
        self.gen += 1

    def factorized(self):
        """a factorization has started: one generation on, and its factor will be that of the values"""
        self.gen += 1
        self.A = None if self.lu else self.A0.copy()

    def update(self, W, downdate=False):
        if self.lu:         # (LUPlan has no such method: the entry point itself)
            Wp, Wi = np.array([0, 1], dtype=np.int64), np.array([int(np.flatnonzero(W)[0])], dtype=np.int64)
            Wx = np.array([W[Wi[0]]])
            lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
            rc = sf.lib.sf_chol_plan_update(self.plan._h, -1 if downdate else 1, 1, Wp.ctypes.data_as(lp), Wi.ctypes.data_as(lp),
                                            Wx.ctypes.data_as(dp), 0)
            return {0: OK, 1: ARG}[rc]
        return code(lambda: self.plan.update(W, downdate=downdate))

    def probe(self, solve, solve_dev, sel, update):
        """the five calls; update last, and when it is accepted the factor is the next generation's, usable, without its inverse"""
        p = self.plan
        x = []
        assert code(lambda: x.append(p.solve(self.b))) == solve, "solve"
        if solve == OK and solve_dev == OK and self.A is not None:
            assert np.max(np.abs(self.A @ x[0] - self.b)) <= 1e-10 * np.max(np.abs(x[0])) * np.max(np.abs(self.A))
        X = []
        assert code(lambda: X.append(p.solve_device(self.B))) == solve_dev, "solve_device"
        if solve == OK and solve_dev == OK:
            assert np.max(np.abs(X[0].cpu().numpy() - x[0])) <= 1e-12 * np.max(np.abs(x[0]))
        assert code(p.selinv_diag) == sel, "selinv_diag"
        assert code(p.logdet_grad_values) == sel, "logdet_grad_values"
        assert self.update(self.bump) == (ARG if self.lu else update), "update"
        if update == OK and not self.lu:
            self.gen += 1
            self.A += np.outer(self.bump, self.bump)
            assert self.stats() == (self.gen, 1, 0)


def walk(lu, graph=False):
    w = Walk(lu)
    p = w.plan
    assert w.stats() == (0, 0, 0)
    # 1. values, no factor
    w.set_values()
    assert w.stats() == (w.gen, 0, 0) and w.gen == 1
    w.probe(OK, ARG, ARG, ARG)              # (the plain solve has never asked for a factorization)
    assert code(p.selinv) == ARG
    # 2. a factorization nobody has waited for: the stat does not collect, the sync does
    p.factorize(sync=False)
    w.factorized()
    assert w.stats() == (w.gen, 0, 0)
    p.sync()
    assert w.stats() == (w.gen, 1, 0)
    w.probe(OK, OK, ARG, OK)
    # 3. the selected inverse (of the updated factor: an update counts as factorized)
    p.selinv()
    assert w.stats() == (w.gen, 1, 1)
    w.probe(OK, OK, OK, OK)
    p.selinv()
    assert w.stats() == (w.gen, 1, 1)
    # 4. new values: the factor stays usable, its inverse is no longer that of the values, a new one is refused
    w.set_values()
    assert w.stats() == (w.gen, 1, 0)
    assert code(p.selinv) == ARG and w.stats() == (w.gen, 1, 0)
    # 5. an update (the probe's)
    w.probe(OK, OK, ARG, OK)
    if not lu:
        # 6. a downdate that loses definiteness, by the reference's account too
        j = w.sym.n // 2
        W = np.zeros(w.sym.n)
        W[j] = 2.0 * np.sqrt(w.A[j, j])
        _, failed, _ = ur.update_emulate(ur.Structure(w.sym), p.get_factor().copy(), W[:, None], -1)
        assert failed
        assert w.update(W, downdate=True) == NOT_POSDEF
        w.gen += 1
        assert w.stats() == (w.gen, 0, 0)
        w.probe(ARG, ARG, ARG, ARG)
        assert code(p.selinv) == ARG and code(p.sync) == OK and w.stats() == (w.gen, 0, 0)
    # 7. a factorization
    p.factorize()
    w.factorized()
    assert w.stats() == (w.gen, 1, 0)
    w.probe(OK, OK, ARG, OK)
    # 8. by phase on a one-rank plan; it has no segments, so that form is refused and changes nothing
    p.factorize_phase(0, sync=False)
    w.factorized()
    assert w.stats() == (w.gen, 0, 0)
    p.sync()                                # nothing to collect before the last launch is enqueued
    assert w.stats() == (w.gen, 0, 0)
    assert p.num_segments() == 0 and code(lambda: p.factorize_segment(0)) == ARG
    assert code(lambda: p.solve_device(w.B)) == ARG and code(p.selinv) == ARG
    p.factorize_phase(1, sync=False)
    assert w.stats() == (w.gen, 0, 0)
    w.probe(OK, OK, ARG, OK)                # (solve_device collects)
    p.selinv()
    assert w.stats() == (w.gen, 1, 1)
    if graph:
        # 9. SF_GRAPH=1: step 2 captured the graph and step 7 replayed it; two more replays nobody waits for
        for _ in range(2):
            p.factorize(sync=False)
            w.factorized()
            assert w.stats() == (w.gen, 0, 0)
            w.probe(OK, OK, ARG, OK)
            p.selinv()
            assert w.stats() == (w.gen, 1, 1)
            w.set_values()
            assert w.stats() == (w.gen, 1, 0)
    p.close()


@pytest.mark.parametrize("lu", [False, True], ids=["cholesky", "lu"])
def test_walk(lu):
    walk(lu)


def test_walk_with_graph_capture_and_replay():
    """the same walk in a fresh process with SF_GRAPH=1 (read when a plan is made), both plans"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, SF_GRAPH="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "FACTOR_STATE_GRAPH_OK" in r.stdout, r.stdout


if __name__ == "__main__":
    walk(False, graph=True)
    walk(True, graph=True)
    print("FACTOR_STATE_GRAPH_OK")
