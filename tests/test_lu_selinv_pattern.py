"""LUPlan.selinv_values / _values_device / selinv_trace / _trace_device / selinv_entries / logdet_grad (sf_lu_plan_selinv_values[_t],
_trace, _entries) on the device: plans with their own U structure and plans whose U aliases L.  As for the Cholesky
plans (test_selinv_pattern.py): the values with `==` against the host gather out of get_selinv(), the trace tied to the
TRANSPOSED values bit for bit through indicator arrays, general V inside T eps sum|terms|."""
import ctypes as C
import types

import numpy as np
import pytest

import selinv_pattern_ref as spr
from util import sf, gen
from test_lu_selinv_abi import lu_selinv_cases

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
CASES = lu_selinv_cases()
IDS = [c[0] for c in CASES]
ALIASED, OWN_U = "sym_lap3d_7_via_lu", "st3d_8_nd"


def _with_duplicates(Cp, Ci, Cx, rng, count):
    """(Cp, Ci, Cx) with `count` entries given twice, the extra copy FIRST in its column and with a wrong value"""
    picks = np.sort(rng.choice(len(Ci), count, replace=False))
    col = np.searchsorted(Cp, picks, side="right") - 1
    Ci2 = np.insert(Ci, picks, Ci[picks])
    Cx2 = np.insert(Cx, picks, Cx[picks] * 3.0 + 1.0)
    Cp2 = Cp + np.concatenate([[0], np.cumsum(np.bincount(col, minlength=len(Cp) - 1))])
    return np.ascontiguousarray(Cp2, dtype=np.int64), np.ascontiguousarray(Ci2, dtype=np.int64), Cx2


class Ctx:
    """a factorized plan with its selected inverse, the packed arena on the host and the reference values (made once, never changed)"""

    def __init__(self, sym, symm):
        self.sym, self.symm = sym, symm
        self.plan = sf.LUPlan(sym, device=0)
        self.plan.set_values(sym.Lx, None if symm else sym.Ux)
        self.plan.factorize()
        self.plan.selinv()
        self.S = self.plan.get_selinv().copy()
        self.S.setflags(write=False)
        self.nnz = len(sym.Li)
        self.unz = 0 if symm else len(sym.Ui)
        self.SL, self.SU = spr.lu_values(sym, self.S, symm)
        self.TL, self.TU = spr.lu_values(sym, self.S, symm, transposed=True)
        self.chunk = int(self.plan.stat("selinv_pattern_chunk"))
        self.tile = int(self.plan.stat("selinv_pattern_tile"))

    def terms(self, VL, VU=None):
        return spr.lu_trace_terms(self.sym, self.S, self.symm, VL, VU)

    def random_V(self, rng, m, pad=0):
        VL = np.asfortranarray(rng.uniform(-1, 1, (self.nnz + pad, m)))[:self.nnz]
        VU = None if self.symm else np.asfortranarray(rng.uniform(-1, 1, (self.unz + pad, m)))[:self.unz]
        return VL, VU


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(key):
        if key not in made:
            if key in ("dup_aliased", "dup_own_u"):
                N = 12
                symm = key == "dup_aliased"
                n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N) if symm else gen.unsymmetric_stencil(N, N, N, seed=3)
                sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30, "lu", symm)
                keys = ("n", "nsuper", "Super", "SuperMap", "Lsip", "Lsi", "Lsxp", "xsize", "lu", "symmetric")
                dup = types.SimpleNamespace(**{k: getattr(sym, k) for k in keys})
                rng = np.random.default_rng(7)
                dup.Lp, dup.Li, dup.Lx = _with_duplicates(sym.Lp, sym.Li, sym.Lx, rng, 3000)
                if not symm:
                    dup.Up, dup.Ui, dup.Ux = _with_duplicates(sym.Up, sym.Ui, sym.Ux, rng, 3000)
                made[key] = Ctx(dup, symm)
            else:
                name, n, Cp, Ci, Cx, perm, slot, symm = CASES[IDS.index(key)]
                made[key] = Ctx(sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", symm), symm)
        return made[key]

    yield get
    for c in made.values():
        c.plan.close()


def _bound_ok(got, terms):
    """|got - sum| <= T eps sum|terms| against the float64 numpy sum of the same products, T = the number of products"""
    ref = terms.sum(axis=0)
    bound = terms.shape[0] * EPS * np.abs(terms).sum(axis=0)
    print("trace: max |got - ref| / bound", float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300))))
    return bool(np.all(np.abs(got - ref) <= bound))


def _same(got, want):
    return (got is None and want is None) or np.array_equal(got, want)


@pytest.mark.parametrize("name", IDS + ["dup_aliased", "dup_own_u"])
def test_values_are_the_host_gather(ctx, name):
    """the unit boundaries (unsym_blocks_64_65, _512_513_3), aliased and explicit-U plans, duplicated entries, and the diagonal
    positions of L, which the assembly skips: Sigma_jj"""
    import torch
    c = ctx(name)
    for transposed, wantL, wantU in ((False, c.SL, c.SU), (True, c.TL, c.TU)):
        got = c.plan.selinv_values(transposed=transposed)
        gotL, gotU = (got, None) if c.symm else got
        assert gotL.shape == (c.nnz,) and np.array_equal(gotL, wantL) and _same(gotU, wantU)
        dL = torch.full((c.nnz,), 7.0, dtype=torch.float64, device="cuda:0")
        dU = None if c.symm else torch.full((c.unz,), 7.0, dtype=torch.float64, device="cuda:0")
        c.plan.selinv_values_device(dL, dU, transposed=transposed)
        assert np.array_equal(dL.cpu().numpy(), wantL) and (dU is None or np.array_equal(dU.cpu().numpy(), wantU))
    j = np.repeat(np.arange(c.sym.n), np.diff(c.sym.Lp))
    diag = np.asarray(c.sym.Li) == j
    assert np.count_nonzero(diag) >= c.sym.n
    assert np.array_equal(c.SL[diag], c.plan.selinv_diag()[j[diag]])
    if c.symm:                                          # U aliasing L: outU must be NULL
        buf = np.full(c.nnz, 7.0)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert sf.lib.sf_lu_plan_selinv_values(c.plan._h, dp(buf), dp(buf)) == 1 and np.all(buf == 7.0)


def _indicator_traces(c, side, positions):
    """selinv_trace of the indicator of every position of L (side 0) or U (side 1), 64 at a time"""
    positions = np.asarray(positions)
    out = np.zeros(len(positions))
    for k0 in range(0, len(positions), 64):
        ps = positions[k0:k0 + 64]
        VL = np.zeros((c.nnz, len(ps)), order="F")
        VU = None if c.symm else np.zeros((c.unz, len(ps)), order="F")
        (VL if side == 0 else VU)[ps, np.arange(len(ps))] = 1.0
        out[k0:k0 + 64] = c.plan.selinv_trace(VL, VU)
    return out


def _boundary_positions(sym, Lp, count):
    edges = np.arange(256, count, 256)
    s = int(np.argmax(np.diff(sym.Super)))
    lastcol = int(sym.Super[s + 1] - 1)
    ps = np.concatenate([[0, count - 1, Lp[lastcol], Lp[lastcol + 1] - 1], edges - 1, edges])
    return np.unique(ps[(ps >= 0) & (ps < count)]).astype(np.int64)


@pytest.mark.parametrize("name", [OWN_U, ALIASED, "one_by_one", "dup_aliased", "dup_own_u"])
def test_trace_of_an_indicator_is_the_transposed_value(ctx, name):
    c = ctx(name)
    sym = c.sym
    if name == OWN_U:
        assert c.nnz > c.tile and c.unz > c.tile        # more than one workgroup on each side
    j = np.repeat(np.arange(sym.n), np.diff(sym.Lp))
    diag = np.asarray(sym.Li) == j
    liveL = spr.live_mask(sym.Lp, sym.Li, skip_diag=True)
    ps = _boundary_positions(sym, sym.Lp, c.nnz)
    got = _indicator_traces(c, 0, ps)
    if c.symm:
        # one structure feeds both triangles: an off-diagonal entry meets Sigma(j, i) and Sigma(i, j), the diagonal Sigma_jj once
        live = spr.live_mask(sym.Lp, sym.Li)
        want = np.where(live[ps], np.where(diag[ps], c.SL[ps], c.TL[ps] + c.SL[ps]), 0.0)
    else:
        want = np.where(liveL[ps], c.TL[ps], 0.0)       # (the L diagonal is not assembled: 0)
    assert np.array_equal(got, want)
    if not c.symm:
        liveU = spr.live_mask(sym.Up, sym.Ui)
        pu = _boundary_positions(sym, sym.Up, c.unz)
        assert np.array_equal(_indicator_traces(c, 1, pu), np.where(liveU[pu], c.TU[pu], 0.0))
        if name == "dup_own_u":
            dead = np.nonzero(~liveU)[0][[0, -1]]
            assert np.array_equal(_indicator_traces(c, 1, dead), np.zeros(2)) and np.all(c.TU[dead] != 0.0)
    if name.startswith("dup"):
        dead = np.nonzero(~liveL & ~diag)[0][[0, -1]]
        assert np.array_equal(_indicator_traces(c, 0, dead), np.zeros(2)) and np.all(c.TL[dead] != 0.0)


def test_exact_arithmetic():
    for d in (np.ones(3), np.ones(4099), 4.0 ** np.arange(-10, 11)):       # diag(2^k), k even: the square roots are exact too
        n = len(d)
        for symm in (True, False):
            sym = sf.analyze(n, np.arange(n + 1), np.arange(n), np.asarray(d, dtype=np.float64), None, 1 << 30, "lu", symm)
            c = Ctx(sym, symm)
            d = np.asarray(sym.Lx)                      # (the diagonal in the plan's own ordering)
            assert len(d) == n and (symm or np.array_equal(sym.Ux, d))
            got = c.plan.selinv_values()
            assert np.array_equal(got if symm else got[0], 1.0 / d) and (symm or np.array_equal(got[1], 1.0 / d))
            rng = np.random.default_rng(n)
            VL = rng.integers(-8, 9, (n, 5)).astype(np.float64)
            VU = None if symm else rng.integers(-8, 9, (n, 5)).astype(np.float64)
            want = ((VL if symm else VU) / d[:, None]).sum(axis=0)     # the diagonal counts once, from the side that stores it
            tr = c.plan.selinv_trace(VL, VU)
            assert np.array_equal(tr, want) and np.array_equal(c.plan.selinv_trace(VL, VU), tr)
            c.plan.close()


@pytest.mark.parametrize("name", IDS + ["dup_aliased", "dup_own_u"])
def test_general_V(ctx, name):
    import torch
    c = ctx(name)
    rng = np.random.default_rng(IDS.index(name) if name in IDS else 99)
    for m in (1, c.chunk - 1, c.chunk, c.chunk + 1, 64):
        VL, VU = c.random_V(rng, m, pad=5)              # column-major with padded leading dimensions
        got = c.plan.selinv_trace(VL, VU)
        assert got.shape == (m,) and _bound_ok(got, c.terms(VL, VU))
        gotc = c.plan.selinv_trace(np.ascontiguousarray(VL), None if VU is None else np.ascontiguousarray(VU))
        assert np.array_equal(gotc, got) and np.array_equal(c.plan.logdet_grad(VL, VU), got)
        dL = torch.from_numpy(np.ascontiguousarray(VL)).to("cuda:0")              # C order: taken via one device copy
        dU = None if VU is None else torch.from_numpy(np.asfortranarray(VU)).to("cuda:0")
        assert np.array_equal(c.plan.selinv_trace_device(dL, dU).cpu().numpy(), got)
    one = c.plan.selinv_trace(VL[:, 0], None if VU is None else VU[:, 0])
    assert isinstance(one, float) and one == got[0]


@pytest.mark.parametrize("name", [OWN_U, ALIASED])
def test_nan_stays_in_its_column(ctx, name):
    c = ctx(name)
    VL, VU = c.random_V(np.random.default_rng(5), 2 * c.chunk + 3)
    clean = c.plan.selinv_trace(VL, VU)
    live = np.nonzero(spr.live_mask(c.sym.Lp, c.sym.Li, skip_diag=True))[0]
    for t in (0, c.chunk, VL.shape[1] - 1):
        W = VL.copy()
        W[live[len(live) // 2], t] = np.nan
        got = c.plan.selinv_trace(W, VU)
        keep = np.arange(VL.shape[1]) != t
        assert np.isnan(got[t]) and np.array_equal(got[keep], clean[keep])


@pytest.mark.parametrize("name", [OWN_U, ALIASED])
def test_mapped(ctx, name):
    c = ctx(name)
    with pytest.raises(ValueError):
        c.plan.selinv_trace(np.ones(c.nnz), mapped=True)
    rng = np.random.default_rng(11)
    nsrc = c.nnz + c.unz + 17
    mapL = rng.integers(-1, nsrc, c.nnz)
    mapL[rng.choice(c.nnz, 40, replace=False)] = -1
    mapU = None if c.symm else rng.integers(-1, nsrc, c.unz)
    c.plan.set_value_map(nsrc, mapL, mapU)
    A = rng.uniform(-1, 1, (nsrc, c.chunk + 1))
    VL = spr.mapped_columns(mapL, A)
    VU = None if c.symm else spr.mapped_columns(mapU, A)
    got = c.plan.selinv_trace(A, mapped=True)
    assert _bound_ok(got, c.terms(VL, VU))
    assert _bound_ok(c.plan.selinv_trace(VL, VU), c.terms(VL, VU))


@pytest.mark.parametrize("name", ["st2d_12x9_nd", "st3d_5_nd", ALIASED])
def test_entries_inside_and_outside(ctx, name):
    c = ctx(name)
    n = c.sym.n
    rr, cc = spr.pattern_pairs(c.sym)
    rows, cols = np.concatenate([rr, cc]), np.concatenate([cc, rr])         # L's pattern and U's: (i, j) is taken literally
    got, outside = c.plan.selinv_entries(rows, cols)
    want, _ = spr.entries(c.sym, c.S, rows, cols, lu=True)
    assert outside == 0 and np.array_equal(got, want)
    inpat = np.zeros((n, n), dtype=bool)
    inpat[rr, cc] = inpat[cc, rr] = True
    oi, oj = np.nonzero(~inpat)
    assert len(oi)
    got, outside = c.plan.selinv_entries(np.concatenate([oi, rr[:5]]), np.concatenate([oj, cc[:5]]))
    assert outside == len(oi) and np.all(np.isnan(got[:len(oi)])) and c.plan.stat("last_selinv_outside") == len(oi)
    assert np.array_equal(got[len(oi):], spr.entries(c.sym, c.S, rr[:5], cc[:5], lu=True)[0])
    got, outside = c.plan.selinv_entries([], [])
    assert got.shape == (0,) and outside == 0
    got, outside = c.plan.selinv_entries([cc[-1]], [rr[-1]])
    assert outside == 0 and got[0] == spr.entries(c.sym, c.S, cc[-1:], rr[-1:], lu=True)[0][0]
    out = np.full(3, 7.0)
    bad = np.array([0, n, 0], dtype=np.int64)
    ok = np.zeros(3, dtype=np.int64)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    for r, cl in ((bad, ok), (ok, bad)):
        assert sf.lib.sf_lu_plan_selinv_entries(c.plan._h, 3, lp(r), lp(cl), out.ctypes.data_as(C.POINTER(C.c_double)), None) == 1
    assert np.all(out == 7.0)


def test_entries_across_the_staging_chunk(ctx):
    c = ctx(OWN_U)
    chunk = int(c.plan.stat("selinv_entries_chunk"))
    rr, cc = spr.pattern_pairs(c.sym)
    k = np.random.default_rng(3).integers(0, len(rr), chunk + 1)
    flip = np.random.default_rng(4).integers(0, 2, chunk + 1).astype(bool)
    rows, cols = np.where(flip, cc[k], rr[k]), np.where(flip, rr[k], cc[k])
    got, outside = c.plan.selinv_entries(rows, cols)
    want, _ = spr.entries(c.sym, c.S, rows, cols, lu=True)
    assert outside == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("symm", [False, True], ids=["own_u", "aliased"])
def test_lifecycle(symm):
    N = 8
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N) if symm else gen.unsymmetric_stencil(N, N, N, seed=4)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30, "lu", symm)
    plan = sf.LUPlan(sym, device=0)
    Ux = None if symm else sym.Ux
    plan.set_values(sym.Lx, Ux)
    plan.factorize()
    rng = np.random.default_rng(1)
    VL = rng.uniform(-1, 1, (len(sym.Li), 3))
    VU = None if symm else rng.uniform(-1, 1, (len(sym.Ui), 3))
    calls = (plan.selinv_values, lambda: plan.selinv_values(transposed=True), lambda: plan.selinv_trace(VL, VU),
             lambda: plan.selinv_entries([0], [0]))

    def all_refused():
        assert plan.stat("selinv_valid") == 0
        for call in calls:
            with pytest.raises(sf.SparseFrameError):
                call()

    all_refused()
    b = 1.0 + np.arange(n) / n
    F0, x0, x0b = plan.get_factor().copy(), plan.solve(b), plan.solve(b)
    plan.selinv()
    S0 = plan.get_selinv().copy()
    tr = plan.selinv_trace(VL, VU)
    got = plan.selinv_values()
    assert np.array_equal(got if symm else got[0], spr.lu_values(sym, S0, symm)[0])
    plan.selinv_entries([0, n - 1], [n - 1, 0])
    assert np.array_equal(plan.get_factor(), F0) and np.array_equal(plan.get_selinv(), S0)
    spread = max(float(np.max(np.abs(x0b - x0))), 8 * EPS * float(np.max(np.abs(x0))))
    assert float(np.max(np.abs(plan.solve(b) - x0))) <= spread
    plan.set_values(4.0 * sym.Lx, None if symm else 4.0 * Ux)
    all_refused()
    plan.factorize()
    all_refused()
    plan.selinv()
    assert np.max(np.abs(plan.selinv_trace(VL, VU) - tr / 4.0)) <= 1e-12 * np.max(np.abs(tr))
    plan.close()
