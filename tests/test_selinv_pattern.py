"""CholPlan.selinv_values / _values_device / selinv_trace / _trace_device / selinv_entries / logdet_grad (sf_chol_plan_selinv_values,
_trace, _entries) on the device.  The values are a gather, so they are compared with `==` against the host gather out
of get_selinv() (selinv_pattern_ref); the trace is tied to the values bit for bit through indicator arrays, is exact on matrices
whose arithmetic is, and for general V stays inside the worst-case bound of any summation order, T eps sum|terms|."""
import ctypes as C
import types

import numpy as np
import pytest

import selinv_pattern_ref as spr
from util import sf, gen
from test_selinv_abi import selinv_cases

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
CASES = selinv_cases()
IDS = [c[0] for c in CASES]


def _with_duplicates(Cp, Ci, Cx, rng, count):
    """(Cp, Ci, Cx) with `count` entries given twice, the extra copy FIRST in its column and with a wrong value"""
    picks = np.sort(rng.choice(len(Ci), count, replace=False))
    col = np.searchsorted(Cp, picks, side="right") - 1
    Ci2 = np.insert(Ci, picks, Ci[picks])
    Cx2 = np.insert(Cx, picks, Cx[picks] * 3.0 + 1.0)
    Cp2 = Cp + np.concatenate([[0], np.cumsum(np.bincount(col, minlength=len(Cp) - 1))])
    return np.ascontiguousarray(Cp2, dtype=np.int64), np.ascontiguousarray(Ci2, dtype=np.int64), Cx2


class Ctx:
    """a factorized plan with its selected inverse, the arena on the host and the reference values (made once, never changed)"""

    def __init__(self, sym, Lx=None):
        self.sym = sym
        self.plan = sf.CholPlan(sym, device=0)
        self.plan.set_values(sym.Lx if Lx is None else Lx)
        self.plan.factorize()
        self.plan.selinv()
        self.S = self.plan.get_selinv().copy()
        self.S.setflags(write=False)
        self.nnz = len(sym.Li)
        self.values = spr.chol_values(sym, self.S)
        self.chunk = int(self.plan.stat("selinv_pattern_chunk"))
        self.tile = int(self.plan.stat("selinv_pattern_tile"))


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(key):
        if key not in made:
            if key == "dup":
                N = 12
                n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
                sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
                keys = ("n", "nsuper", "Super", "SuperMap", "Lsip", "Lsi", "Lsxp", "xsize")
                dup = types.SimpleNamespace(**{k: getattr(sym, k) for k in keys})
                dup.Lp, dup.Li, dup.Lx = _with_duplicates(sym.Lp, sym.Li, sym.Lx, np.random.default_rng(7), 3000)
                made[key] = Ctx(dup)
            else:
                name, n, Cp, Ci, Cx, perm, slot = CASES[IDS.index(key)]
                made[key] = Ctx(sf.analyze(n, Cp, Ci, Cx, perm, slot))
        return made[key]

    yield get
    for c in made.values():
        c.plan.close()


def _diag_plan(d):
    """the plan of diag(d), factorized and inverted"""
    n = len(d)
    sym = sf.analyze(n, np.arange(n + 1), np.arange(n), np.asarray(d, dtype=np.float64), None, 1 << 30)
    return Ctx(sym)


def _bound_ok(got, terms):
    """|got - sum| <= T eps sum|terms| against the float64 numpy sum of the same products, T = the number of products"""
    ref = terms.sum(axis=0)
    bound = terms.shape[0] * EPS * np.abs(terms).sum(axis=0)
    print("trace: max |got - ref| / bound", float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300))))
    return bool(np.all(np.abs(got - ref) <= bound))


@pytest.mark.parametrize("name", IDS + ["dup"])
def test_values_are_the_host_gather(ctx, name):
    import torch
    c = ctx(name)
    got = c.plan.selinv_values()
    assert got.shape == (c.nnz,) and np.array_equal(got, c.values)
    out = torch.full((c.nnz,), 7.0, dtype=torch.float64, device="cuda:0")
    assert c.plan.selinv_values_device(out) is out
    assert np.array_equal(out.cpu().numpy(), c.values)
    assert c.plan.stat("bytes_selinv_pattern") > 0 and c.plan.stat("last_selinv_pattern_ms") >= 0


def _indicator_traces(c, positions):
    """selinv_trace of the indicator of every position, 64 at a time"""
    positions = np.asarray(positions)
    out = np.zeros(len(positions))
    for k0 in range(0, len(positions), 64):
        ps = positions[k0:k0 + 64]
        V = np.zeros((c.nnz, len(ps)), order="F")
        V[ps, np.arange(len(ps))] = 1.0
        out[k0:k0 + 64] = c.plan.selinv_trace(V)
    return out


def _boundary_positions(c):
    """the first and the last entry, one in a supernode's last column, and one either side of every 256-entry boundary (the
    lanes' stride, which the workgroups' tiles are multiples of)"""
    sym = c.sym
    edges = np.arange(256, c.nnz, 256)
    s = int(np.argmax(np.diff(sym.Super)))
    lastcol = int(sym.Super[s + 1] - 1)
    ps = np.concatenate([[0, c.nnz - 1, sym.Lp[lastcol], sym.Lp[lastcol + 1] - 1], edges - 1, edges])
    return np.unique(ps[(ps >= 0) & (ps < c.nnz)]).astype(np.int64)


@pytest.mark.parametrize("name", ["lap3d_16_nd", "dense_70", "one_by_one", "dup"])
def test_trace_of_an_indicator_is_the_value(ctx, name):
    c = ctx(name)
    assert c.tile % 256 == 0
    if name == "lap3d_16_nd":
        assert c.nnz > 3 * c.tile           # several workgroups
    ps = _boundary_positions(c)
    got = _indicator_traces(c, ps)
    j = np.repeat(np.arange(c.sym.n), np.diff(c.sym.Lp))
    live = spr.live_mask(c.sym.Lp, c.sym.Li)
    want = np.where(np.asarray(c.sym.Li)[ps] == j[ps], 1.0, 2.0) * c.values[ps]
    want = np.where(live[ps], want, 0.0)
    assert np.array_equal(got, want)
    if name == "dup":
        dead = np.nonzero(~live)[0]
        assert len(dead) == 3000
        pick = dead[[0, len(dead) // 2, -1]]
        assert np.array_equal(_indicator_traces(c, pick), np.zeros(3))      # superseded: exactly 0.0
        assert np.all(c.values[pick] != 0.0)                                # ... though the value is there


def test_exact_arithmetic():
    for d in (np.ones(3), np.ones(4099), 4.0 ** np.arange(-10, 11)):       # diag(2^k), k even: the square roots are exact too
        c = _diag_plan(d)
        n = len(d)
        d = np.asarray(c.sym.Lx)                        # (the diagonal in the plan's own ordering)
        assert len(d) == n
        assert np.array_equal(c.plan.selinv_values(), 1.0 / d)
        rng = np.random.default_rng(n)
        V = rng.integers(-8, 9, (n, 5)).astype(np.float64)
        want = (V / d[:, None]).sum(axis=0)             # integers over powers of two: every partial sum is exact
        got = c.plan.selinv_trace(V)
        assert np.array_equal(got, want)
        assert np.array_equal(c.plan.selinv_trace(V), got)
        assert c.plan.selinv_trace(V[:, 0]) == want[0]
        c.plan.close()


@pytest.mark.parametrize("name", IDS + ["dup"])
def test_general_V(ctx, name):
    import torch
    c = ctx(name)
    rng = np.random.default_rng(IDS.index(name) if name in IDS else 99)
    for m in (1, c.chunk - 1, c.chunk, c.chunk + 1, 64):
        big = np.asfortranarray(rng.uniform(-1, 1, (c.nnz + 5, m)))
        V = big[:c.nnz]                                 # column-major with ldv = nnz + 5
        terms = spr.chol_trace_terms(c.sym, c.S, V)
        got = c.plan.selinv_trace(V)
        assert got.shape == (m,) and _bound_ok(got, terms)
        gotc = c.plan.selinv_trace(np.ascontiguousarray(V))           # C order: the same numbers, the same bits
        assert np.array_equal(gotc, got)
        assert np.array_equal(c.plan.logdet_grad(V), got)
        dV = torch.from_numpy(big).to("cuda:0")[:c.nnz]                 # (the strides travel: column-major, ldv = nnz + 5)
        assert np.array_equal(c.plan.selinv_trace_device(dV).cpu().numpy(), got)
    one = c.plan.selinv_trace(V[:, 0])
    assert isinstance(one, float) and one == got[0]


def test_nan_stays_in_its_column(ctx):
    c = ctx("lap3d_8_nd")
    V = np.random.default_rng(5).uniform(-1, 1, (c.nnz, 2 * c.chunk + 3))
    clean = c.plan.selinv_trace(V)
    for t in (0, c.chunk, V.shape[1] - 1):
        W = V.copy()
        W[c.nnz // 2, t] = np.nan
        got = c.plan.selinv_trace(W)
        keep = np.arange(V.shape[1]) != t
        assert np.isnan(got[t]) and np.array_equal(got[keep], clean[keep])


def test_mapped(ctx):
    import torch
    c = ctx("lap3d_8_nd")
    with pytest.raises(ValueError):
        c.plan.selinv_trace(np.ones(c.nnz), mapped=True)
    A1 = np.ones(7)
    rc = sf.lib.sf_chol_plan_selinv_trace(c.plan._h, 1, A1.ctypes.data_as(C.POINTER(C.c_double)), 7, 1, A1.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 1 and np.all(A1 == 1.0)                # SF_ERR_ARG without a stored map
    rng = np.random.default_rng(11)
    nsrc = c.nnz + 17
    vmap = rng.integers(-1, nsrc, c.nnz)
    vmap[rng.choice(c.nnz, 40, replace=False)] = -1
    c.plan.set_value_map(nsrc, vmap)
    A = rng.uniform(-1, 1, (nsrc, c.chunk + 1))
    V = spr.mapped_columns(vmap, A)
    got = c.plan.selinv_trace(A, mapped=True)
    assert _bound_ok(got, spr.chol_trace_terms(c.sym, c.S, V))
    assert np.array_equal(got, c.plan.selinv_trace(V))          # the map changes where a term is read from, not the term
    dA = torch.from_numpy(np.asfortranarray(A)).to("cuda:0")
    assert np.array_equal(c.plan.selinv_trace_device(dA, mapped=True).cpu().numpy(), got)
    with pytest.raises(ValueError):
        c.plan.selinv_trace(V, mapped=True)             # nnz rows where nsrc are due


@pytest.mark.parametrize("name", ["lap2d_8x8_nd", "arrow_40_3"])
def test_entries_inside_and_outside(ctx, name):
    c = ctx(name)
    n = c.sym.n
    rr, cc = spr.pattern_pairs(c.sym)
    rows, cols = np.concatenate([rr, cc]), np.concatenate([cc, rr])         # either triangle
    got, outside = c.plan.selinv_entries(rows, cols)
    want, _ = spr.entries(c.sym, c.S, rows, cols)
    assert outside == 0 and np.array_equal(got, want)
    assert c.plan.stat("last_selinv_outside") == 0
    inpat = np.zeros((n, n), dtype=bool)
    inpat[rr, cc] = inpat[cc, rr] = True
    oi, oj = np.nonzero(~inpat)
    if len(oi):
        mix_r, mix_c = np.concatenate([oi, rr[:5]]), np.concatenate([oj, cc[:5]])
        got, outside = c.plan.selinv_entries(mix_r, mix_c)
        assert outside == len(oi) and np.all(np.isnan(got[:len(oi)])) and c.plan.stat("last_selinv_outside") == len(oi)
        assert np.array_equal(got[len(oi):], spr.entries(c.sym, c.S, rr[:5], cc[:5])[0])
    got, outside = c.plan.selinv_entries([], [])
    assert got.shape == (0,) and outside == 0
    got, outside = c.plan.selinv_entries([rr[-1]], [cc[-1]])
    assert outside == 0 and got[0] == spr.entries(c.sym, c.S, rr[-1:], cc[-1:])[0][0]
    # an index of n: SF_ERR_ARG with the output untouched
    out = np.full(3, 7.0)
    bad = np.array([0, n, 0], dtype=np.int64)
    ok = np.zeros(3, dtype=np.int64)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    for r, cl in ((bad, ok), (ok, bad)):
        assert sf.lib.sf_chol_plan_selinv_entries(c.plan._h, 3, lp(r), lp(cl), out.ctypes.data_as(C.POINTER(C.c_double)), None) == 1
    assert np.all(out == 7.0)


def test_entries_across_the_staging_chunk(ctx):
    c = ctx("lap3d_8_nd")
    chunk = int(c.plan.stat("selinv_entries_chunk"))
    rr, cc = spr.pattern_pairs(c.sym)
    k = np.random.default_rng(3).integers(0, len(rr), chunk + 1)
    rows, cols = rr[k].copy(), cc[k].copy()
    s0 = c.sym.SuperMap[0]
    absent = np.setdiff1d(np.arange(c.sym.Super[s0 + 1], c.sym.n), c.sym.Lsi[c.sym.Lsip[s0]:c.sym.Lsip[s0 + 1]])
    rows[-1], cols[-1] = absent[-1], 0                  # the pair behind the chunk boundary: a row column 0 does not have
    got, outside = c.plan.selinv_entries(rows, cols)
    want, want_out = spr.entries(c.sym, c.S, rows, cols)
    assert want_out == 1 and outside == 1
    assert np.array_equal(got[:-1], want[:-1]) and np.isnan(got[-1])


def test_lifecycle():
    N = 16
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    plan = sf.CholPlan(sym, device=0)
    plan.set_values(sym.Lx)
    plan.factorize()
    nnz = len(sym.Li)
    V = np.random.default_rng(1).uniform(-1, 1, (nnz, 3))
    calls = (plan.selinv_values, lambda: plan.selinv_trace(V), lambda: plan.selinv_entries([0], [0]), lambda: plan.logdet_grad(V[:, 0]))

    def all_refused():
        assert plan.stat("selinv_valid") == 0
        for call in calls:
            with pytest.raises(sf.SparseFrameError):
                call()

    all_refused()                                       # factorized, no arena yet
    b = 1.0 + np.arange(n) / n
    F0, x0, x0b = plan.get_factor().copy(), plan.solve(b), plan.solve(b)
    plan.selinv()
    S0 = plan.get_selinv().copy()
    vals = plan.selinv_values()
    tr = plan.selinv_trace(V)
    ent = plan.selinv_entries([0, n - 1], [0, n - 1])[0]
    assert np.array_equal(vals, spr.chol_values(sym, S0))
    # nothing else moved: the factor, the arena, and a solve within the run-to-run spread of the forward sweep's atomics
    assert np.array_equal(plan.get_factor(), F0) and np.array_equal(plan.get_selinv(), S0)
    spread = max(float(np.max(np.abs(x0b - x0))), 8 * EPS * float(np.max(np.abs(x0))))
    assert float(np.max(np.abs(plan.solve(b) - x0))) <= spread
    assert plan.stat("bytes_selinv_pattern") > 0
    plan.set_values(4.0 * sym.Lx)
    all_refused()                                       # a stale arena
    plan.factorize()
    all_refused()
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    assert np.max(np.abs(plan.selinv_values() - vals / 4.0)) <= 1e-14 * np.max(np.abs(vals))
    assert np.max(np.abs(plan.selinv_trace(V) - tr / 4.0)) <= 1e-12 * np.max(np.abs(tr))
    assert np.max(np.abs(plan.selinv_entries([0, n - 1], [0, n - 1])[0] - ent / 4.0)) <= 1e-14 * np.max(np.abs(ent))
    plan.close()
