"""adjoint_values / logdet_grad_values of CholPlan and LUPlan on the device (sf_*_plan_adjoint_values[_device],
sf_*_plan_logdet_grad_values[_device]) against tests/adjoint_ref.py.

Accuracy is a derived bound, nothing measured: out[p] is one accumulator over at most 2k fused multiply-adds and one multiplication
by alpha, so |out[p] - ref[p]| <= (2k + 2) 2^-53 |alpha| sum_c (|Y_ic X_jc| + |Y_jc X_ic|) against the longdouble reference; a
position the assembly ignores holds exactly 0.  Everything else is compared bit for bit: repeats, SF_DEV_PERM_IN against the call
on the permuted blocks, SF_ADJ_MAPPED against the scatter of the unmapped result through the map, host against device entry points.
logdet_grad_values is tied to selinv_trace: sum(out * dV) within the summation bound (nnz + 2) 2^-53 sum|out * dV|."""
import ctypes as C
import types

import numpy as np
import pytest

import adjoint_ref as ar
from util import sf, gen, small_cases, wide_cases
from test_lu_selinv_abi import lu_selinv_cases

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KS = (0, 1, 15, 16, 17, 33)
ALPHAS = (1.0, -1.0, 0.3)
LU_CASES = {c[0]: c for c in lu_selinv_cases()}
ALIASED, OWN_U = "sym_lap3d_7_via_lu", "st3d_8_nd"
CHOL = {c[0]: c for c in small_cases() + wide_cases()}


def _dense_column_arrow(n):
    """column 0 dense (n positions: longer than a workgroup of 256), every other column its diagonal only"""
    Cp = np.concatenate([[0], n + np.arange(n)]).astype(np.int64)
    Ci = np.concatenate([np.arange(n), np.arange(1, n)]).astype(np.int64)
    Cx = np.concatenate([[float(n)], np.full(n - 1, 0.5), np.full(n - 1, float(n))])
    return n, Cp, Ci, Cx


def _with_duplicates(ptr, idx, val, rng, count):
    """`count` entries given twice, the extra copy FIRST in its column (the assembly ignores it) and with a wrong value"""
    picks = np.sort(rng.choice(len(idx), count, replace=False))
    col = np.searchsorted(ptr, picks, side="right") - 1
    idx2 = np.insert(idx, picks, idx[picks])
    val2 = np.insert(val, picks, val[picks] * 3.0 + 1.0)
    ptr2 = ptr + np.concatenate([[0], np.cumsum(np.bincount(col, minlength=len(ptr) - 1))])
    return np.ascontiguousarray(ptr2, dtype=np.int64), np.ascontiguousarray(idx2, dtype=np.int64), val2


class Case:
    """a plan (no values yet) with its structure for the reference"""

    def __init__(self, key):
        rng = np.random.default_rng(5)
        dup = key.startswith("dup_")
        base = key[4:] if dup else key
        if base in ("chol", "arrow_col") or base in CHOL:
            if base == "arrow_col":
                n, Cp, Ci, Cx, perm, slot = _dense_column_arrow(600) + (None, 1 << 30)
            elif base == "chol":
                n, Cp, Ci, Cx = gen.laplacian_lower(8, 8, 8)
                perm, slot = sf.grid_nd_perm(8, 8, 8), 1 << 30
            else:
                _, n, Cp, Ci, Cx, perm, slot = CHOL[base]
            sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
            self.lu = self.own_u = False
        else:
            _, n, Cp, Ci, Cx, perm, slot, symm = LU_CASES[base]
            sym = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", symm)
            self.lu, self.own_u = True, not symm
        if dup:
            keys = ("n", "nsuper", "Super", "SuperMap", "Lsip", "Lsi", "Lsxp", "xsize") + (("lu", "symmetric") if self.lu else ())
            d = types.SimpleNamespace(**{k: getattr(sym, k) for k in keys})
            d.Lp, d.Li, d.Lx = _with_duplicates(sym.Lp, sym.Li, sym.Lx, rng, min(200, len(sym.Li) // 3))
            if self.own_u:
                d.Up, d.Ui, d.Ux = _with_duplicates(sym.Up, sym.Ui, sym.Ux, rng, min(200, len(sym.Ui) // 3))
            sym = d
        self.sym, self.n = sym, int(sym.n)
        self.plan = (sf.LUPlan if self.lu else sf.CholPlan)(sym, device=0)
        Lp, Li = np.asarray(sym.Lp), np.asarray(sym.Li)
        self.S = (self.n, Lp, Li) if not self.lu else (self.n, Lp, Li, None, None) if not self.own_u else \
            (self.n, Lp, Li, np.asarray(sym.Up), np.asarray(sym.Ui))
        self.nnz = len(Li)
        self.unz = len(sym.Ui) if self.own_u else 0
        self.marks = ar.marks(self.S)
        self.valued = False

    def blocks(self, rng, k, pad=3):
        """column-major (n, k) blocks with leading dimension n + pad"""
        mk = lambda: np.asfortranarray(rng.uniform(-1, 1, (self.n + pad, max(k, 1))))[:self.n, :k]
        return mk(), mk()

    def outs(self, r):
        return list(r) if isinstance(r, tuple) else [r]

    def factorize(self):
        if not self.valued:
            self.plan.set_values(self.sym.Lx, *((self.sym.Ux,) if self.own_u else ((None,) if self.lu else ())))
            self.plan.factorize()
            self.plan.selinv()
            self.valued = True


@pytest.fixture(scope="module")
def case():
    made = {}

    def get(key):
        if key not in made:
            made[key] = Case(key)
        return made[key]

    yield get
    for c in made.values():
        c.plan.close()


ALL = sorted(CHOL) + ["arrow_col", "dup_chol", ALIASED, OWN_U, "dup_" + ALIASED, "dup_" + OWN_U]
SOME = ["lap3d_8_nd", "one_by_one", "arrow_col", "dup_chol", ALIASED, "dup_" + ALIASED, "dup_" + OWN_U]


@pytest.mark.parametrize("key", ALL)
def test_values_within_the_derived_bound(case, key):
    """every k and alpha, leading dimensions > n, on a plan that has no values and no factor yet; repeats give the same bits"""
    c = case(key)
    rng = np.random.default_rng(1)
    Y, X = c.blocks(rng, max(KS))
    # the padded views go to the library as they are: the leading dimension it is given is n + 3
    assert sf.api._host_block(Y[:, :17], c.n, "Y")[1:] == (17, c.n + 3) and np.shares_memory(sf.api._host_block(Y[:, :17], c.n, "Y")[0], Y)
    Yl, Xl = Y.astype(ar.LD), X.astype(ar.LD)
    worst = 0.0
    for k in KS:
        ref, sums = ar.adjoint_values(c.S, Yl[:, :k], Xl[:, :k], 1.0)
        for alpha in ALPHAS:
            got = c.outs(c.plan.adjoint_values(Y[:, :k], X[:, :k], alpha=alpha))
            again = c.outs(c.plan.adjoint_values(Y[:, :k], X[:, :k], alpha=alpha))
            assert len(got) == len(ref) == (2 if c.own_u else 1)
            for g, g2, r, s, (_, _, a, b) in zip(got, again, ref, sums, c.marks):
                assert g.shape == r.shape and np.array_equal(g, g2)
                dead = ~(a | b)
                assert not np.any(g[dead]) and (k > 0 or not np.any(g))
                bound = (2 * k + 2) * U * abs(alpha) * s
                err = np.abs(g.astype(ar.LD) - ar.LD(alpha) * r)
                assert np.all(err <= bound), (k, alpha, float(np.max(err - bound)))
                if k:
                    worst = max(worst, float(np.max(err[~dead] / np.maximum(bound[~dead], 1e-300))))
    print(f"ADJOINT_BOUND {key}: worst error / bound {worst:.3f}")
    assert c.plan.stat("bytes_adjoint") > 0 and c.plan.stat("last_adjoint_ms") >= 0


@pytest.mark.parametrize("key", SOME)
def test_host_device_perm_and_mapped_agree_bit_for_bit(case, key):
    import torch
    c = case(key)
    rng = np.random.default_rng(2)
    for k in (1, 17):
        Y, X = c.blocks(rng, k)
        host = c.outs(c.plan.adjoint_values(Y, X, alpha=0.3))
        packed = c.outs(c.plan.adjoint_values(np.ascontiguousarray(Y), np.ascontiguousarray(X), alpha=0.3))    # (copied: ld == n)
        assert all(np.array_equal(a, b) for a, b in zip(packed, host))
        dev = lambda a, pad: _dev_padded(torch, a, pad)
        dY, dX = dev(Y, 5), dev(X, 2)                  # leading dimensions n + 5 and n + 2, NaN in the padding rows
        assert k == 1 or (dY.stride(), dX.stride()) == ((1, c.n + 5), (1, c.n + 2))
        got = c.outs(c.plan.adjoint_values_device(dY, dX, alpha=0.3))
        assert all(np.array_equal(g.cpu().numpy(), h) for g, h in zip(got, host))
        # SF_DEV_PERM_IN: the blocks in the caller's numbering
        perm = rng.permutation(c.n)
        c.plan.set_ordering(perm)
        Yc, Xc = np.empty_like(Y), np.empty_like(X)
        Yc[perm], Xc[perm] = Y, X                       # row perm[i] of the caller's block is row i of the permuted one
        got = c.outs(c.plan.adjoint_values_device(dev(Yc, 1), dev(Xc, 4), alpha=0.3, perm_in=True))
        assert all(np.array_equal(g.cpu().numpy(), h) for g, h in zip(got, host))
        # SF_ADJ_MAPPED: several positions name one source entry, some name none, some entries are named by nobody
        nsrc = max(c.nnz // 2, 1) + 5
        mapL = rng.integers(-1, nsrc - 3, c.nnz)
        mapU = rng.integers(-1, nsrc - 3, c.unz) if c.own_u else None
        c.plan.set_value_map(nsrc, mapL, mapU)
        want = np.zeros(nsrc)
        for m, h in zip((mapL, mapU), host):
            np.add.at(want, m[m >= 0], h[m >= 0])       # (unbuffered: in ascending position, L's before U's)
        got = c.plan.adjoint_values(Y, X, alpha=0.3, mapped=True)
        assert got.shape == (nsrc,) and np.array_equal(got, want) and not np.any(got[nsrc - 3:])
        out = torch.full((nsrc,), 7.0, dtype=torch.float64, device="cuda:0")
        c.plan.adjoint_values_device(dY, dX, out=out, alpha=0.3, mapped=True)
        assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("key", ["lap3d_8_nd", "dup_chol", "dup_" + OWN_U, ALIASED])
def test_a_nan_row_stays_in_its_positions(case, key):
    c = case(key)
    rng = np.random.default_rng(3)
    Y, X = c.blocks(rng, 5)
    clean = c.outs(c.plan.adjoint_values(Y, X))
    r = c.n // 2
    Xn = X.copy(order="F")
    Xn[r, 2] = np.nan
    got = c.outs(c.plan.adjoint_values(Y, Xn))
    hit_any = False
    for g, cl, (i, j, a, b) in zip(got, clean, c.marks):
        hit = (a & (j == r)) | (b & (i == r))           # Y[i] X[j] reads row j of X, Y[j] X[i] row i
        assert np.array_equal(np.isnan(g), hit) and np.array_equal(g[~hit], cl[~hit])
        hit_any = hit_any or bool(np.any(hit))
    assert hit_any


def _dev_padded(torch, a, pad):
    """the host block `a` as a device tensor with leading dimension rows + pad, the padding rows NaN"""
    if a.ndim == 1:
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n, k = a.shape
    buf = torch.full(((n + pad) * k,), float("nan"), dtype=torch.float64, device="cuda:0")
    T = buf.as_strided((n, k), (1, n + pad))
    T.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return T


def _trace(c, dV):
    return c.plan.selinv_trace(dV[0], *((dV[1],) if c.own_u else ()))


@pytest.mark.parametrize("key", ["lap3d_8_nd", "dup_chol", "arrow_col", "dense_70", ALIASED, OWN_U, "dup_" + ALIASED, "dup_" + OWN_U])
def test_logdet_grad_values_is_the_gradient_selinv_trace_implies(case, key):
    import torch
    c = case(key)
    fresh = (sf.LUPlan if c.lu else sf.CholPlan)(c.sym, device=0)
    try:
        fresh.set_values(c.sym.Lx, *((c.sym.Ux,) if c.own_u else ((None,) if c.lu else ())))
        fresh.factorize()
        with pytest.raises(sf.SparseFrameError):
            fresh.logdet_grad_values()                  # no selinv arena
    finally:
        fresh.close()
    c.factorize()
    rng = np.random.default_rng(4)
    counts = [c.nnz] + ([c.unz] if c.own_u else [])
    for alpha in ALPHAS:
        out = c.outs(c.plan.logdet_grad_values(alpha=alpha))
        assert all(np.array_equal(a, b) for a, b in zip(out, c.outs(c.plan.logdet_grad_values(alpha=alpha))))
        devs = c.outs(c.plan.logdet_grad_values_device(alpha=alpha))
        assert all(np.array_equal(d.cpu().numpy(), o) for d, o in zip(devs, out))
        dead = [~(a | b) for _, _, a, b in c.marks]
        assert all(not np.any(o[d]) for o, d in zip(out, dead))
        probes = [[rng.uniform(-1, 1, m) for m in counts]]
        for side, (i, j, a, b) in enumerate(c.marks):       # unit dV at a diagonal, an off-diagonal and an ignored position of every side
            live = a | b
            picks = [np.flatnonzero(live & (i == j))[:1], np.flatnonzero(live & (i != j))[:1], np.flatnonzero(~live)[:1],
                     np.flatnonzero(~live & (i == j))[:1]]
            for pick in picks:
                if len(pick):
                    unit = [np.zeros(m) for m in counts]
                    unit[side][pick[0]] = 1.0
                    probes.append(unit)
        assert len(probes) >= 1 + (3 if key.startswith("dup_") or c.own_u else 2)
        for dV in probes:
            terms = np.concatenate([o * v for o, v in zip(out, dV)])
            got, want = float(np.sum(terms.astype(ar.LD))), alpha * _trace(c, dV)
            bound = (sum(counts) + 2) * U * float(np.abs(terms).sum())
            print(f"LOGDET_GRAD {key} alpha={alpha}: |sum - trace| = {abs(got - want):.3e}, bound {bound:.3e}")
            assert abs(got - want) <= bound
    # mapped: the scatter of the unmapped result
    nsrc = c.nnz + 4
    mapL = rng.integers(-1, nsrc - 2, c.nnz)
    mapU = rng.integers(-1, nsrc - 2, c.unz) if c.own_u else None
    c.plan.set_value_map(nsrc, mapL, mapU)
    out = c.outs(c.plan.logdet_grad_values())
    want = np.zeros(nsrc)
    for m, h in zip((mapL, mapU), out):
        np.add.at(want, m[m >= 0], h[m >= 0])
    assert np.array_equal(c.plan.logdet_grad_values(mapped=True), want)
    dm = torch.full((nsrc,), 7.0, dtype=torch.float64, device="cuda:0")
    c.plan.logdet_grad_values_device(out=dm, mapped=True)
    assert np.array_equal(dm.cpu().numpy(), want)


def test_refusals_leave_the_outputs_untouched(case):
    """every SF_ERR_ARG of the device entry points, the outputs pre-filled with a sentinel"""
    import torch
    SENT = 7.0
    for key in ("lap2d_8x8_nd", OWN_U, ALIASED):
        c = Case(key)               # (a plan of its own: no ordering, no map)
        try:
            n, k = c.n, 3
            t = lambda *shape: torch.full(shape, SENT, dtype=torch.float64, device="cuda:0")
            ly, lx = n + 2, n + 1                           # leading dimensions > n: the blocks span (k - 1) ld + n doubles
            Y, X = t(k * ly), t(k * lx)
            outL, outU = t(c.nnz + k * n), t(max(c.unz, 1))
            pre = "sf_lu_plan_" if c.lu else "sf_chol_plan_"
            fn, fl = getattr(sf.lib, pre + "adjoint_values_device"), getattr(sf.lib, pre + "logdet_grad_values_device")

            def call(flags=0, kk=k, y=Y.data_ptr(), ldy=ly, x=X.data_ptr(), ldx=lx, oL=outL.data_ptr(), oU=outU.data_ptr()):
                tail = (oL, oU if c.own_u else None) if c.lu else (oL,)
                return fn(c.plan._h, flags, kk, y, ldy, x, ldx, 0.5, *tail)

            assert call() == 0
            outL.fill_(SENT), outU.fill_(SENT)
            bad = [dict(kk=-1), dict(y=None), dict(x=None), dict(oL=None), dict(ldy=n - 1), dict(ldx=n - 1), dict(flags=8), dict(flags=2),
                   dict(flags=1), dict(flags=4), dict(oL=Y.data_ptr()), dict(oL=X.data_ptr() + 8 * ((k - 1) * lx + n - 1)),
                   dict(y=outL.data_ptr() + 8 * (c.nnz - 1))]
            if c.own_u:
                bad += [dict(oU=None), dict(oU=outL.data_ptr())]
            for kw in bad:
                assert call(**kw) == 1, kw
            if c.lu and not c.own_u:
                assert fn(c.plan._h, 0, k, Y.data_ptr(), ly, X.data_ptr(), lx, 0.5, outL.data_ptr(), outU.data_ptr()) == 1
            host = np.full(c.nnz, SENT)
            hp = host.ctypes.data_as(C.POINTER(C.c_double))
            tail = (hp, None) if c.lu else (hp,)
            assert getattr(sf.lib, pre + "adjoint_values")(c.plan._h, k, None, n, None, n, 1.0, 0, *tail) == 1
            assert getattr(sf.lib, pre + "adjoint_values")(c.plan._h, 1, hp, n, hp, n, 1.0, 1, *tail) == 1     # PERM_IN is the device form's
            # logdet_grad_values: no arena, and the flag checks
            tail = (outL.data_ptr(), outU.data_ptr() if c.own_u else None) if c.lu else (outL.data_ptr(),)
            for flags in (0, 1, 4, 8):
                assert fl(c.plan._h, 1.0, flags, *tail) == 1
            assert bool(torch.all(outL == SENT)) and bool(torch.all(outU == SENT)) and np.all(host == SENT)
            assert bool(torch.all(Y == SENT)) and bool(torch.all(X == SENT))
        finally:
            c.plan.close()


def test_a_new_value_map_replaces_the_old_one(case):
    c = case("lap3d_8_nd")
    rng = np.random.default_rng(6)
    Y, X = c.blocks(rng, 2)
    host = c.plan.adjoint_values(Y, X)
    for nsrc in (c.nnz, 11):
        m = rng.integers(0, nsrc, c.nnz)
        c.plan.set_value_map(nsrc, m)
        want = np.zeros(nsrc)
        np.add.at(want, m, host)
        assert np.array_equal(c.plan.adjoint_values(Y, X, mapped=True), want)


def test_needs_no_factor_and_survives_a_failed_one():
    """the structure is all adjoint_values reads: the same bits before the first set_values and after a failed factorization"""
    c = Case("lap2d_8x8_nd")
    try:
        rng = np.random.default_rng(8)
        Y, X = c.blocks(rng, 4)
        before = c.plan.adjoint_values(Y, X, alpha=-1.0)
        ref, sums = ar.adjoint_values(c.S, Y, X, -1.0)
        assert np.all(np.abs(before.astype(ar.LD) - ref[0]) <= 10 * U * sums[0])
        c.plan.set_values(-np.asarray(c.sym.Lx))        # negative definite
        with pytest.raises(sf.SparseFrameError):
            c.plan.factorize()
        assert np.array_equal(c.plan.adjoint_values(Y, X, alpha=-1.0), before)
    finally:
        c.plan.close()
