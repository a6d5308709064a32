"""Single-launch tests of the selected inversion's kernels (csrc/sf_selinv.hip, sf_selinv_lu.hip, sf_selinv_common.h) through the
launchers the plans themselves call (sf_kernels.h: launch_selinv_*, launch_lu_selinv_*, launch_logdet, launch_lu_logdet).

One hand-built elimination tree (STRUCT): leaves whose rows below fall into up to four ancestors of widths 7, 70, 300 and 400, every
ancestor's row list a strict superset of the leaf's rows there, so no relative map is the identity and map_off - i is negative for
the first pair.  Sigma's entries are independent random values scaled per row and column over 1e-6 .. 1e6 (a wrong index cannot
cancel); everything a launch must not read holds NaN -- guard bands, every arena entry outside the gathered lower triangles, the
strict upper triangle of a Cholesky diagonal block, the diagonal and upper triangle of a PL diagonal block -- and everything outside
a launch's write footprint is compared bit for bit.  References and bounds: tests/kernel_ref.py.

Every numeric case is registered by name (CASES): the CPU tests run a float64 emulation of the launch through the case's checker,
and the emulation with one named fault (kernel_ref.SEL_FAULTS) must be rejected; the GPU tests launch on the same cases.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_ref as kr
import selinv_ref
from test_kernels import SEL_PAIR, SEL_UNIT, _ok, P, kp  # noqa: F401
from util import sf, small_cases

SMALL_W, SMALL_M, SMALL_Y, UW = 64, 512, 4096, 512          # sf_kernels.h: SEL_SMALL_*, SEL_UW
G = kr.GUARD


class KpSel(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("Super", "SuperMap", "Lsip", "Lsi", "Xp", "pairs", "relmap")] + \
               [(k, C.c_int64) for k in ("nsuper", "n", "nLsi", "npair", "nrel")]


@pytest.fixture(scope="module")
def ks(kp):
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    kp.kp_selinv_small.argtypes = [vp, vp, i64, vp, i32, vp]
    kp.kp_lu_selinv_small.argtypes = [vp, vp, vp, vp, i64, vp, i32, vp]
    kp.kp_selinv_trinv.argtypes = [vp, i64, vp, i32, i32, vp, i64]
    kp.kp_selinv_gemm.argtypes = [i32, i32, i32, i32, vp, i64, i64, i64, i64, i64, i64, i64, i32, i64, i32, vp, vp, vp, i64, vp]
    kp.kp_selinv_sum.argtypes = [vp, i64, i64, i32, i64, i64, i64, i32]
    kp.kp_selinv_finish.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, i64]
    kp.kp_selinv_diag.argtypes = [i64, vp, i64, vp, i32, vp, i64]
    kp.kp_logdet.argtypes = [i64, vp, i64, vp, i32, vp, i64, vp, i64]
    kp.kp_lu_selinv_pack.argtypes = [vp, vp, vp, vp, i64, vp, i64, i64, i64]
    return kp


def _report(name, worst):
    print(f"SELINV_RATIO {name}: worst err / bound = {worst:.3g}")
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# structures
# ---------------------------------------------------------------------------------------------------------------------
class Structure(kr.SelTables):
    """SelTables over panels laid out back to back behind a guard band, with the arrays in the device's types"""

    def __init__(self, Super, rowlists, pad=0):
        Lsip = np.concatenate([[0], np.cumsum([len(r) for r in rowlists])]).astype(np.int64)
        Lsi = np.concatenate(rowlists).astype(np.int32)
        ncol = np.diff(Super)
        Xp = (G + np.concatenate([[0], np.cumsum(ncol * np.diff(Lsip))])).astype(np.int64)
        super().__init__(np.asarray(Super, dtype=np.int32), Lsip, Lsi, Xp, pad)
        self.narena = int(Xp[-1]) + G
        self.pairs_dev = np.zeros(max(1, len(self.pairs)), dtype=SEL_PAIR)
        for k, (off, i) in enumerate(self.pairs):
            self.pairs_dev[k] = (off, i, 0)
        self.relmap_dev = self.relmap.astype(np.int32)
        self.keep = (self.Super, self.SuperMap, self.Lsip, self.Lsi, self.Xp, self.pairs_dev, self.relmap_dev)
        self.c = KpSel(*[a.ctypes.data for a in self.keep], self.nsuper, self.n, len(Lsi), len(self.pairs_dev), len(self.relmap_dev))

    def unit(self, J, cb=0, w=None):
        u = np.zeros(1, dtype=SEL_UNIT)
        u[0] = (self.Xp[J], self.Lsip[J], self.nsrow(J), self.ncol(J), cb, self.ncol(J) - cb if w is None else w, self.pair0[J],
                self.pair0[J + 1] - self.pair0[J])
        return u

    def panel(self, a, J):
        """view of panel J of arena image a: rows x columns"""
        return a[self.Xp[J]:self.Xp[J] + self.ncol(J) * self.nsrow(J)].reshape(self.ncol(J), self.nsrow(J)).T


# leaves (ncol, rows below) by name, then the ancestors (g_130 first: its first pair has map_off = 0, so map_off - i < 0).  s_*: the (w, m) pairs of the narrow kernels; g_*: units of the gathered GEMM
LEAVES = {"g_130": (12, 125), "s_1_0": (1, 0), "s_64_0": (64, 0), "s_1_512": (1, 512), "s_8_512": (8, 512), "s_16_256": (16, 256), "s_17_240": (17, 240),
          "s_64_64": (64, 64), "s_15_1": (15, 1), "g_65": (4, 65), "g_17": (6, 13), "g_1": (3, 1), "f_in": (40, 0),
          "f_mixed": (20, 9)}
ANCESTORS = (7, 70, 300, 400)


def _struct():
    rng = np.random.default_rng(2024)
    names = list(LEAVES)
    ncols = [LEAVES[k][0] for k in names] + list(ANCESTORS)
    Super = np.concatenate([[0], np.cumsum(ncols)])
    first = Super[len(names):]                      # first column of each ancestor
    acols = [np.arange(first[k], first[k + 1]) for k in range(len(ANCESTORS))]
    rowlists = []
    for k, name in enumerate(names):
        below = LEAVES[name][1]
        forced = [int(rng.choice(c[1:-1])) for c in acols[:3]][:below] if below >= 3 else ([int(acols[1][5])] if below else [])
        rest = np.setdiff1d(np.arange(first[0], Super[-1]), forced)
        rows = np.sort(np.concatenate([forced, rng.choice(rest, below - len(forced), replace=False)])).astype(np.int64)
        rowlists.append(np.concatenate([np.arange(Super[k], Super[k + 1]), rows]))
    for k in range(len(ANCESTORS)):
        rowlists.append(np.arange(first[k], Super[-1]))
    st = Structure(Super, rowlists)
    st.names = {name: k for k, name in enumerate(names)}
    st.scale = kr.scalings(np.random.default_rng(7), st.n)
    return st


STRUCT = _struct()


def test_structure_is_what_the_tests_claim():
    st = STRUCT
    J = st.names["g_130"]
    prs = st.pairs[st.pair0[J]:st.pair0[J + 1]]
    assert len(prs) >= 3 and len({st.ncol(st.SuperMap[st.rows(J)[i]]) for _, i in prs}) >= 3
    assert prs[0][0] - prs[0][1] < 0                            # map_off - i of the first pair
    for off, i in prs:
        a = st.SuperMap[st.rows(J)[i]]
        rm = st.relmap[off:off + st.nsrow(J) - i]
        assert np.array_equal(st.rows(a)[rm], st.rows(J)[i:]) and not np.array_equal(rm, np.arange(len(rm)))
    for name, (w, m) in LEAVES.items():
        if name.startswith("s_"):
            assert w <= SMALL_W and m <= SMALL_M and w * m <= SMALL_Y


@pytest.mark.parametrize("case", [c for c in small_cases() if c[0] in ("lap2d_8x8_nd", "lap3d_8_nd")], ids=lambda c: c[0])
def test_tables_agree_with_the_analysis(case):
    """units as selinv_ref.units lists them; the pair table and the relative maps place every gathered entry where the factor's
    layout holds it: with the arena filled from a symmetric matrix of distinct values, Sigma(R,R) comes back exactly"""
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    Super, Lsip, Lsi, Lsxp = (np.asarray(getattr(sym, k)) for k in ("Super", "Lsip", "Lsi", "Lsxp"))
    tb = kr.SelTables(Super, Lsip, Lsi, Lsxp)
    assert np.array_equal(tb.SuperMap, np.asarray(sym.SuperMap))
    mine = []
    lev = selinv_ref._levels(Super, tb.SuperMap, Lsip, Lsi, tb.nsuper)
    for lv in range(int(lev.max()), -1, -1):
        for s in np.nonzero(lev == lv)[0]:
            w, m = tb.ncol(s), tb.nsrow(s) - tb.ncol(s)
            if w <= SMALL_W and m <= SMALL_M and w * m <= SMALL_Y:
                mine.append((int(s), 0, w))
            else:
                mine += [(int(s), cb, min(UW, w - cb)) for cb in range((w - 1) // UW * UW, -1, -UW)]
    assert mine == selinv_ref.units(sym)
    # k_build_relmaps as selinv_ref.py states it: positions inside a's columns, then searchsorted in a's rows below
    for s in range(tb.nsuper):
        for off, i in tb.pairs[tb.pair0[s]:tb.pair0[s + 1]]:
            g = tb.rows(s)[i:]
            a = tb.SuperMap[g[0]]
            inside = g < Super[a + 1]
            want = np.where(inside, g - Super[a], tb.ncol(a) + np.searchsorted(tb.rows(a)[tb.ncol(a):], g))
            assert np.array_equal(tb.relmap[off:off + len(g)], want)
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    M = (np.maximum(ii, jj) * n + np.minimum(ii, jj)).astype(np.float64)
    S = np.full(int(sym.xsize), np.nan)
    for s in range(tb.nsuper):
        pan = S[Lsxp[s]:Lsxp[s] + tb.ncol(s) * tb.nsrow(s)].reshape(tb.ncol(s), tb.nsrow(s)).T
        pan[:] = M[np.ix_(tb.rows(s), np.arange(Super[s], Super[s + 1]))]
        pan[:tb.ncol(s)][np.triu(np.ones((tb.ncol(s),) * 2, dtype=bool), 1)] = np.nan
    for J, cb, w in mine:
        r = tb.rows(J)[cb + w:]
        got, _ = tb.gather(J, cb + w, S, S)
        assert np.array_equal(got, M[np.ix_(r, r)]), (J, cb, w)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
def _sigma_values(rng, st, idx, rows):
    """independent random values scaled per row and column, for the arena positions idx (m x m, symmetric) of the rows `rows`"""
    sc = st.scale[rows]
    return sc[:, None] * sc[None, :] * rng.uniform(-1, 1, idx.shape)


class GatherMixin:
    def fill_sigma(self, rng, J, ce, lu):
        """arenas (SL, SU) -- Cholesky: SU is SL -- NaN but for the lower-triangle positions Sigma(R,R) of the unit is read from"""
        st = STRUCT
        idx = st.gather_index(J, ce)
        rows = st.rows(J)[ce:]
        low = np.tril(np.ones(idx.shape, dtype=bool))
        SL = np.full(st.narena, np.nan)
        SL[idx[low]] = _sigma_values(rng, st, idx, rows)[low]
        SU = SL
        if lu:
            SU = np.full(st.narena, np.nan)
            SU[idx[low]] = _sigma_values(rng, st, idx, rows)[low]
            d = idx[np.diag_indices(len(rows))]
            SU[d] = SL[d]                   # a diagonal entry of Sigma is the same number in both sets
        return SL, SU


class GemmCase(GatherMixin):
    """one k_selinv_gemm launch.  am 0 / 1: op(A) from a NaN-padded scratch image; am 2 (kind chol / lu / lut): op(A) = Sigma(R,R) of
    unit (leaf, cb, w) gathered from (S, S2) = (S, S) / (SL, SU) / (SU, SL).  Slab z of C at c_off + z cstride, NaN between slabs."""

    def __init__(self, seed, am, M, N, K, slabs, acc_in, kind=None, unit=None):
        rng = np.random.default_rng(seed)
        self.am, self.M, self.N, self.K, self.slabs, self.acc_in, self.kind = am, M, N, K, slabs, acc_in, kind
        st = STRUCT
        self.u = st.unit(0, 0, 1)
        self.S = self.S2 = None
        if am == 2:
            J, cb, w = st.names[unit[0]], unit[1], unit[2]
            self.u, self.J, self.ce = st.unit(J, cb, w), J, cb + w
            assert st.nsrow(J) - self.ce == M == K
            SL, SU = self.fill_sigma(rng, J, self.ce, kind != "chol")
            self.S, self.S2 = (SU, SL) if kind == "lut" else (SL, SU)
            self.opA = self.operand()
            rs = st.scale[st.rows(J)[self.ce:]]
        else:
            rs = kr.scalings(rng, K)
            self.opA = kr.scalings(rng, M)[:, None] * rng.uniform(-1, 1, (M, K)) / rs[None, :]
        self.B = rs[:, None] * rng.uniform(-1, 1, (K, N)) * kr.scalings(rng, N, 1e-3, 1e3)[None, :]
        if am == 2:
            self.B = self.B / rs[:, None] ** 2          # Sigma(R,R) carries both scalings: keep the terms of a sum comparable
        self.C0 = np.abs(self.opA) @ np.abs(self.B) * rng.uniform(-1, 1, (slabs, M, N)) if acc_in else np.full((slabs, M, N), np.nan)
        ar = kr.Arena()
        self.lda, self.ldb, self.ldc = (K if am == 1 else M) + 3, K + 2, M + 5
        self.a_off = ar.alloc(self.lda * (M if am == 1 else K)) if am != 2 else -1
        self.b_off = ar.alloc(self.ldb * N)
        self.cstride = self.ldc * N + 37
        self.c_off = ar.alloc(self.cstride * slabs)
        self.buf = ar.image()
        if am != 2:
            A = self.buf[self.a_off:self.a_off + self.lda * (M if am == 1 else K)].reshape(-1, self.lda)
            A[:, :(K if am == 1 else M)] = self.opA if am == 1 else self.opA.T
        self.buf[self.b_off:self.b_off + self.ldb * N].reshape(N, self.ldb)[:, :K] = self.B.T
        self.cview(self.buf)[:] = self.C0

    def operand(self, fault=None):
        Gm, _ = STRUCT.gather(self.J, self.ce, self.S, self.S2, fault)
        return Gm

    def cview(self, buf):
        """slabs x M x N view of C in an image"""
        v = np.lib.stride_tricks.as_strided(buf[self.c_off:], (self.slabs, self.M, self.N), (buf.itemsize * self.cstride, buf.itemsize, buf.itemsize * self.ldc))
        return v

    def emulate(self, fault=None):
        out = self.buf.copy()
        opA = self.operand(fault) if self.am == 2 and fault in ("swap arenas", "wrong pair") else self.opA
        self.cview(out)[:] = kr.selgemm_emulate(opA, self.B, self.C0, self.slabs, self.acc_in, fault)
        return out

    def launch(self, ks):
        out = self.buf.copy()
        _ok(ks.kp_selinv_gemm(self.am, self.M, self.N, self.K, P(out), len(out), self.a_off, self.lda, self.b_off, self.ldb, self.c_off,
                              self.ldc, self.slabs, self.cstride, self.acc_in, P(self.u), P(self.S), P(self.S2),
                              STRUCT.narena, C.addressof(STRUCT.c) if self.am == 2 else None))
        return out

    def check(self, out, what):
        written = np.zeros(len(out), dtype=bool)
        self.cview(written)[:] = True
        kr.assert_unchanged(self.buf, out, written, what)
        return kr.selgemm_check(np.array(self.cview(out)), self.opA, self.B, self.C0, self.slabs, self.acc_in, what)


def _diag_dominant(rng, w):
    T = rng.uniform(-1, 1, (w, w)) / max(w, 1)
    T[np.diag_indices(w)] = rng.uniform(1, 2, w) * rng.choice([-1.0, 1.0], w)
    return T


class TrinvCase:
    """one k_selinv_trinv (variant chol) or k_lu_selinv_trinv (lu0: stored diagonal, lu1: unit) launch on a panel of its own: the
    block at (cb, cb) of an nsrow x (cb + w) panel; only the triangle the launch reads is finite"""

    def __init__(self, seed, variant, w, cb, extra):
        rng = np.random.default_rng(seed)
        self.variant, self.w, self.unitd = variant, w, int(variant == "lu1")
        ns = cb + w + extra
        ar = kr.Arena()
        lx = ar.alloc(ns * (cb + w))
        self.P = ar.image()
        sc = kr.scalings(rng, w, 1e-3, 1e3)
        T = _diag_dominant(rng, w) * sc[:, None] / sc[None, :]
        keep = np.tril(np.ones((w, w), dtype=bool), -self.unitd)
        self.T = np.where(keep, T, np.nan)
        self.P[lx:lx + ns * (cb + w)].reshape(cb + w, ns)[cb:, cb:cb + w] = self.T.T
        self.u = np.zeros(1, dtype=SEL_UNIT)
        self.u[0] = (lx, 0, ns, cb + w, cb, w, 0, 0)
        self.out0 = np.full(w * w + 64, np.nan)

    def emulate(self, fault=None):
        out = self.out0.copy()
        out[:self.w ** 2] = kr.trinv_emulate(self.T, self.unitd, fault).T.ravel()
        return out

    def launch(self, ks):
        out = self.out0.copy()
        _ok(ks.kp_selinv_trinv(P(self.P), len(self.P), P(self.u), int(self.variant != "chol"), self.unitd, P(out), len(out)))
        return out

    def check(self, out, what):
        written = np.arange(len(out)) < self.w ** 2
        kr.assert_unchanged(self.out0, out, written, what)
        return kr.trinv_check(self.T, out[:self.w ** 2].reshape(self.w, self.w).T, self.unitd, what)


class SmallCase(GatherMixin):
    """one k_selinv_small / k_lu_selinv_small launch on the named leaves of STRUCT (each a whole unit)"""

    def __init__(self, seed, lu, leaves):
        rng = np.random.default_rng(seed)
        st = STRUCT
        self.lu, self.Js = lu, [st.names[k] for k in leaves]
        self.units = np.concatenate([st.unit(J) for J in self.Js])
        self.PL, self.PU = np.full(st.narena, np.nan), np.full(st.narena, np.nan)
        self.SL, self.SU = np.full(st.narena, np.nan), np.full(st.narena, np.nan)
        self.G = {}
        for J in self.Js:
            w, ns = st.ncol(J), st.nsrow(J)
            SL, SU = self.fill_sigma(rng, J, w, lu)
            for dst, src in ((self.SL, SL), (self.SU, SU)):
                dst[~np.isnan(src)] = src[~np.isnan(src)]
            rs = st.scale[st.rows(J)[w:]]
            for Pn, unitd in ((self.PL, lu), (self.PU, 0)):
                pan = st.panel(Pn, J)
                pan[:w] = np.where(np.tril(np.ones((w, w), dtype=bool), -unitd), _diag_dominant(rng, w), np.nan)
                pan[w:] = rng.uniform(-1, 1, (ns - w, w)) / rs[:, None]
        if not lu:
            self.PU, self.SU = self.PL, self.SL
        for J in self.Js:
            self.G[J] = st.gather(J, st.ncol(J), self.SL, self.SU)[0]

    def parts(self, J):
        st, w = STRUCT, STRUCT.ncol(J)
        pl, pu = st.panel(self.PL, J), st.panel(self.PU, J)
        return pl[:w], int(self.lu), pl[w:], pu[:w], 0, pu[w:]

    def emulate(self, fault=None):
        st = STRUCT
        SL, SU = self.SL.copy(), self.SU.copy()
        for J in self.Js:
            w = st.ncol(J)
            Gm = st.gather(J, w, self.SL, self.SU, fault)[0] if fault in ("swap arenas", "wrong pair") else self.G[J]
            Zl, Zu, Scc = kr.small_emulate(*self.parts(J), Gm, fault)
            if not self.lu:
                Scc = np.tril(Scc) + np.tril(Scc, -1).T
            st.panel(SL, J)[w:], st.panel(SL, J)[:w] = -Zl, Scc
            if self.lu:
                st.panel(SU, J)[w:], st.panel(SU, J)[:w] = -Zu, Scc.T
        return SL, (SU if self.lu else SL)

    def launch(self, ks):
        SL, SU = self.SL.copy(), self.SU.copy()
        if self.lu:
            _ok(ks.kp_lu_selinv_small(P(self.PL), P(self.PU), P(SL), P(SU), STRUCT.narena, P(self.units), len(self.units), C.addressof(STRUCT.c)))
        else:
            _ok(ks.kp_selinv_small(P(self.PL), P(SL), STRUCT.narena, P(self.units), len(self.units), C.addressof(STRUCT.c)))
        return SL, (SU if self.lu else SL)

    def refs(self, J):
        if not hasattr(self, "_refs"):
            self._refs = {}
        if J not in self._refs:
            self._refs[J] = kr.small_ref(*self.parts(J), self.G[J])
        return self._refs[J]

    def check(self, out, what):
        st = STRUCT
        SL, SU = out
        written = np.zeros(st.narena, dtype=bool)
        for J in self.Js:
            written[st.Xp[J]:st.Xp[J + 1]] = True
        kr.assert_unchanged(self.SL, SL, written, what + " SL")
        kr.assert_unchanged(self.SU, SU, written, what + " SU")
        worst = 0.0
        for J in self.Js:
            w = st.ncol(J)
            Zl, dZl, Zu, dZu, Scc, dScc = self.refs(J)
            tag = f"{what} unit (w={w}, m={st.nsrow(J) - w})"
            worst = max(worst, kr.within_ratio(st.panel(SL, J)[w:], -Zl, dZl, tag + " Sigma(R,C)"),
                        kr.within_ratio(st.panel(SL, J)[:w], Scc, dScc, tag + " Sigma(C,C)"))
            if self.lu:
                worst = max(worst, kr.within_ratio(st.panel(SU, J)[w:], -Zu, dZu, tag + " Sigma(C,R)^T"),
                            kr.within_ratio(st.panel(SU, J)[:w], Scc.T, dScc.T, tag + " Sigma(C,C)^T"))
            else:
                assert np.array_equal(kr.bits(st.panel(SL, J)[:w]), kr.bits(st.panel(SL, J)[:w].T)), tag + ": the mirror differs"
        return worst


class FinishCase:
    """one k_selinv_finish / k_lu_selinv_finish launch: pure moves.  Z, Sc: random; Cholesky: the strict upper triangle of Sc NaN.
    The arenas hold distinct finite sentinels everywhere but in the guard bands."""

    def __init__(self, seed, lu, leaf, cb, w):
        rng = np.random.default_rng(seed)
        st = STRUCT
        self.lu, self.J, self.cb, self.w = lu, st.names[leaf], cb, w
        self.u = st.unit(self.J, cb, w)
        self.m = st.nsrow(self.J) - cb - w
        self.Z, self.Zu = (rng.uniform(-1, 1, (w, self.m)) for _ in range(2))             # [column][row]: leading dimension m
        self.Sc = rng.uniform(-1, 1, (w, w))
        if not lu:
            self.Sc[np.tril(np.ones((w, w), dtype=bool), -1)] = np.nan                      # [j][i] with i < j: the strict upper triangle
        self.S0 = [np.full(st.narena, np.nan) for _ in range(2)]
        for a in self.S0:
            a[G:-G] = rng.uniform(1, 2, st.narena - 2 * G)

    def emulate(self, fault=None):
        st = STRUCT
        SL, SU = self.S0[0].copy(), self.S0[1].copy()
        cb, w, m, nc = self.cb, self.w, self.m, st.ncol(self.J)
        ce = cb + w
        inside = max(0, nc - ce)
        pl, pu = st.panel(SL, self.J), st.panel(SU, self.J)
        mir = inside + 1 if fault == "mirror outside J" and m > inside else inside
        if self.lu:
            pl[ce:, cb:ce], pu[ce:, cb:ce] = -self.Z.T, -self.Zu.T
            pl[cb:ce, cb:ce], pu[cb:ce, cb:ce] = self.Sc.T, self.Sc
            zl, zu = -self.Z.T[:mir].T, -self.Zu.T[:mir].T
        else:
            pl[ce:, cb:ce] = -self.Z.T
            low = np.tril(self.Sc.T)
            pl[cb:ce, cb:ce] = low + np.tril(low, -1).T
            zl = zu = -self.Z.T[:mir].T
        # the mirrors of the R rows inside J ("mirror outside J": one row more, past the panel's columns), by flat index
        for x in range(mir):
            at = st.Xp[self.J] + (ce + x) * st.nsrow(self.J) + cb + np.arange(w)
            (SU if self.lu else SL)[at] = zl[:, x]
            if self.lu:
                SL[at] = zu[:, x]
        return SL, SU

    def launch(self, ks):
        SL, SU = self.S0[0].copy(), self.S0[1].copy()
        Z, Zu = (v.ravel() if v.size else np.full(1, np.nan) for v in (self.Z, self.Zu))         # m = 0: nothing of Z is read
        _ok(ks.kp_selinv_finish(P(self.u), P(Z), P(Zu) if self.lu else None, len(Z), P(self.Sc), self.Sc.size, P(SL),
                                P(SU) if self.lu else None, STRUCT.narena))
        return SL, SU

    def check(self, out, what):
        want = self.emulate()
        for k in range(2 if self.lu else 1):
            diff = kr.bits(out[k]) != kr.bits(want[k])
            written = kr.bits(want[k]) != kr.bits(self.S0[k])
            kr.assert_unchanged(self.S0[k], out[k], written, what)
            if not np.all(np.isfinite(out[k][written])):
                raise AssertionError(f"{what}: non-finite stored results")
            assert not diff.any(), f"{what}: {int(diff.sum())} moved entries differ, first at {np.flatnonzero(diff)[:4].tolist()}"
        return 0.0


GEMM_DIMS = [1, 15, 16, 17, 63, 64, 65, 129]


def _registry():
    reg = {}
    rng = np.random.default_rng(99)
    seed = 1000
    for am in (0, 1):
        # every value on every axis at least once; the slab counts cycle with period 4 and acc_in with period 8, so each slab
        # count is seen with both acc_in values (am = 1, one slab, acc_in = 0 is run_big's Sc = X^T X)
        for k, d in enumerate(GEMM_DIMS):
            for ax in range(3):
                dims = [int(rng.choice(GEMM_DIMS)) for _ in range(3)]
                dims[ax] = d
                M, N, K = dims
                t = 3 * k + ax
                slabs, acc = (1, 2, 3, 16)[t % 4], (t // 4 + am) % 2
                seed += 1
                reg[f"gemm am={am} M={M} N={N} K={K} slabs={slabs} acc={acc} #{seed}"] = (GemmCase, (seed, am, M, N, K, slabs, acc))
        for acc in (0, 1):
            reg[f"gemm am={am} K=40 slabs=16 acc={acc}"] = (GemmCase, (2000 + am + 2 * acc, am, 65, 17, 40, 16, acc))
            reg[f"gemm am={am} K=200 slabs=3 acc={acc}"] = (GemmCase, (2010 + am + 2 * acc, am, 17, 65, 200, 3, acc))
    units = {1: ("g_1", 0, 3), 17: ("g_17", 0, 2), 65: ("g_65", 1, 3), 130: ("g_130", 2, 5)}    # g_17, g_130: cb + w < ncol
    for kind in ("chol", "lu", "lut"):
        for k, (m, unit) in enumerate(units.items()):
            for slabs in (1, 2):
                N = (1, 16, 65)[(k + slabs) % 3]
                reg[f"gemm am=2 {kind} R={m} N={N} slabs={slabs}"] = (GemmCase, (3000 + 10 * k + slabs, 2, m, N, m, slabs, 0, kind, unit))
    for variant in ("chol", "lu0", "lu1"):
        for k, w in enumerate((1, 2, 63, 64, 65)):
            for cb, extra in ((0, 0), (5, 9)):
                reg[f"trinv {variant} w={w} cb={cb}"] = (TrinvCase, (4000 + k, variant, w, cb, extra))
        reg[f"trinv {variant} w=511 cb=0"] = (TrinvCase, (4100, variant, 511, 0, 0))         # the two large sizes once per variant
        reg[f"trinv {variant} w=512 cb=3"] = (TrinvCase, (4101, variant, 512, 3, 2))         # (512 = SEL_UW: every lane has a row)
    small = ["s_1_0", "s_64_0", "s_1_512", "s_8_512", "s_16_256", "s_17_240", "s_64_64", "s_15_1"]
    for lu in (0, 1):
        reg[f"small lu={lu} all"] = (SmallCase, (5000 + lu, lu, small))
        reg[f"small lu={lu} one"] = (SmallCase, (5010 + lu, lu, ["s_17_240"]))
        # m = 0; R wholly inside J; R wholly below; mixed -- m w + w w on both sides of 256 and 512
        for k, (leaf, cb, w) in enumerate((("s_64_0", 48, 16), ("f_in", 0, 6), ("f_in", 30, 10), ("f_in", 0, 11), ("f_mixed", 20 - 15, 15),
                                           ("f_mixed", 2, 7), ("g_65", 0, 4), ("g_1", 0, 3), ("s_15_1", 0, 15), ("s_17_240", 0, 17))):
            reg[f"finish lu={lu} {leaf} cb={cb} w={w}"] = (FinishCase, (6000 + k, lu, leaf, cb, w))
    return reg


CASES = _registry()
_built = {}


def _case(name):
    """cases are built once and shared (their references too); nothing mutates them"""
    if name not in _built:
        cls, args = CASES[name]
        _built[name] = cls(*args)
    return _built[name]


def _names(prefix):
    return [k for k in CASES if k.startswith(prefix)]


def test_finish_cases_straddle_the_block_sizes():
    tot = sorted({_case(k).m * _case(k).w + _case(k).w ** 2 for k in _names("finish lu=0")})
    assert tot[0] < 256 and any(256 < t < 512 for t in tot) and tot[-1] > 512 and any(_case(k).m == 0 for k in _names("finish lu=0"))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the checkers against the float64 emulations and their single faults
# ---------------------------------------------------------------------------------------------------------------------
needs_ld = pytest.mark.skipif(not kr.have_longdouble(), reason="np.longdouble has no 64-bit mantissa on this platform")


@needs_ld
@pytest.mark.parametrize("name", list(CASES))
def test_checker_accepts_the_emulation(name):
    case = _case(name)
    assert case.check(case.emulate(), f"emulation, {name}") <= 1.0


# each fault on the smallest registered case where it changes anything
REJECTS = [("gemm am=2 lu R=17 N=1 slabs=2", "swap arenas"), ("gemm am=2 lut R=17 N=1 slabs=2", "swap arenas"),
           ("gemm am=2 chol R=17 N=1 slabs=2", "wrong pair"), ("gemm am=2 lu R=65 N=16 slabs=2", "wrong pair"),
           ("gemm am=0 K=40 slabs=16 acc=0", "dropped chunk"), ("gemm am=1 K=200 slabs=3 acc=1", "dropped chunk"),
           ("gemm am=2 chol R=17 N=1 slabs=2", "dropped chunk"),
           ("gemm am=0 K=40 slabs=16 acc=0", "slab overlap"), ("gemm am=2 lu R=65 N=16 slabs=2", "slab overlap"),
           ("trinv lu1 w=2 cb=0", "stored diagonal"), ("small lu=1 one", "stored diagonal"),
           ("small lu=1 one", "swap arenas"), ("small lu=0 one", "wrong pair"), ("small lu=1 all", "wrong pair"),
           ("finish lu=0 f_mixed cb=2 w=7", "mirror outside J"), ("finish lu=1 f_mixed cb=5 w=15", "mirror outside J")]


@needs_ld
@pytest.mark.parametrize("name,fault", REJECTS)
def test_checker_rejects_single_faults(name, fault):
    assert fault in kr.SEL_FAULTS
    case = _case(name)
    with pytest.raises(AssertionError, match="beyond the bound|outside the write footprint|non-finite"):
        case.check(case.emulate(fault), f"{fault}, {name}")


def test_every_fault_is_rejected_somewhere():
    assert {f for _, f in REJECTS} == set(kr.SEL_FAULTS)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: one launch per case
# ---------------------------------------------------------------------------------------------------------------------
def _run(ks, names, label):
    worst = 0.0
    for name in names:
        case = _case(name)
        worst = max(worst, case.check(case.launch(ks), name))
    return _report(label, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("am", [0, 1])
def test_selinv_gemm_shapes(ks, am):
    """plain and transposed operand: edge sizes on every axis, acc_in, 1 / 2 / 3 / 16 slabs with NaN between the slab copies, slabs
    without a K range (K = 40 over 16 slabs: 3 .. 15 hold +0.0) and a partial last slab (K = 200 over 3: kslab = 80)"""
    assert kr.sel_slabs(40, 16)[3:] == [(40, 40)] * 13 and kr.sel_slabs(200, 3) == [(0, 80), (80, 160), (160, 200)]
    _run(ks, _names(f"gemm am={am}"), f"k_selinv_gemm<{am}>")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["chol", "lu", "lut"])
def test_selinv_gemm_gathered(ks, kind):
    """the gathered operand on units of the synthetic leaves: Cholesky (S2 = S), LU as (SL, SU) and as (SU, SL)"""
    _run(ks, _names(f"gemm am=2 {kind} "), f"k_selinv_gemm<2> {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["chol", "lu0", "lu1"])
def test_selinv_trinv(ks, variant):
    _run(ks, _names(f"trinv {variant}"), {"chol": "k_selinv_trinv", "lu0": "k_lu_selinv_trinv unit=0", "lu1": "k_lu_selinv_trinv unit=1"}[variant])


@pytest.mark.gpu
@pytest.mark.parametrize("lu", [0, 1])
def test_selinv_small(ks, lu):
    """eight units in one launch, then one unit alone; the whole arena outside the units' panels bit-identical"""
    _run(ks, _names(f"small lu={lu}"), "k_lu_selinv_small" if lu else "k_selinv_small")


@pytest.mark.gpu
@pytest.mark.parametrize("lu", [0, 1])
def test_selinv_finish(ks, lu):
    _run(ks, _names(f"finish lu={lu}"), "k_lu_selinv_finish" if lu else "k_selinv_finish")


@pytest.mark.gpu
@pytest.mark.parametrize("acc_in", [0, 1])
def test_selinv_sum(ks, acc_in):
    """bit for bit the float64 loop over z in increasing order"""
    rng = np.random.default_rng(70 + acc_in)
    for nslab in (1, 2, 16):
        for count in (1, 255, 256, 257, 1000):
            stride = count + 11
            ar = kr.Arena()
            src, dst = ar.alloc(stride * nslab), ar.alloc(count)
            buf = ar.image()
            v = buf[src:src + stride * nslab].reshape(nslab, stride)
            v[:, :count] = kr.scalings(rng, count)[None, :] * rng.uniform(-1, 1, (nslab, count))
            if acc_in:
                buf[dst:dst + count] = rng.uniform(-1, 1, count)
            want = buf[dst:dst + count].copy() if acc_in else np.zeros(count)
            for z in range(nslab):
                want = want + v[z, :count]
            out = buf.copy()
            _ok(ks.kp_selinv_sum(P(out), len(out), src, nslab, stride, count, dst, acc_in))
            written = np.zeros(len(out), dtype=bool)
            written[dst:dst + count] = True
            kr.assert_unchanged(buf, out, written, f"k_selinv_sum nslab={nslab} count={count}")
            assert np.array_equal(kr.bits(out[dst:dst + count]), kr.bits(want)), f"k_selinv_sum nslab={nslab} count={count} acc_in={acc_in}"


@pytest.mark.gpu
@pytest.mark.parametrize("lu", [0, 1])
def test_both_paths_on_one_unit(ks, lu):
    """the (17, 240) leaf through the wide path's launches in run_big's order and through the narrow kernel: each within the one
    reference's bound, and the two within the sum of their bounds of each other.  The wide sequence, all with one slab -- Cholesky:
    trinv, Sc = X^T X, Y = P X, Z = G Y, Sc += Y^T Z, finish; LU: trinv of PL (unit) and of PU, Sc = Xu^T Xl, Yl = PL Xl,
    Yu = PU Xu, Zl = G Yl, Zu = G^T Yu, Sc += Yu^T Zl, finish.  (run_big passes the panel itself with lda = nsrow for P; here the
    rows below travel in the scratch image with lda = m.)"""
    st = STRUCT
    case = _case(f"small lu={lu} one")
    J = case.Js[0]
    u, w, ns = case.units[:1], st.ncol(J), st.nsrow(J)
    m = ns - w
    narrow = case.launch(ks)
    worst_narrow = case.check(narrow, "narrow path")
    sides = (("l", case.PL, 1), ("u", case.PU, 0)) if lu else (("l", case.PL, 0),)
    up = "u" if lu else "l"                 # Cholesky: the one L plays both roles
    ar = kr.Arena()
    o = {k + side: ar.alloc(sz) for side, _, _ in sides for k, sz in (("X", w * w), ("Y", m * w), ("Z", m * w), ("P", m * w))}
    o["Sc"] = ar.alloc(w * w)
    buf = ar.image()
    for side, arena, unitd in sides:
        buf[o["P" + side]:o["P" + side] + m * w] = st.panel(arena, J)[w:].T.ravel()
        t = np.full(w * w, np.nan)
        _ok(ks.kp_selinv_trinv(P(arena), st.narena, P(u), lu, unitd, P(t), len(t)))
        buf[o["X" + side]:o["X" + side] + w * w] = t

    def gemm(am, M, N, K, a, lda, b, c, ldc, acc, S=None, S2=None):
        _ok(ks.kp_selinv_gemm(am, M, N, K, P(buf), len(buf), a, lda, b, K, c, ldc, 1, 0, acc, P(u), P(S), P(S2), st.narena,
                              C.addressof(st.c) if am == 2 else None))

    gemm(1, w, w, w, o["X" + up], w, o["Xl"], o["Sc"], w, 0)
    for side, _, _ in sides:
        gemm(0, m, w, w, o["P" + side], m, o["X" + side], o["Y" + side], m, 0)
    gemm(2, m, w, m, -1, 0, o["Yl"], o["Zl"], m, 0, case.SL, case.SU)
    if lu:
        gemm(2, m, w, m, -1, 0, o["Yu"], o["Zu"], m, 0, case.SU, case.SL)
    gemm(1, w, w, m, o["Y" + up], m, o["Zl"], o["Sc"], w, 1)
    SL, SU = case.SL.copy(), case.SU.copy()
    Zl, Zu, Sc = (buf[o[k]:o[k] + cnt].copy() for k, cnt in (("Zl", m * w), ("Z" + up, m * w), ("Sc", w * w)))
    _ok(ks.kp_selinv_finish(P(u), P(Zl), P(Zu) if lu else None, m * w, P(Sc), w * w, P(SL), P(SU) if lu else None, st.narena))
    wide = (SL, SU if lu else SL)
    worst_wide = case.check(wide, "wide path")
    _report(f"both paths lu={lu}: narrow", worst_narrow)
    _report(f"both paths lu={lu}: wide", worst_wide)
    Zl, dZl, Zu, dZu, Scc, dScc = case.refs(J)
    for k, (lo, hi) in enumerate(((dZl, dScc), (dZu, dScc.T))[:1 + lu]):
        pn, pw = st.panel(narrow[k], J), st.panel(wide[k], J)
        assert np.all(np.abs(pn[w:].astype(kr.LD) - pw[w:]) <= 2 * lo) and np.all(np.abs(pn[:w].astype(kr.LD) - pw[:w]) <= 2 * hi)


def _narrow_structure(n):
    """one-column and few-column supernodes with a few rows below each (the rows' ids do not matter to diag / pack / logdet)"""
    widths = []
    while sum(widths) < n:
        widths.append(min((1, 1, 3, 2, 1, 4)[len(widths) % 6], n - sum(widths)))
    Super = np.concatenate([[0], np.cumsum(widths)])
    rowlists = [np.concatenate([np.arange(Super[s], Super[s + 1]), np.full(s % 3 if Super[s + 1] < n else 0, n - 1)]) for s in range(len(widths))]
    return Structure(Super, rowlists)


NARROW_N = [1, 255, 256, 257, 65537 + 300]


@pytest.mark.gpu
@pytest.mark.parametrize("n", NARROW_N)
def test_diag_pack_logdet(ks, n):
    """k_selinv_diag / k_lu_selinv_diag and k_lu_selinv_pack bit for bit; k_logdet_* and k_lu_logdet_* against longdouble sums (n =
    65837: 258 partial sums, so lanes 0 and 1 of the final kernel add a second one), the LU sign exact"""
    st = _narrow_structure(n)
    rng = np.random.default_rng(n)
    A = np.full(st.narena, np.nan)
    A[G:-G] = kr.scalings(rng, st.narena - 2 * G, 1e-3, 1e3)
    s = st.SuperMap
    cols = np.arange(n)
    dpos = st.Xp[s] + (cols - st.Super[s]) * (np.diff(st.Lsip)[s] + 1)
    for lu in (0, 1):
        d = np.full(n + 64, np.nan)
        _ok(ks.kp_selinv_diag(n, P(A), st.narena, C.addressof(st.c), lu, P(d), len(d)))
        assert np.array_equal(kr.bits(d[:n]), kr.bits(A[dpos])) and np.all(np.isnan(d[n:])), f"diag lu={lu}"
    nb = (n + 255) // 256
    buf = np.full(nb + 1 + 64, np.nan)
    _ok(ks.kp_logdet(n, P(A), st.narena, C.addressof(st.c), 0, P(buf), len(buf), None, 0))
    logs = np.log(A[dpos].astype(kr.LD))
    err, bound = abs(kr.LD(buf[nb]) - 2 * np.sum(logs)), 2 * kr.logdet_bound(logs)
    assert np.isfinite(buf[nb]) and err <= bound and np.all(np.isnan(buf[nb + 1:])), (float(err), float(bound))
    worst = float(err / bound)
    negsets = [[], [n // 2], sorted({0, n - 1}) if n > 1 else [0, 0], list(range(0, n, 255))[:2 * (len(range(0, n, 255)) // 2)]]
    for neg_at in negsets:
        B = A.copy()
        B[dpos[neg_at]] *= -1.0
        buf = np.full(nb + 2 + 64, np.nan)
        neg = np.full(nb + 8, -7, dtype=np.int32)
        _ok(ks.kp_logdet(n, P(B), st.narena, C.addressof(st.c), 1, P(buf), len(buf), P(neg), len(neg)))
        err, bound = abs(kr.LD(buf[nb]) - np.sum(logs)), kr.logdet_bound(logs)
        assert np.isfinite(buf[nb]) and err <= bound, (float(err), float(bound))
        assert buf[nb + 1] == float(len(set(neg_at)) % 2) and np.all(np.isnan(buf[nb + 2:])) and np.all(neg[nb:] == -7), neg_at
        worst = max(worst, float(err / bound))
    _report(f"logdet n={n}", worst)
    # pack: a range that starts and ends inside panels
    ncol, nsrow = np.diff(st.Super), np.diff(st.Lsip)
    RefXp = np.concatenate([[0], np.cumsum((2 * nsrow - ncol) * ncol)]).astype(np.int64)
    SU = np.full(st.narena, np.nan)
    SU[G:-G] = rng.uniform(-1, 1, st.narena - 2 * G)
    want = np.concatenate([np.hstack([st.panel(A, J).T, st.panel(SU, J).T[:, st.ncol(J):]]).ravel() for J in range(st.nsuper)])
    for e0, e1 in {(0, int(RefXp[-1])), (min(2, int(RefXp[-1]) - 1), max(int(RefXp[-1]) - 3, min(2, int(RefXp[-1]) - 1) + 1))}:
        out = np.full(e1 - e0 + 64, np.nan)
        _ok(ks.kp_lu_selinv_pack(C.addressof(st.c), P(RefXp), P(A), P(SU), st.narena, P(out), len(out), e0, e1))
        assert np.array_equal(kr.bits(out[:e1 - e0]), kr.bits(want[e0:e1])) and np.all(np.isnan(out[e1 - e0:])), (e0, e1)
