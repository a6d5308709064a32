"""Single-launch tests of the kernels that read Sigma = A^-1 on A's own pattern (csrc/sf_selinv_pattern.hip): k_selpat_build,
k_selpat_gather, k_selpat_part<MAPPED>, k_selpat_final and k_selpat_entries, through the launchers the plans call (sf_kernels.h:
launch_selpat_*) on operands the test builds itself.

Every double operand of a launch lies in ONE host image (kernel_ref.Arena).  NaN fills the guard bands and everything a launch must
not read: the V of a dead position (map -1, or the row a dead position's vmap names), the padding rows [rows, ldv) of V, 8 further
columns of V behind m, Sigma wherever no live map entry points (with a shift: everywhere but the shifted positions), the map entries
and marks past count (they name a NaN position), every arena entry no queried pair addresses.  Everything outside the documented write
set -- the other side's part slots, the part columns >= m, out[m..], out past count, pos / offd past nnz -- is compared bit for bit.
Reductions get integer inputs (|S|, |V| <= 8: every partial sum is an exact double, the parts must equal the exact sums) and inputs
scaled over 1e-6 .. 1e6, held to SAFETY depth u sum |terms| with depth = 16 for a part (the lane's 8 fused multiply-adds, 6 shuffle
levels, 2 additions of the waves' sums; the weight 2 is exact) and ceil(nparts / 256) + 8 for the final sum -- derived, not measured.

The CPU tests run numpy emulations of the launches (kernel_ref.selpat_*_emulate) through the same checkers: the clean emulation
passes, each single fault of kernel_ref.SELPAT_FAULTS is rejected, and it is rejected with finite junk in place of every NaN too, so
no fault is caught only by a NaN -- no kernel is ever made wrong.

Not tested here: the product (col - c0) * nsrow of k_selpat_entries beyond 2^31.  It is the expression k_selpat_build has (tested
below with offsets only, since the build dereferences none), but entries reads the arena at the offset: one launch would need an
arena of more than 20 GB.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_ref as kr
from test_kernels import _ok, P, kp  # noqa: F401
from test_kernels_apply import Img, _rejects
from test_kernels_selinv import Structure
from util import sf, small_cases

NAN = np.nan
TILE = kr.SELPAT_TILE
SENTINEL = 12345.678                # what the part slots hold before a launch
PART_COUNTS = (1, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 5)
PART_M = (1, 7, 8, 9, 64)
VARIANTS = ("offd", "shift_up", "shift_down")       # shift = 0 with the off-diagonal marks; shift = +K; shift = -K
FINAL_NPARTS = (1, 255, 256, 257, 1000)
GATHER_COUNTS = (1, 255, 256, 257, (1 << 20) + 4321)         # the last: above the 4096 x 256 grid, the launch strides
ENT_COUNTS = (1, 256, 257, 3 * 256 + 9)


@pytest.fixture(scope="module")
def ks(kp):
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    kp.kp_build_loadmap.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, i64, i32, vp]
    kp.kp_selpat_build.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i64]
    kp.kp_selpat_gather.argtypes = [vp, i64, i64, vp, i64, i64]
    kp.kp_selpat_part.argtypes = [i32, vp, vp, vp, i64, i64, vp, i64, i64, i64, i64, i64, i32, i64, i64, i64, vp]
    kp.kp_selpat_final.argtypes = [vp, i64, i64, i64, i32, i64]
    kp.kp_selpat_entries.argtypes = [vp, vp, i64, i32, i64, vp, i64, i64, vp, i64, vp]
    return kp


def _report(name, worst):
    print(f"SELPAT_RATIO {name}: worst err / bound = {worst:.3g}")
    return worst


def _junk(a):
    """finite junk in place of every NaN: a fault must then show in a value or in the write set, not in a NaN"""
    bad = np.flatnonzero(np.isnan(a))
    a[bad] = 1000.0 + bad % 97
    return a


def _nonzero_ints(rng, shape):
    return (rng.integers(1, 9, shape) * rng.choice([-1, 1], shape)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the hand-built structure of the build and entries tests
# ---------------------------------------------------------------------------------------------------------------------
def _hand_structure():
    """supernodes: width 1 without rows below (column 0), width 1 with rows below (1), width 3 (2 .. 4), width 64 with one row below
    (5 .. 68), a last supernode of one column (69).  The row list of column 1's supernode follows column 0's in Lsi."""
    Super = np.array([0, 1, 2, 5, 69, 70])
    rowlists = [np.array([0]), np.array([1, 3, 7, 30]), np.array([2, 3, 4, 7, 30, 69]), np.arange(5, 70), np.array([69])]
    return Structure(Super, rowlists)


HAND = _hand_structure()


def _where(st):
    """(row, column) -> offset in a panel set, for every position of the lower trapezoids: a dictionary, no search"""
    out = {}
    for s in range(st.nsuper):
        c0, rows = int(st.Super[s]), st.rows(s)
        for c in range(st.ncol(s)):
            for k, r in enumerate(rows):
                if r >= c0 + c:
                    out[(int(r), c0 + c)] = int(st.Xp[s]) + c * st.nsrow(s) + k
    return out


HAND_WHERE = _where(HAND)


def test_hand_structure_is_what_the_tests_claim():
    st = HAND
    assert [st.ncol(s) for s in range(st.nsuper)] == [1, 1, 3, 64, 1]
    assert [st.nsrow(s) - st.ncol(s) for s in range(st.nsuper)] == [0, 3, 3, 1, 0]
    # the nb = 0 case: behind supernode 0's (empty) rows below lies the first row of the next list, which is the queried row 1
    assert st.Lsi[st.Lsip[0] + st.ncol(0)] == 1 == st.Super[1]
    assert (1, 0) not in HAND_WHERE and (69, 1) not in HAND_WHERE and (10, 1) not in HAND_WHERE and (10, 3) not in HAND_WHERE
    assert (30, 1) in HAND_WHERE and (7, 3) in HAND_WHERE and (30, 3) in HAND_WHERE


# ---------------------------------------------------------------------------------------------------------------------
# k_selpat_build
# ---------------------------------------------------------------------------------------------------------------------
class BuildCase:
    def __init__(self, st, Lp, Li, want_pos, tail=5):
        self.st, self.Lp, self.Li = st, np.ascontiguousarray(Lp, dtype=np.int64), np.ascontiguousarray(Li, dtype=np.int32)
        self.nnz, self.npos = len(Li), len(Li) + tail
        self.want_pos = np.asarray(want_pos, dtype=np.int64)
        cols = np.repeat(np.arange(len(Lp) - 1), np.diff(Lp))
        self.want_offd = (self.Li != cols).astype(np.uint8)

    def fresh(self, with_offd):
        return np.full(self.npos, -7, dtype=np.int64), (np.full(self.npos, 0xAB, dtype=np.uint8) if with_offd else None)

    def check(self, pos, offd, what):
        assert np.array_equal(pos[:self.nnz], self.want_pos), f"{what}: pos"
        assert np.all(pos[self.nnz:] == -7), f"{what}: pos beyond nnz changed"
        if offd is not None:
            assert np.array_equal(offd[:self.nnz], self.want_offd), f"{what}: offd"
            assert np.all(offd[self.nnz:] == 0xAB), f"{what}: offd beyond nnz changed"

    def emulate(self, with_offd, fault=None):
        pos, offd = self.fresh(with_offd)
        return kr.selpat_build_emulate(self.st, self.Lp, self.Li, pos, offd, fault)

    def launch(self, ks, with_offd):
        st = self.st
        pos, offd = self.fresh(with_offd)
        _ok(ks.kp_selpat_build(P(self.Lp), P(self.Li), st.n, P(st.Super), P(st.SuperMap), st.nsuper, P(st.Lsip), P(st.Lsi), P(st.Xp), P(pos),
                               P(offd), self.npos))
        return pos, offd


def _hand_build():
    """columns with 0, 1 and many entries; the first and the last row below, duplicates and unsorted order inside a column"""
    st = HAND
    rng = np.random.default_rng(11)
    cols = {0: [0], 1: [30, 1, 3, 7, 30, 3], 2: [], 3: [69, 4, 3, 7, 30, 7], 4: [], 69: [69]}
    for j in range(5, 69):
        if j % 3 == 0:
            cols[j] = []
        elif j % 3 == 1:
            cols[j] = [69]                          # the one row below: the first and the last
        else:
            cols[j] = rng.choice(np.arange(j, 70), 9).tolist() + [j, 69, j]
    Li = np.concatenate([np.asarray(cols[j], dtype=np.int64) for j in range(st.n)])
    Lp = np.concatenate([[0], np.cumsum([len(cols[j]) for j in range(st.n)])])
    want = [HAND_WHERE[(i, j)] for j in range(st.n) for i in cols[j]]
    return BuildCase(st, Lp, Li, want)


BIG_W, BIG_R = 40000, 70000


def _big_build():
    """offsets only: one supernode of 40,000 columns and 70,000 rows whose panel starts at 2^33 + 3; all columns empty but its first,
    middle and last, each with its diagonal entry, the first and the last row below"""
    nb = BIG_R - BIG_W
    n = 1 + BIG_W + 2 * nb + 1
    Super = np.array([0, 1, 1 + BIG_W, n])
    below = 1 + BIG_W + 2 * np.arange(nb)
    st = Structure(Super, [np.array([0]), np.concatenate([np.arange(1, 1 + BIG_W), below]), np.arange(1 + BIG_W, n)])
    st.Xp[1] = (1 << 33) + 3
    st.Xp[2] = st.Xp[1] + BIG_W * BIG_R
    st.Xp[3] = st.Xp[2] + (n - 1 - BIG_W) ** 2
    cols = (1, 1 + BIG_W // 2, BIG_W)
    cnt = np.zeros(n, dtype=np.int64)
    cnt[list(cols)] = 3
    Lp = np.concatenate([[0], np.cumsum(cnt)])
    Li = np.concatenate([[j, below[0], below[-1]] for j in cols])
    want = [int(st.Xp[1]) + (j - 1) * BIG_R + si for j in cols for si in (j - 1, BIG_W, BIG_R - 1)]
    return BuildCase(st, Lp, Li, want), cols


def test_build_emulation_and_faults():
    hand = _hand_build()
    lens = np.diff(hand.Lp)
    assert 0 in lens and 1 in lens and lens.max() >= 12
    for with_offd in (True, False):
        hand.check(*hand.emulate(with_offd), "clean")
    for fault in ("diagonal row searched", "offd inverted"):
        _rejects(hand.check, *hand.emulate(True, fault), fault)
    big, cols = _big_build()
    assert (cols[-1] - 1) * BIG_R >= 1 << 31 and int(big.st.Xp[1]) >= 1 << 32
    assert big.want_pos[-1] == (1 << 33) + 3 + 39999 * 70000 + 69999
    big.check(*big.emulate(True), "clean big")
    _rejects(big.check, *big.emulate(True, "32-bit product"), "32-bit product")


@pytest.mark.gpu
@pytest.mark.parametrize("with_offd", [True, False], ids=["offd", "no_offd"])
def test_selpat_build_hand_structure(ks, with_offd):
    hand = _hand_build()
    pos, offd = hand.launch(ks, with_offd)
    hand.check(pos, offd, "k_selpat_build")
    epos, eoffd = hand.emulate(with_offd)
    assert np.array_equal(pos, epos) and (offd is None or np.array_equal(offd, eoffd))


@pytest.mark.gpu
def test_selpat_build_offsets_beyond_32_bits(ks):
    big, cols = _big_build()
    assert (cols[-1] - 1) * BIG_R >= 1 << 31
    pos, offd = big.launch(ks, True)
    big.check(pos, offd, "k_selpat_build, 64-bit offsets")
    assert np.array_equal(pos, big.emulate(True)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in small_cases() if c[0] in ("lap2d_8x8_nd", "lap3d_8_nd")], ids=lambda c: c[0])
def test_selpat_build_agrees_with_the_load_map(ks, case):
    """on a real analysis: pos = the emulation everywhere and = k_build_loadmap's map wherever that map keeps the entry"""
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    i64 = lambda x: np.ascontiguousarray(x, dtype=np.int64)
    Lp, Li, Super, SuperMap, Lsip, Lsi, Lsxp = i64(sym.Lp), i32(sym.Li), i32(sym.Super), i32(sym.SuperMap), i64(sym.Lsip), i32(sym.Lsi), i64(sym.Lsxp)
    ns, nnz = int(sym.nsuper), len(Li)
    tb = kr.SelTables(Super, Lsip, Lsi, Lsxp)
    m = np.full(nnz, -9, dtype=np.int64)
    _ok(ks.kp_build_loadmap(P(Lp), P(Li), n, P(Super), P(SuperMap), ns, P(Lsip), P(Lsi), P(Lsxp), 0, 0, P(m)))
    pos, offd = np.full(nnz + 5, -7, dtype=np.int64), np.full(nnz + 5, 0xAB, dtype=np.uint8)
    _ok(ks.kp_selpat_build(P(Lp), P(Li), n, P(Super), P(SuperMap), ns, P(Lsip), P(Lsi), P(Lsxp), P(pos), P(offd), nnz + 5))
    epos, eoffd = kr.selpat_build_emulate(tb, Lp, Li, np.full(nnz + 5, -7, dtype=np.int64), np.full(nnz + 5, 0xAB, dtype=np.uint8))
    assert np.array_equal(pos, epos) and np.array_equal(offd, eoffd)
    assert np.all(m >= 0) and np.array_equal(pos[:nnz][m >= 0], m[m >= 0])


# ---------------------------------------------------------------------------------------------------------------------
# k_selpat_gather
# ---------------------------------------------------------------------------------------------------------------------
def _gather_case(count, poison=NAN):
    rng = np.random.default_rng(count)
    nS = count // 3 + 5
    pos = rng.integers(0, nS - 1, count).astype(np.int64)            # repeats; the last entry of S is never selected
    im = Img(s=nS, out=count + 3)
    sel = np.unique(pos)
    im["s"][sel] = rng.standard_normal(len(sel))
    if not np.isnan(poison):
        _junk(im.a)
    im.writes("out", np.arange(count))
    return im, pos


def _gather_check(im, pos, count, what):
    im.unchanged(what)
    kr.assert_bits(im["out"][:count], im["s"][pos], what)


def test_gather_emulation_and_fault():
    for count in (257, GATHER_COUNTS[-1]):
        for fault in (None, "gather no stride"):
            im, pos = _gather_case(count, poison=0.0)
            im.start()
            kr.selpat_gather_emulate(pos, count, im["s"], im["out"], fault)
            if fault and count > kr.SELPAT_GATHER_GRID * 256:
                _rejects(_gather_check, im, pos, count, fault)
            else:
                _gather_check(im, pos, count, "clean")


@pytest.mark.gpu
@pytest.mark.parametrize("count", GATHER_COUNTS)
def test_selpat_gather(ks, count):
    im, pos = _gather_case(count)
    buf, nbuf = im.start()
    _ok(ks.kp_selpat_gather(buf, nbuf, im.off["s"], P(pos), count, im.off["out"]))
    _gather_check(im, pos, count, f"gather count={count}")


# ---------------------------------------------------------------------------------------------------------------------
# k_selpat_part<false / true>, k_selpat_final
# ---------------------------------------------------------------------------------------------------------------------
class Side:
    """the operands of one k_selpat_part launch; the values are placed into the image by TraceCase"""

    def __init__(self, seed, count, mapped, variant, integer):
        rng = np.random.default_rng([seed, count, int(mapped), VARIANTS.index(variant), int(integer)])
        self.count, self.mapped, self.variant, self.integer = count, mapped, variant, integer
        self.nt = kr.selpat_tiles(count)
        nS = count + 7
        K = nS + 6 if variant != "offd" else 0      # K > nS: the unshifted positions lie in the part of S that holds NaN
        self.shift = {"offd": 0, "shift_up": K, "shift_down": -K}[variant]
        up, down = (K if variant == "shift_up" else 0), (K if variant == "shift_down" else 0)
        self.slen = nS + 1 + K                      # position nS is never live: the map entries past count name it
        nmap = self.nmap = count + 5
        idx = rng.integers(0, nS, count)
        dead = rng.random(count) < 0.1
        dead[0] = False
        if count > 1:
            dead[1] = True
        self.live = ~dead
        self.map = np.full(nmap, nS + down, dtype=np.int64)
        self.map[:count] = np.where(dead, -1, idx + down)
        self.offd = None
        if variant == "offd":
            self.offd = np.ones(nmap, dtype=np.uint8)
            self.offd[:count] = rng.random(count) < 0.7
            self.offd[0] = 0
        sval = _nonzero_ints(rng, nS) if integer else rng.standard_normal(nS) * kr.scalings(rng, nS)
        self.S = np.full(self.slen, NAN)
        self.S[idx[self.live] + up] = sval[idx[self.live]]
        self.s_live = sval[idx]                      # Sigma of entry p (meaningless where dead)
        self.rows = count + 3 if mapped else count
        self.ldv = self.rows + 5
        self.vmap = None
        if mapped:                                  # sources repeat; row rows - 1 is never live: dead positions and the tail name it
            vm = rng.integers(0, self.rows - 1, count)
            vm[self.live & (rng.random(count) < 0.1)] = -1
            vm[dead] = self.rows - 1
            self.vmap = np.full(nmap, self.rows - 1, dtype=np.int64)
            self.vmap[:count] = vm
            self.vrow = vm
            used = np.zeros(self.rows, dtype=bool)
            used[vm[self.live & (vm >= 0)]] = True
        else:
            self.vrow = np.where(dead, -1, np.arange(count))
            used = np.zeros(self.rows, dtype=bool)
            used[:count] = self.live
        self.has_v = self.live & (self.vrow >= 0)
        V = _nonzero_ints(rng, (self.rows, 64)) if integer else rng.standard_normal((self.rows, 64)) * kr.scalings(rng, self.rows)[:, None]
        V[~used] = NAN
        self.V = V

    def vblock(self, m):
        """column-major ldv x (m + 8): the first m columns of V, NaN in the padding rows and in the 8 columns behind"""
        blk = np.full((m + 8, self.ldv), NAN)
        blk[:m, :self.rows] = self.V[:, :m].T
        return blk.ravel()

    def terms(self, m):
        """w_p S_p V_pt for every entry (0 where the entry does not count), longdouble: count x m"""
        w = np.where(self.offd[:self.count] != 0, 2.0, 1.0) if self.offd is not None else np.ones(self.count)
        v = np.where(self.has_v[:, None], self.V[np.maximum(self.vrow, 0), :m], 0.0)
        return np.where(self.has_v[:, None], (w * np.where(self.live, self.s_live, 0.0)).astype(kr.LD)[:, None] * v.astype(kr.LD), kr.LD(0))

    def tile_sums(self, m):
        t = np.zeros((self.nt * TILE, m), dtype=kr.LD)
        t[:self.count] = self.terms(m)
        t = t.reshape(self.nt, TILE, m)
        return t.sum(axis=1), np.abs(t).sum(axis=1)


class TraceCase:
    """sides sharing one part array, in one image; single-launch tests: one side, part0 = 3, nparts = tiles + 7"""

    def __init__(self, sides, m, poison=NAN, lone=True):
        self.sides, self.m = sides, m
        total = sum(s.nt for s in sides)
        self.nparts = total + 7 if lone else total
        self.part0 = np.cumsum([3 if lone else 0] + [s.nt for s in sides])[:-1]
        sizes = {"part": (m + 8) * self.nparts + 3, "out": m + 3}
        for k, s in enumerate(sides):
            sizes[f"s{k}"], sizes[f"v{k}"] = s.slen, s.ldv * (m + 8)
        self.im = im = Img(**sizes)
        im["part"] = SENTINEL
        for k, s in enumerate(sides):
            im[f"s{k}"], im[f"v{k}"] = s.S, s.vblock(m)
        if not np.isnan(poison):
            _junk(im.a)

    def slots(self, k):
        """offsets inside the part region of the slots side k writes: columns t < m, its tiles"""
        return (np.arange(self.m)[:, None] * self.nparts + self.part0[k] + np.arange(self.sides[k].nt)[None, :]).ravel()

    def parts(self, k):
        return self.im["part"][self.slots(k)].reshape(self.m, self.sides[k].nt).T      # tiles x m

    def run_part(self, k, launch, what):
        """one part launch of side k through `launch` (the probe or an emulation); returns the worst err / bound"""
        im, s = self.im, self.sides[k]
        im.written[:] = False
        im.writes("part", self.slots(k))
        im.start()
        got = launch(self, k)
        im.unchanged(what)
        assert got == s.nt, f"{what}: {got} workgroups reported, {s.nt} tiles"
        parts = self.parts(k)
        ref, mag = s.tile_sums(self.m)
        if s.integer:
            assert np.array_equal(parts, ref.astype(np.float64)), f"{what}: integer inputs, the parts are not the exact sums"
        return kr.within_ratio(parts, ref, kr.SAFETY * kr.SELPAT_PART_DEPTH * kr.U * mag, what)

    def run_final(self, launch, what, extra_depth=0):
        """the final launch over the part array as it stands; the reference is the longdouble sum of those parts"""
        im = self.im
        im.written[:] = False
        im.writes("out", np.arange(self.m))
        im.start()
        launch(self)
        im.unchanged(what)
        P_ = im["part"][:self.m * self.nparts].reshape(self.m, self.nparts).astype(kr.LD)
        bound = kr.SAFETY * kr.selpat_final_depth(self.nparts) * kr.U * np.abs(P_).sum(axis=1)
        return kr.within_ratio(im["out"][:self.m], P_.sum(axis=1), bound, what)


def _emu_part(fault=None):
    def launch(c, k):
        s, im = c.sides[k], c.im
        return kr.selpat_part_emulate(im.a, s.mapped, s.map, s.offd, s.vmap, s.count, im.off[f"s{k}"], s.shift, im.off[f"v{k}"], s.ldv, c.m,
                                      im.off["part"], int(c.part0[k]), c.nparts, fault)
    return launch


def _emu_final(fault=None):
    return lambda c: kr.selpat_final_emulate(c.im.a, c.im.off["part"], c.nparts, c.m, c.im.off["out"], fault)


def _gpu_part(ks):
    def launch(c, k):
        s, im = c.sides[k], c.im
        n = C.c_int64(-1)
        _ok(ks.kp_selpat_part(int(s.mapped), P(s.map), P(s.offd), P(s.vmap), s.nmap, s.count, P(im.a), im.a.size, im.off[f"s{k}"], s.shift,
                              im.off[f"v{k}"], s.ldv, c.m, im.off["part"], int(c.part0[k]), c.nparts, C.byref(n)))
        return n.value
    return launch


def _gpu_final(ks):
    return lambda c: _ok(ks.kp_selpat_final(P(c.im.a), c.im.a.size, c.im.off["part"], c.nparts, c.m, c.im.off["out"]))


def _part_grid(launch, mapped, variant, counts=PART_COUNTS, ms=PART_M, poison=NAN):
    """every count x m x (integer, scaled) of one kernel instance and variant; a column has the bits it has with m = 64"""
    worst = 0.0
    for count in counts:
        for integer in (True, False):
            side = Side(0, count, mapped, variant, integer)
            full = None
            for m in sorted(ms, reverse=True):
                c = TraceCase([side], m, poison)
                what = f"part mapped={mapped} {variant} count={count} m={m} integer={integer}"
                r = c.run_part(0, launch, what)
                worst = max(worst, 0.0 if integer else r)
                if full is None:
                    full = c.parts(0).copy()
                kr.assert_bits(c.parts(0), full[:, :m], what + ": the columns' bits with the largest m")
    return worst


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mapped", [False, True], ids=["plain", "mapped"])
def test_part_checker_accepts_the_emulation(mapped, variant):
    assert np.isfinite(_part_grid(_emu_part(), mapped, variant))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mapped", [False, True], ids=["plain", "mapped"])
def test_selpat_part(ks, mapped, variant):
    """the whole grid of counts and m; then a NaN in one column of V, and count = 0"""
    _report(f"part mapped={mapped} {variant}", _part_grid(_gpu_part(ks), mapped, variant))
    side = Side(1, 2048 + 257, mapped, variant, False)
    c = TraceCase([side], 9)
    c.run_part(0, _gpu_part(ks), "clean")
    clean = c.parts(0).copy()
    p = int(np.flatnonzero(side.has_v & (np.arange(side.count) >= TILE))[0])          # an entry of the second tile
    c.im[f"v0"][side.vrow[p] + 3 * side.ldv] = NAN
    c.im["part"] = SENTINEL
    c.im.written[:] = False
    c.im.writes("part", c.slots(0))
    buf, nbuf = c.im.start()
    assert _gpu_part(ks)(c, 0) == 2
    c.im.unchanged("a NaN in column 3")
    got = c.parts(0)
    hit = np.zeros(side.nt, dtype=bool)             # the tiles with an entry that reads the row (mapped: sources repeat)
    hit[np.flatnonzero(side.has_v & (side.vrow == side.vrow[p])) // TILE] = True
    assert hit[1] and np.all(np.isnan(got[hit, 3])) and np.all(np.isfinite(np.delete(got, 3, axis=1)))
    kr.assert_bits(np.delete(got, 3, axis=1), np.delete(clean, 3, axis=1), "a NaN in column 3 of V reaches column 3 only")
    kr.assert_bits(got[~hit, 3], clean[~hit, 3], "and only the tiles of the entries that read it")
    # count = 0: nothing launched, nothing written
    c.im.written[:] = False
    c.im.start()
    n = C.c_int64(-1)
    _ok(ks.kp_selpat_part(int(mapped), P(side.map), P(side.offd), P(side.vmap), side.nmap, 0, P(c.im.a), c.im.a.size, c.im.off["s0"], side.shift,
                          c.im.off["v0"], side.ldv, 9, c.im.off["part"], 3, c.nparts, C.byref(n)))
    assert n.value == 0
    c.im.unchanged("count = 0")


class FinalCase(TraceCase):
    """a part array of m columns, nparts apart, and nothing else"""

    def __init__(self, nparts, m, integer, poison=NAN):
        rng = np.random.default_rng([nparts, m, int(integer)])
        self.sides, self.m, self.nparts, self.integer = [], m, nparts, integer
        self.im = im = Img(part=m * nparts, out=m + 3)
        im["part"] = _nonzero_ints(rng, m * nparts) if integer else rng.standard_normal(m * nparts) * kr.scalings(rng, m * nparts)
        if not np.isnan(poison):
            _junk(im.a)

    def run(self, launch, what):
        r = self.run_final(launch, what)
        if self.integer:
            assert np.array_equal(self.im["out"][:self.m], self.im["part"].reshape(self.m, self.nparts).sum(axis=1)), f"{what}: not exact"
        return r


def _final_grid(launch, poison=NAN):
    worst = 0.0
    for nparts in FINAL_NPARTS:
        for m in (1, 64):
            for integer in (True, False):
                r = FinalCase(nparts, m, integer, poison).run(launch, f"final nparts={nparts} m={m} integer={integer}")
                worst = max(worst, 0.0 if integer else r)
    return worst


def test_final_checker_accepts_the_emulation():
    assert np.isfinite(_final_grid(_emu_final()))


@pytest.mark.gpu
def test_selpat_final(ks):
    _report("final", _final_grid(_gpu_final(ks)))


def _together(part, final, lu):
    """the parts of every side, then the final sum, against the longdouble sum of all products; twice, the same bits"""
    m = 9
    if lu:
        sides = [Side(2, 2049, False, "shift_up", False), Side(3, 2048 + 257, False, "shift_down", False)]
    else:
        sides = [Side(2, 3 * 2048 + 5, False, "offd", False)]
    c = TraceCase(sides, m, lone=False)
    outs = []
    for trip in range(2):
        c.im["part"][:(m + 8) * c.nparts] = SENTINEL
        c.im["out"] = NAN
        for k in range(len(sides)):
            c.run_part(k, part, f"together lu={lu} side {k}")
        c.run_final(final, f"together lu={lu} final")
        outs.append(c.im["out"][:m].copy())
    kr.assert_bits(outs[1], outs[0], "two runs")
    t = np.concatenate([s.terms(m) for s in sides])
    depth = kr.SELPAT_PART_DEPTH + kr.selpat_final_depth(c.nparts)
    return kr.within_ratio(outs[0], t.sum(axis=0), kr.SAFETY * depth * kr.U * np.abs(t).sum(axis=0), f"together lu={lu}")


@pytest.mark.parametrize("lu", [False, True], ids=["cholesky", "lu"])
def test_part_and_final_together_emulated(lu):
    assert np.isfinite(_together(_emu_part(), _emu_final(), lu))


@pytest.mark.gpu
@pytest.mark.parametrize("lu", [False, True], ids=["cholesky", "lu"])
def test_selpat_part_and_final_together(ks, lu):
    _report(f"part + final lu={lu}", _together(_gpu_part(ks), _gpu_final(ks), lu))


# ---------------------------------------------------------------------------------------------------------------------
# k_selpat_entries
# ---------------------------------------------------------------------------------------------------------------------
def _entry_pairs():
    """the nb = 0 case first, then its mirror, a row beyond the last row below, rows between two rows below, then every pair of the
    70 x 70 grid in a fixed random order: all pairs of the pattern in both triangles and all pairs outside it"""
    n = HAND.n
    grid = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 2)
    grid = grid[np.random.default_rng(5).permutation(len(grid))]
    return np.concatenate([[(1, 0), (0, 1), (69, 1), (10, 1), (10, 3), (1, 69)], grid]).astype(np.int64)


ENT_PAIRS = _entry_pairs()


class EntCase:
    def __init__(self, lu, count, poison=NAN):
        st = HAND
        self.lu, self.count, self.xC = lu, count, st.narena
        self.rows, self.cols = np.ascontiguousarray(ENT_PAIRS[:count, 0]), np.ascontiguousarray(ENT_PAIRS[:count, 1])
        self.im = im = Img(s=st.narena * (2 if lu else 1), out=count + 3)
        rng = np.random.default_rng(3)
        for (r, c), off in HAND_WHERE.items():      # the two arenas hold different values; the second has no diagonal
            im["s"][off] = rng.standard_normal()
            if lu and r > c:
                im["s"][self.xC + off] = rng.standard_normal()
        if not np.isnan(poison):
            _junk(im.a)
        self.want = np.full(count, NAN)
        self.n_out = 0
        for k in range(count):
            i, j = int(self.rows[k]), int(self.cols[k])
            off = HAND_WHERE.get((max(i, j), min(i, j)))
            if off is None:
                self.n_out += 1
            else:
                self.want[k] = im["s"][off + (self.xC if lu and i < j else 0)]
        im.writes("out", np.arange(count))

    def run(self, launch, what):
        self.im.start()
        after = launch(self, 5)
        self.im.unchanged(what)
        got = self.im["out"][:self.count]
        inside = ~np.isnan(self.want)
        assert np.all(np.isnan(got[~inside])), f"{what}: a pair outside the pattern came back with a number"
        kr.assert_bits(got[inside], self.want[inside], what)
        assert after == 5 + self.n_out, f"{what}: the counter went from 5 to {after}, {self.n_out} pairs are outside"
        if not self.lu:                             # both triangles give the same bits
            seen = {}
            for k in range(self.count):
                key = (max(self.rows[k], self.cols[k]), min(self.rows[k], self.cols[k]))
                seen.setdefault(key, got[k:k + 1].view(np.uint64)[0])
                assert seen[key] == got[k:k + 1].view(np.uint64)[0], f"{what}: the two triangles differ at {key}"


def _emu_entries(fault=None):
    def launch(c, start):
        im = c.im
        return kr.selpat_entries_emulate(HAND, c.rows, c.cols, c.count, c.lu, c.xC, im.a, im.off["s"], im.off["out"], start, fault)
    return launch


def _gpu_entries(ks):
    def launch(c, start):
        im = c.im
        cnt = C.c_uint64(start)
        _ok(ks.kp_selpat_entries(P(c.rows), P(c.cols), c.count, int(c.lu), c.xC, P(im.a), im.a.size, im.off["s"], C.byref(HAND.c), im.off["out"],
                                 C.byref(cnt)))
        return cnt.value
    return launch


def test_entry_pairs_cover_what_the_tests_claim():
    inside = [(int(i), int(j)) for i, j in ENT_PAIRS[6:] if (max(i, j), min(i, j)) in HAND_WHERE]
    assert len(inside) == 2 * len(HAND_WHERE) - HAND.n                     # every position of the pattern, both triangles
    assert any(5 <= j < i < 69 for i, j in inside) and any(5 <= i < j < 69 for i, j in inside)       # inside a diagonal block
    for count in ENT_COUNTS[1:]:
        c = EntCase(True, count)
        assert 0 < c.n_out < count                   # mixed pairs in every workgroup's share
    assert EntCase(False, 1).n_out == 1


@pytest.mark.parametrize("lu", [False, True], ids=["cholesky", "lu"])
def test_entries_checker_accepts_the_emulation(lu):
    for count in ENT_COUNTS + (len(ENT_PAIRS),):
        EntCase(lu, count).run(_emu_entries(), f"entries lu={lu} count={count}")


@pytest.mark.gpu
@pytest.mark.parametrize("lu", [False, True], ids=["cholesky", "lu"])
@pytest.mark.parametrize("count", ENT_COUNTS + (len(ENT_PAIRS),))
def test_selpat_entries(ks, count, lu):
    EntCase(lu, count).run(_gpu_entries(ks), f"entries lu={lu} count={count}")


# ---------------------------------------------------------------------------------------------------------------------
# every fault of kernel_ref.SELPAT_FAULTS, by name: the emulation with that one fault goes through the checker the GPU test of the same
# launch uses.  Each scenario runs with NaN and with finite junk where a launch must not read; a fault counts as rejected only if it
# is rejected with the junk, where no NaN exists.
# ---------------------------------------------------------------------------------------------------------------------
def _part_scenario(fault, poison):
    hits = 0
    for mapped in (False, True):
        for variant in VARIANTS:
            try:
                _part_grid(_emu_part(fault), mapped, variant, counts=(257, 2049), ms=(9, 64), poison=poison)
            except AssertionError:
                hits += 1
    return hits


def _final_scenario(fault, poison):
    try:
        _final_grid(_emu_final(fault), poison)
    except AssertionError:
        return 1
    return 0


def _build_scenario(fault, poison):
    hits = 0
    for case in (_hand_build(), _big_build()[0]):
        try:
            case.check(*case.emulate(True, fault), str(fault))
        except AssertionError:
            hits += 1
    return hits


def _entries_scenario(fault, poison):
    hits = 0
    for lu in (False, True):
        for count in (1, 3 * 256 + 9):
            try:
                EntCase(lu, count, poison).run(_emu_entries(fault), str(fault))
            except AssertionError:
                hits += 1
    return hits


def _gather_scenario(fault, poison):
    count = GATHER_COUNTS[-1]
    im, pos = _gather_case(count, poison)
    im.start()
    kr.selpat_gather_emulate(pos, count, im["s"], im["out"], fault)
    try:
        _gather_check(im, pos, count, str(fault))
    except AssertionError:
        return 1
    return 0


FAULT_SCENARIOS = {"weight everywhere": (_part_scenario,), "dead entry read": (_part_scenario,), "tail lane dropped": (_part_scenario,),
                   "part0 ignored": (_part_scenario,), "stride is own tiles": (_part_scenario,), "column past m": (_part_scenario,),
                   "shift ignored": (_part_scenario,), "vmap ignored": (_part_scenario,), "first 256 parts": (_final_scenario,),
                   "32-bit product": (_build_scenario,), "diagonal row searched": (_build_scenario, _entries_scenario),
                   "offd inverted": (_build_scenario,), "no end guard": (_entries_scenario,), "triangle swapped": (_entries_scenario,),
                   "counter reset": (_entries_scenario,), "gather no stride": (_gather_scenario,)}


def test_every_fault_has_a_scenario():
    assert set(FAULT_SCENARIOS) == set(kr.SELPAT_FAULTS)


def test_clean_emulations_pass_every_scenario():
    for scenario in {s for v in FAULT_SCENARIOS.values() for s in v}:
        for poison in (NAN, 0.0):
            assert scenario(None, poison) == 0


@pytest.mark.parametrize("fault", kr.SELPAT_FAULTS)
def test_every_fault_is_rejected_somewhere(fault):
    for scenario in FAULT_SCENARIOS[fault]:
        assert scenario(fault, 0.0) >= 1, f"{fault}: not rejected without a NaN ({scenario.__name__})"
        assert scenario(fault, NAN) >= 1, f"{fault}: not rejected ({scenario.__name__})"
