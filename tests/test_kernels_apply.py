"""Single-launch tests of the kernels every entry point runs before and after the sweeps: the residual of validate (k_resid_*,
k_loadmap_drop: csrc/sf_kernels.hip), the refinement kernels (sf_refine.hip), the Gram, dot and quadratic-form reductions
(sf_gram.hip, sf_gram_lu.hip, sf_sample.hip), the normal generator (k_sample_fill) and the transfers of sf_device_io.hip, through the
launchers the plans call (sf_kernels.h) on operands the test builds itself.

Every double operand of a launch lies in ONE host image (kernel_ref.Arena): guard bands, padding and everything a launch must not
read hold NaN, everything outside the documented write set is compared bit for bit.  Reductions get integer inputs (|v| <= 8: every
partial sum is an exact double, the result must be exact) and inputs scaled over 1e-6 .. 1e6 checked per element against
SAFETY depth u sum |terms| (kernel_ref: the derivations of depth).  The CPU tests run numpy emulations of the launches through the same
checkers: the clean emulation passes, each single fault of kernel_ref.APPLY_FAULTS is rejected -- no kernel is ever made wrong.
"""
import ctypes as C

import numpy as np
import pytest

import kernel_ref as kr
import sample_ref
from test_kernels import _ok, P, kp  # noqa: F401
from util import sf, gen

W = kr.SVM_W
CAP = 1024 * 256                 # elements one pass of a capped launch covers (width 1)
OVER = CAP + 4321                # "above the cap": the launches stride
NAN = np.nan


@pytest.fixture(scope="module")
def ka(kp):
    vp, i64, i32, u64 = C.c_void_p, C.c_int64, C.c_int, C.c_uint64
    kp.kp_residual.argtypes = [vp, vp, i64, vp, vp, i64, i32, vp, i64, i64, i64, i64, i64, i64, i64, i64]
    kp.kp_loadmap_drop.argtypes = [vp, i64, vp, i64]
    kp.kp_refine_resid.argtypes = [vp, vp, vp, i64, i64, vp, i64, i64, i64, i64, i64, i64, i64, i32, i64]
    kp.kp_refine_norms.argtypes = [i64, vp, i64, i64, i64, i64, i64, i64, i32, i32]
    kp.kp_refine_update.argtypes = [i64, vp, i64, i64, i64, i64, i32]
    kp.kp_gram_slabs.argtypes = [i64, vp]
    kp.kp_gram_row.argtypes = [vp, i64, i64, i64, i32, i64, i64, i64, i64]
    kp.kp_gram2_col.argtypes = [vp, i64, i64, i64, i64, i32, i32, i64, i64, i64, i64, i64]
    kp.kp_dot.argtypes = [vp, i64, i64, i64, i64, i64, i64]
    kp.kp_quadform.argtypes = [vp, i64, i64, i64, i32, i64]
    kp.kp_sample_fill.argtypes = [vp, i64, i64, i64, i32, u64, u64]
    kp.kp_dev_load1.argtypes = [vp, i64, i64, vp, i64, i64]
    kp.kp_dev_store1.argtypes = [vp, i64, i64, vp, i64, i64]
    kp.kp_dev_pack.argtypes = [vp, i64, i64, i64, vp, i64, i32, i64]
    kp.kp_dev_unpack.argtypes = [vp, i64, i64, vp, i64, i32, i64, i64]
    kp.kp_dev_gather_values.argtypes = [vp, i64, i64, vp, i64, i64]
    kp.kp_dev_absmax.argtypes = [vp, i64, i64, i64, i64, vp]
    return kp


def _report(name, worst):
    print(f"APPLY_RATIO {name}: worst err / bound = {worst:.3g}")
    return worst


class Img:
    """named regions of one arena image; `written` collects the documented write set of the launch under test"""

    def __init__(self, **sizes):
        self.ar = kr.Arena()
        self.off = {k: self.ar.alloc(max(int(v), 1), align=2, skew=0) for k, v in sizes.items()}
        self.len = {k: int(v) for k, v in sizes.items()}
        self.a = self.ar.image()
        self.written = np.zeros(self.a.size, dtype=bool)

    def __getitem__(self, k):
        return self.a[self.off[k]:self.off[k] + self.len[k]]

    def __setitem__(self, k, v):
        self.a[self.off[k]:self.off[k] + self.len[k]] = v

    def writes(self, k, idx=None):
        m = self.written[self.off[k]:self.off[k] + self.len[k]]
        if idx is None:
            m[:] = True
        else:
            m[idx] = True

    def start(self):
        self.before = self.a.copy()
        return P(self.a), self.a.size

    def unchanged(self, what):
        kr.assert_unchanged(self.before, self.a, self.written, what)


def _rejects(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


# ---------------------------------------------------------------------------------------------------------------------
# launch_residual: k_resid_init, k_resid_cols, k_resid_urows, k_resid_norms
# ---------------------------------------------------------------------------------------------------------------------
def _resid_matrix(n, unsym, rng, integer=False):
    """L by column (diagonal first) and, unsymmetric, U by row (diagonal first, skipped by the kernel): columns / rows with 0, 1, 7
    and more than 27 off-diagonal entries; column 0 (n > 1: also the last) holds only its diagonal"""
    def tri():
        wants = np.array([0, 1, 7, 30])[np.arange(n) % 4]
        wants[[0, n - 1]] = 0
        own = np.repeat(np.arange(n), wants)
        step = rng.integers(1, 40, len(own))
        run = np.cumsum(step)
        first = (np.cumsum(wants) - wants)[wants > 0]
        other = own + run - np.repeat((run - step)[first], wants[wants > 0])     # strictly increasing inside a column, > the column
        keep = other < n
        j, i = np.concatenate([np.arange(n), own[keep]]), np.concatenate([np.arange(n), other[keep]])
        order = np.lexsort((i, j))
        return np.concatenate([[0], np.cumsum(np.bincount(j, minlength=n))]).astype(np.int64), i[order].astype(np.int32)
    Lp, Li = tri()
    Up, Ui = tri() if unsym else (None, None)
    def vals(cnt):
        if integer:
            return rng.integers(-8, 9, cnt).astype(np.float64)
        return rng.standard_normal(cnt)
    return Lp, Li, vals(len(Li)), Up, Ui, (vals(len(Ui)) if unsym else None)


def _resid_case(n, unsym, seed=0, scaled=True):
    rng = np.random.default_rng(seed + n)
    Lp, Li, Lx, Up, Ui, Ux = _resid_matrix(n, unsym, rng)
    x = rng.standard_normal(n)
    if scaled:
        s = kr.scalings(rng, n)
        Lx = Lx * s[Li] / s[np.repeat(np.arange(n), np.diff(Lp))]
        if unsym:
            Ux = Ux * s[np.repeat(np.arange(n), np.diff(Up))] / s[Ui]
        x = x * s
    return Lp, Li, Lx, Up, Ui, Ux, x


def _resid_launch(ka, n, Lp, Li, Lx, Up, Ui, Ux, x):
    im = Img(lx=len(Lx), ux=len(Ux) if Ux is not None else 1, x=n, r=n, c=n, b=n, norms=4)
    im["lx"], im["x"], im["norms"] = Lx, x, 0.0
    if Ux is not None:
        im["ux"] = Ux
        im["ux"][Up[:-1]] = NAN                     # U's own diagonal entries: the L part holds the diagonal, these are never read
    for k in ("r", "c", "b", "norms"):
        im.writes(k)
    buf, nbuf = im.start()
    _ok(ka.kp_residual(P(Lp), P(Li), len(Li), P(Up), P(Ui), len(Ui) if Ui is not None else 0, n, buf, nbuf, im.off["lx"], im.off["ux"],
                       im.off["x"], im.off["r"], im.off["c"], im.off["b"], im.off["norms"]))
    im.unchanged(f"residual n={n}")
    return im


def test_resid_norms_checker_rejects_the_nan_dropping_maximum():
    """the emulation of k_resid_norms through resid_norms_check: clean passes for finite and non-finite inputs; "nan dropped" -- fmax,
    the maximum of the kernel before it kept a NaN, the fault this change fixes -- is rejected, and so is a launch that never strides"""
    rng = np.random.default_rng(1)
    n = OVER
    r, c, x, b = rng.standard_normal(n), np.abs(rng.standard_normal(n)), rng.standard_normal(n), 1.0 + np.arange(n) / n
    res = kr.resid_norms_check(kr.resid_norms_emulate(r, c, x, b), r, c, x, b, "finite")
    assert np.isfinite(res)
    xb = x.copy(); xb[CAP + 7] = 50.0               # the largest |x| lies past the first pass
    _rejects(kr.resid_norms_check, kr.resid_norms_emulate(r, c, xb, b, "no stride"), r, c, xb, b, "no stride")
    for name, rr, xx in (("nan in x", r, np.where(np.arange(n) == 5, NAN, x)), ("x all nan", np.full(n, NAN), np.full(n, NAN)),
                         ("inf in x", np.where(np.arange(n) == 9, np.inf, r), np.where(np.arange(n) == 9, np.inf, x))):
        assert np.isnan(kr.resid_norms_check(kr.resid_norms_emulate(rr, c, xx, b), rr, c, xx, b, name))
        if "nan" in name:
            bad = kr.resid_norms_emulate(rr, c, xx, b, "nan dropped")
            _rejects(kr.resid_norms_check, bad, rr, c, xx, b, name)
    # the hole itself: with the parent's maximum an all-NaN x reports the residual 0.0
    bad = kr.resid_norms_emulate(np.full(n, NAN), c, np.full(n, NAN), b, "nan dropped")
    assert bad[0] / (bad[1] * bad[2] + bad[3]) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("unsym", [False, True], ids=["symmetric", "u_by_row"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, OVER])
def test_residual_launch(ka, n, unsym):
    """r, colsum per element, b bit for bit, norms[] = the maxima of the launch's own arrays and within the bound of the reference's"""
    Lp, Li, Lx, Up, Ui, Ux, x = _resid_case(n, unsym)
    im = _resid_launch(ka, n, Lp, Li, Lx, Up, Ui, Ux, x)
    ref = kr.resid_ref(n, Lp, Li, Lx, Up, Ui, Ux, x)
    _report(f"residual n={n} unsym={unsym}", kr.resid_check(ref, im["r"], im["c"], im["b"], f"residual n={n}"))
    res = kr.resid_norms_check(im["norms"], im["r"], im["c"], x, im["b"], f"residual n={n}")
    assert np.isfinite(res)
    bound = kr.SAFETY * (ref.cnt + 1) * kr.U * ref.mag
    assert abs(kr.LD(im["norms"][0]) - np.max(np.abs(ref.r))) <= np.max(bound)
    assert abs(kr.LD(im["norms"][1]) - np.max(ref.colsum)) <= np.max(kr.SAFETY * np.maximum(ref.ccnt, 1) * kr.U * ref.colsum)
    assert im["norms"][2] == np.max(np.abs(x)) and im["norms"][3] == np.max(ref.b)


@pytest.mark.gpu
@pytest.mark.parametrize("unsym", [False, True], ids=["symmetric", "u_by_row"])
@pytest.mark.parametrize("what", ["nan_in_x", "inf_in_x", "x_all_nan", "nan_value", "finite"])
def test_residual_launch_reports_non_finite(ka, what, unsym):
    """a non-finite x or matrix value makes the residual formed from norms[] NaN; the finite control stays within its bound"""
    n = 257
    Lp, Li, Lx, Up, Ui, Ux, x = _resid_case(n, unsym, seed=3, scaled=False)
    if what == "nan_in_x":
        x[100] = NAN
    elif what == "inf_in_x":
        x[101] = np.inf
    elif what == "x_all_nan":
        x[:] = NAN
    elif what == "nan_value":
        Lx[Lp[50]] = NAN
    im = _resid_launch(ka, n, Lp, Li, Lx, Up, Ui, Ux, x)
    nm = im["norms"]
    with np.errstate(invalid="ignore"):
        res = nm[0] / (nm[1] * nm[2] + nm[3])
    print(f"residual {what}: norms = {nm.tolist()} residual = {res}")
    if what == "finite":
        ref = kr.resid_ref(n, Lp, Li, Lx, Up, Ui, Ux, x)
        kr.resid_check(ref, im["r"], im["c"], im["b"], what)
        assert np.isfinite(kr.resid_norms_check(nm, im["r"], im["c"], x, im["b"], what))
    else:
        assert np.isnan(res), (what, nm.tolist())
        if what != "nan_value":
            assert np.isnan(kr.resid_norms_check(nm, im["r"], im["c"], x, im["b"], what))


@pytest.mark.gpu
def test_plan_refuses_a_nan_value_before_validate():
    """The suggested public route to a non-finite x -- an LU plan without pivoting (tolerance 0) and one NaN matrix value -- is refused:
    the NaN reaches a pivot and sf_lu_plan_factorize returns SF_ERR_NOT_POSDEF.  Only this route was tried (an overflowing solve,
    say, is not refused at factorize).  The test records the refusal and is no evidence for validate's rule: what validate does with
    a non-finite x is checked at the kernel level (test_residual_launch_reports_non_finite) and on the host validates
    (tests/test_validate_nonfinite.py)."""
    N = 6
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, extra_per_row=0, drop=0.2, seed=4)
    S = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N, 3, 2), 1 << 30, "lu", False)
    plan = sf.LUPlan(S, device=0)
    try:
        plan.set_values(S.Lx, S.Ux)
        plan.factorize()
        assert plan.validate() <= 1e-13
        Lx = np.array(S.Lx, dtype=np.float64)
        Lx[len(Lx) // 2] = NAN
        plan.set_values(Lx, S.Ux)
        with pytest.raises(sf.SparseFrameError, match="SF_ERR_NOT_POSDEF"):
            plan.factorize()
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# k_loadmap_drop, k_dev_gather_values, k_dev_absmax
# ---------------------------------------------------------------------------------------------------------------------
def _drop_case(count):
    rng = np.random.default_rng(count)
    nmap = 2 * count + 5
    m = rng.integers(0, 1 << 40, nmap).astype(np.int64)
    return rng.choice(nmap, count, replace=False).astype(np.int64), m


def test_loadmap_drop_emulation():
    drop, m = _drop_case(OVER)
    want = m.copy(); want[drop] = -1
    assert np.array_equal(kr.loadmap_drop_emulate(drop, m.copy()), want)
    assert not np.array_equal(kr.loadmap_drop_emulate(drop, m.copy(), "no stride"), want)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 257, OVER])
def test_loadmap_drop(ka, count):
    drop, m = _drop_case(count)
    want = m.copy(); want[drop] = -1
    _ok(ka.kp_loadmap_drop(P(drop), count, P(m), len(m)))
    assert np.array_equal(m, want)                   # the listed entries -1, everything else untouched


def _absmax_case():
    rng = np.random.default_rng(5)
    v = rng.standard_normal(OVER)
    v[CAP + 99] = -77.0                             # the maximum: negative, beyond the first pass of the stride
    v[1234] = NAN                                   # dropped, as documented
    return v


def test_absmax_emulation():
    v = _absmax_case()
    assert np.max(kr.absmax_emulate(v)) == 77.0
    assert np.max(kr.absmax_emulate(v, "no stride")) != 77.0


@pytest.mark.gpu
def test_dev_absmax(ka):
    v = _absmax_case()
    im = Img(v=len(v), part=1024 + 3)
    im["v"] = v
    nparts = C.c_int(-1)
    im.writes("part", np.arange(1024))
    buf, nbuf = im.start()
    _ok(ka.kp_dev_absmax(buf, nbuf, im.off["v"], len(v), im.off["part"], C.byref(nparts)))
    im.unchanged("absmax")
    assert nparts.value == 1024
    kr.assert_bits(im["part"][:1024], kr.absmax_emulate(v), "absmax parts")
    assert np.max(im["part"][:1024]) == 77.0


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 257, 1000])
def test_dev_gather_values(ka, count):
    rng = np.random.default_rng(count)
    nsrc = count // 2 + 3
    m = rng.integers(-1, nsrc - 1, count).astype(np.int64)       # -1 entries give 0.0; sources repeat; the last source is never read
    m[0] = -1
    im = Img(ax=nsrc, out=count + 3)
    im["ax"][:nsrc - 1] = rng.standard_normal(nsrc - 1)
    im.writes("out", np.arange(count))
    buf, nbuf = im.start()
    _ok(ka.kp_dev_gather_values(buf, nbuf, im.off["ax"], P(m), count, im.off["out"]))
    im.unchanged("gather_values")
    kr.assert_bits(im["out"][:count], kr.gather_values_emulate(im["ax"], m, np.empty(count)), "gather_values")


# ---------------------------------------------------------------------------------------------------------------------
# refinement: k_refine_resid<false / true>, k_refine_norms, k_refine_update
# ---------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 7, 8, 9, 16, 17, 100)          # brackets RF_G = 8


def _form(n, seed=0, shift=0, scaled=True):
    """a row form over n rows with the lengths above in turn; every entry's value sits in a slot of its own in Vd (pos >= 0) or Vt
    (~pos), followed by a slot no position names -- a superseded duplicate, left out of the form -- which holds NaN.
    shift: rotates the lengths (shift = 2: rows 0, 8, 256 have 7 entries, row 7 has 1)."""
    rng = np.random.default_rng(seed + n)
    lens = np.array([ROW_LENGTHS[(i + shift) % len(ROW_LENGTHS)] for i in range(n)])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nent = int(ptr[-1])
    col = rng.integers(0, n, max(nent, 1)).astype(np.int32)
    direct = rng.random(nent) < 0.5
    slot = 2 * rng.permutation(nent)
    Vd, Vt = np.full(2 * nent + 2, NAN), np.full(2 * nent + 2, NAN)
    s = kr.scalings(rng, n) if scaled else np.ones(n)
    rows = np.repeat(np.arange(n), lens)
    vals = rng.standard_normal(nent) * s[rows] / s[col[:nent]]
    Vd[slot[direct]], Vt[slot[~direct]] = vals[direct], vals[~direct]
    pos = np.where(direct, slot, ~slot).astype(np.int64)
    if nent == 0:
        pos = np.zeros(1, dtype=np.int64)
    x, b = rng.standard_normal(n) * s, rng.standard_normal(n) * s
    return ptr, col, pos, nent, Vd, Vt, x, b


@pytest.mark.parametrize("n", [9, 33])
def test_refine_checker_on_emulations(n):
    ptr, col, pos, nent, Vd, Vt, x, b = _form(n)
    ref = kr.refine_ref(ptr, col, pos[:nent], Vd, Vt, x, b)
    kr.refine_check(ref, *kr.refine_emulate(ptr, col, pos, Vd, Vt, x, b), "clean")
    for fault in ("duplicate summed", "pos from direct"):
        _rejects(kr.refine_check, ref, *kr.refine_emulate(ptr, col, pos, Vd, Vt, x, b, fault), fault)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 257])
def test_refine_resid(ka, n):
    ptr, col, pos, nent, Vd, Vt, x, b = _form(n)
    im = Img(vd=len(Vd), vt=len(Vt), x=n, b=n, r=n + 3, w=n + 3)
    im["vd"], im["vt"], im["x"], im["b"] = Vd, Vt, x, b
    im.writes("r", np.arange(n)); im.writes("w", np.arange(n))
    buf, nbuf = im.start()
    _ok(ka.kp_refine_resid(P(ptr), P(col), P(pos), nent, n, buf, nbuf, im.off["vd"], im.off["vt"], im.off["x"], im.off["b"], im.off["r"],
                           im.off["w"], 0, 0))
    im.unchanged(f"refine_resid n={n}")
    ref = kr.refine_ref(ptr, col, pos[:nent], Vd, Vt, x, b)
    _report(f"refine_resid n={n}", kr.refine_check(ref, im["r"][:n], im["w"][:n], f"refine_resid n={n}"))


@pytest.mark.gpu
@pytest.mark.parametrize("peak", [0, 256, 7, 8], ids=["first", "last", "end_of_a_wave", "start_of_a_wave"])
def test_refine_abs_sums(ka, peak):
    """*amax = the largest row sum of |a|: the row that holds it first, last, and on both sides of a wave boundary (8 rows per wave)"""
    n = 257
    ptr, col, pos, nent, Vd, Vt, x, b = _form(n, seed=1, shift=2, scaled=False)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    assert ptr[peak + 1] > ptr[peak]
    for V, sel in ((Vd, pos[:nent] >= 0), (Vt, pos[:nent] < 0)):
        idx = np.where(sel, pos[:nent], ~pos[:nent])[sel & (rows == peak)]
        V[idx] *= 1e4                               # unscaled N(0, 1) values, 100 at most in a row: the largest sum by far
    im = Img(vd=len(Vd), vt=len(Vt), amax=1)
    im["vd"], im["vt"], im["amax"] = Vd, Vt, 0.0
    im.writes("amax")
    buf, nbuf = im.start()
    _ok(ka.kp_refine_resid(P(ptr), P(col), P(pos), nent, n, buf, nbuf, im.off["vd"], im.off["vt"], 0, 0, 0, 0, 1, im.off["amax"]))
    im.unchanged("abs_sums")
    _, _, sums, depth = kr.refine_ref(ptr, col, pos[:nent], Vd, Vt, x, b)
    assert int(np.argmax(sums)) == peak
    _report(f"abs_sums peak={peak}", kr.within_ratio(im["amax"], sums[peak:peak + 1], kr.SAFETY * depth[peak] * kr.U * sums[peak:peak + 1], "abs_sums"))


def _norms_inputs(n, seed=0):
    rng = np.random.default_rng(seed + n)
    r, x, b = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    w = np.abs(rng.standard_normal(n)) + 0.5
    return r, w, x, b


def _norms_launch(ka, n, r, w, x, b, info, use_info=1, s0=0.0):
    im = Img(r=n, w=n, x=n, b=n, s=5)
    im["r"], im["w"], im["x"], im["b"], im["s"] = r, w, x, b, s0
    im.writes("s")
    buf, nbuf = im.start()
    _ok(ka.kp_refine_norms(n, buf, nbuf, im.off["r"], im.off["w"], im.off["x"], im.off["b"], im.off["s"], use_info, info))
    im.unchanged("refine_norms")
    return im["s"][:4].copy(), int(im["s"][4:5].view(np.uint64)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257, OVER])
def test_refine_norms(ka, n):
    """the four maxima bit for bit (maxima do not round; the quotient r_i / w_i is one correctly rounded division), rows with
    w_i = 0 skipped for berr, the largest entries beyond the first pass of the stride"""
    r, w, x, b = _norms_inputs(n)
    w[::3] = 0.0
    r[0] = 1e3                                      # the largest r_i / w_i candidate sits on a skipped row
    if n > CAP:
        r[CAP + 5], x[CAP + 6], b[CAP + 7] = -40.0, 41.0, -42.0
    got, flags = _norms_launch(ka, n, r, w, x, b, 0)
    want, wflags = kr.refine_norms_ref(r, w, x, b, 0)
    kr.assert_bits(got, want, f"refine_norms n={n}")
    assert flags == wflags == 0
    kr.assert_bits(got, kr.refine_norms_emulate(r, w, x, b, 0, (np.zeros(4), 0))[0], "the emulation's words")


@pytest.mark.gpu
def test_refine_norms_flags_and_zero_r(ka):
    n = 257
    r, w, x, b = _norms_inputs(n)
    # an all-zero r leaves berr and |r|_inf untouched: non-zero sentinels in the two words survive bit for bit (a store of 0.0 or of
    # anything else would show), the other two maxima are taken as usual, the flag word stays 0
    sentinel = np.array([3e-300, 7e-300, 0.0, 0.0, 0.0])
    got, flags = _norms_launch(ka, n, np.zeros(n), w, x, b, 0, use_info=0, s0=sentinel)
    kr.assert_bits(got[:2], sentinel[:2], "the words of an all-zero r")
    kr.assert_bits(got[2:], [np.max(np.abs(x)), np.max(np.abs(b))], "|x|_inf and |b|_inf beside an all-zero r")
    assert flags == 0
    emu, eflags = kr.refine_norms_emulate(np.zeros(n), w, x, b, 0, (sentinel[:4], 0))
    kr.assert_bits(got, emu, "the emulation's words")
    assert eflags == 0
    for k, bad in enumerate((NAN, np.inf, -np.inf)):
        for which in range(3):
            arrs = [r.copy(), x.copy(), b.copy()]
            arrs[which][(64 * k + 7) % n] = bad
            got, flags = _norms_launch(ka, n, arrs[0], w, arrs[1], arrs[2], 0)
            assert flags == 1, (which, bad, flags)
    got, flags = _norms_launch(ka, n, r, w, x, b, 5)
    assert flags == 2
    x2 = x.copy(); x2[200] = NAN
    assert _norms_launch(ka, n, r, w, x2, b, 1)[1] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("save", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_refine_update(ka, n, save):
    rng = np.random.default_rng(n)
    x, d = rng.standard_normal(n) * kr.scalings(rng, n), rng.standard_normal(n)
    im = Img(x=n + 3, d=n, best=n + 3)
    im["x"][:n], im["d"] = x, d
    im.writes("x", np.arange(n))
    if save:
        im.writes("best", np.arange(n))             # save == 0: best is untouched (all of it stays NaN)
    buf, nbuf = im.start()
    _ok(ka.kp_refine_update(n, buf, nbuf, im.off["x"], im.off["d"], im.off["best"], save))
    im.unchanged(f"refine_update n={n} save={save}")
    kr.assert_bits(im["x"][:n], x + d, "x + d")
    if save:
        kr.assert_bits(im["best"][:n], x, "best")


# ---------------------------------------------------------------------------------------------------------------------
# launch_dot, launch_quadform
# ---------------------------------------------------------------------------------------------------------------------
def _sum_inputs(n, Wd, integer, seed=0):
    rng = np.random.default_rng(seed + n + Wd)
    if integer:
        return rng.integers(-8, 9, (n, Wd)).astype(np.float64), rng.integers(-8, 9, (n, Wd)).astype(np.float64)
    s = kr.scalings(rng, n)[:, None]
    return rng.standard_normal((n, Wd)) * s, rng.standard_normal((n, Wd)) / s


@pytest.mark.parametrize("Wd", [1, 16])
def test_two_pass_sum_checker_on_emulations(Wd):
    n = (OVER if Wd == 1 else 16384 + 77)
    for integer in (True, False):
        X, _ = _sum_inputs(n, Wd, integer)
        kr.sum_check(kr.two_pass_sum(X * X, Wd), X * X, Wd, "clean")
        if integer:
            assert np.array_equal(kr.two_pass_sum(X * X, Wd), (X * X).sum(axis=0))
        _rejects(kr.sum_check, kr.two_pass_sum(X * X, Wd, "no stride"), X * X, Wd, "no stride")


@pytest.mark.gpu
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "scaled"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, OVER])
def test_dot(ka, n, integer):
    x, y = _sum_inputs(n, 1, integer)
    im = Img(x=n, y=n, scratch=1024 + 1 + 2)        # the result follows the parts
    im["x"], im["y"] = x[:, 0], y[:, 0]
    nb = min(1024, -(-n // 256))
    im.writes("scratch", np.r_[np.arange(nb), 1024])
    outs = []
    for _ in range(2):
        buf, nbuf = im.start()
        _ok(ka.kp_dot(buf, nbuf, im.off["x"], im.off["y"], n, im.off["scratch"], im.off["scratch"] + 1024))
        im.unchanged(f"dot n={n}")
        outs.append(im["scratch"][1024:1025].copy())
    kr.assert_bits(outs[1], outs[0], "two calls")
    if integer:
        assert outs[0][0] == float((x * y).sum())
    _report(f"dot n={n} integer={integer}", kr.sum_check(outs[0], x * y, 1, f"dot n={n}"))


@pytest.mark.gpu
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "scaled"])
@pytest.mark.parametrize("n,Wd", [(1, 1), (255, 1), (256, 1), (257, 1), (OVER, 1), (1, 16), (255, 16), (256, 16), (257, 16), (16384 + 77, 16)])
def test_quadform(ka, n, Wd, integer):
    X, _ = _sum_inputs(n, Wd, integer)
    im = Img(x=n * Wd, scratch=1024 * Wd + Wd + 2)
    im["x"] = X.ravel()
    nb = min(1024, -(-n // (256 // Wd)))
    im.writes("scratch", np.r_[np.arange(nb * Wd), 1024 * Wd + np.arange(Wd)])
    outs = []
    for _ in range(2):
        buf, nbuf = im.start()
        _ok(ka.kp_quadform(buf, nbuf, im.off["x"], n, Wd, im.off["scratch"]))
        im.unchanged(f"quadform n={n}")
        outs.append(im["scratch"][1024 * Wd:1024 * Wd + Wd].copy())
    kr.assert_bits(outs[1], outs[0], "two calls")
    if integer:
        assert np.array_equal(outs[0], (X * X).sum(axis=0))
    _report(f"quadform n={n} W={Wd} integer={integer}", kr.sum_check(outs[0], X * X, Wd, f"quadform n={n} W={Wd}"))
    if Wd == 16:                                     # a NaN stays in its column
        im["x"][min(n - 1, 200) * Wd + 5] = NAN
        buf, nbuf = im.start()
        _ok(ka.kp_quadform(buf, nbuf, im.off["x"], n, Wd, im.off["scratch"]))
        out = im["scratch"][1024 * Wd:1024 * Wd + Wd]
        assert np.isnan(out[5]) and np.all(bits_eq(np.delete(out, 5), np.delete(outs[0], 5)))


def bits_eq(a, b):
    return kr.bits(np.ascontiguousarray(a)) == kr.bits(np.ascontiguousarray(b))


# ---------------------------------------------------------------------------------------------------------------------
# gram_slabs, launch_gram_row, launch_gram2_col
# ---------------------------------------------------------------------------------------------------------------------
GRAM_SMALL = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65)
GRAM_LARGE = (2047, 2049, 4099)
GRAM_HUGE = 524288 + 64 * 256 + 5                  # slab_rows = 2176 > 2048, 249 slabs


def _slab_rule(n, ns, rows):
    assert 1 <= ns <= 256 and rows % 64 == 0 and (ns - 1) * rows < n <= ns * rows, (n, ns, rows)


def test_gram_slabs_rule():
    rng = np.random.default_rng(0)
    for n in list(GRAM_SMALL) + list(GRAM_LARGE) + [GRAM_HUGE, 524288, 524289, 1 << 22] + rng.integers(1, 1 << 23, 300).tolist():
        _slab_rule(n, *kr.gram_slabs(int(n)))
    assert kr.gram_slabs(GRAM_HUGE)[1] > 2048 and kr.gram_slabs(2049)[0] == 2 and kr.gram_slabs(2047)[0] == 1


@pytest.mark.gpu
def test_gram_slabs_of_the_library(ka):
    rng = np.random.default_rng(0)
    for n in list(GRAM_SMALL) + list(GRAM_LARGE) + [GRAM_HUGE, 524288, 524289] + rng.integers(1, 1 << 23, 300).tolist():
        rows = C.c_int64()
        ns = ka.kp_gram_slabs(int(n), C.byref(rows))
        _slab_rule(n, ns, rows.value)
        assert (ns, rows.value) == kr.gram_slabs(int(n))


def _gram_chunks(n, nch, integer, seed):
    rng = np.random.default_rng(seed + n)
    if integer:
        return [rng.integers(-8, 9, (n, W)).astype(np.float64) for _ in range(nch)]
    s = kr.scalings(rng, nch * W).reshape(nch, 1, W)
    return [rng.standard_normal((n, W)) * s[c] for c in range(nch)]


def _gram_view(flat, ldg, ncols):
    """the column-major block as a [row, column] view with the padding rows of the leading dimension"""
    return flat[:ldg * ncols].reshape(ncols, ldg).T


@pytest.mark.parametrize("n", [5, 17, 65, 2049, 4099])
def test_gram_checker_on_emulations(n):
    a, k = 1, 2 * W - 1
    Y = _gram_chunks(n, 2, False, 0)
    ldg = k + 3
    def run(fault):
        G0 = np.full((ldg, k), NAN)
        G1 = kr.gram_row_emulate(Y, n, a, k, G0.copy(), fault)
        return kr.gram_check(G0, G1, Y, Y, n, [a], lambda a_: range(a_ + 1), k, k, True, f"gram {fault}")
    run(None)
    faults = ["no mirror", "padding written", "wave offset"] + (["dropped tail group"] if n % 4 else []) + (["slab overlap"] if n > 2048 else [])
    for fault in faults:
        _rejects(run, fault)
    Z = _gram_chunks(n, 2, False, 9)
    m = W + 3
    def run2(fault):
        G0 = np.full((m + 2, k), NAN)
        G1 = kr.gram2_col_emulate(Z, Y[1], n, 1, m, k, G0.copy(), fault)
        return kr.gram_check(G0, G1, Z, Y, n, [0, 1], lambda a_: [1], m, k, False, f"gram2 {fault}")
    run2(None)
    for fault in ["padding written", "wave offset"] + (["dropped tail group"] if n % 4 else []) + (["slab overlap"] if n > 2048 else []):
        _rejects(run2, fault)


def _gram_row_launch(ka, Y, n, a, k, ldg):
    ns, _ = kr.gram_slabs(n)
    nch = a + 1
    im = Img(y=nch * n * W, part=nch * ns * 256, g=ldg * k)
    for c in range(nch):
        im["y"][c * n * W:(c + 1) * n * W] = Y[c].ravel()
    im.writes("part")
    gw = np.zeros((ldg, k), dtype=bool)
    lo, hi = a * W, min(k, (a + 1) * W)
    gw[lo:hi, :hi] = True
    gw[:hi, lo:hi] = True
    im.writes("g", np.flatnonzero(gw.T.ravel()))
    buf, nbuf = im.start()
    _ok(ka.kp_gram_row(buf, nbuf, im.off["y"], n, a, k, im.off["part"], im.off["g"], ldg))
    im.unchanged(f"gram_row n={n} a={a} k={k}")
    return im


@pytest.mark.gpu
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "scaled"])
@pytest.mark.parametrize("n", GRAM_SMALL + GRAM_LARGE)
def test_gram_row(ka, n, integer):
    """chunk rows a = 0, 1, 2 with 1, 15 and 16 live columns in the last chunk, ldg > k; mirrors bit for bit; a NaN column"""
    worst = 0.0
    for a, live in ((0, 1), (1, 15), (2, 16)) if n in (5, 65, 2049) else ((1, 15),):
        k = a * W + live
        ldg = k + 3
        Y = _gram_chunks(n, a + 1, integer, a)
        im = _gram_row_launch(ka, Y, n, a, k, ldg)
        G1, G0 = _gram_view(im["g"], ldg, k), _gram_view(im.before[im.off["g"]:im.off["g"] + ldg * k], ldg, k)
        worst = max(worst, kr.gram_check(G0, G1, Y, Y, n, [a], lambda a_: range(a_ + 1), k, k, True, f"gram_row n={n} a={a}"))
        if integer:
            full = np.concatenate(Y, axis=1)[:, :k]
            assert np.array_equal(G1[a * W:k, :k], (full[:, a * W:k].T @ full))
    _report(f"gram_row n={n} integer={integer}", worst)


@pytest.mark.gpu
def test_gram_row_nan_column(ka):
    """a NaN in one column of Y reaches exactly that row and column of the written part of G"""
    n, a, k = 65, 1, 2 * W - 1
    Y = _gram_chunks(n, 2, False, 3)
    clean = _gram_view(_gram_row_launch(ka, Y, n, a, k, k)["g"], k, k).copy()
    Y[0][40, 3] = NAN
    G = _gram_view(_gram_row_launch(ka, Y, n, a, k, k)["g"], k, k)
    hit = np.zeros((k, k), dtype=bool)
    hit[3, W:] = hit[W:, 3] = True
    assert np.all(np.isnan(G[hit])) and np.all(bits_eq(G[~hit & ~np.isnan(clean)], clean[~hit & ~np.isnan(clean)]))
    assert np.array_equal(np.isnan(G) & ~hit, np.isnan(clean))


@pytest.mark.gpu
def test_gram_row_above_the_slab_cap(ka):
    """n above 524,288: the slab count is capped and a slab has more than 2048 rows; integer inputs, the result exact"""
    n = GRAM_HUGE
    Y = _gram_chunks(n, 1, True, 0)
    im = _gram_row_launch(ka, Y, n, 0, W, W)
    G = _gram_view(im["g"], W, W)
    want = Y[0].astype(np.int64).T @ Y[0].astype(np.int64)
    assert np.array_equal(G, want.astype(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("integer", [True, False], ids=["integer", "scaled"])
@pytest.mark.parametrize("n", GRAM_SMALL + GRAM_LARGE)
def test_gram2_col(ka, n, integer):
    """Z^T Y_b, b = 1, m and k ragged independently, nothing mirrored; then a NaN column of Z reaches its row of G only"""
    nza, b, m, k = 2, 1, W + 5, 2 * W - 2
    ldg = m + 3
    Z, Yb = _gram_chunks(n, nza, integer, 1), _gram_chunks(n, 1, integer, 2)[0]
    ns, _ = kr.gram_slabs(n)
    im = Img(z=nza * n * W, yb=n * W, part=nza * ns * 256, g=ldg * k)
    for c in range(nza):
        im["z"][c * n * W:(c + 1) * n * W] = Z[c].ravel()
    im["yb"] = Yb.ravel()
    im.writes("part")
    gw = np.zeros((ldg, k), dtype=bool)
    gw[:m, b * W:k] = True
    im.writes("g", np.flatnonzero(gw.T.ravel()))
    buf, nbuf = im.start()
    _ok(ka.kp_gram2_col(buf, nbuf, im.off["z"], im.off["yb"], n, nza, b, m, k, im.off["part"], im.off["g"], ldg))
    im.unchanged(f"gram2_col n={n}")
    G1, G0 = _gram_view(im["g"], ldg, k), _gram_view(im.before[im.off["g"]:im.off["g"] + ldg * k], ldg, k)
    _report(f"gram2_col n={n} integer={integer}",
            kr.gram_check(G0, G1, Z, {b: Yb}, n, range(nza), lambda a_: [b], m, k, False, f"gram2_col n={n}"))
    if integer:
        assert np.array_equal(G1[:m, b * W:k], (np.concatenate(Z, axis=1)[:, :m].T @ Yb[:, :k - b * W]))
    clean = G1.copy()
    im["z"][(n // 2) * W + 4] = NAN
    buf, nbuf = im.start()
    _ok(ka.kp_gram2_col(buf, nbuf, im.off["z"], im.off["yb"], n, nza, b, m, k, im.off["part"], im.off["g"], ldg))
    G = _gram_view(im["g"], ldg, k)
    assert np.all(np.isnan(G[4, b * W:k])) and np.all(bits_eq(np.delete(G[:m, b * W:k], 4, axis=0), np.delete(clean[:m, b * W:k], 4, axis=0)))


@pytest.mark.gpu
def test_gram2_col_above_the_slab_cap(ka):
    """launch_gram2_col at n above 524,288 (nza = 1, b = 1): k_gram2_part over 249 slabs of 2176 rows with two different operands,
    k_gram2_final over 249 parts; integer inputs, the result exact; m and k ragged; the footprint as everywhere"""
    n, nza, b, m, k = GRAM_HUGE, 1, 1, W - 3, 2 * W - 5
    ldg = m + 2
    ns, rows = kr.gram_slabs(n)
    assert ns == 249 and rows == 2176
    Z, Yb = _gram_chunks(n, 1, True, 4)[0], _gram_chunks(n, 1, True, 5)[0]
    im = Img(z=n * W, yb=n * W, part=nza * ns * 256, g=ldg * k)
    im["z"], im["yb"] = Z.ravel(), Yb.ravel()
    im.writes("part")
    gw = np.zeros((ldg, k), dtype=bool)
    gw[:m, b * W:k] = True
    im.writes("g", np.flatnonzero(gw.T.ravel()))
    buf, nbuf = im.start()
    _ok(ka.kp_gram2_col(buf, nbuf, im.off["z"], im.off["yb"], n, nza, b, m, k, im.off["part"], im.off["g"], ldg))
    im.unchanged("gram2_col above the slab cap")
    G = _gram_view(im["g"], ldg, k)
    want = Z.astype(np.int64)[:, :m].T @ Yb.astype(np.int64)[:, :k - b * W]
    assert np.array_equal(G[:m, b * W:k], want.astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# k_sample_fill
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed,s0", [(5, 0), (5, 7), ((0xFEDCBA98 << 32) | 0x80000001, (1 << 34) + 6), (0xFFFFFFFFFFFFFFFF, (3 << 33) + 1)])
@pytest.mark.parametrize("n", [1, 31, 33])
def test_sample_fill(ka, n, seed, s0):
    """the block against sample_ref.normals for cw in {1, 2, 15, 16}: s0 even and odd, a pair index with a high word, seeds with high
    bits; columns >= cw exactly 0.0; nothing past row n written.  1e-13: the tolerance of tests/test_sample.py for the same
    transcendental chain (device and numpy log / cos / sin / sqrt each within about 1e-14 for |z| <= 8.6)"""
    for cw in (1, 2, 15, 16):
        im = Img(x=n * W + 5)
        im.writes("x", np.arange(n * W))
        buf, nbuf = im.start()
        _ok(ka.kp_sample_fill(buf, nbuf, im.off["x"], n, cw, seed, s0))
        im.unchanged(f"sample_fill n={n} cw={cw}")
        X = im["x"][:n * W].reshape(n, W)
        want = sample_ref.normals(seed, n, s0, cw)
        err = float(np.max(np.abs(X[:, :cw] - want)))
        print(f"sample_fill n={n} cw={cw} s0={s0}: max |X - reference| = {err:.3e}")
        assert np.all(np.isfinite(X)) and err <= 1e-13
        assert np.all(kr.bits(np.ascontiguousarray(X[:, cw:])) == 0)


# ---------------------------------------------------------------------------------------------------------------------
# the transfers: k_dev_load1, k_dev_store1, k_dev_pack, k_dev_unpack, each with and without PERM
# ---------------------------------------------------------------------------------------------------------------------
PERMS = ("none", "identity", "reversal", "random")
XFER_N = (1, 63, 64, 65, 257)


def _perm(kind, n):
    if kind == "none":
        return None
    if kind == "identity":
        return np.arange(n, dtype=np.int32)
    if kind == "reversal":
        return np.arange(n, dtype=np.int32)[::-1].copy()
    return np.random.default_rng(n).permutation(n).astype(np.int32)


def test_transfer_emulations_and_faults():
    n, cw = 65, 5
    rng = np.random.default_rng(0)
    perm = _perm("random", n)
    ld = n + 3
    B = rng.standard_normal(ld * cw)
    x = kr.load1_emulate(B, perm, n, np.full(n, NAN))
    assert np.array_equal(x, B[perm]) and not np.array_equal(kr.load1_emulate(B, perm, n, np.full(n, NAN), "inverse perm"), x)
    back = kr.store1_emulate(x, perm, n, np.full(n, NAN))
    assert np.array_equal(back, B[:n]) and not np.array_equal(kr.store1_emulate(x, perm, n, np.full(n, NAN), "inverse perm"), back)
    X = kr.pack_emulate(B, ld, perm, n, cw, np.full(n * W + 2, NAN))
    want = np.zeros((n, W)); want[:, :cw] = B[:ld * cw].reshape(cw, ld).T[perm]
    assert np.array_equal(X[:n * W], want.ravel()) and np.all(np.isnan(X[n * W:]))
    for fault in ("inverse perm", "ld is n", "padding written"):
        assert not np.array_equal(kr.pack_emulate(B, ld, perm, n, cw, np.full(n * W + 2, NAN), fault)[:n * W], want.ravel()), fault
    D = kr.unpack_emulate(X, perm, n, cw, np.full(ld * (cw + 1), NAN), ld)
    assert np.array_equal(D[:ld * cw].reshape(cw, ld)[:, :n], B.reshape(cw, ld)[:, :n])
    assert np.all(np.isnan(D[:ld * cw].reshape(cw, ld)[:, n:])) and np.all(np.isnan(D[ld * cw:]))
    for fault in ("inverse perm", "ld is n", "padding written"):
        assert not np.array_equal(kr.bits(kr.unpack_emulate(X, perm, n, cw, np.full(ld * (cw + 1), NAN), ld, fault)), kr.bits(D)), fault


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PERMS)
@pytest.mark.parametrize("n", XFER_N)
def test_dev_load1_store1(ka, n, kind):
    perm = _perm(kind, n)
    B = np.random.default_rng(n).standard_normal(n)
    im = Img(b=n, x=n + 3, back=n + 3)
    im["b"] = B
    im.writes("x", np.arange(n))
    buf, nbuf = im.start()
    _ok(ka.kp_dev_load1(buf, nbuf, im.off["b"], P(perm), n, im.off["x"]))
    im.unchanged("load1")
    kr.assert_bits(im["x"][:n], kr.load1_emulate(B, perm, n, np.empty(n)), "load1")
    im.writes("back", np.arange(n))
    buf, nbuf = im.start()
    _ok(ka.kp_dev_store1(buf, nbuf, im.off["x"], P(perm), n, im.off["back"]))
    im.unchanged("store1")
    kr.assert_bits(im["back"][:n], B, "store1 after load1 is the identity")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PERMS)
@pytest.mark.parametrize("n", XFER_N)
def test_dev_pack_unpack(ka, n, kind):
    perm = _perm(kind, n)
    rng = np.random.default_rng(n)
    for cw in (1, 5, 16):
        for ld in (n, n + 3):
            im = Img(b=ld * cw, x=n * W + 3, d=ld * cw + 3)
            blk = rng.standard_normal((cw, ld))
            blk[:, n:] = NAN                         # the padding rows of the leading dimension are never read
            im["b"] = blk.ravel()
            im.writes("x", np.arange(n * W))
            buf, nbuf = im.start()
            _ok(ka.kp_dev_pack(buf, nbuf, im.off["b"], ld, P(perm), n, cw, im.off["x"]))
            im.unchanged(f"pack n={n} cw={cw} ld={ld}")
            kr.assert_bits(im["x"][:n * W], kr.pack_emulate(blk.ravel(), ld, perm, n, cw, np.empty(n * W)), f"pack n={n} cw={cw} ld={ld}")
            assert np.all(kr.bits(np.ascontiguousarray(im["x"][:n * W].reshape(n, W)[:, cw:])) == 0)
            dm = np.zeros((cw, ld), dtype=bool)
            dm[:, :n] = True
            im.writes("d", np.flatnonzero(dm.ravel()))
            if cw < W:
                im["x"][:n * W].reshape(n, W)[:, cw:] = NAN      # columns >= cw of the block are not read on the way back
            buf, nbuf = im.start()
            _ok(ka.kp_dev_unpack(buf, nbuf, im.off["x"], P(perm), n, cw, im.off["d"], ld))
            im.unchanged(f"unpack n={n} cw={cw} ld={ld}")
            kr.assert_bits(im["d"][:ld * cw].reshape(cw, ld)[:, :n], blk[:, :n], "unpack after pack is the identity")


# ---------------------------------------------------------------------------------------------------------------------
# every fault of kernel_ref.APPLY_FAULTS, by name: the emulation with that one fault goes through the checker the GPU test of the
# same launch uses and must be rejected (the clean emulation of each passes first)
# ---------------------------------------------------------------------------------------------------------------------
def _gram_scenario(fault):
    n, a, k = 4099, 1, 2 * W - 1                    # two slabs, a ragged tail group, an off-diagonal tile, padding rows
    Y = _gram_chunks(n, 2, False, 0)
    G0 = np.full((k + 3, k), NAN)
    G1 = kr.gram_row_emulate(Y, n, a, k, G0.copy(), fault)
    kr.gram_check(G0, G1, Y, Y, n, [a], lambda a_: range(a_ + 1), k, k, True, f"gram {fault}")


def _pack_scenario(fault):
    n, cw, ld = 65, 5, 68
    perm = _perm("random", n)
    B = np.random.default_rng(0).standard_normal(ld * cw)
    want = np.zeros((n, W)); want[:, :cw] = B.reshape(cw, ld).T[perm]
    kr.assert_bits(kr.pack_emulate(B, ld, perm, n, cw, np.empty(n * W), fault), want.ravel(), f"pack {fault}")


def _sum_scenario(fault):
    X, _ = _sum_inputs(OVER, 1, True)
    kr.sum_check(kr.two_pass_sum(X * X, 1, fault), X * X, 1, f"quadform {fault}")
    r, w, x, b = _norms_inputs(OVER)
    x[CAP + 6] = 41.0
    got, flags = kr.refine_norms_emulate(r, w, x, b, 0, (np.zeros(4), 0), fault)
    kr.assert_bits(got, kr.refine_norms_ref(r, w, x, b, 0)[0], f"refine_norms {fault}")


def _refine_scenario(fault):
    ptr, col, pos, nent, Vd, Vt, x, b = _form(33)
    kr.refine_check(kr.refine_ref(ptr, col, pos[:nent], Vd, Vt, x, b), *kr.refine_emulate(ptr, col, pos, Vd, Vt, x, b, fault), f"refine {fault}")


def _resid_norms_scenario(fault):
    n = 300
    r, c, x, b = _norms_inputs(n)
    x[7] = NAN
    kr.resid_norms_check(kr.resid_norms_emulate(r, np.abs(c), x, b, fault), r, np.abs(c), x, b, f"resid_norms {fault}")


def _gather_scenario(fault):
    Ax = np.array([1.0, 2.0, 3.0, NAN])             # the last source is never named: -1 used as an index reads it
    m = np.array([-1, 2, 0, 0, -1, 1])
    kr.assert_bits(kr.gather_values_emulate(Ax, m, np.full(6, NAN), fault), [0.0, 3.0, 1.0, 1.0, 0.0, 2.0], f"gather_values {fault}")


def _update_scenario(fault):
    x, d, best = np.arange(5.0), np.ones(5), np.full(5, NAN)
    before = best.copy()
    x1, best1 = kr.refine_update_emulate(x.copy(), d, best, 0, fault)
    kr.assert_bits(x1, x + d, f"update {fault}")
    kr.assert_unchanged(before, best1, np.zeros(5, dtype=bool), f"update {fault}")


FAULT_SCENARIOS = {"dropped tail group": _gram_scenario, "slab overlap": _gram_scenario, "wave offset": _gram_scenario, "no mirror": _gram_scenario,
                   "padding written": _gram_scenario, "inverse perm": _pack_scenario, "ld is n": _pack_scenario, "no stride": _sum_scenario,
                   "duplicate summed": _refine_scenario, "pos from direct": _refine_scenario, "nan dropped": _resid_norms_scenario,
                   "map -1 read": _gather_scenario, "best overwritten": _update_scenario}


def test_clean_emulations_pass_their_checkers():
    for scenario in set(FAULT_SCENARIOS.values()):
        scenario(None)


@pytest.mark.parametrize("fault", kr.APPLY_FAULTS)
def test_every_listed_fault_is_rejected(fault):
    with pytest.raises(AssertionError):
        FAULT_SCENARIOS[fault](fault)
    if fault == "no stride":                         # both capped families of the scenario, one by one
        r, w, x, b = _norms_inputs(OVER)
        x[CAP + 6] = 41.0
        with pytest.raises(AssertionError):
            kr.assert_bits(kr.refine_norms_emulate(r, w, x, b, 0, (np.zeros(4), 0), fault)[0], kr.refine_norms_ref(r, w, x, b, 0)[0], fault)
