"""Single-launch tests of csrc/sf_solve_t.hip -- the four transposed backward kernels (six instantiations) and the condition
estimate's three kernels -- and of the two layout kernels of the SVM_W-column solves (k_solve_many_pack / _unpack, csrc/sf_solve.hip).

The transposed launches run on the cases, arenas and task lists of the plain solve's one-launch tests (test_kernels.py), the
arena filled with unit = 1: the stored diagonal and upper triangle of every L block hold NaN, which the kernels load and must
select away.  The statement (test_kernels._tsolve_check_bwd): the launch is the adjoint of the forward launch with unit = 1 and
the same interchanges, checked as equations on the stored result with the residual bound of a substitution, SAFETY nterms u mag.
The CPU tests hold that checker to a float64 emulation of the launch and to three single corruptions of it.

The condition estimate's kernels take decisions (signs, the first of equal maxima, the stop rule, flag bits) and fill vectors
with one division and one addition per entry: everything but the 1-norm is compared exactly.  n runs over {1, 2, 255, 1023, 1024,
1025, 2500}: the two reductions are ONE workgroup of CE_T = 1024 threads striding over the vector, so 1025 gives thread 0 a second
element and 2500 gives 452 threads a third.
"""
import copy

import numpy as np
import pytest

import condest_ref
import kernel_ref as kr
from test_kernels import (COND_SCALARS, NB, SOLVE_B, SOLVE_BELOW, SOLVE_FAR, SOLVE_NAN_COL, SOLVE_NARROW, SVM_W,  # noqa: F401
                          _ok, P, kp, _solve_arena, _solve_case, _solve_check_bwd, _solve_shapes, _solve_tasks, _tsolve_check_bwd,
                          _tsolve_run)

CE_T = 1024
COND_N = [1, 2, 255, 1023, 1024, 1025, 2500]
TAIL = 64                       # sentinel doubles behind a vector

PIVOT_BIG = [(65, 65, False), (200, 64, False), (256, SOLVE_FAR, True)]
PIVOT_SMALL = [(1, 0, False), (63, 1, False), (64, 65, False)]
TILES_ALONE = [(b, below, False) for b in (65, 200, 256) for below in (1, 64, 65)]
NAN_WIDE = [(64, 1, False), (65, 65, False), (256, SOLVE_FAR, True)]
# the narrow kernels: one wave per task, four to a workgroup -- five tasks (a full workgroup and a one-wave one), exactly four,
# and the five again with another task alone in the second workgroup
NARROW_LISTS = {"five": SOLVE_NARROW, "four": SOLVE_NARROW[1:], "five_rotated": SOLVE_NARROW[1:] + SOLVE_NARROW[:1]}


def _tname(width, big=None):
    return f"k_tsolve{'_many' if width > 1 else ''}" + ("_small_bwd" if big is None else f"_bwd<{bool(big)}>")


def _report(name, worst):
    print(f"TSOLVE_RATIO {name}: worst err / bound = {worst:.3g}")


# every (shapes, narrow, pivot, seed) the GPU tests below launch on, by name: the CPU tests run the emulation on each of them
def _registry():
    reg = {}
    for big in (0, 1):
        for tdiag in (False, True):
            reg[f"plain big={big} tdiag={tdiag}"] = (_solve_shapes(big), False, False, 151 + 4 * big + tdiag)
    for tdiag in (False, True):
        reg[f"pivot big=1 tdiag={tdiag}"] = (PIVOT_BIG, False, True, 161 + tdiag)
    reg["pivot big=0"] = (PIVOT_SMALL, False, True, 163)
    reg["tiles alone"] = (TILES_ALONE, False, True, 164)
    for key, shapes in NARROW_LISTS.items():
        for pivot in (False, True):
            reg[f"narrow {key} pivot={pivot}"] = (shapes, True, pivot, 171 + pivot)
    reg["nan wide"] = (NAN_WIDE, False, True, 181)
    reg["nan narrow"] = (SOLVE_NARROW, True, True, 182)
    for big in (0, 1):
        reg[f"identity big={big}"] = ([(b, 0, False) for b in SOLVE_B if big or b <= NB], False, False, 191 + big)
    reg["identity narrow"] = (SOLVE_NARROW, True, False, 193)
    return reg


CASES = _registry()


def _case(name, width, nan_col=None):
    shapes, narrow, pivot, seed = CASES[name]
    return _solve_case(np.random.default_rng(seed), shapes, width, narrow=narrow, pivot=pivot, nan_col=nan_col)


def _emulate(case, fault=None):
    x1 = case.x.copy()
    for p in case.panels:
        x1[p["blk"]] = kr.tsolve_emulate(p["D"], p["Lb"], p["pos"], case.x[p["blk"]], case.x[p["gi"]], fault)
    return x1


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the checker against a float64 emulation of the launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [1, SVM_W])
@pytest.mark.parametrize("name", [k for k in CASES if k != "tiles alone"])
def test_checker_accepts_the_emulation(name, width):
    if not kr.have_longdouble():
        pytest.skip("np.longdouble has no 64-bit mantissa on this platform: no extended-precision reference")
    case = _case(name, width, SOLVE_NAN_COL if name.startswith("nan") and width > 1 else None)
    worst = _tsolve_check_bwd(case, _emulate(case), f"emulation, {name}")
    assert worst <= 1.0


# (only a block of more than 64 columns has earlier sub-blocks: elsewhere a late interchange changes nothing)
CORRUPTIONS = [(name, fault) for name in ("pivot big=1 tdiag=False", "pivot big=0", "narrow five pivot=True") for fault in kr.TSOLVE_FAULTS
               if fault != "late interchange" or name == "pivot big=1 tdiag=False"]


@pytest.mark.parametrize("name,fault", CORRUPTIONS)
def test_checker_rejects_single_corruptions(name, fault):
    """the forward permutation in place of the inverse, the interchange applied after the earlier sub-blocks have read, the stored
    diagonal in place of the implied 1"""
    if not kr.have_longdouble():
        pytest.skip("np.longdouble has no 64-bit mantissa on this platform: no extended-precision reference")
    case = _case(name, 1)
    with pytest.raises(AssertionError, match="beyond the bound"):
        _tsolve_check_bwd(case, _emulate(case, fault), f"{fault}, {name}")


def _unit_diagonal(case):
    """the case with the diagonal of every D set to 1: what _solve_check_bwd needs to state the same equations"""
    twin = copy.copy(case)
    twin.panels = [dict(p, D=np.tril(p["D"], -1) + np.eye(p["b"])) for p in case.panels]
    return twin


@pytest.mark.parametrize("name", ["plain big=1 tdiag=False", "narrow five pivot=False"])
def test_checker_without_pivoting_is_the_plain_backward_check(name):
    """pivot = False: M = the unit lower S, the equations are _solve_check_bwd's with a unit-diagonal D -- the same verdicts"""
    if not kr.have_longdouble():
        pytest.skip("np.longdouble has no 64-bit mantissa on this platform: no extended-precision reference")
    case = _case(name, SVM_W)
    twin = _unit_diagonal(case)
    good = _emulate(case)
    _tsolve_check_bwd(case, good, name)
    _solve_check_bwd(twin, good, name)
    for fault in ("stored diagonal", None):
        bad = _emulate(case, fault)
        if fault is None:                   # one stored entry doubled
            blk = case.panels[-1]["blk"]
            bad[blk.start, 3] *= 2.0
        for check, c in ((_tsolve_check_bwd, case), (_solve_check_bwd, twin)):
            with pytest.raises(AssertionError, match="beyond the bound"):
                check(c, bad, name)
    stray = good.copy()
    stray[case.nx - 1, 0] = 0.0             # outside every block (held NaN)
    for check, c in ((_tsolve_check_bwd, case), (_solve_check_bwd, twin)):
        with pytest.raises(AssertionError, match="outside the write footprint"):
            check(c, stray, name)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the transposed backward launch
# ---------------------------------------------------------------------------------------------------------------------
def _launch(kp, name, width, big, small=0, tdiag=False, nan_col=None, tiles_only=False, pivpos="case"):
    case = _case(name, width, nan_col)
    narrow = CASES[name][1]
    tasks, nT = _solve_tasks(case, 1, narrow=narrow, tdiag=tdiag, tiles_only=tiles_only)
    piv = (case.pivpos if CASES[name][2] else None) if isinstance(pivpos, str) else pivpos
    return case, _tsolve_run(kp, case, _solve_arena(case, 1), tasks, width, big, small, pivpos=piv, nT=nT)


@pytest.mark.gpu
@pytest.mark.parametrize("tdiag", [False, True])
@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("width", [1, SVM_W])
def test_tsolve_bwd_step(kp, width, big, tdiag):
    name = f"plain big={big} tdiag={tdiag}"
    case, x1 = _launch(kp, name, width, big, tdiag=tdiag)
    _report(_tname(width, big), _tsolve_check_bwd(case, x1, f"{_tname(width, big)} tdiag={tdiag}"))


@pytest.mark.gpu
@pytest.mark.parametrize("tdiag", [False, True])
@pytest.mark.parametrize("width", [1, SVM_W])
def test_tsolve_bwd_step_pivoting(kp, width, tdiag):
    """the interchanges are undone after a sub-block's chain and before the waves above read it"""
    case, x1 = _launch(kp, f"pivot big=1 tdiag={tdiag}", width, 1, tdiag=tdiag)
    _report(_tname(width, 1), _tsolve_check_bwd(case, x1, f"{_tname(width, 1)} pivoting tdiag={tdiag}"))


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, SVM_W])
def test_tsolve_bwd_step_pivoting_one_sub_block(kp, width):
    case, x1 = _launch(kp, "pivot big=0", width, 0)
    _report(_tname(width, 0), _tsolve_check_bwd(case, x1, f"{_tname(width, 0)} pivoting"))


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, SVM_W])
def test_tsolve_bwd_tiles_alone(kp, width):
    """the two-launch form's first launch: <false> with b > 64, pivpos given -- x_blk' = x_blk - Lb^T x[rows], nothing is permuted"""
    case, x1 = _launch(kp, "tiles alone", width, 0, tiles_only=True)
    x0, what = case.x, f"{_tname(width, 0)} tiles alone"
    written = np.zeros(x0.shape, dtype=bool)
    worst = 0.0
    for p in case.panels:
        xr, Lb = x0[p["gi"]], p["Lb"]
        worst = max(worst, kr.assert_equations(x1[p["blk"]], x0[p["blk"]].astype(kr.LD) - kr.matmul_ld(Lb.T, xr), np.full(p["b"], p["below"] + 1),
                                               np.abs(x0[p["blk"]]) + kr.matmul_ld(np.abs(Lb.T), np.abs(xr)), case.cols,
                                               f"{what} b={p['b']} below={p['below']}"))
        written[p["blk"]] = True
    kr.assert_unchanged(x0, x1, written, what)
    _report(what, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("pivot", [False, True])
@pytest.mark.parametrize("tasks", list(NARROW_LISTS))
@pytest.mark.parametrize("width", [1, SVM_W])
def test_tsolve_small_bwd(kp, width, tasks, pivot):
    case, x1 = _launch(kp, f"narrow {tasks} pivot={pivot}", width, 0, small=1)
    _report(_tname(width), _tsolve_check_bwd(case, x1, f"{_tname(width)} {tasks} pivot={pivot}"))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["bwd", "small_bwd"])
def test_tsolve_many_columns_are_independent(kp, kernel):
    """one of the SVM_W right-hand sides is NaN throughout: every other column still meets its bound"""
    narrow = kernel == "small_bwd"
    case, x1 = _launch(kp, "nan narrow" if narrow else "nan wide", SVM_W, int(not narrow), small=int(narrow), tdiag=True, nan_col=SOLVE_NAN_COL)
    assert np.all(np.isnan(x1[:, SOLVE_NAN_COL]))
    _tsolve_check_bwd(case, x1, f"k_tsolve_many_{kernel} with a NaN column")


@pytest.mark.gpu
@pytest.mark.parametrize("name,big,small", [("identity big=0", 0, 0), ("identity big=1", 1, 0), ("identity narrow", 0, 1)])
@pytest.mark.parametrize("width", [1, SVM_W])
def test_tsolve_identity_interchanges(kp, width, name, big, small):
    """pivpos = the identity: bit-identical to the launch without a record.  No tiles (below = 0; the narrow kernels have none:
    one wave sums its rows itself), so the summation order is fixed."""
    case, plain = _launch(kp, name, width, big, small=small, pivpos=None)
    assert np.array_equal(case.pivpos, np.arange(case.nx))
    _, ident = _launch(kp, name, width, big, small=small, pivpos=case.pivpos)
    assert np.array_equal(kr.bits(plain), kr.bits(ident))
    _tsolve_check_bwd(case, plain, f"{_tname(width, None if small else big)} identity")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the condition estimate's kernels
# ---------------------------------------------------------------------------------------------------------------------
def _sentinel(n, rng):
    """n finite values and a NaN tail that must come back bit for bit"""
    v = np.full(n + TAIL, np.nan)
    v[:n] = kr.scalings(rng, n) * rng.uniform(-1, 1, n)
    return v


def _scalars(nrm, flags, j):
    s = np.zeros(1, dtype=COND_SCALARS)
    s[0] = (nrm, flags, j)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("n", COND_N)
def test_condest_fill(kp, n):
    """one correctly rounded division (and one addition) per entry: bit-equal to numpy float64"""
    rng = np.random.default_rng(n)
    for mode, want in ((0, np.full(n, 1.0 / n)), (2, condest_ref.altsgn(n) if n > 1 else None)):
        if want is None:
            continue
        x = _sentinel(n, rng)
        before = x.copy()
        _ok(kp.kp_condest_fill(P(x), len(x), n, mode))
        assert np.array_equal(kr.bits(x[:n]), kr.bits(want)), f"mode {mode}: {int((kr.bits(x[:n]) != kr.bits(want)).sum())} entries differ"
        assert np.array_equal(kr.bits(x[n:]), kr.bits(before[n:])), f"mode {mode}: written past n"


def _signs(v):
    return np.where(v >= 0.0, 1.0, -1.0)


def _sign_norm(kp, y, xi, n, info, flags, j=12345):
    y, xi, s = y.copy(), xi.copy(), _scalars(-7.0, flags, j)
    _ok(kp.kp_condest_sign_norm(P(y), P(xi), len(y), n, info, P(s)))
    return y, xi, s[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", COND_N)
def test_condest_sign_norm(kp, n):
    rng = np.random.default_rng(100 + n)
    y0 = _sentinel(n, rng)
    if n >= 2:
        y0[0] = 0.0
        y0[n // 2] = -0.0               # sign(-0.0) = +1
    want = _signs(y0[:n])
    assert n < 2 or (want[n // 2] == 1.0 and np.signbit(y0[n // 2]))
    exact = np.sum(np.abs(y0[:n]).astype(kr.LD))
    tail = kr.bits(y0[n:])
    xi_same = np.concatenate([want, np.full(TAIL, np.nan)])
    variants = [("zeros", np.concatenate([np.zeros(n), np.full(TAIL, np.nan)]), 0), ("same", xi_same, 1)]
    for at in sorted({0, n - 1}):       # exactly one entry differs: the first, and the last (n = 2500: a thread's third stride)
        xi = xi_same.copy()
        xi[at] = -xi[at]
        variants.append((f"differs at {at}", xi, 0))
    nrm_bits = set()
    for what, xi0, bit0 in variants:
        for flags_in, info in ((0, 0), (2, 0), (0x7FFFFFFD, 2), (0x7FFFFFFF, -2147483648)):
            y, xi, s = _sign_norm(kp, y0, xi0, n, info, flags_in)
            ctx = f"n={n} xi {what} flags_in={flags_in:#x} info={info}"
            assert np.array_equal(kr.bits(y[:n]), kr.bits(want)) and np.array_equal(kr.bits(xi[:n]), kr.bits(want)), ctx
            assert np.array_equal(kr.bits(y[n:]), tail) and np.array_equal(kr.bits(xi[n:]), kr.bits(xi0[n:])), ctx + ": written past n"
            assert int(s["flags"]) == (flags_in & 2) | bit0 | (4 if info else 0), (ctx, int(s["flags"]))
            assert int(s["j"]) == 12345, ctx
            assert abs(kr.LD(s["nrm"]) - exact) <= n * kr.U * exact, (ctx, float(s["nrm"]), float(exact))
            nrm_bits.add(int(kr.bits(np.array([s["nrm"]]))[0]))
    assert len(nrm_bits) == 1, "the same y gave different norms"
    # a NaN: its sign is -1, the norm is NaN
    y1 = y0.copy()
    y1[n // 3] = np.nan
    y, xi, s = _sign_norm(kp, y1, xi_same, n, 0, 0)
    want1 = want.copy()
    want1[n // 3] = -1.0
    assert np.array_equal(kr.bits(y[:n]), kr.bits(want1)) and np.array_equal(kr.bits(xi[:n]), kr.bits(want1))
    assert np.isnan(s["nrm"]) and int(s["j"]) == 12345
    assert int(s["flags"]) == (1 if want[n // 3] == -1.0 else 0)


def _argmax_rule(x, jlast, first, last):
    """(j, stop): the first index of the largest |x_i| (NaN never wins; all NaN: 0); the signed stop rule"""
    a = np.abs(x)
    a[np.isnan(a)] = -1.0
    j = int(np.argmax(a)) if a.max() >= 0 else 0
    best = a.max()
    stop = (not first) and bool(last or (0 <= jlast < len(x) and x[jlast] == best))
    return j, stop


def _argmax_next(kp, x0, n, jlast, first, last, want=None, what=""):
    """one launch, checked against `want` = (j, stop) (default: _argmax_rule); returns (j, stop)"""
    x, s = x0.copy(), _scalars(3.25, 5, jlast)
    _ok(kp.kp_condest_argmax_next(P(x), len(x), n, P(s), first, last))
    j, stop = want if want is not None else _argmax_rule(x0[:n], jlast, first, last)
    ctx = f"{what} n={n} jlast={jlast} first={first} last={last}"
    assert kr.bits(s["nrm"])[0] == kr.bits(np.array([3.25]))[0], ctx
    assert (int(s["j"][0]), int(s["flags"][0])) == (j, 2 if stop else 0), (ctx, int(s["j"][0]), int(s["flags"][0]), "want", j, stop)
    e = np.zeros(n)
    e[j] = 1.0
    assert np.array_equal(kr.bits(x[:n]), kr.bits(condest_ref.altsgn(n) if stop else e)), ctx
    assert np.array_equal(kr.bits(x[n:]), kr.bits(x0[n:])), ctx + ": written past n"
    return j, stop


@pytest.mark.gpu
@pytest.mark.parametrize("n", [n for n in COND_N if n >= 2])
def test_condest_argmax_next(kp, n):
    rng = np.random.default_rng(200 + n)
    base = _sentinel(n, rng)
    big = 4.0 * np.max(np.abs(base[:n]))
    for at in sorted({0, n // 2, n - 1}):
        x = base.copy()
        x[at] = -big
        other = (at + 1) % n
        # first = 1 never stops, whatever jlast; afterwards: stop iff x[jlast] == +max, or last
        for jlast in (-1, at, other, n, n + 5):
            assert _argmax_next(kp, x, n, jlast, 1, 0, (at, False), "first") == (at, False)
            assert _argmax_next(kp, x, n, jlast, 1, 1, (at, False), "first and last") == (at, False)
            assert _argmax_next(kp, x, n, jlast, 0, 1, (at, True), "last") == (at, True)
        for jlast in (-1, n, n + 5, other, at):         # x[at] = -max: no stop even at jlast = at
            _argmax_next(kp, x, n, jlast, 0, 0, (at, False), "x[jlast] = -max or no jlast")
        x[at] = big
        _argmax_next(kp, x, n, at, 0, 0, (at, True), "x[jlast] = +max")
        _argmax_next(kp, x, n, other, 0, 0, (at, False), "x[jlast] smaller")
    # every entry NaN: j = 0, x = e_0
    x = np.full(n + TAIL, np.nan)
    _argmax_next(kp, x, n, -1, 1, 0, (0, False), "all NaN")
    _argmax_next(kp, x, n, 0, 0, 0, (0, False), "all NaN, jlast = 0")
    # one finite entry among NaN
    x[n - 1] = -0.0
    _argmax_next(kp, x, n, -1, 1, 0, (n - 1, False), "one zero among NaN")


@pytest.mark.gpu
def test_condest_argmax_first_of_equal_maxima(kp):
    """n = 2500, the pair of maxima at i1 < i2 with i1 in a HIGHER thread than i2 (1000 -> thread 1000, 1030 -> thread 6): only the
    tree's tie-break on the index keeps i1; the mirror placements (signs swapped; i1 in the lower thread) and a jlast on either"""
    n = 2500
    rng = np.random.default_rng(7)
    base = _sentinel(n, rng)
    m = 4.0 * np.max(np.abs(base[:n]))
    for i1, i2 in ((1000, 1030), (6, 1000), (1000, 2054), (1030, 2024), (0, n - 1)):
        for v1, v2 in ((-m, m), (m, -m), (m, m)):
            x = base.copy()
            x[i1], x[i2] = v1, v2
            what = f"maxima {v1:+.3g} at {i1}, {v2:+.3g} at {i2}"
            _argmax_next(kp, x, n, -1, 1, 0, (i1, False), what)
            _argmax_next(kp, x, n, i1, 0, 0, (i1, v1 > 0), what)        # the signed rule on either of the two
            _argmax_next(kp, x, n, i2, 0, 0, (i1, v2 > 0), what)


def _ref_inputs(x_first, x_second):
    """condest_ref over solves that return prescribed vectors: the inputs it hands to its second and third A^{-1} solve, i.e. e_j
    of the first A^{-T} result, then e_j of the second or -- if its stop rule fires -- the safeguard vector"""
    n = len(x_first)
    seen, ys, xs = [], [np.ones(n), -2.0 * np.ones(n), np.ones(n), np.ones(n)], [x_first, x_second]

    def solve(v):
        seen.append(v.copy())
        return ys[len(seen) - 1]

    def solve_t(v):
        return xs.pop(0)

    condest_ref.condest_ref(solve, solve_t, n)
    return seen[1], seen[2]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 1025, 2500])
def test_condest_argmax_next_against_condest_ref(kp, n):
    """random vectors with planted ties: what the kernel leaves in x is what condest_ref hands to its next solve"""
    rng = np.random.default_rng(300 + n)
    for trial in range(12):
        x1, x2 = _sentinel(n, rng), _sentinel(n, rng)
        for x in (x1, x2):
            ties = rng.choice(n, 4, replace=False)
            x[ties] = 4.0 * np.max(np.abs(x[:n])) * rng.choice([-1.0, 1.0], 4)
        if trial % 2:                       # the second vector's maximum where the first one's was: the stop rule can fire
            j1 = int(np.argmax(np.abs(x1[:n])))
            x2[j1] = np.max(np.abs(x2[:n])) * (1.0 if trial % 4 == 1 else -1.0)
        in2, in3 = _ref_inputs(x1[:n].copy(), x2[:n].copy())
        a, s = x1.copy(), _scalars(1.0, 0, -1)
        _ok(kp.kp_condest_argmax_next(P(a), len(a), n, P(s), 1, 0))
        assert np.array_equal(kr.bits(a[:n]), kr.bits(in2)), f"trial {trial}: first pass"
        b = x2.copy()
        _ok(kp.kp_condest_argmax_next(P(b), len(b), n, P(s), 0, 0))
        assert np.array_equal(kr.bits(b[:n]), kr.bits(in3)), f"trial {trial}: second pass, flags {int(s['flags'][0])}"
        assert int(s["flags"][0]) == (2 if np.array_equal(in3, condest_ref.altsgn(n)) else 0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the layout kernels of the SVM_W-column solves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cw", [1, 5, 16])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_solve_many_pack_unpack(kp, n, cw):
    rng = np.random.default_rng(1000 * n + cw)
    # pack: column-major n x cw -> row-major n x SVM_W, columns [cw, SVM_W) zero, over a NaN destination
    Bc = np.full(n * cw + TAIL, np.nan)
    Bc[:n * cw] = rng.uniform(-1, 1, n * cw)
    X = np.full(n * SVM_W + TAIL, np.nan)
    before = X.copy()
    _ok(kp.kp_solve_many_pack(P(Bc), len(Bc), n, cw, P(X), len(X)))
    want = np.zeros((n, SVM_W))
    want[:, :cw] = Bc[:n * cw].reshape(cw, n).T
    assert np.array_equal(kr.bits(X[:n * SVM_W]), kr.bits(want.ravel())), "k_solve_many_pack"
    assert np.array_equal(kr.bits(X[n * SVM_W:]), kr.bits(before[n * SVM_W:])), "k_solve_many_pack: written past n x SVM_W"
    # unpack: the first n * cw entries of a NaN-filled Bc of n * SVM_W, nothing else
    X = np.full(n * SVM_W + TAIL, np.nan)
    X[:n * SVM_W] = rng.uniform(-1, 1, n * SVM_W)
    out = np.full(n * SVM_W, np.nan)
    before = out.copy()
    _ok(kp.kp_solve_many_unpack(P(X), len(X), n, cw, P(out), len(out)))
    want = X[:n * SVM_W].reshape(n, SVM_W)[:, :cw].T.ravel()
    assert np.array_equal(kr.bits(out[:n * cw]), kr.bits(want)), "k_solve_many_unpack"
    assert np.array_equal(kr.bits(out[n * cw:]), kr.bits(before[n * cw:])), "k_solve_many_unpack: written past n * cw"
