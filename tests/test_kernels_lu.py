"""Single-launch tests of the LU kernels: the fused 64-column step k_step<true> (csrc/sf_step.hip) on task lists built here the
way fused_step() (sf_plan_build.hip) builds them, and the three LU layout kernels (k_pack_lu, k_lu_fill_u11, k_factor_hash;
csrc/sf_kernels.hip).

The step tests check the STORED factor of every panel against the panel's matrix element by element (kernel_ref.lu_panel_check:
|A - L~ U~| <= SAFETY (terms + 2) u |L~| |U~|, rows scaled over 1e-3 .. 1e3), the pivot records against the longdouble rule
(kernel_ref.lu_panel_ref, inputs regenerated until every decision has a relative margin >= 1e-8), the flags, info, and the write
footprint bit for bit.  Operands that a task loads and selects away hold finite garbage, everything else outside the operands NaN.
The layout kernels move data or do integer arithmetic: exact equality with a numpy restatement of their layout comments.
"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import kernel_ref as kr
from test_kernels import (FILL_TILE, GEMM_PROB, GEMM_TASK, NB, OUTER_NB, POTRF_TASK, SOLVE_TASK, ST_ROWS, STEP_TASK, TRSM_TASK,  # noqa: F401
                          _make, _ok, P, kp)

LU_PANELS = [(1, 0), (17, 1), (64, 63), (65, 64), (130, 65), (100, 300), (320, 130)]       # (nscol, rows below)
LU_PARAMS = [(0.0, 0.0), (0.1, 0.0), (1.0, 0.0)]
MARGIN, TRIES = 1e-8, 50
HASH_K = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------------------------------------------------------------
# inputs: one registry, so that the CPU tests see every parametrization the GPU tests use; references computed once
# ---------------------------------------------------------------------------------------------------------------------
def _draw(rng, nscol, below, tol, kind):
    """[[A11, A12], [A21, .]] of one panel.  random / dominant: rows scaled log-uniformly over 1e-3 .. 1e3.  The kinds that need
    natural pivots to PASS a column test (natural, handover) scale over 1e-1 .. 1e1: a row 1e6 times its neighbour would win
    every column whatever the diagonal holds."""
    nsrow = nscol + below
    wide = kind in ("random", "dominant", "deficient")
    s = kr.scalings(rng, nsrow, 1e-3, 1e3) if wide else kr.scalings(rng, nsrow, 1e-1, 1e1)
    B = rng.uniform(-1, 1, (nsrow, nsrow))
    if kind in ("dominant", "natural") or (kind == "deficient" and tol == 0):
        B[:nscol, :nscol] += np.diag(np.full(nscol, 2.0 * nsrow))
    if kind == "handover":                  # columns 0 .. 31 strongly dominant, the rest random
        B[:32, :32] += np.diag(np.full(32, 4.0 * nsrow))
    A = s[:, None] * B
    if kind == "deficient":                 # as _getrf_input: one row of the diagonal block twice its neighbour, the zero is exact
        A[nscol // 2, :nscol] = 2 * A[nscol // 2 - 1, :nscol]
    return A[:nscol, :nscol].copy(), A[nscol:, :nscol].copy(), A[:nscol, nscol:].copy()


@functools.lru_cache(maxsize=None)
def _inputs(shapes, J, tol, eps, kind, seed):
    """per panel a dict with the matrix, the reference's pivots / perturbed columns / factor and the number of tries it took"""
    rng = np.random.default_rng(seed)
    out = []
    for nscol, below in shapes:
        for tries in range(1, TRIES + 1):
            A11, A21, A12 = _draw(rng, nscol, below, tol, kind)
            pos, PL, PU, pert, margin = kr.lu_panel_ref(A11, A21, A12, tol, eps, J)
            if margin >= MARGIN:
                break
        else:
            tries = TRIES + 1
        out.append(dict(nscol=nscol, below=below, A11=A11, A21=A21, A12=A12, pos=pos, PL=PL, PU=PU, pert=pert, tries=tries))
    return out


def _kind(tol):
    return "dominant" if tol == 0 else "random"


# every (shapes, J, tol, eps, kind, seed) a GPU test below factors
CASES = {}
for _tol, _eps in LU_PARAMS:
    for _ep in (1, 2):
        CASES[f"outer tol={_tol} epoch={_ep}"] = (tuple(LU_PANELS), 0, _tol, _eps, _kind(_tol), 100 + int(10 * _tol) + 1000 * _ep)
        CASES[f"second tol={_tol} epoch={_ep}"] = (((577, 3),), 512, _tol, _eps, _kind(_tol), 200 + int(10 * _tol) + 1000 * _ep)
CASES["handover"] = (((64, 70),), 0, 0.5, 0.0, "handover", 300)
CASES["natural"] = (((17, 1), (64, 70), (130, 65)), 0, 0.1, 0.0, "natural", 301)
for _tol in (0.0, 1.0):
    CASES[f"perturb tol={_tol}"] = (((33, 70), (64, 10)), 0, _tol, 1e-8, "deficient", 302 + int(_tol))


def _case(name):
    shapes, J, tol, eps, kind, seed = CASES[name]
    return _inputs(shapes, J, tol, eps, kind, seed), J, tol, eps


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the probe, the dtypes, the reference and the checker
# ---------------------------------------------------------------------------------------------------------------------
def test_probe_lu_entries_and_dtype_sizes(tmp_path):
    """the probe builds, exports the LU layout entries, and every task dtype has the size of its struct (no GPU needed)"""
    out = tmp_path / "libsf_kprobe.so"
    r = _make([f"OUT={out}"], 300)
    assert r.returncode == 0, r.stdout
    nm = subprocess.run(["nm", "-D", str(out)], stdout=subprocess.PIPE, text=True).stdout
    for name in ("kp_step", "kp_getrf", "kp_pack_lu", "kp_lu_fill_u11", "kp_factor_hash", "kp_sizeof"):
        assert f" T {name}" in nm
    L = C.CDLL(str(out))
    for name, dt in (("GemmProb", GEMM_PROB), ("GemmTask", GEMM_TASK), ("PotrfTask", POTRF_TASK), ("TrsmTask", TRSM_TASK),
                     ("StepTask", STEP_TASK), ("SolveTask", SOLVE_TASK), ("FillTile", FILL_TILE)):
        assert L.kp_sizeof(name.encode()) == dt.itemsize, name
    assert L.kp_sizeof(b"NoSuchStruct") == -1


needs_ld = pytest.mark.skipif(not kr.have_longdouble(), reason="np.longdouble has no 64-bit mantissa on this platform")


@needs_ld
@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_are_generated_within_the_cap(name):
    """every parametrization of the GPU tests finds an input whose pivot decisions all have a relative margin >= 1e-8 in at
    most 50 tries"""
    for inp in _case(name)[0]:
        assert inp["tries"] <= TRIES, (name, inp["nscol"], inp["below"])


def _stored(inp, J):
    """the reference factor rounded to fp64, laid out as the device stores it"""
    PL, PU = inp["PL"].astype(np.float64), inp["PU"].astype(np.float64)
    assert np.all(np.isnan(PL[:, :J])) and np.all(np.isnan(PU[:, :J]))
    return PL, PU


def _check(inp, PL, PU, J, what, pos=None):
    return kr.lu_panel_check(inp["A11"], inp["A21"], inp["A12"], PL, PU, inp["pos"] if pos is None else pos, inp["pert"], J, what)


@needs_ld
@pytest.mark.parametrize("name", sorted(CASES))
def test_checker_accepts_the_reference_factor(name):
    inputs, J, tol, eps = _case(name)
    for inp in inputs:
        PL, PU = _stored(inp, J)
        ratio = _check(inp, PL, PU, J, f"{name} nscol={inp['nscol']}")
        assert ratio <= 0.5         # a correctly rounded factor: one rounding per stored entry, far inside (terms + 2) u


def _panel(name, nscol):
    inputs, J, tol, eps = _case(name)
    inp = next(i for i in inputs if i["nscol"] == nscol)
    return inp, J


@needs_ld
def test_checker_rejects_a_small_error_in_a_small_row():
    """one L21 entry of a row scaled by about 1e-3 changed by a relative 1e-10"""
    inp, J = _panel("outer tol=0.1 epoch=1", 100)
    PL, PU = _stored(inp, J)
    scale = np.max(np.abs(inp["A21"]), axis=1)
    r = int(np.argmin(np.abs(np.log(scale / (1e-3 * np.median(scale))))))       # a row about 1e-3 of the typical one
    assert scale[r] <= 1e-2 * np.max(scale)
    PL[100 + r, 70] *= 1 + 1e-10
    with pytest.raises(AssertionError, match="beyond the bound"):
        _check(inp, PL, PU, J, "corrupted L21")


@needs_ld
def test_checker_rejects_swapped_u_rows():
    inp, J = _panel("outer tol=0.1 epoch=1", 130)
    PL, PU = _stored(inp, J)
    i, k = 64 + 3, 64 + 9                       # two U rows of the second block: columns of the U^T panel, from the later diagonal on
    PU[k:, [i, k]] = PU[k:, [k, i]]
    with pytest.raises(AssertionError, match="beyond the bound"):
        _check(inp, PL, PU, J, "swapped U rows")


@needs_ld
def test_checker_rejects_left_of_block_l_rows_in_pivot_order():
    inp, J = _panel("outer tol=0.1 epoch=1", 130)
    PL, PU = _stored(inp, J)
    pos = inp["pos"]
    r = next(r for r in range(64, 128) if pos[r] != r)
    PL[pos[r], :64], PL[r, :64] = PL[r, :64].copy(), PL[pos[r], :64].copy()       # that row's left part moved with the interchange
    with pytest.raises(AssertionError, match="beyond the bound"):
        _check(inp, PL, PU, J, "left-of-block L in pivot order")


@needs_ld
def test_directed_inputs_are_what_they_claim():
    """hand-over: the reference keeps positions 0 .. 31 natural and moves a row in the block's third 16-column panel; natural:
    nothing moves although pivoting is on; deficient: exactly one replaced pivot per panel"""
    (inp,), J, tol, eps = _case("handover")
    assert np.array_equal(inp["pos"][:32], np.arange(32))
    assert not np.array_equal(inp["pos"][32:48], np.arange(32, 48))
    for inp in _case("natural")[0]:
        assert np.array_equal(inp["pos"], np.arange(inp["nscol"]))
    for t in (0.0, 1.0):
        for inp in _case(f"perturb tol={t}")[0]:
            assert len(inp["pert"]) == 1
    assert any(not np.array_equal(i["pos"], np.arange(i["nscol"])) for i in _case("perturb tol=1.0")[0])


# ---------------------------------------------------------------------------------------------------------------------
# k_step<true>
# ---------------------------------------------------------------------------------------------------------------------
def _lu_step_launches(panels, J, u_shift):
    """the task lists of the fused LU steps of the outer block [J, J + 512), one launch per step, as fused_step()
    (sf_plan_build.hip) builds them: the diagonal tasks (xpanel = the U^T panel; their own update starts at J for steps 0 and 1,
    at diag - 64 from step 2 on: the far part was applied by a pre-update task one launch earlier), right behind them the
    pre-update tasks of the NEXT step's diagonal blocks (steps 1 .. 6: mode 2, no flag, diag = row0 = diag + 64), then per 64
    rows below a block the L rows (mode 0) and the U^T rows (mode 1, panels swapped).  panels: (off, nscol, nsrow, ld, first_col)"""
    launches, nflags, ninner = [], 0, OUTER_NB // NB
    for ti in range(ninner):
        diag = J + ti * NB
        tasks, flag_of, slot_of = [], [], []
        for off, nscol, nsrow, ld, fc in panels:
            if diag >= nscol:
                flag_of.append(-1)
                slot_of.append(-1)
                continue
            b = min(NB, nscol - diag)
            flag_of.append(nflags)
            slot_of.append(len(tasks))
            tasks.append((off, off + u_shift, ld, J if ti < 2 else diag - NB, diag, b, diag, b, nflags, 0, len(tasks), 0, fc, 0))
            nflags += 1
        ndiag = len(tasks)
        if 1 <= ti and ti + 1 < ninner:
            dnext = diag + NB
            for off, nscol, nsrow, ld, fc in panels:
                if dnext < nscol:
                    bn = min(NB, nscol - dnext)
                    tasks.append((off, off + u_shift, ld, J, dnext, bn, dnext, bn, -1, 2, 0, 0, fc, 0))
        for (off, nscol, nsrow, ld, fc), fl, sl in zip(panels, flag_of, slot_of):
            if fl < 0:
                continue
            b = min(NB, nscol - diag)
            for r in range(diag + b, nsrow, ST_ROWS):
                nr = min(ST_ROWS, nsrow - r)
                tasks.append((off, off + u_shift, ld, J, diag, b, r, nr, fl, 0, sl, 0, fc, 0))
                tasks.append((off + u_shift, off, ld, J, diag, b, r, nr, fl, 1, sl, 0, fc, 0))
        if tasks:
            launches.append((np.array(tasks, dtype=STEP_TASK), ndiag))
    return launches, nflags


class LuArena:
    """L panels, then the U^T panels at the same offsets + u_shift (odd skews, guard bands, leading dimension nsrow + 3).  Operands
    from column J on; in the diagonal blocks the L panel's upper triangle AND diagonal and the U^T panel's strict upper triangle
    hold finite garbage (loaded and selected away: must come back bit-identical); everything else, all of the columns left of J
    included, NaN."""

    def __init__(self, inputs, J, seed):
        rng = np.random.default_rng(seed)
        ar = kr.Arena()
        self.J, self.inputs, self.panels, fc = J, inputs, [], 3
        for inp in inputs:
            nscol, nsrow = inp["nscol"], inp["nscol"] + inp["below"]
            ld = nsrow + 3
            self.panels.append((ar.alloc(ld * nscol, skew=1), nscol, nsrow, ld, fc))
            fc += nscol + 5
        self.npiv = fc + 64
        self.u_shift = ar.size + 7
        ar.size = self.u_shift + ar.size + kr.GUARD
        self.a = ar.image()
        self.written = np.zeros(len(self.a), dtype=bool)
        self.idx = []
        for inp, (off, nscol, nsrow, ld, _) in zip(inputs, self.panels):
            r, c = np.arange(nsrow)[:, None], np.arange(nscol)[None, :]
            iL = off + r + c * ld
            iU = iL + self.u_shift
            self.idx.append((iL, iU))
            A = kr.lu_full(inp["A11"], inp["A21"], inp["A12"])[:, :nscol], kr.lu_full(inp["A11"], inp["A21"], inp["A12"]).T[:, :nscol]
            c0 = J + (np.maximum(c - J, 0) // NB) * NB            # first column of c's block
            for i, (ix, strict) in enumerate(((iL, True), (iU, False))):
                own = (c >= J) & ((r > c) if strict else (r >= c))
                junk = (c >= J) & (r >= c0) & ~own
                self.a[ix[own]] = A[i][own]
                self.a[ix[junk]] = rng.uniform(-1e3, 1e3, int(junk.sum()))
                self.written[ix[own]] = True
        self.before = self.a.copy()
        self.launches, self.nflags = _lu_step_launches(self.panels, J, self.u_shift)

    def run(self, kp, flags, epoch, tol, eps, lu=1):
        """every launch of the outer block; returns (info, nperturb, pivpos, pivinv) -- no pivot records when tol == 0"""
        info, nper = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        pivpos = np.full(self.npiv, -5, dtype=np.int32) if tol > 0 else None
        pivinv = np.full(self.npiv, -5, dtype=np.int32) if tol > 0 else None
        for tasks, ndiag in self.launches:
            _ok(kp.kp_step(P(self.a), len(self.a), P(tasks), len(tasks), lu, P(flags), self.nflags, epoch, P(info), 2048 * ndiag,
                           tol, eps, P(pivpos), P(pivinv), self.npiv, P(nper)))
        return int(info[0]), int(nper[0]), pivpos, pivinv

    def check(self, pivpos, pivinv, what):
        """footprint, pivot records (exactly the reference's, nothing else written), the residual check; worst err / bound"""
        kr.assert_unchanged(self.before, self.a, self.written, what)
        if pivpos is not None:
            want_pos, want_inv = np.full(self.npiv, -5, dtype=np.int32), np.full(self.npiv, -5, dtype=np.int32)
            for inp, (off, nscol, nsrow, ld, fc) in zip(self.inputs, self.panels):
                want_pos[fc + self.J:fc + nscol] = fc + inp["pos"][self.J:]
                want_inv[fc + inp["pos"][self.J:]] = fc + np.arange(self.J, nscol)
            assert np.array_equal(pivpos, want_pos), f"{what}: pivpos"
            assert np.array_equal(pivinv, want_inv), f"{what}: pivinv"
        worst = 0.0
        for inp, (iL, iU) in zip(self.inputs, self.idx):
            ratio = _check(inp, self.a[iL], self.a[iU], self.J, f"{what} nscol={inp['nscol']} below={inp['below']}")
            print(f"{what} nscol={inp['nscol']} below={inp['below']}: worst err / bound = {ratio:.3f}")
            worst = max(worst, ratio)
        return worst


def _factor_and_check(kp, name, flags, epoch):
    inputs, J, tol, eps = _case(name)
    ar = LuArena(inputs, J, seed=epoch)
    if flags is None:
        flags = np.zeros(ar.nflags, dtype=np.int32)
    info, nper, pivpos, pivinv = ar.run(kp, flags, epoch, tol, eps)
    assert info == 0, info
    assert len(flags) == ar.nflags and np.all(flags == epoch)
    assert nper == sum(len(i["pert"]) for i in inputs)
    worst = ar.check(pivpos, pivinv, f"k_step<true> {name}")
    print(f"k_step<true> {name}: worst err / bound over the panels = {worst:.3f}")
    return ar, flags, pivpos


@pytest.mark.gpu
@pytest.mark.parametrize("tol,eps", LU_PARAMS)
def test_step_lu_outer_block(kp, tol, eps):
    """the fused steps of one outer block over seven panels in the same launches (one column without rows below; b crossing one
    16-column panel with a 1-row tile; a full block; b = 1 and b = 36 in a second step; pre-updates with bn = 2 and with K = 64,
    128, 192), then a refactorization with epoch 2 on the same flags with fresh values.
    Worst err / bound measured on an MI355X with the plain bound (the inverse-solve term |R^| |T_q^-T| |T_q^T| was not needed
    for any case of this file): tol 0: 0.133 (epoch 1) / 0.133 (epoch 2); tol 0.1: 0.155 / 0.178; tol 1.0: 0.163 / 0.127."""
    ar, flags, _ = _factor_and_check(kp, f"outer tol={tol} epoch=1", None, 1)
    assert sum(1 for t, _ in ar.launches for m in t["mode"] if m == 2) == 1 + 3       # (130, 65): one; (320, 130): K = 64, 128, 192
    _factor_and_check(kp, f"outer tol={tol} epoch=2", flags, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("tol,eps", LU_PARAMS)
def test_step_lu_second_outer_block(kp, tol, eps):
    """J = 512 of a 577-column panel with 3 rows below: two steps (b = 64, then b = 1) that touch only columns >= 512; the 512
    columns to the left hold NaN.  Worst err / bound measured: tol 0: 0.128 / 0.114; tol 0.1: 0.087 / 0.103; tol 1.0: 0.108 / 0.117."""
    ar, flags, _ = _factor_and_check(kp, f"second tol={tol} epoch=1", None, 1)
    assert all(int(t["J"].min()) >= 512 and int(t["diag"].min()) >= 512 for t, _ in ar.launches)
    _factor_and_check(kp, f"second tol={tol} epoch=2", flags, 2)


@pytest.mark.gpu
def test_step_lu_fast_path_hand_over(kp):
    """tol = 0.5, columns 0 .. 31 dominant: getrf_panel_natural does two 16-column panels, gives up in the third, and
    getrf_panel_wave goes on with the lanes' state; rows below, so both kinds of row task see a non-identity pivinv.
    Worst err / bound measured: 0.108."""
    _, _, pivpos = _factor_and_check(kp, "handover", None, 1)
    assert not np.array_equal(pivpos[3 + 32:3 + 64], 3 + np.arange(32, 64))


@pytest.mark.gpu
def test_step_lu_natural_order_with_pivoting_on(kp):
    """dominant input, tol = 0.1: nothing moves, yet pivpos is WRITTEN (the identity) -- the store path without reordering and
    the row tasks' identity skip.  Worst err / bound measured: 0.143."""
    ar, _, pivpos = _factor_and_check(kp, "natural", None, 1)
    for off, nscol, nsrow, ld, fc in ar.panels:
        assert np.array_equal(pivpos[fc:fc + nscol], fc + np.arange(nscol))


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [0.0, 1.0])
def test_step_lu_perturbation(kp, tol):
    """eps = 1e-8 on one-step panels whose diagonal block has one row twice its neighbour: nperturb equals the reference's
    count (asserted in _factor_and_check), the residual check holds with the replaced diagonal entry exempt.
    Worst err / bound measured: tol 0: 0.138; tol 1.0: 0.127."""
    _factor_and_check(kp, f"perturb tol={tol}", None, 1)


# ---------------------------------------------------------------------------------------------------------------------
# failure reporting: info bit 0 from both LU factorization kernels
# ---------------------------------------------------------------------------------------------------------------------
def _failing_block(rng, b, below, kind):
    inp = dict(nscol=b, below=below, pos=np.arange(b), pert=[])
    inp["A11"], inp["A21"], inp["A12"] = _draw(rng, b, below, 0.0, "dominant")
    if kind == "zero first column":
        inp["A11"][:, 0] = 0.0
    elif kind == "zero column":
        inp["A11"][:, b // 2] = 0.0
    else:
        inp["A11"][b // 3, b // 3] = np.nan
    return inp


FAILURES = [("zero first column", 0.0), ("zero column", 1.0), ("nan pivot", 0.0), ("nan pivot", 1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("b", [9, 33, 64])
@pytest.mark.parametrize("kind,tol", FAILURES)
def test_getrf_reports_zero_and_nan_pivots(kp, kind, tol, b):
    """k_getrf_block: a zero pivot that is not perturbed, and a NaN pivot, set info bit 0 (sf_panel.h, getrf_panel_wave)"""
    inp = _failing_block(np.random.default_rng(b), b, 0, kind)
    ar = LuArena([inp], 0, seed=b)
    off, nscol, nsrow, ld, fc = ar.panels[0]
    tasks = np.array([(off, ld, 0, b, fc)], dtype=POTRF_TASK)
    pivpos = np.full(ar.npiv, -5, dtype=np.int32) if tol > 0 else None
    pivinv = np.full(ar.npiv, -5, dtype=np.int32) if tol > 0 else None
    info, nper = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    _ok(kp.kp_getrf(P(ar.a), len(ar.a), P(tasks), 1, ar.u_shift, P(info), tol, 0.0, P(pivpos), P(pivinv), ar.npiv, P(nper)))
    assert info[0] & 1 and not info[0] & 2, info[0]
    kr.assert_unchanged(ar.before, ar.a, ar.written, f"k_getrf_block {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("b", [9, 33, 64])
@pytest.mark.parametrize("kind,tol", FAILURES)
def test_step_lu_reports_zero_and_nan_pivots(kp, kind, tol, b):
    """k_step<true>, step 0 of a panel with rows below: the same cases; the diagonal task still publishes its flag, so no row
    task runs into its wait limit (bit 1)"""
    inp = _failing_block(np.random.default_rng(b), b, 70, kind)
    ar = LuArena([inp], 0, seed=b)
    flags = np.zeros(ar.nflags, dtype=np.int32)
    info, _, _, _ = ar.run(kp, flags, 1, tol, 0.0)
    assert info & 1 and not info & 2, info
    assert np.all(flags == 1)
    kr.assert_unchanged(ar.before, ar.a, ar.written, f"k_step<true> {kind}")


# ---------------------------------------------------------------------------------------------------------------------
# the LU layout kernels: exact
# ---------------------------------------------------------------------------------------------------------------------
LAYOUT_PANELS = [(1, 1), (3, 10), (64, 64), (65, 130), (130, 131), (200, 260)]       # (nscol, nsrow)


class Layout:
    """a synthetic supernode table: L panels (nsrow x nscol, column-major) at Xp[s] in an arena, the U^T panels u_shift further;
    RefXp = the offsets of the (2 nsrow - nscol) x nscol panels of the host layout (lu) or of the nsrow x nscol ones (Cholesky)"""

    def __init__(self, shapes, seed, absent=()):
        rng = np.random.default_rng(seed)
        self.shapes, self.nsuper = shapes, len(shapes)
        self.Super = np.concatenate([[0], np.cumsum([c for c, r in shapes])]).astype(np.int32)
        self.Lsip = np.concatenate([[0], np.cumsum([r for c, r in shapes])]).astype(np.int64)
        ar = kr.Arena()
        self.Xp = np.array([ar.alloc(r * c, skew=s % 2) for s, (c, r) in enumerate(shapes)], dtype=np.int64)
        self.off = self.Xp.copy()
        for s in absent:                    # a sharded plan: the panel lives on another rank
            self.Xp[s] = -1
        self.u_shift = ar.size + 5
        ar.size = self.u_shift + ar.size + kr.GUARD
        self.a = ar.image()
        for c, r, off in ((c, r, off) for (c, r), off in zip(shapes, self.off)):
            for base in (off, off + self.u_shift):
                v = rng.uniform(-1, 1, r * c) * 10.0 ** rng.integers(-3, 4, r * c)
                v[rng.integers(0, r * c, max(1, r * c // 50))] = -0.0
                v[rng.integers(0, r * c, max(1, r * c // 50))] = 5e-324
                self.a[base:base + r * c] = v
        self.RefXp = {1: np.concatenate([[0], np.cumsum([(2 * r - c) * c for c, r in shapes])]).astype(np.int64),
                      0: np.concatenate([[0], np.cumsum([r * c for c, r in shapes])]).astype(np.int64)}

    def packed(self, s, lu=1):
        """panel s in the host layout, bit patterns: R < nscol: L(R, j) below the diagonal, U(R, j) = PU(j, R) from it on;
        R < nsrow: L21; else U12^T"""
        c, r = self.shapes[s]
        if self.Xp[s] < 0:
            return None
        PL = self.a[self.off[s]:self.off[s] + r * c].reshape(c, r).T
        PU = self.a[self.off[s] + self.u_shift:self.off[s] + self.u_shift + r * c].reshape(c, r).T
        if not lu:
            return kr.bits(PL.T.ravel())
        out = np.empty((2 * r - c, c))
        R, j = np.arange(c)[:, None], np.arange(c)[None, :]
        out[:c] = np.where(R > j, PL[:c], PU[:c].T)
        out[c:r] = PL[c:]
        out[r:] = PU[c:]
        return kr.bits(out.T.ravel())

    def packed_all(self):
        return np.concatenate([self.packed(s) if self.Xp[s] >= 0 else np.zeros(int(self.RefXp[1][s + 1] - self.RefXp[1][s]), dtype=np.uint64)
                               for s in range(self.nsuper)])

    def hashes(self, lu):
        H = np.zeros(self.nsuper, dtype=np.uint64)
        with np.errstate(over="ignore"):
            for s in range(self.nsuper):
                v = self.packed(s, lu)
                if v is not None:
                    e = np.arange(int(self.RefXp[lu][s]), int(self.RefXp[lu][s + 1]), dtype=np.uint64)
                    H[s] = np.sum(v * ((np.uint64(2) * e + np.uint64(1)) * np.uint64(HASH_K)), dtype=np.uint64)
        return H

    def args(self, lu=1):
        return P(self.Super), P(self.Lsip), P(self.Xp), P(self.RefXp[lu]), self.nsuper


@pytest.mark.gpu
def test_pack_lu_is_the_layout_comment(kp):
    """k_pack_lu against a numpy gather, bit for bit: the whole range, ranges that begin and end mid-column and mid-panel, an
    empty range, and a panel with Xp = -1 (zeros); nothing behind the range's end is written"""
    for absent in ((), (3,)):
        lay = Layout(LAYOUT_PANELS, 60, absent)
        want = lay.packed_all()
        total, rx = len(want), lay.RefXp[1]
        assert total == rx[-1]
        ranges = [(0, total), (0, 0), (7, 7), (int(rx[2]) + 70, int(rx[2]) + 75), (int(rx[1]) + 5, int(rx[4]) + 1000),
                  (int(rx[3]), int(rx[4])), (int(rx[5]) + 12345, total), (total - 1, total)]
        for e0, e1 in ranges:
            out = np.full(e1 - e0 + 64, -7.25)
            _ok(kp.kp_pack_lu(P(lay.a), len(lay.a), lay.u_shift, *lay.args(), P(out), len(out), e0, e1))
            assert np.array_equal(kr.bits(out[:e1 - e0]), want[e0:e1]), (absent, e0, e1)
            assert np.all(out[e1 - e0:] == -7.25), (absent, e0, e1)


def _fill_tiles(lay, windows):
    """the 64 x 64 tiles of the upper block triangle of columns [cb, ce) of each panel, as the plan cuts them"""
    tiles = []
    for s, (cb, ce) in windows.items():
        nscol, nsrow = lay.shapes[s]
        for c0 in range(cb // 64 * 64, ce, 64):
            for r0 in range(0, c0 + 1, 64):
                tiles.append((lay.off[s], nsrow, r0, c0, cb, ce))
    return np.array(tiles, dtype=FILL_TILE)


def _fill_expected(lay, windows):
    a, written = lay.a.copy(), np.zeros(len(lay.a), dtype=bool)
    for s, (cb, ce) in windows.items():
        nscol, nsrow = lay.shapes[s]
        j, R = np.nonzero(np.triu(np.ones((nscol, nscol), dtype=bool)).T)        # R <= j
        keep = (j >= cb) & (j < ce)
        j, R = j[keep], R[keep]
        iL = lay.off[s] + R + j * nsrow
        a[iL] = lay.a[lay.off[s] + lay.u_shift + j + R * nsrow]                   # PL(R, j) = PU(j, R)
        written[iL] = True
    return a, written


FILL_WINDOWS = {0: (0, 1), 1: (1, 3), 2: (0, 64), 3: (0, 65), 4: (70, 129), 5: (65, 190)}


@pytest.mark.gpu
def test_lu_fill_u11_windows(kp):
    """k_lu_fill_u11 on 64 x 64 tiles with column windows that start and end inside a tile: PL(R, j) == PU(j, R) for R <= j
    inside the window, bit for bit; everything else in both arenas unchanged"""
    lay = Layout(LAYOUT_PANELS, 61)
    tiles = _fill_tiles(lay, FILL_WINDOWS)
    want, written = _fill_expected(lay, FILL_WINDOWS)
    before = lay.a.copy()
    _ok(kp.kp_lu_fill_u11(P(lay.a), len(lay.a), lay.u_shift, P(tiles), len(tiles)))
    kr.assert_unchanged(before, lay.a, written, "k_lu_fill_u11")
    assert written.sum() > 20000
    assert np.array_equal(kr.bits(lay.a)[written], kr.bits(want)[written])


_SMALL = [(1, 1), (3, 10), (2, 5), (4, 4), (5, 40), (7, 9)]
HASH_TABLES = {         # name: (Cholesky table, LU table); the totals and boundaries are asserted in the test
    "under 256 values": ([(1, 1), (3, 10)], [(1, 1), (3, 10)]),
    "several small panels in one chunk": (_SMALL, _SMALL),
    "just over one chunk": ([(64, 257)], [(127, 129)]),                         # 257 * 64 = 16448; (258 - 127) * 127 = 16637
    "a chunk boundary on a panel boundary": ([(64, 256), (3, 10), (65, 130)], [(64, 160), (3, 10), (65, 130)]),   # 16384 first
    "several chunks": (LAYOUT_PANELS, LAYOUT_PANELS),
}


@pytest.mark.gpu
@pytest.mark.parametrize("lu", [0, 1])
@pytest.mark.parametrize("table", sorted(HASH_TABLES))
def test_factor_hash_is_the_documented_sum(kp, table, lu):
    """H[s] = sum bits(v_e) (2 e + 1) K mod 2^64 over the values of panel s in the host layout, exactly; a panel with Xp = -1 adds
    nothing; H is added to, not overwritten"""
    shapes = HASH_TABLES[table][lu]
    for absent in ((), (len(shapes) - 1,), (0,)):
        lay = Layout(shapes, 62 + lu, absent)
        total = int(lay.RefXp[lu][-1])
        if table == "under 256 values":
            assert total < 256
        elif table == "just over one chunk":
            assert 16384 < total < 16384 + 512 and total % 256
        elif table == "a chunk boundary on a panel boundary":
            assert lay.RefXp[lu][1] == 16384 and total > 16384
        elif table == "several chunks":
            assert total > 3 * 16384 and total % 256 and all(x % 16384 for x in lay.RefXp[lu][1:])
        H = np.arange(lay.nsuper, dtype=np.uint64) * np.uint64(3)
        want = H + lay.hashes(lu)
        _ok(kp.kp_factor_hash(P(lay.a), len(lay.a), lay.u_shift, *lay.args(lu), lu, total, P(H)))
        assert np.array_equal(H, want), (table, lu, absent, H, want)
        assert all(want[s] == 3 * s for s in absent)


@pytest.mark.gpu
def test_factor_hash_does_not_see_the_u11_fill(kp):
    """lu: the same hash before and after k_lu_fill_u11 has run on the arena (the value is gathered as k_pack_lu gathers it)"""
    lay = Layout(LAYOUT_PANELS, 64)
    total = int(lay.RefXp[1][-1])
    H0 = np.zeros(lay.nsuper, dtype=np.uint64)
    _ok(kp.kp_factor_hash(P(lay.a), len(lay.a), lay.u_shift, *lay.args(), 1, total, P(H0)))
    assert np.array_equal(H0, lay.hashes(1))
    tiles = _fill_tiles(lay, FILL_WINDOWS)
    before = lay.a.copy()
    _ok(kp.kp_lu_fill_u11(P(lay.a), len(lay.a), lay.u_shift, P(tiles), len(tiles)))
    assert not np.array_equal(kr.bits(before), kr.bits(lay.a))
    H1 = np.zeros(lay.nsuper, dtype=np.uint64)
    _ok(kp.kp_factor_hash(P(lay.a), len(lay.a), lay.u_shift, *lay.args(), 1, total, P(H1)))
    assert np.array_equal(H1, H0)
