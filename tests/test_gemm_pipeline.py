"""k_gemm's K-loop pipeline and its tile changes, through single launches of the probe (tests/kernels/sf_kprobe.hip).

The LDS-DMA instantiation of k_gemm multiplies out of a ring of four 8-deep stages (csrc/sf_kernels.hip).  What can go wrong in
such a loop is specific to where a K range starts and ends in the ring, and to what one tile leaves behind for the next one of
the same workgroup: every K from one stage to one full turn of the ring plus one stage, unit windows that begin and end
mid-tile (the ring is filled and drained without ever being full), and task lists in which tiles of different problems, K
lengths, leading dimensions and relative maps follow one another inside ONE workgroup.

Bounds are kernel_ref's (SAFETY (K + 2) u (|C0| + |Y| |X|^T)).  Where a tile's K range is applied in p pieces (windows), the
result carries p roundings of the running sum in place of one; first-order error (K + p) u (|C0| + |Y| |X|^T), which the same
bound covers as long as p <= 3 K + 6 -- p is at most the tile's number of 16-deep K steps here.
"""
import numpy as np
import pytest

import kernel_ref as kr
from test_kernels import GEMM_PROB, GEMM_TASK, GemmCase, _gemm_tiles, _kt_prefix, _ok, _relmap, _run_gemm, P, kp  # noqa: F401

pytestmark = pytest.mark.gpu

RING_K = [1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 40, 41, 47, 49, 65]     # every stage boundary up to 4 stages + 1, and past it
RING_M = [1, 65, 129]


def _launch(kp, case, tasks, **kw):
    rel = _relmap(kp, case) if case.mode == 1 else None
    return _run_gemm(kp, case, tasks, relmap=rel, **kw)


@pytest.mark.parametrize("mode", [0, 1])
def test_ring_fill_and_drain(kp, mode):
    """one problem, one workgroup: K over every stage boundary of the ring, M = N below, at and past one tile"""
    rng = np.random.default_rng(40 + mode)
    for K in RING_K:
        for M in RING_M:
            for strict in (0, 1):
                case = GemmCase(rng, M, M, K, strict, mode, 1)
                assert case.prob[0]["lda"] % 2 == 1
                out = _launch(kp, case, _gemm_tiles(M, M, K), cap=1, ticket=(K + M + strict) % 2)
                case.check(out, f"k_gemm<{mode}> M=N={M} K={K} strict={strict} cap=1")


@pytest.mark.parametrize("mode", [0, 1])
def test_mid_tile_windows(kp, mode):
    """three tiles of nkt K steps each.  [1, U - 1) makes one workgroup run a head share that begins at unit 1 of a tile, a
    whole tile, and a tail share that ends one unit before its tile's end; [0, 1) and [U - 1, U) are shares of one unit (two
    stages: the ring is never full).  The three windows, and every unit on its own, add up to the full update."""
    rng = np.random.default_rng(50 + mode)
    for i, K in enumerate([17, 33, 49, 65]):
        case = GemmCase(rng, 129, 129, K, i % 2, mode, 1)
        rel = _relmap(kp, case) if mode == 1 else None
        tasks = _gemm_tiles(129, 129, K)
        pre = _kt_prefix(tasks)
        U = int(pre[-1])
        assert len(tasks) == 3 and U == 3 * ((K + 15) // 16)
        for cap in (1, 2, 9):
            a = case.arena
            for lo, hi in ((1, U - 1), (0, 1), (U - 1, U)):
                a = _run_gemm(kp, case, tasks, lo, hi, relmap=rel, cap=cap, arena=a)
            case.check(a, f"k_gemm<{mode}> K={K} windows [1, {U - 1}) [0, 1) [{U - 1}, {U}) cap={cap}")
        a = case.arena
        for u in range(U):
            a = _run_gemm(kp, case, tasks, u, u + 1, relmap=rel, cap=1, ticket=u % 2, arena=a)
        case.check(a, f"k_gemm<{mode}> K={K} every unit alone")


class Problems:
    """several GemmCases of one mode in one arena (their own arenas, NaN guards included, one behind the other)"""

    def __init__(self, cases):
        self.cases, self.mode = cases, cases[0].mode
        self.prob = np.concatenate([c.prob for c in cases])
        base = np.concatenate([[0], np.cumsum([len(c.arena) for c in cases])])
        mbase = np.concatenate([[0], np.cumsum([len(c.relmap_want) for c in cases])]) if self.mode == 1 else np.zeros(len(cases) + 1)
        for i in range(len(cases)):
            for f in ("y_off", "x_off", "c_off"):
                self.prob[i][f] += base[i]
            self.prob[i]["map_off"] += int(mbase[i])
        self.arena = np.concatenate([c.arena for c in cases])
        self.before = self.arena.copy()
        self.tgt = [c.tgt + base[i] for i, c in enumerate(cases)]

    def relmap(self, kp):
        return np.concatenate([_relmap(kp, c) for c in self.cases]) if self.mode == 1 else None

    def check(self, after, what):
        written = np.zeros(len(after), dtype=bool)
        for i, c in enumerate(self.cases):
            written[self.tgt[i]] = True
            ci, cj = np.nonzero(c.mask)
            kr.assert_within(after[self.tgt[i]], c.ref[ci, cj], c.bound[ci, cj], f"{what}, problem {i} (M={c.M} N={c.N} K={c.K})")
        kr.assert_unchanged(self.before, after, written, what)


def _hand_over(mode):
    """problem 0: 257 x 129, K = 200 (a diagonal tile, a FULL tile, a diagonal tile one column wide, two tiles one row high);
    problem 1: 17 x 17, K = 24 (one tile, diagonal and ragged); problem 2: 129 x 129, K = 1.  Different lda / ldc / maps each.
    The order puts a tile with idle waves (diagonal or ragged), a full tile and a tile of another problem behind one another;
    the reversed list gives the other direction."""
    rng = np.random.default_rng(60 + mode)
    pr = Problems([GemmCase(rng, 257, 129, 200, 0, mode, 1), GemmCase(rng, 17, 17, 24, 1, mode, 0), GemmCase(rng, 129, 129, 1, 0, mode, 1)])
    assert len({int(p["lda"]) for p in pr.prob}) == 3 and len({int(p["ldc"]) for p in pr.prob}) == 3
    t = {(p, tm, tn): (p, tm, tn, 0, (K + 15) // 16) for p, (M, N, K) in enumerate([(257, 129, 200), (17, 17, 24), (129, 129, 1)])
         for tm in range((M + 127) // 128) for tn in range((N + 127) // 128) if tm >= tn}
    order = [(0, 0, 0), (0, 1, 0), (2, 0, 0), (0, 2, 0), (1, 0, 0), (0, 1, 1), (2, 1, 0), (0, 2, 1), (2, 1, 1)]
    assert sorted(order) == sorted(t)
    return pr, np.array([t[k] for k in order], dtype=GEMM_TASK)


def _run_problems(kp, pr, tasks, rel, **kw):
    return _run_gemm(kp, pr, tasks, relmap=rel, **kw)


@pytest.mark.parametrize("mode", [0, 1])
def test_tile_hand_over(kp, mode):
    """one workgroup takes tiles of three problems one after the other: each problem's targets are right and nothing else
    changed (a row / column map or an operand stage left over from the previous tile would show as either)"""
    pr, tasks = _hand_over(mode)
    rel = pr.relmap(kp)
    for name, tl in (("forward", tasks), ("reversed", tasks[::-1].copy())):
        for ticket in (0, 1):
            out = _run_problems(kp, pr, tl, rel, cap=1, ticket=ticket)
            pr.check(out, f"k_gemm<{mode}> hand-over {name} ticket={ticket}")


@pytest.mark.parametrize("mode", [0, 1])
def test_last_tile(kp, mode):
    """task lists of one and of two tiles: the last (partial) round has no next tile"""
    rng = np.random.default_rng(70 + mode)
    for M, N, K in ((65, 65, 24), (129, 65, 40)):
        case = GemmCase(rng, M, N, K, 0, mode, 1)
        rel = _relmap(kp, case) if mode == 1 else None
        tasks = _gemm_tiles(M, N, K)
        assert len(tasks) == (1 if M == 65 else 2)
        for cap in (1, 5):
            for whole in (0, 1):
                out = _run_gemm(kp, case, tasks, relmap=rel, cap=cap, whole=whole, ticket=(cap + whole) % 2)
                case.check(out, f"k_gemm<{mode}> {len(tasks)} tiles cap={cap} whole={whole}")


@pytest.mark.parametrize("mode", [0, 1])
def test_whole_tiles_bit_equal_over_grids(kp, mode):
    """whole_tiles: the hand-over list gives the same bits whatever the grid and the deal (one addition per element, and the
    order in which k is accumulated inside a tile does not depend on what the workgroup ran before)"""
    pr, tasks = _hand_over(mode)
    rel = pr.relmap(kp)
    first = None
    for cap in (1, 5, 64):
        for ticket in (0, 1):
            out = _run_problems(kp, pr, tasks, rel, cap=cap, ticket=ticket, whole=1)
            if first is None:
                pr.check(out, f"k_gemm<{mode}> whole_tiles")
                first = out
            else:
                assert np.array_equal(kr.bits(out), kr.bits(first)), f"k_gemm<{mode}> whole_tiles: cap={cap} ticket={ticket} differs"
