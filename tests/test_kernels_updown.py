"""Single-launch tests of the update / downdate kernels (csrc/sf_updown.hip): k_updown_diag and k_updown_rows through the
launchers the plan calls (sf_kernels.h: launch_updown_diag, launch_updown_rows), on operands the test builds itself.  The probe
tests/kernels/sf_kprobe_updown.hip is built by this module with the hipcc line of tests/kernels/Makefile.

Every double operand of a launch lies in ONE host image (kernel_ref.Arena) whose guard bands and every element a launch must not
read hold NaN: the strict upper triangle of the diagonal block, the panel rows around the ones a launch owns, the rows of W of other
supernodes (the gaps of the row list), the columns of W and the rotation pairs behind the kernel's width, the pairs of columns
j >= b.  Everything outside the documented write set is compared bit for bit:
    diag   writes the lower triangle of the b x b block, the pairs (j < b, t < kw), ALL 16 columns of the block's b rows of W (zeros)
    rows   writes the b columns of its nrows panel rows and the columns t < kw of the rows of W its row list names
Results are compared with tests/updown_ref.py's emulation of the same launch.  The two differ by the device's fused multiply-adds
only; the bound is per rotation count, not measured: a value passes through at most b kw rotations of at most 4 roundings each
(multiply, add, multiply by 1 / c; the pair itself carries 3 more), relative to the launch's largest operand:
SAFETY (4 b kw + 8) u max(|L|, |W|).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kernel_ref as kr
import updown_ref as ur
from util import ROOT

pytestmark = pytest.mark.gpu

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KDIR = os.path.join(ROOT, "tests", "kernels")
PKG = os.path.join(ROOT, "sparse-matrix-factorization-library_amd")
NAN = np.nan
UPD_W, UPD_B = 16, 64
BS = (1, 63, 64)
KS = (1, 16)
BELOW = (0, 1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def kp(tmp_path_factory):
    src = os.path.join(KDIR, "sf_kprobe_updown.hip")
    out = str(tmp_path_factory.mktemp("kprobe_updown") / "libsf_kprobe_updown.so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(PKG, "csrc"),
                        "-I" + os.path.join(ROOT, "include"), src, "-o", out, "-L" + PKG, "-lsparseframe_hip", "-Wl,-rpath," + PKG],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(out)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.kp_updown_diag.argtypes = [vp, i64, i64, i64, i32, i32, i32, i64, i64, i64, vp]
    L.kp_updown_rows.argtypes = [vp, i64, i64, i64, i32, i64, vp, i32, i32, i64, i64]
    return L


def _bound(b, kw, *operands):
    return kr.SAFETY * (4 * b * kw + 8) * kr.U * max(float(np.max(np.abs(o))) for o in operands if o.size)


def _block(rng, b):
    """a well-conditioned lower factor"""
    D = np.tril(rng.uniform(-1, 1, (b, b))) * 0.3
    D[np.arange(b), np.arange(b)] = rng.uniform(1.5, 2.5, b)
    return D


def _w_for(rng, D, kw, sign):
    """b x kw rows of W; for a downdate scaled so that sum_t |D^-1 w_t|^2 <= 1/2: the block stays definite with a margin"""
    W = rng.uniform(-1, 1, (D.shape[0], kw))
    if sign < 0:
        W *= np.sqrt(0.5 / np.sum(np.linalg.solve(D, W) ** 2))
    return W


class DiagCase:
    """the image of one k_updown_diag launch"""

    def __init__(self, b, kw, sign, seed):
        rng = np.random.default_rng(seed)
        self.b, self.kw, self.sign = b, kw, sign
        self.ld, self.r0, self.col0, self.nw = b + 7, 3, 5, b + 9       # the block sits at rows r0 .. of a taller panel; W has rows around it
        ar = kr.Arena()
        self.offP = ar.alloc(self.ld * b, align=2, skew=1)
        self.offW = ar.alloc(self.nw * UPD_W)
        self.offR = ar.alloc(2 * UPD_B * UPD_W)
        self.img = ar.image()
        self.D = _block(rng, b)
        self.W = _w_for(rng, self.D, kw, sign)
        P = self.panel(self.img)
        low = np.tril(np.ones((b, b), dtype=bool))
        P[self.r0:self.r0 + b][low] = self.D[low]
        self.wblock(self.img)[self.col0:self.col0 + b, :kw] = self.W
        self.written = np.zeros(self.img.size, dtype=bool)
        m = self.panel(self.written)
        m[self.r0:self.r0 + b][low] = True
        self.wblock(self.written)[self.col0:self.col0 + b, :] = True
        self.rot(self.written)[:b, :kw, :] = True

    def panel(self, a):
        return a[self.offP:self.offP + self.ld * self.b].reshape(self.b, self.ld).T

    def wblock(self, a):
        return a[self.offW:self.offW + self.nw * UPD_W].reshape(self.nw, UPD_W)

    def rot(self, a):
        return a[self.offR:self.offR + 2 * UPD_B * UPD_W].reshape(UPD_B, UPD_W, 2)

    def launch(self, kp, info=0):
        out = self.img.copy()
        word = np.array([info], dtype=np.int32)
        rc = kp.kp_updown_diag(out.ctypes.data, out.size, self.offP + self.r0, self.ld, self.b, self.kw, self.sign, self.offW, self.col0,
                               self.offR, word.ctypes.data)
        assert rc == 0, f"HIP error {rc}"
        return out, int(word[0])


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("kw", KS)
@pytest.mark.parametrize("b", BS)
def test_diag_launch(kp, b, kw, sign):
    c = DiagCase(b, kw, sign, 1000 * b + 10 * kw + sign)
    out, info = c.launch(kp)
    assert info == 0
    kr.assert_unchanged(c.img, out, c.written, f"diag b={b} kw={kw}")
    D, W = np.tril(c.D), c.W.copy()
    rot, bad = ur.diag_emulate(D, W, sign)
    assert not bad
    tol = _bound(b, kw, c.D, c.W)
    low = np.tril(np.ones((b, b), dtype=bool))
    got = c.panel(out)[c.r0:c.r0 + b]
    assert np.all(np.isfinite(got[low])) and np.max(np.abs(got[low] - D[low])) <= tol
    assert np.max(np.abs(c.rot(out)[:b, :kw] - rot)) <= tol
    assert not np.any(c.wblock(out)[c.col0:c.col0 + b])                # zeros, all 16 columns
    assert not np.any(np.signbit(c.wblock(out)[c.col0:c.col0 + b]))


@pytest.mark.parametrize("b,kw", [(1, 1), (63, 16), (64, 1)])
def test_diag_failure_and_identity(kp, b, kw):
    """a radicand that is not positive sets the word and makes every later rotation the identity; a word that is set on entry makes
    all of them identities: pairs (1, 0), the block's values unchanged, the rows of W zeroed all the same"""
    c = DiagCase(b, kw, -1, 77 + b)
    jbad = b // 2
    c.wblock(c.img)[c.col0 + jbad, 0] = 2.0 * c.D[jbad, jbad] + 1.0
    out, info = c.launch(kp)
    assert info == 1
    kr.assert_unchanged(c.img, out, c.written, "failing downdate")
    assert np.all(c.rot(out)[jbad + 1:b, :kw] == np.array([1.0, 0.0]))
    low = np.tril(np.ones((b, b), dtype=bool))
    after = low.copy()
    after[:, :jbad + 1] = False                                         # the columns behind the failing one keep their values
    assert np.array_equal(c.panel(out)[c.r0:c.r0 + b][after], c.D[after])
    # NaN takes the same branch
    c2 = DiagCase(b, kw, +1, 78 + b)
    c2.wblock(c2.img)[c2.col0, 0] = NAN
    assert c2.launch(kp)[1] == 1
    # set on entry
    c3 = DiagCase(b, kw, -1, 79 + b)
    out, info = c3.launch(kp, info=1)
    assert info == 1
    kr.assert_unchanged(c3.img, out, c3.written, "word set on entry")
    assert np.all(c3.rot(out)[:b, :kw] == np.array([1.0, 0.0]))
    assert np.array_equal(c3.panel(out)[c3.r0:c3.r0 + b][low], c3.D[low])
    assert not np.any(c3.wblock(out)[c3.col0:c3.col0 + b])


class RowsCase:
    """the image of one k_updown_rows launch: nrows panel rows in the middle of a taller panel, a row list with gaps"""

    def __init__(self, b, kw, nrows, sign, seed):
        rng = np.random.default_rng(seed)
        self.b, self.kw, self.nrows, self.sign = b, kw, nrows, sign
        self.r0, self.ld = 2, nrows + 5
        i = np.arange(nrows)
        self.rows = (4 + 2 * i + (i % 3 == 0) + 3 * (i // 64)).astype(np.int32)       # distinct, ascending, gaps of 1 .. 5 rows
        self.nw = int(self.rows[-1]) + 4 if nrows else 8
        ar = kr.Arena()
        self.offP = ar.alloc(self.ld * b, align=2, skew=1)
        self.offW = ar.alloc(self.nw * UPD_W)
        self.offR = ar.alloc(2 * UPD_B * UPD_W)
        self.img = ar.image()
        # pairs that a diagonal launch would leave: those of a random block
        D = _block(rng, b)
        self.rotv, bad = ur.diag_emulate(D, _w_for(rng, D, kw, sign), sign)
        assert not bad
        self.rot(self.img)[:b, :kw] = self.rotv
        self.P = rng.uniform(-1, 1, (nrows, b))
        self.W = rng.uniform(-1, 1, (nrows, kw))
        self.panel(self.img)[self.r0:self.r0 + nrows] = self.P
        self.wblock(self.img)[self.rows, :kw] = self.W
        self.written = np.zeros(self.img.size, dtype=bool)
        self.panel(self.written)[self.r0:self.r0 + nrows] = True
        self.wblock(self.written)[self.rows, :kw] = True

    panel, wblock, rot = DiagCase.panel, DiagCase.wblock, DiagCase.rot

    def launch(self, kp):
        out = self.img.copy()
        rows = self.rows if self.nrows else np.zeros(1, dtype=np.int32)
        rc = kp.kp_updown_rows(out.ctypes.data, out.size, self.offP + self.r0, self.ld, self.b, self.nrows, rows.ctypes.data, self.kw,
                               self.sign, self.offW, self.offR)
        assert rc == 0, f"HIP error {rc}"
        return out


def test_row_list_has_gaps():
    c = RowsCase(3, 1, 257, +1, 0)
    d = np.diff(c.rows)
    assert len(set(c.rows.tolist())) == 257 and d.min() >= 1 and d.max() >= 4 and set(d.tolist()) >= {1, 2, 3}


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("nrows", BELOW)
@pytest.mark.parametrize("kw", KS)
@pytest.mark.parametrize("b", BS)
def test_rows_launch(kp, b, kw, nrows, sign):
    c = RowsCase(b, kw, nrows, sign, 100000 * b + 1000 * kw + 2 * nrows + (sign > 0))
    out = c.launch(kp)
    kr.assert_unchanged(c.img, out, c.written, f"rows b={b} kw={kw} nrows={nrows}")
    if nrows == 0:
        assert np.array_equal(kr.bits(out), kr.bits(c.img))            # no launch at all
        return
    P, W = c.P.copy(), c.W.copy()
    ur.rows_emulate(P, W, c.rotv, sign)
    tol = _bound(b, kw, c.P, c.W, P, W)
    gotP, gotW = c.panel(out)[c.r0:c.r0 + nrows], c.wblock(out)[c.rows, :kw]
    assert np.all(np.isfinite(gotP)) and np.all(np.isfinite(gotW))
    assert np.max(np.abs(gotP - P)) <= tol and np.max(np.abs(gotW - W)) <= tol


@pytest.mark.parametrize("kw", KS)
def test_rows_identity_pairs_keep_the_bits(kp, kw):
    """pairs (1, 0) -- a column of W that is zero on the block, or a failed downdate -- reproduce the panel and W bit for bit"""
    c = RowsCase(64, kw, 65, -1, 5)
    c.rot(c.img)[:64, :kw] = (1.0, 0.0)
    out = c.launch(kp)
    assert np.array_equal(kr.bits(out), kr.bits(c.img))
