"""Python mirror of the reference's operator interface for the numeric-factorization path.

Two views of the same C ABI (include/sparseframe_hip.h):

* ``MatrixInfo`` / ``CommonInfo`` wrap ``struct matrix_info_struct`` / ``struct common_info_struct``
  (reference Cholesky/Include/info.h:12-29, :70-150) and call the struct-based entry points with the
  reference's own names: ``analyze`` -> SparseFrame_analyze (SparseFrame.c:1916), ``factorize`` ->
  SparseFrame_factorize (:3019), ``solve`` -> SparseFrame_solve_supernodal (:3036), ``validate`` ->
  SparseFrame_validate (:3141), ``cleanup`` -> SparseFrame_cleanup_matrix (:3268).
* ``Symbolic`` / ``CholPlan`` wrap the flat plan ABI (sf_symbolic_*, sf_chol_plan_*), which keeps the
  factor resident in HBM between calls -- this is what bench.py times.
"""
import ctypes as C

import numpy as np

from ._lib import lib, lu_lib, check, c_long_p, c_double_p, SparseFrameError

# devSlotSize the reference computes (SparseFrame.c:82-87,199) for 288 GiB devices
REFERENCE_SLOT_1GPU = 8_694_792_192     # 1 device  -> numSplit 4
REFERENCE_SLOT_8GPU = 34_781_265_920    # >=4 devices -> numSplit 1


def _lp(a):
    return a.ctypes.data_as(c_long_p)


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _solve_many(fn, name, h, n, B):
    """(n, k) right-hand sides in any memory order -> (n, k) float64 solution, through the column-major flat ABI"""
    B = np.asarray(B)
    if B.ndim != 2 or B.shape[0] != n:
        raise ValueError(f"solve_many: B must have shape ({n}, k), got {B.shape}")
    Bf = np.asfortranarray(B, dtype=np.float64)
    k = B.shape[1]
    X = np.empty((n, k), dtype=np.float64, order="F")
    if k:
        check(fn(h, k, _dp(Bf), max(n, 1), _dp(X), max(n, 1)), name)
    return X


def _lu_solve_guarded(S, r, message):
    """S^-1 r by LU with partial pivoting on the host (S: (k, k), small).  ValueError(message) when S is singular: a zero pivot, one
    that is not finite, or one below 8 k eps of the largest entry its column of S had before the elimination -- a pivot that
    rounding alone could have produced; the solution would be noise"""
    A = np.array(S, dtype=np.float64)
    y = np.array(r, dtype=np.float64)
    k = A.shape[0]
    floor = 8 * k * np.finfo(np.float64).eps * np.abs(A).max(axis=0)
    for j in range(k):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        piv = A[p, j]
        if not np.isfinite(piv) or abs(piv) <= floor[j]:
            raise ValueError(message)
        if p != j:
            A[[j, p]] = A[[p, j]]
            y[[j, p]] = y[[p, j]]
        l = A[j + 1:, j] / piv
        A[j + 1:, j + 1:] -= np.outer(l, A[j, j + 1:])
        y[j + 1:] -= l * y[j]
    for j in range(k - 1, -1, -1):
        y[j] = (y[j] - A[j, j + 1:] @ y[j + 1:]) / A[j, j]
    return y


def device_count():
    return int(lib.sf_device_count())


def grid_nd_perm(nx, ny=1, nz=1, leaf=3, sep_width=1):
    """Deterministic geometric nested dissection of a regular grid; perm[new] = old."""
    perm = np.empty(nx * ny * nz, dtype=np.int64)
    check(lib.sf_grid_nd_perm(nx, ny, nz, leaf, sep_width, _lp(perm)), "sf_grid_nd_perm")
    return perm


def graph_nd_perm(n, Cp, Ci, leaf=64):
    """Built-in nested dissection (BFS level-structure separators) for a general symmetric pattern; perm[new] = old."""
    Cp, Ci = _i64(Cp), _i64(Ci)
    perm = np.empty(max(n, 1), dtype=np.int64)
    check(lib.sf_graph_nd_perm(n, _lp(Cp), _lp(Ci), leaf, _lp(perm)), "sf_graph_nd_perm")
    return perm[:n]


class Symbolic:
    """Result of the host-side symbolic analysis (flat ABI)."""

    LONG_ARRAYS = ("Perm", "Parent", "Parent0", "Post", "ColCount", "ColCount0", "Lp", "Li", "LTp", "LTi",
                   "Up", "Ui", "UTp", "UTi", "Super", "SuperMap", "Sparent", "Lsip", "Lsxp", "Lsi", "LeafQueue",
                   "ST_Map", "ST_Pointer", "ST_Index", "Aoffset", "Moffset")
    SCALARS = ("n", "nnz", "nfsuper", "nsuper", "nstage", "isize", "xsize", "csize", "nsleaf", "lu", "symmetric", "unz")

    def __init__(self, n, Cp, Ci, Cx, perm=None, dev_slot_size=REFERENCE_SLOT_1GPU, method="cholesky", symmetric=True):
        """method 'cholesky' (input = one triangle) or 'lu' (symmetric=True: one triangle, else the whole matrix)"""
        Cp, Ci, Cx = _i64(Cp), _i64(Ci), _f64(Cx)
        if perm is not None:
            perm = _i64(perm)
        h = C.c_void_p()
        if method == "cholesky":
            check(lib.sf_symbolic_create(C.byref(h), n, _lp(Cp), _lp(Ci), _dp(Cx),
                                         _lp(perm) if perm is not None else None, dev_slot_size),
                  "sf_symbolic_create")
        elif method == "lu":
            check(lib.sf_symbolic_create_lu(C.byref(h), n, _lp(Cp), _lp(Ci), _dp(Cx),
                                            _lp(perm) if perm is not None else None, dev_slot_size,
                                            1 if symmetric else 0), "sf_symbolic_create_lu")
        else:
            raise ValueError(method)
        self.method = method
        self._h = h
        self._cache = {}
        self.dev_slot_size = dev_slot_size
        self._input = (n, Cp, Ci, perm, bool(symmetric))

    def close(self):
        if getattr(self, "_h", None):
            lib.sf_symbolic_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name in Symbolic.SCALARS:
            return int(lib.sf_symbolic_scalar(self._h, name.encode()))
        if name in Symbolic.LONG_ARRAYS:
            if name not in self._cache:
                ln = C.c_int64()
                p = lib.sf_symbolic_long_array(self._h, name.encode(), C.byref(ln))
                self._cache[name] = (np.ctypeslib.as_array(p, shape=(ln.value,)).copy()
                                     if ln.value else np.zeros(0, np.int64))
            return self._cache[name]
        if name in ("Lx", "LTx", "Ux", "UTx"):
            if name not in self._cache:
                ln = C.c_int64()
                p = lib.sf_symbolic_float_array(self._h, name.encode(), C.byref(ln))
                self._cache[name] = (np.ctypeslib.as_array(p, shape=(ln.value,)).copy()
                                     if ln.value else np.zeros(0))
            return self._cache[name]
        raise AttributeError(name)

    def value_map(self):
        """(nsrc, mapL, mapU) for set_value_map: mapL[p] (mapU[p]) is the position in the caller's own value array Cx -- the one
        this analysis was given, nsrc = Cp[n] entries -- that entry p of Lx (Ux) is taken from, or -1 for an entry the caller does
        not supply (value 0); mapU is None unless this is an LU analysis of an unsymmetric input.  So Lx == where(mapL >= 0,
        Cx[mapL], 0) for ANY values on the same pattern; an entry given more than once follows the analysis' own rule.
        Costs one more analysis: the pattern is analysed again with the values 1, 2, ..., nsrc (exact in fp64 below 2^53) and
        the positions are read off the resulting Lx / Ux."""
        n, Cp, Ci, perm, symmetric = self._input
        nsrc = int(Cp[n]) if n > 0 else 0
        if nsrc >= 1 << 53:
            raise ValueError("value_map: more than 2^53 entries")
        tag = np.zeros(len(Ci), dtype=np.float64)
        tag[:nsrc] = 1.0 + np.arange(nsrc, dtype=np.float64)
        twin = Symbolic(n, Cp, Ci, tag, perm, self.dev_slot_size, self.method, symmetric)
        mapL = np.rint(twin.Lx).astype(np.int64) - 1
        mapU = np.rint(twin.Ux).astype(np.int64) - 1 if self.method == "lu" and not symmetric else None
        twin.close()
        return nsrc, mapL, mapU

    @property
    def flops_struct(self):
        return float(lib.sf_symbolic_flops(self._h, 0))

    @property
    def flops_exec(self):
        return float(lib.sf_symbolic_flops(self._h, 1))

    @property
    def flops_update(self):
        return float(lib.sf_symbolic_flops(self._h, 2))

    @property
    def scatter_elems(self):
        return float(lib.sf_symbolic_flops(self._h, 3))


def analyze(n, Cp, Ci, Cx, perm=None, dev_slot_size=REFERENCE_SLOT_1GPU, method="cholesky", symmetric=True):
    return Symbolic(n, Cp, Ci, Cx, perm, dev_slot_size, method, symmetric)


def validate_solution(sym, x, b=None):
    """the reference's SparseFrame_validate residual (SparseFrame.c:3182-3263) for a given solution x of the permuted
    system: b_i = 1 + i/n, r = A x - b with the stored triangle used symmetrically,
    |r|_inf / (|A|_1 |x|_inf + |b|_inf).  Vectorised numpy (host check of a device solve)."""
    n = sym.n
    if b is None:
        b = 1 + np.arange(n) / n
    Lp, Li, Lx = sym.Lp, sym.Li, sym.Lx
    cols = np.repeat(np.arange(n), np.diff(Lp))
    # (np.bincount with weights: the same sums as np.add.at, an order of magnitude faster at n = 16.8 M)
    r = -np.asarray(b, dtype=np.float64).copy()
    r += np.bincount(Li, weights=Lx * x[cols], minlength=n)
    off = Li != cols
    r += np.bincount(cols[off], weights=Lx[off] * x[Li[off]], minlength=n)
    ax = np.abs(Lx)
    colsum = np.bincount(cols, weights=ax, minlength=n) + np.bincount(Li[off], weights=ax[off], minlength=n)
    return float(np.abs(r).max() / (colsum.max() * np.abs(x).max() + np.abs(b).max()))


def subtree_partition(sym, nranks, top_weight=1.0):
    """owner[s] = rank of the elimination-tree subtree holding supernode s, -1 for the top supernodes.
    top_weight: cost of a top flop relative to a subtree flop (1 = replicated top, ~1/nranks = distributed top).
    Returns (owner int32[nsuper], top flop fraction, heaviest rank's subtree flop fraction)."""
    owner = np.empty(max(sym.nsuper, 1), dtype=np.int32)
    tf, ml = C.c_double(), C.c_double()
    check(lib.sf_subtree_partition_weighted(sym.nsuper, _lp(sym.Super), _lp(sym.SuperMap), _lp(sym.Lsip), _lp(sym.Lsi),
                                            nranks, float(top_weight), owner.ctypes.data_as(C.POINTER(C.c_int32)),
                                            C.byref(tf), C.byref(ml)),
          "sf_subtree_partition_weighted")
    return owner[:sym.nsuper], tf.value, ml.value


class OocCut(tuple):
    """(group, ngroups, largest group, top entries, need, fits) of ooc_partition, + .top_mode (0: top panels resident throughout,
    1: only while active)"""
    top_mode = 0


def ooc_partition(sym, budget_entries):
    """Out-of-core grouping (sf_ooc_partition): group[s] = streamed group of supernode s or -1 (top) for a budget of
    `budget_entries` resident panel entries.  Returns (group int32[nsuper], ngroups, entries of the largest group, top entries,
    entries the cut needs, fits) with the attribute .top_mode to pass on to the plan."""
    group = np.zeros(max(sym.nsuper, 1), dtype=np.int32)
    ng, mode = C.c_int(), C.c_int()
    ge, te, nd = C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib.sf_ooc_partition(sym.nsuper, _lp(sym.Super), _lp(sym.SuperMap), _lp(sym.Lsip), _lp(sym.Lsi), int(budget_entries),
                              group.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ng), C.byref(ge), C.byref(te), C.byref(nd), C.byref(mode))
    if rc not in (0, 3):          # 3 = SF_ERR_ALLOC: no cut fits, the cheapest one is returned
        check(rc, "sf_ooc_partition")
    out = OocCut((group[:sym.nsuper], ng.value, ge.value, te.value, nd.value, rc == 0))
    out.top_mode = mode.value
    return out


def top_groups(sym, owner):
    """mask[s] for the top supernodes (owner[s] < 0): bit r set = rank r owns a subtree below s -- the group of ranks that
    holds s under the proportional mapping (what sf_chol_plan_create_mapped derives internally); 0 for subtree supernodes"""
    ns = sym.nsuper
    mask = np.zeros(ns, dtype=np.uint32)
    own = np.asarray(owner)
    mask[own >= 0] = np.left_shift(np.uint32(1), own[own >= 0].astype(np.uint32))
    Super, Lsip, Lsi, SuperMap = sym.Super, sym.Lsip, sym.Lsi, sym.SuperMap
    for s in range(ns):
        nscol, nsrow = Super[s + 1] - Super[s], Lsip[s + 1] - Lsip[s]
        if nscol < nsrow:
            mask[SuperMap[Lsi[Lsip[s] + nscol]]] |= mask[s]
    mask[own >= 0] = 0
    return mask


def phases_for_rank(owner, rank):
    """phase array of sf_chol_plan_create_sharded for `rank`: 0 own subtree, 1 top (replicated), -1 elsewhere"""
    return np.where(owner == rank, 0, np.where(owner < 0, 1, -1)).astype(np.int32)


class Comm:
    """one rank's RCCL communicator, created and used inside the C library (sf_comm_*): the unique id comes from rank 0
    (`Comm.unique_id()`) and reaches the other ranks by whatever the launcher offers (torch.distributed here)"""

    def __init__(self, device, rank, nranks, uid):
        h = C.c_void_p()
        check(lib.sf_comm_create_rccl(C.byref(h), device, rank, nranks, uid), "sf_comm_create_rccl")
        self._h, self.rank, self.nranks = h, rank, nranks

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib.sf_comm_unique_id(buf), "sf_comm_unique_id")
        return buf.raw

    def allreduce_sum(self, device_ptr, count, stream=0):
        check(lib.sf_comm_allreduce_sum(self._h, C.c_void_p(device_ptr), count, C.c_void_p(stream)), "sf_comm_allreduce_sum")

    def close(self):
        if getattr(self, "_h", None):
            lib.sf_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class _ShardedPlanMixin:
    """multi-GPU entry points shared by CholPlan and LUPlan (one handle type in the C ABI)"""

    def factorize_distributed(self, comm, host_out=None, sync=True):
        """the whole sharded factorization from this rank's side, driven in C (sf_chol_plan_factorize_distributed): own
        subtrees, then per segment pack -> RCCL all-reduce -> chain + this rank's share of the split GEMMs"""
        out = _dp(host_out) if host_out is not None else None
        check(lib.sf_chol_plan_factorize_distributed(self._h, comm._h, out, 1 if sync else 0), "sf_chol_plan_factorize_distributed")

    def prepare_comm(self, comm):
        """collective: sub-communicators of the plan's groups + one checked 8-byte sum per communicator (sf_chol_plan_prepare_comm)"""
        check(lib.sf_chol_plan_prepare_comm(self._h, comm._h), "sf_chol_plan_prepare_comm")

    def solve_distributed(self, comm, b):
        """the solve with the factor left distributed (sf_chol_plan_solve_distributed): returns x with this rank's entries filled
        in (its subtrees' columns, the shared supernodes it leads) and zeros elsewhere -- the sum over the ranks is the solution"""
        b = _f64(b)
        x = np.zeros_like(b)
        check(lib.sf_chol_plan_solve_distributed(self._h, comm._h, _dp(b), _dp(x)), "sf_chol_plan_solve_distributed")
        return x

    def factorize_phase(self, which, sync=True):
        check(lib.sf_chol_plan_factorize_phase(self._h, which, 1 if sync else 0), "sf_chol_plan_factorize_phase")

    def num_segments(self):
        return int(lib.sf_chol_plan_num_segments(self._h))

    def segment_group(self, k):
        """bit mask of the ranks that sum segment k's block columns"""
        return int(lib.sf_chol_plan_segment_group(self._h, k))

    def segment_regions(self, k):
        """[(offset, count)] in doubles relative to factor_device_ptr: regions to sum over the ranks before segment k"""
        nr = C.c_int64()
        check(lib.sf_chol_plan_segment_regions(self._h, k, 0, C.byref(nr), None, None), "sf_chol_plan_segment_regions")
        off = np.zeros(max(nr.value, 1), dtype=np.int64)
        cnt = np.zeros(max(nr.value, 1), dtype=np.int64)
        check(lib.sf_chol_plan_segment_regions(self._h, k, nr.value, C.byref(nr), _lp(off), _lp(cnt)),
              "sf_chol_plan_segment_regions")
        return [(int(off[i]), int(cnt[i])) for i in range(nr.value)]

    def segment_pack(self, k):
        """gather segment k's possibly non-zero block parts into the plan's contiguous scratch buffer (enqueued on the
        plan's stream); returns (device pointer, number of doubles) to all-reduce before factorize_segment(k)"""
        ptr, cnt = C.c_void_p(), C.c_int64()
        check(lib.sf_chol_plan_segment_pack(self._h, k, C.byref(ptr), C.byref(cnt)), "sf_chol_plan_segment_pack")
        return ptr.value or 0, cnt.value

    def factorize_segment(self, k, sync=False):
        check(lib.sf_chol_plan_factorize_segment(self._h, k, 1 if sync else 0), "sf_chol_plan_factorize_segment")

    def set_stream(self, stream_handle):
        """run on a caller-owned HIP stream (integer handle, e.g. torch.cuda.current_stream().cuda_stream)"""
        check(lib.sf_chol_plan_set_stream(self._h, C.c_void_p(stream_handle)), "sf_chol_plan_set_stream")

    def top_region(self):
        """(device pointer, number of doubles) of the contiguous top-panel region"""
        ptr, cnt = C.c_void_p(), C.c_int64()
        check(lib.sf_chol_plan_top_region(self._h, C.byref(ptr), C.byref(cnt)), "sf_chol_plan_top_region")
        return ptr.value or 0, cnt.value

    @property
    def factor_device_ptr(self):
        return lib.sf_chol_plan_factor_device_ptr(self._h)


class _ScheduleMixin:
    """schedule inspection (sf_chol_plan_launch_info & co.): works on real plans and on schedule-only ones"""

    LAUNCH_FIELDS = ("kind", "tasks", "items", "split", "lo", "hi", "replicated", "segment", "group_index", "group_size")
    SEGMENT_FIELDS = ("mask", "l0", "l1", "packed", "early", "regions")

    def _table(self, count, fn, width):
        out = np.zeros((max(count, 0), width), dtype=np.int64)
        row = np.zeros(width, dtype=np.int64)
        for k in range(count):
            check(fn(self._h, k, _lp(row)), fn.__name__)
            out[k] = row
        return out

    def launch_table(self):
        """int64[launches, 10]: LAUNCH_FIELDS per launch, in issue order"""
        return self._table(int(lib.sf_chol_plan_num_launches(self._h)), lib.sf_chol_plan_launch_info, 10)

    def segment_table(self):
        """int64[segments, 6]: SEGMENT_FIELDS per segment = per all-reduce of the factorization, in issue order"""
        return self._table(int(lib.sf_chol_plan_num_segments(self._h)), lib.sf_chol_plan_segment_info, 6)

    def segment_owner_table(self):
        """int64[segments, 2]: (owner's group index or -1, launches of the owner's part) -- the owner-computes prototype, SF_TOP_OWNER=1"""
        return self._table(int(lib.sf_chol_plan_num_segments(self._h)), lib.sf_chol_plan_segment_owner, 2)

    def solve_reduce_table(self):
        """int64[reduces, 3]: (group mask, first column, columns) of the forward sweep's sums, in issue order"""
        return self._table(int(lib.sf_chol_plan_num_solve_reduces(self._h)), lib.sf_chol_plan_solve_reduce_info, 3)

    def panel_offsets(self, nsuper):
        xp = np.zeros(max(nsuper, 1), dtype=np.int64)
        check(lib.sf_chol_plan_panel_offsets(self._h, _lp(xp)), "sf_chol_plan_panel_offsets")
        return xp[:nsuper]


def _sparse_columns(W, n, what):
    """W as k sparse columns: an (n,) or (n, k) array (each column's non-zeros are its pattern) or a (Wp, Wi, Wx) triple (Wx may
    be None where only the pattern matters) -> (k, Wp, Wi, Wx), int64 / float64 and contiguous"""
    # (a triple is three array-likes: a plain list of three numbers is a dense vector for n = 3)
    if isinstance(W, (tuple, list)) and len(W) == 3 and np.ndim(W[0]) == 1 and np.ndim(W[1]) == 1:
        Wp, Wi = _i64(W[0]), _i64(W[1])
        Wx = None if W[2] is None else _f64(W[2])
        if Wp.ndim != 1 or len(Wp) < 1 or Wi.ndim != 1 or len(Wi) < (int(Wp[-1]) if len(Wp) else 0) or \
                (Wx is not None and Wx.shape != Wi.shape):
            raise ValueError(f"{what}: (Wp, Wi, Wx) must be k + 1 offsets and Wp[k] rows and values")
        return len(Wp) - 1, Wp, Wi, Wx
    W = np.asarray(W, dtype=np.float64)
    if W.ndim == 1:
        W = W.reshape(-1, 1)
    if W.ndim != 2 or W.shape[0] != n:
        raise ValueError(f"{what}: W must have shape ({n},) or ({n}, k), got {W.shape}")
    cols, rows = np.nonzero(W.T)
    Wp = np.zeros(W.shape[1] + 1, dtype=np.int64)
    np.add.at(Wp, cols + 1, 1)
    return W.shape[1], np.cumsum(Wp), _i64(rows), _f64(W[rows, cols])


class _UpdatePathMixin:
    """which supernodes a rank-k update would rewrite (sf_chol_plan_update_path): real and schedule-only Cholesky plans"""

    def update_path(self, W, perm_in=False, return_bad=False):
        """the supernodes, ascending, that update(W) rewrites.  An inadmissible column (or any other bad argument) raises;
        return_bad: (path or None, first inadmissible column or -1) instead"""
        k, Wp, Wi, _ = _sparse_columns(W, self.n, "update_path")
        count, bad = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        supers = np.zeros(max(self.nsuper, 1), dtype=np.int64)
        rc = lib.sf_chol_plan_update_path(self._h, k, _lp(Wp), _lp(Wi), 1 if perm_in else 0, _lp(count), _lp(supers), _lp(bad))
        if return_bad and (rc == 0 or bad[0] >= 0):
            return (supers[:int(count[0])].copy() if rc == 0 else None), int(bad[0])
        check(rc, "sf_chol_plan_update_path")
        return supers[:int(count[0])].copy()

    def rowmod_path(self, row, idx=None, perm_in=False):
        """what rowdel(row) and rowadd(row, idx, ...) touch (sf_chol_plan_rowmod_path): {"rows": [(supernode, position)] of the
        panels that hold the row below their own columns, "sweep": the supernodes of rowadd's forward sweep (idx None: empty),
        "update": the path of the rank-1 update that follows}.  An inadmissible index (or any other bad argument) raises"""
        Ai = _i64([] if idx is None else idx)
        cnt = np.zeros(3, dtype=np.int64)
        out = np.zeros((4, max(self.nsuper, 1)), dtype=np.int64)
        check(lib.sf_chol_plan_rowmod_path(self._h, int(row), len(Ai), _lp(Ai), 1 if perm_in else 0, _lp(cnt[0:]), _lp(out[0]),
                                           _lp(out[1]), _lp(cnt[1:]), _lp(out[2]), _lp(cnt[2:]), _lp(out[3]), None),
              "sf_chol_plan_rowmod_path")
        return {"rows": list(zip(out[0, :cnt[0]].tolist(), out[1, :cnt[0]].tolist())), "sweep": out[2, :cnt[1]].tolist(),
                "update": out[3, :cnt[2]].tolist()}


class Schedule(_ScheduleMixin, _ShardedPlanMixin, _UpdatePathMixin):
    """Rank `rank`'s plan of an nranks-way factorization WITHOUT a device (sf_chol_plan_schedule_mapped /
    sf_lu_plan_schedule_mapped): the launch list, segments, storage map and byte counts of the real plan, nothing allocated."""

    def __init__(self, sym, owner, rank, nranks, lu=False, ooc_group=None, ooc_ngroups=0, ooc_top_mode=0):
        """ooc_group / ooc_ngroups (owner None): the schedule of an out-of-core plan (sf_chol_plan_schedule_ooc)"""
        h = C.c_void_p()
        self.n = sym.n
        self._keep = [sym.Super, sym.SuperMap, sym.Lsip, sym.Lsi, sym.Lsxp, sym.Lp, sym.Li]
        if ooc_group is not None:
            grp = np.ascontiguousarray(ooc_group, dtype=np.int32)
            check(lib.sf_chol_plan_schedule_ooc(C.byref(h), sym.n, sym.nsuper, *[_lp(a) for a in self._keep],
                                                grp.ctypes.data_as(C.POINTER(C.c_int32)), int(ooc_ngroups), int(ooc_top_mode)), "sf_chol_plan_schedule_ooc")
            self._h, self.rank, self.nranks, self.nsuper = h, 0, 1, sym.nsuper
            return
        owner = np.ascontiguousarray(owner, dtype=np.int32)
        if lu:
            sym_in = bool(sym.symmetric)
            self._keep += [None, None] if sym_in else [sym.Up, sym.Ui]
            args = [_lp(a) if a is not None else None for a in self._keep]
            check(lib.sf_lu_plan_schedule_mapped(C.byref(h), sym.n, sym.nsuper, *args,
                                                 owner.ctypes.data_as(C.POINTER(C.c_int32)), int(rank), int(nranks)),
                  "sf_lu_plan_schedule_mapped")
        else:
            check(lib.sf_chol_plan_schedule_mapped(C.byref(h), sym.n, sym.nsuper, *[_lp(a) for a in self._keep],
                                                   owner.ctypes.data_as(C.POINTER(C.c_int32)), int(rank), int(nranks)),
                  "sf_chol_plan_schedule_mapped")
        self._h, self.rank, self.nranks, self.nsuper = h, rank, nranks, sym.nsuper

    def stat(self, name):
        return float(lib.sf_chol_plan_stat(self._h, name.encode()))

    def close(self):
        if getattr(self, "_h", None):
            lib.sf_chol_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class _ValidateMixin:
    def validate(self, return_x=False):
        """SparseFrame_validate on the device: b_i = 1 + i/n, solve, residual |Ax - b|_inf / (|A|_1 |x|_inf + |b|_inf).
        The residual is NaN when any r_i or x_i is not finite (a NaN fails every `<=`): a NaN that a kernel let through is
        never reported as a perfect solve.  No exception is raised for it."""
        res = C.c_double()
        x = np.empty(max(self.n, 1), dtype=np.float64) if return_x else None
        check(lib.sf_chol_plan_validate(self._h, C.byref(res), _dp(x) if return_x else None), "sf_chol_plan_validate")
        return (res.value, x[:self.n]) if return_x else res.value


class _RefineMixin:
    """residual and iterative refinement on the device (sf_chol_plan_residual / _refine, sf_lu_plan_*)"""

    def _refine_fn(self, what):
        return getattr(lib, ("sf_lu_plan_" if isinstance(self, LUPlan) else "sf_chol_plan_") + what)

    def residual(self, b, x):
        """(r, berr, nerr) for the plan's current values, permuted space: r = b - A x, berr = max_i |r_i| / (|A| |x| + |b|)_i,
        nerr = |r|_inf / (|A|_1 |x|_inf + |b|_inf); berr and nerr are NaN when r, x or b holds a non-finite entry"""
        b, x = _f64(b), _f64(x)
        if b.shape != (self.n,) or x.shape != (self.n,):
            raise ValueError(f"residual: b and x must have shape ({self.n},)")
        r = np.empty(max(self.n, 1), dtype=np.float64)
        berr, nerr = C.c_double(), C.c_double()
        fn = self._refine_fn("residual")
        check(fn(self._h, _dp(b), _dp(x), _dp(r), C.byref(berr), C.byref(nerr)), fn.__name__)
        return r[:self.n], berr.value, nerr.value

    def residual_weights(self):
        """w = |A| |x| + |b| of the plan's last residual evaluation"""
        w = np.empty(max(self.n, 1), dtype=np.float64)
        check(lib.sf_chol_plan_residual_weights(self._h, _dp(w)), "sf_chol_plan_residual_weights")
        return w[:self.n]

    def refine(self, b, max_iter=5, tol=0.0, return_info=False):
        """x = solve(b) followed by at most max_iter refinement steps against the plan's current values (stops at berr <= tol,
        tol <= 0: 2^-52, or on stagnation); the iterate with the smallest berr is returned.
        return_info: (x, {"iters", "berr0", "berr"})"""
        b = _f64(b)
        if b.shape != (self.n,):
            raise ValueError(f"refine: b must have shape ({self.n},)")
        x = np.empty(max(self.n, 1), dtype=np.float64)
        berr = C.c_double()
        fn = self._refine_fn("refine")
        check(fn(self._h, _dp(b), _dp(x), int(max_iter), float(tol), C.byref(berr)), fn.__name__)
        x = x[:self.n]
        if not return_info:
            return x
        return x, {"iters": int(self.stat("last_refine_iters")), "berr0": self.stat("last_refine_berr0"), "berr": berr.value}


class _CondestMixin:
    def condest(self, return_parts=False):
        """1-norm condition estimate kappa_1(A) ~ |A|_1 * est(|A^-1|_1) (Hager / Higham, at most 11 device sweeps with the
        resident factor; the estimate of |A^-1|_1 is a lower bound).  return_parts: (|A|_1, estimate of |A^-1|_1)"""
        fn = lib.sf_lu_plan_condest if isinstance(self, LUPlan) else lib.sf_chol_plan_condest
        anorm, ainv = C.c_double(), C.c_double()
        check(fn(self._h, C.byref(anorm), C.byref(ainv)), fn.__name__)
        return (anorm.value, ainv.value) if return_parts else anorm.value * ainv.value


_DEV_OPS = {"solve": 0, "half_L": 1, "half_Lt": 2, "trans": 3}


def _dev_tensor(T, rows, device, what, writable=False):
    """checks a device tensor (anything with data_ptr(), dtype, shape, stride(), is_cuda and device: a torch tensor) and returns
    (tensor to pass, columns, leading dimension, was 1-D).  float64, on the plan's device, 1-D of `rows` entries or 2-D
    (rows, k) with unit stride along the rows, i.e. column-major.  A C-contiguous 2-D INPUT is taken via .t().contiguous().t()
    (one device copy); an output must be column-major already."""
    for attr in ("data_ptr", "dtype", "shape", "stride", "is_cuda", "device"):
        if not hasattr(T, attr):
            raise TypeError(f"{what}: expected a device tensor (missing .{attr}), got {type(T).__name__}")
    if not str(T.dtype).endswith("float64"):
        raise TypeError(f"{what}: tensor must be float64, got {T.dtype}")
    if not T.is_cuda:
        raise ValueError(f"{what}: tensor must live on the device, got device {T.device}")
    if getattr(T.device, "index", None) != device:
        raise ValueError(f"{what}: tensor is on {T.device}, the plan on device {device}")
    shape, one = tuple(T.shape), len(T.shape) == 1
    if len(shape) not in (1, 2) or shape[0] != rows:
        raise ValueError(f"{what}: tensor must have shape ({rows},) or ({rows}, k), got {shape}")
    k = 1 if one else shape[1]
    st = tuple(T.stride())
    ldmin = max(rows, 1)
    ok = (rows <= 1 or st[0] == 1) and (one or k <= 1 or st[1] >= ldmin)
    if not ok:
        if writable or one or st[1] != 1 or st[0] != k:
            raise ValueError(f"{what}: tensor must be column-major (unit stride along the rows), got strides {st}")
        T = T.t().contiguous().t()
        st = tuple(T.stride())
    ld = ldmin if (one or k <= 1) else st[1]
    return T, k, ld, one


class _DeviceIOMixin:
    """right-hand sides, solutions, samples and matrix values that stay on the device (sf_*_plan_*_device).  The
    arguments are torch tensors on the plan's device; torch is imported by these methods only.  Every method waits for the
    current torch stream of the device before the C call (the tensors' producers) and returns with the result complete."""

    def _dev_fn(self, what):
        return getattr(lib, ("sf_lu_plan_" if isinstance(self, LUPlan) else "sf_chol_plan_") + what)

    def _dev_sync(self):
        import torch
        torch.cuda.current_stream(self.device).synchronize()
        return torch

    def _dev_out(self, torch, k, one):
        if one:
            return torch.empty(self.n, dtype=torch.float64, device=f"cuda:{self.device}")
        return torch.empty_strided((self.n, k), (1, max(self.n, 1)), dtype=torch.float64, device=f"cuda:{self.device}")

    def set_ordering(self, perm=None):
        """the ordering perm[new] = old (what analyze was given; None: the identity) for perm_in / perm_out / permute_device"""
        if perm is not None:
            perm = _i64(perm)
            if perm.shape != (self.n,):
                raise ValueError(f"set_ordering: perm must have shape ({self.n},), got {perm.shape}")
        fn = self._dev_fn("set_ordering")
        check(fn(self._h, _lp(perm) if perm is not None else None), fn.__name__)

    def solve_device(self, B, out=None, op="solve", perm_in=False, perm_out=False):
        """X = op(B) with the resident factor, B and X device tensors ((n,) or column-major (n, k)); out=None allocates X
        (torch.empty_strided, column-major), out=B solves in place.  op: "solve"; "half_L" / "half_Lt" (CholPlan, as
        solve_half); "trans" (LUPlan).  perm_in: B is in the caller's numbering (row perm[i] of B is row i of the permuted
        system); perm_out: so is X.  Both with op="solve" solve the caller's own system A x = b."""
        lu = isinstance(self, LUPlan)
        if op not in (("solve", "trans") if lu else ("solve", "half_L", "half_Lt")):
            raise ValueError(f"solve_device: op {op!r} is not one of this plan's")
        B, k, ldb, one = _dev_tensor(B, self.n, self.device, "solve_device")
        torch = None
        if out is None:
            torch = self._dev_sync()
            out = self._dev_out(torch, k, one)
        X, kx, ldx, onex = _dev_tensor(out, self.n, self.device, "solve_device (out)", writable=True)
        if (kx, onex) != (k, one):
            raise ValueError(f"solve_device: out must have the shape of B, got {tuple(out.shape)}")
        if k and self.n:
            if torch is None:
                self._dev_sync()
            fn = self._dev_fn("solve_device")
            check(fn(self._h, _DEV_OPS[op], (1 if perm_in else 0) | (2 if perm_out else 0), k, B.data_ptr(), ldb, X.data_ptr(), ldx),
                  fn.__name__)
        return out

    def permute_device(self, B, out=None, inverse=False):
        """out = B[perm] (row i = row perm[i] of B: caller's numbering -> permuted), or with inverse out[perm] = B; not in place"""
        B, k, ldb, one = _dev_tensor(B, self.n, self.device, "permute_device")
        torch = None
        if out is None:
            torch = self._dev_sync()
            out = self._dev_out(torch, k, one)
        X, kx, ldx, onex = _dev_tensor(out, self.n, self.device, "permute_device (out)", writable=True)
        if (kx, onex) != (k, one):
            raise ValueError(f"permute_device: out must have the shape of B, got {tuple(out.shape)}")
        if k and self.n:
            if torch is None:
                self._dev_sync()
            fn = self._dev_fn("permute_device")
            check(fn(self._h, 1 if inverse else 0, k, B.data_ptr(), ldb, X.data_ptr(), ldx), fn.__name__)
        return out

    def set_values_device(self, Lx, Ux=None):
        """set_values from device tensors (1-D float64, nnz / unz entries; Ux: LUPlan with an unsymmetric input)"""
        lu = isinstance(self, LUPlan)
        L, _, _, one = _dev_tensor(Lx, self._nnz, self.device, "set_values_device")
        if not one:
            raise ValueError("set_values_device: Lx must be 1-D")
        args = [L.data_ptr() or None]
        if lu:
            if self._alias:
                args.append(None)
            else:
                U, _, _, _ = _dev_tensor(Ux, self._unz, self.device, "set_values_device (Ux)")
                args.append(U.data_ptr() or None)
        self._dev_sync()
        fn = self._dev_fn("set_values_device")
        check(fn(self._h, *args), fn.__name__)

    def set_value_map(self, nsrc, mapL, mapU=None):
        """(nsrc, mapL, mapU) of Symbolic.value_map(): uploaded once for set_values_mapped_device"""
        mapL = _i64(mapL)
        mapU = _i64(mapU) if mapU is not None else None
        fn = self._dev_fn("set_value_map")
        check(fn(self._h, int(nsrc), _lp(mapL), _lp(mapU) if mapU is not None else None), fn.__name__)
        self._nsrc = int(nsrc)

    def set_values_mapped_device(self, Ax):
        """set_values from the caller's own value array on the device (1-D float64, nsrc entries, the entry order analyze was
        given): one gather kernel through the map of set_value_map"""
        if getattr(self, "_nsrc", None) is None:
            raise ValueError("set_values_mapped_device: no value map (set_value_map)")
        A, _, _, _ = _dev_tensor(Ax, self._nsrc, self.device, "set_values_mapped_device")
        self._dev_sync()
        fn = self._dev_fn("set_values_mapped_device")
        check(fn(self._h, A.data_ptr() or None), fn.__name__)


SEL_MAX_M = 64      # SF_SEL_MAX_M


def _value_block(V, rows, what):
    """a host block of value arrays: 1-D (rows,) or 2-D (rows, m), any memory order -> (array, m, leading dimension, was 1-D).
    A float64 block with unit stride along the rows (a column-major array or a row slice of one) is passed as it is."""
    V = np.asarray(V)
    if V.ndim not in (1, 2) or V.shape[0] != rows:
        raise ValueError(f"{what}: expected shape ({rows},) or ({rows}, m), got {V.shape}")
    one = V.ndim == 1
    m = 1 if one else V.shape[1]
    if m > SEL_MAX_M:
        raise ValueError(f"{what}: at most {SEL_MAX_M} value arrays per call, got {m}")
    ldmin = max(rows, 1)
    if one:
        return _f64(V), 1, ldmin, True
    direct = V.dtype == np.float64 and (rows <= 1 or V.strides[0] == 8) and (m <= 1 or (V.strides[1] % 8 == 0 and V.strides[1] >= 8 * ldmin))
    if not direct:
        V = np.asfortranarray(V, dtype=np.float64)
    ld = ldmin if m <= 1 else V.strides[1] // 8
    return V, m, ld, False


class _SelinvPatternMixin:
    """Sigma = A^-1 read where the caller wants it, after selinv() (sf_*_plan_selinv_values / _trace / _entries).
    Everything is in permuted space, like get_selinv."""

    def _sel_fn(self, what):
        return getattr(lib, ("sf_lu_plan_" if isinstance(self, LUPlan) else "sf_chol_plan_") + what)

    def _own_u(self):
        return isinstance(self, LUPlan) and not self._alias

    def selinv_values(self, transposed=False):
        """Sigma on the structure the plan was created with: CholPlan -> S with S[p] = Sigma(Li[p], j) for every position p of
        column j; LUPlan -> (SL, SU) with SU[p] = Sigma(j, Ui[p]) for every position of row j of U, or SL alone when U aliases L.
        transposed (LUPlan): Sigma(j, Li[p]) and Sigma(Ui[p], j) instead."""
        lu = isinstance(self, LUPlan)
        if transposed and not lu:
            raise ValueError("selinv_values: Sigma of a Cholesky plan is symmetric, there is no transposed form")
        SL = np.zeros(max(self._nnz, 1), dtype=np.float64)
        if not lu:
            check(lib.sf_chol_plan_selinv_values(self._h, _dp(SL)), "sf_chol_plan_selinv_values")
            return SL[:self._nnz]
        SU = np.zeros(max(self._unz, 1), dtype=np.float64) if self._own_u() else None
        fn = lib.sf_lu_plan_selinv_values_t if transposed else lib.sf_lu_plan_selinv_values
        check(fn(self._h, _dp(SL), _dp(SU) if SU is not None else None), fn.__name__)
        return (SL[:self._nnz], SU[:self._unz]) if SU is not None else SL[:self._nnz]

    def selinv_values_device(self, out, outU=None, transposed=False):
        """selinv_values into device tensors (1-D float64, nnz / unz entries; outU: LUPlan with its own U structure)"""
        lu = isinstance(self, LUPlan)
        if transposed and not lu:
            raise ValueError("selinv_values_device: Sigma of a Cholesky plan is symmetric, there is no transposed form")
        if (outU is not None) != self._own_u():
            raise ValueError("selinv_values_device: outU is for an LUPlan with its own U structure, and needed there")
        L, _, _, one = _dev_tensor(out, self._nnz, self.device, "selinv_values_device", writable=True)
        args = [L.data_ptr() or None]
        if outU is not None:
            U, _, _, oneu = _dev_tensor(outU, self._unz, self.device, "selinv_values_device (outU)", writable=True)
            one = one and oneu
            args.append(U.data_ptr() or None)
        elif lu:
            args.append(None)
        if not one:
            raise ValueError("selinv_values_device: the outputs must be 1-D")
        self._dev_sync()
        fn = self._sel_fn("selinv_values_t_device" if transposed else "selinv_values_device")
        check(fn(self._h, *args), fn.__name__)
        return (out, outU) if outU is not None else out

    def _trace_rows(self, mapped, what):
        if not mapped:
            return self._nnz
        if getattr(self, "_nsrc", None) is None:
            raise ValueError(f"{what}: mapped=True needs a value map (set_value_map)")
        return self._nsrc

    def selinv_trace(self, V, VU=None, mapped=False):
        """tr(Sigma M(V)) for the matrix set_values(V) would assemble: V 1-D (nnz,) -> float, 2-D (nnz, m) -> (m,), m <= 64, any
        memory order.  LUPlan with its own U structure: VU likewise with unz rows.  mapped: V is in the caller's own layout
        (nsrc rows) and read through the map of set_value_map (VU: None)."""
        what = "selinv_trace"
        need_u = self._own_u() and not mapped
        if (VU is not None) != need_u:
            raise ValueError(f"{what}: VU is for an LUPlan with its own U structure (unmapped), and needed there")
        A, m, ld, one = _value_block(V, self._trace_rows(mapped, what), what)
        args = [m, _dp(A), ld]
        if isinstance(self, LUPlan):
            if need_u:
                B, mu, ldu, oneu = _value_block(VU, self._unz, what + " (VU)")
                if (mu, oneu) != (m, one):
                    raise ValueError(f"{what}: VU must have as many columns as V")
                args += [_dp(B), ldu]
            else:
                args += [None, 0]
        out = np.zeros(max(m, 1), dtype=np.float64)
        if m:
            fn = self._sel_fn("selinv_trace")
            check(fn(self._h, *args, 1 if mapped else 0, _dp(out)), fn.__name__)
        return float(out[0]) if one else out[:m]

    def selinv_trace_device(self, V, VU=None, out=None, mapped=False):
        """selinv_trace on device tensors ((rows,) or column-major (rows, m)); out: (m,) float64 on the device, allocated when None"""
        what = "selinv_trace_device"
        need_u = self._own_u() and not mapped
        if (VU is not None) != need_u:
            raise ValueError(f"{what}: VU is for an LUPlan with its own U structure (unmapped), and needed there")
        A, m, ld, one = _dev_tensor(V, self._trace_rows(mapped, what), self.device, what)
        if m > SEL_MAX_M:
            raise ValueError(f"{what}: at most {SEL_MAX_M} value arrays per call, got {m}")
        args = [m, A.data_ptr() or None, ld]
        if isinstance(self, LUPlan):
            if need_u:
                B, mu, ldu, oneu = _dev_tensor(VU, self._unz, self.device, what + " (VU)")
                if (mu, oneu) != (m, one):
                    raise ValueError(f"{what}: VU must have as many columns as V")
                args += [B.data_ptr() or None, ldu]
            else:
                args += [None, 0]
        torch = None
        if out is None:
            torch = self._dev_sync()
            out = torch.empty(m, dtype=torch.float64, device=f"cuda:{self.device}")
        O, ko, _, oneo = _dev_tensor(out, m, self.device, what + " (out)", writable=True)
        if not oneo:
            raise ValueError(f"{what}: out must have shape ({m},), got {tuple(out.shape)}")
        if m:
            if torch is None:
                self._dev_sync()
            fn = self._sel_fn("selinv_trace_device")
            check(fn(self._h, *args, 1 if mapped else 0, O.data_ptr()), fn.__name__)
        return out

    def selinv_entries(self, rows, cols):
        """(values, outside): values[k] = Sigma(rows[k], cols[k]) for permuted indices (CholPlan: either triangle; LUPlan: (i, j)
        literally); a pair outside the factor's pattern gets NaN and is counted in `outside`"""
        rows, cols = _i64(rows), _i64(cols)
        if rows.ndim != 1 or rows.shape != cols.shape:
            raise ValueError(f"selinv_entries: rows and cols must be 1-D of one length, got {rows.shape} and {cols.shape}")
        out = np.zeros(max(rows.size, 1), dtype=np.float64)
        outside = C.c_int64(0)
        fn = self._sel_fn("selinv_entries")
        check(fn(self._h, rows.size, _lp(rows), _lp(cols), _dp(out), C.byref(outside)), fn.__name__)
        return out[:rows.size], int(outside.value)

    def logdet_grad(self, dA, dAU=None):
        """selinv_trace(dA): for dA = dA/dtheta in set_values order the derivative of logdet() with respect to theta -- of
        log det A for a CholPlan, of log|det A| for an LUPlan (dAU: the U part, LUPlan with its own U structure)"""
        return self.selinv_trace(dA, dAU)


ADJ_MAPPED = 4      # SF_ADJ_MAPPED


def _host_block(B, rows, what):
    """a host block of columns: 1-D (rows,) or 2-D (rows, k), any memory order -> (float64 array with unit stride along the rows,
    k, leading dimension).  A float64 block with unit stride along the rows (a column-major array or a row slice of one) is
    passed as it is, with its own leading dimension; anything else is copied."""
    B = np.asarray(B)
    if B.ndim not in (1, 2) or B.shape[0] != rows:
        raise ValueError(f"{what}: expected shape ({rows},) or ({rows}, k), got {B.shape}")
    ldmin = max(rows, 1)
    if B.ndim == 1:
        return _f64(B), 1, ldmin
    k = B.shape[1]
    direct = B.dtype == np.float64 and (rows <= 1 or B.strides[0] == 8) and (k <= 1 or (B.strides[1] % 8 == 0 and B.strides[1] >= 8 * ldmin))
    if not direct:
        B = np.asfortranarray(B, dtype=np.float64)
    return B, k, (ldmin if k <= 1 else B.strides[1] // 8)


class _AdjointMixin:
    """the gradient of solves, quadratic forms and log-determinants with respect to the matrix values, as arrays in set_values
    order or (mapped) in the caller's own value layout (sf_*_plan_adjoint_values / _logdet_grad_values).  Permuted
    space unless perm_in says otherwise.  The autograd module builds on the device forms."""

    def _adj_fn(self, what):
        return getattr(lib, ("sf_lu_plan_" if isinstance(self, LUPlan) else "sf_chol_plan_") + what)

    def _adj_counts(self, mapped, what):
        """(entries of the first output, entries of the second or None)"""
        if mapped:
            if getattr(self, "_nsrc", None) is None:
                raise ValueError(f"{what}: mapped=True needs a value map (set_value_map)")
            return self._nsrc, None
        own_u = isinstance(self, LUPlan) and not self._alias
        return self._nnz, (self._unz if own_u else None)

    def _adj_host(self, what, head, alpha, mapped):
        nl, nu = self._adj_counts(mapped, what)
        out = np.zeros(max(nl, 1), dtype=np.float64)
        outU = np.zeros(max(nu, 1), dtype=np.float64) if nu is not None else None
        args = head + [float(alpha), ADJ_MAPPED if mapped else 0, _dp(out)]
        if isinstance(self, LUPlan):
            args.append(_dp(outU) if outU is not None else None)
        fn = self._adj_fn(what)
        check(fn(self._h, *args), fn.__name__)
        return (out[:nl], outU[:nu]) if outU is not None else out[:nl]

    def _adj_dev_outs(self, what, out, outU, mapped):
        nl, nu = self._adj_counts(mapped, what)
        if (outU is not None) and nu is None:
            raise ValueError(f"{what}: outU is for an LUPlan with its own U structure (unmapped)")
        torch = self._dev_sync()
        dev = f"cuda:{self.device}"
        if out is None:
            out = torch.empty(nl, dtype=torch.float64, device=dev)
        if outU is None and nu is not None:
            outU = torch.empty(nu, dtype=torch.float64, device=dev)
        L, _, _, one = _dev_tensor(out, nl, self.device, what + " (out)", writable=True)
        ptrs = [L.data_ptr() or None]
        if nu is not None:
            U, _, _, oneu = _dev_tensor(outU, nu, self.device, what + " (outU)", writable=True)
            one = one and oneu
            ptrs.append(U.data_ptr() or None)
        elif isinstance(self, LUPlan):
            ptrs.append(None)
        if not one:
            raise ValueError(f"{what}: the outputs must be 1-D")
        return out, outU, ptrs

    def adjoint_values(self, Y, X, alpha=1.0, mapped=False):
        """out with sum(out * dV) = alpha * sum_c y_c^T M(dV) x_c for every dV, M(dV) the matrix set_values(dV) assembles: Y, X
        (n,) or (n, k) host arrays.  CholPlan -> (nnz,); LUPlan -> (outL, outU), or outL alone when U aliases L; mapped -> (nsrc,)
        in the caller's own value layout.  Positions the assembly ignores get 0.  Needs no factor."""
        what = "adjoint_values"
        Yb, k, ldy = _host_block(Y, self.n, what + " (Y)")
        Xb, kx, ldx = _host_block(X, self.n, what + " (X)")
        if kx != k:
            raise ValueError(f"{what}: Y and X must have as many columns, got {k} and {kx}")
        return self._adj_host(what, [k, _dp(Yb), ldy, _dp(Xb), ldx], alpha, mapped)

    def adjoint_values_device(self, Y, X, out=None, outU=None, alpha=1.0, perm_in=False, mapped=False):
        """adjoint_values on device tensors ((n,) or column-major (n, k)); perm_in: Y and X are in the caller's numbering
        (set_ordering).  out / outU: 1-D float64 on the device, allocated when None.  Returns out, or (out, outU)."""
        what = "adjoint_values_device"
        Yt, k, ldy, _ = _dev_tensor(Y, self.n, self.device, what + " (Y)")
        Xt, kx, ldx, _ = _dev_tensor(X, self.n, self.device, what + " (X)")
        if kx != k:
            raise ValueError(f"{what}: Y and X must have as many columns, got {k} and {kx}")
        out, outU, ptrs = self._adj_dev_outs(what, out, outU, mapped)
        fn = self._adj_fn(what)
        flags = (1 if perm_in else 0) | (ADJ_MAPPED if mapped else 0)
        check(fn(self._h, flags, k, Yt.data_ptr() or None, ldy, Xt.data_ptr() or None, ldx, float(alpha), *ptrs), fn.__name__)
        return (out, outU) if outU is not None else out

    def logdet_grad_values(self, alpha=1.0, mapped=False):
        """alpha times the gradient of logdet() with respect to the values, after selinv(): the Sigma of every position the
        assembly reads -- twice off the diagonal of a CholPlan, the transposed entry for an LUPlan -- and 0 at the others.
        Shapes as adjoint_values.  logdet_grad(dA) == sum(logdet_grad_values() * dA) up to rounding."""
        return self._adj_host("logdet_grad_values", [], alpha, mapped)

    def logdet_grad_values_device(self, out=None, outU=None, alpha=1.0, mapped=False):
        """logdet_grad_values into device tensors"""
        what = "logdet_grad_values_device"
        out, outU, ptrs = self._adj_dev_outs(what, out, outU, mapped)
        fn = self._adj_fn(what)
        check(fn(self._h, float(alpha), ADJ_MAPPED if mapped else 0, *ptrs), fn.__name__)
        return (out, outU) if outU is not None else out


class CholPlan(_ShardedPlanMixin, _ValidateMixin, _ScheduleMixin, _RefineMixin, _CondestMixin, _DeviceIOMixin, _SelinvPatternMixin,
               _AdjointMixin, _UpdatePathMixin):
    """Device-resident supernodal Cholesky (flat ABI).  Raises if no HIP device is present.
    phase/load_top: multi-GPU sharding (sf_chol_plan_create_sharded); default = the whole matrix on one device.
    rank/nranks (with phase): distributed top (sf_chol_plan_create_distributed), run with factorize_phase(0) and then
    factorize_segment(k) after summing segment_regions(k) over the ranks."""

    def __init__(self, sym, device=0, phase=None, load_top=True, rank=0, nranks=1, owner=None, ooc_group=None, ooc_ngroups=0, ooc_top_mode=0):
        """owner (with rank / nranks): the owner map of subtree_partition -> proportionally mapped plan
        (sf_chol_plan_create_mapped): own subtrees + the top supernodes above them, groups of ranks per top supernode.
        ooc_group / ooc_ngroups (from ooc_partition): out-of-core plan -- factorize_to_host only"""
        h = C.c_void_p()
        self._keep = [sym.Super, sym.SuperMap, sym.Lsip, sym.Lsi, sym.Lsxp, sym.Lp, sym.Li]
        if ooc_group is not None:
            grp = np.ascontiguousarray(ooc_group, dtype=np.int32)
            check(lib.sf_chol_plan_create_ooc(C.byref(h), device, sym.n, sym.nsuper, *[_lp(a) for a in self._keep],
                                              grp.ctypes.data_as(C.POINTER(C.c_int32)), int(ooc_ngroups), int(ooc_top_mode)), "sf_chol_plan_create_ooc")
        elif owner is not None:
            owner = np.ascontiguousarray(owner, dtype=np.int32)
            check(lib.sf_chol_plan_create_mapped(C.byref(h), device, sym.n, sym.nsuper, *[_lp(a) for a in self._keep],
                                                 owner.ctypes.data_as(C.POINTER(C.c_int32)), int(rank), int(nranks)),
                  "sf_chol_plan_create_mapped")
        elif phase is None:
            check(lib.sf_chol_plan_create(C.byref(h), device, sym.n, sym.nsuper, *[_lp(a) for a in self._keep]),
                  "sf_chol_plan_create")
        elif nranks <= 1:
            phase = np.ascontiguousarray(phase, dtype=np.int32)
            check(lib.sf_chol_plan_create_sharded(C.byref(h), device, sym.n, sym.nsuper, *[_lp(a) for a in self._keep],
                                                  phase.ctypes.data_as(C.POINTER(C.c_int32)), 1 if load_top else 0),
                  "sf_chol_plan_create_sharded")
        else:
            phase = np.ascontiguousarray(phase, dtype=np.int32)
            check(lib.sf_chol_plan_create_distributed(C.byref(h), device, sym.n, sym.nsuper, *[_lp(a) for a in self._keep],
                                                      phase.ctypes.data_as(C.POINTER(C.c_int32)), 1 if load_top else 0,
                                                      int(rank), int(nranks)),
                  "sf_chol_plan_create_distributed")
        self.device = device
        self._h = h
        self.xsize = sym.xsize
        self.n = sym.n
        self.nsuper = sym.nsuper
        self._nnz = int(self._keep[5][-1]) if len(self._keep[5]) else 0        # Lp[n]

    def set_values(self, Lx):
        Lx = _f64(Lx)
        check(lib.sf_chol_plan_set_values(self._h, _dp(Lx)), "sf_chol_plan_set_values")

    def update(self, W, downdate=False, perm_in=False):
        """the resident factor of A becomes that of A + W W^T (downdate: A - W W^T) without a factorization (permuted space;
        perm_in: W's rows are in the caller's numbering, set_ordering).  W: (n,), (n, k) or (Wp, Wi, Wx); every column must be
        admissible (see update_path): its rows lie in the row list of the supernode of its smallest row -- a diagonal entry or
        the weight of an existing edge always is.  The stored VALUES stay: set_values(A') first for a consistent plan.  A
        downdate that loses positive definiteness raises (SF_ERR_NOT_POSDEF) and leaves the plan unfactorized"""
        k, Wp, Wi, Wx = _sparse_columns(W, self.n, "update")
        if Wx is None:
            raise ValueError("update: the values Wx are missing")
        check(lib.sf_chol_plan_update(self._h, -1 if downdate else 1, k, _lp(Wp), _lp(Wi), _dp(Wx), 1 if perm_in else 0),
              "sf_chol_plan_update")

    def rowdel(self, row, perm_in=False):
        """row and column `row` of A become the identity's in the resident factor (permuted space, perm_in: the
        caller's numbering): the variable leaves the system, the pattern stays.  An iterable deletes its rows one after the
        other.  The stored VALUES stay: set_values(A') first for a consistent plan"""
        for r in (row if np.ndim(row) else [row]):
            check(lib.sf_chol_plan_rowdel(self._h, int(r), 1 if perm_in else 0), "sf_chol_plan_rowdel")

    def rowadd(self, row, idx, vals, perm_in=False):
        """the inverse of rowdel: row and column `row` of the factor, currently the identity's, take the column (idx, vals) of
        the new A, the diagonal among its entries; every index must be admissible (see rowmod_path) -- the pattern of A's own
        column always is.  A column that leaves A indefinite raises (SF_ERR_NOT_POSDEF) and leaves the plan unfactorized"""
        Ai, Ax = _i64(idx), _f64(vals)
        if Ai.ndim != 1 or Ax.shape != Ai.shape:
            raise ValueError("rowadd: idx and vals must be 1-D and of one length")
        check(lib.sf_chol_plan_rowadd(self._h, int(row), len(Ai), _lp(Ai), _dp(Ax), 1 if perm_in else 0), "sf_chol_plan_rowadd")

    def update_device(self, Wp, Wi, dWx, downdate=False, perm_in=False):
        """update((Wp, Wi, Wx)) with the values in a 1-D float64 device tensor aligned with Wi"""
        Wp, Wi = _i64(Wp), _i64(Wi)
        T, _, _, one = _dev_tensor(dWx, len(Wi), self.device, "update_device")
        if not one or Wp.ndim != 1 or len(Wp) < 1 or int(Wp[-1]) > len(Wi):
            raise ValueError("update_device: Wp must hold k + 1 offsets into Wi, dWx one value per row of Wi")
        self._dev_sync()
        check(lib.sf_chol_plan_update_device(self._h, -1 if downdate else 1, len(Wp) - 1, _lp(Wp), _lp(Wi), T.data_ptr() or None,
                                             1 if perm_in else 0), "sf_chol_plan_update_device")

    def factorize(self, sync=True):
        check(lib.sf_chol_plan_factorize(self._h, 1 if sync else 0), "sf_chol_plan_factorize")

    def sync(self):
        check(lib.sf_chol_plan_sync(self._h), "sf_chol_plan_sync")

    def get_factor(self, out=None):
        """D2H in the reference layout; a sharded plan fills only the panels stored on this rank"""
        if out is None:
            out = np.zeros(max(self.xsize, 1), dtype=np.float64)
        check(lib.sf_chol_plan_get_factor(self._h, _dp(out)), "sf_chol_plan_get_factor")
        return out[:self.xsize]

    def factorize_to_host(self, Lx, out=None):
        """values H2D + factorize + factor D2H into `out` (pageable numpy memory), the download overlapped with the
        computation -- what one SparseFrame_factorize call does once its plan exists"""
        Lx = _f64(Lx)
        if out is None:
            out = np.empty(max(self.xsize, 1), dtype=np.float64)
        check(lib.sf_chol_plan_factorize_to_host(self._h, _dp(Lx), None, _dp(out)), "sf_chol_plan_factorize_to_host")
        return out[:self.xsize]

    def solve(self, b):
        if np.ndim(b) == 2:
            return self.solve_many(b)
        b = _f64(b)
        x = np.empty_like(b)
        check(lib.sf_chol_plan_solve(self._h, _dp(b), _dp(x)), "sf_chol_plan_solve")
        return x

    def solve_many(self, B):
        """X = A^-1 B for an (n, k) block of right-hand sides (any memory order), permuted space, 16 columns per device sweep"""
        return _solve_many(lib.sf_chol_plan_solve_many, "sf_chol_plan_solve_many", self._h, self.n, B)

    def _block(self, B, what):
        """1-D or (n, k) input in any memory order -> (column-major float64 (n, k), was 1-D)"""
        B = np.asarray(B)
        one = B.ndim == 1
        if one:
            B = B.reshape(-1, 1)
        if B.ndim != 2 or B.shape[0] != self.n:
            raise ValueError(f"{what}: B must have shape ({self.n},) or ({self.n}, k), got {B.shape}")
        return np.asfortranarray(B, dtype=np.float64), one

    def solve_half(self, B, which="L"):
        """one half of the solve with the resident factor L (A = L L^T, permuted space): L^-1 B (which="L", whitening) or
        L^-T B (which="Lt"); "L" then "Lt" is solve_many.  B: (n,) or (n, k) in any memory order"""
        if which not in ("L", "Lt"):
            raise ValueError(f"solve_half: which must be 'L' or 'Lt', got {which!r}")
        Bf, one = self._block(B, "solve_half")
        k, ld = Bf.shape[1], max(self.n, 1)
        X = np.empty((self.n, k), dtype=np.float64, order="F")
        if k:
            check(lib.sf_chol_plan_solve_half(self._h, 0 if which == "L" else 1, k, _dp(Bf), ld, _dp(X), ld), "sf_chol_plan_solve_half")
        return X[:, 0] if one else X

    def quadform(self, B):
        """b^T A^-1 b = |L^-1 b|^2, reduced on the device: a float for a 1-D b, an array of k values for an (n, k) block"""
        Bf, one = self._block(B, "quadform")
        k = Bf.shape[1]
        q = np.zeros(max(k, 1), dtype=np.float64)
        if k:
            check(lib.sf_chol_plan_quadform(self._h, k, _dp(Bf), max(self.n, 1), _dp(q)), "sf_chol_plan_quadform")
        return float(q[0]) if one else q[:k]

    GRAM_MAX_K = 1024       # SF_GRAM_MAX_K

    def gram(self, B):
        """G = B^T A^-1 B, the dense Schur complement of the border B (permuted space): one forward sweep per 16 columns and a
        reduction on the device, only the (k, k) result comes back.  B: (n, k) in any memory order -> (k, k) float64, bit-for-bit
        symmetric; a 1-D b -> the float quadform(b).  k <= 1024"""
        Bf, one = self._block(B, "gram")
        k = Bf.shape[1]
        if k > self.GRAM_MAX_K:
            raise ValueError(f"gram: at most {self.GRAM_MAX_K} columns, got {k}")
        G = np.zeros((k, k), dtype=np.float64, order="F")
        if k:
            check(lib.sf_chol_plan_gram(self._h, k, _dp(Bf), max(self.n, 1), _dp(G), k), "sf_chol_plan_gram")
        return float(G[0, 0]) if one else G

    def gram_device(self, B, out=None, perm_in=False):
        """gram(B) for a device tensor B ((n,) or column-major (n, k)) into a device tensor: out (column-major (k, k), not
        overlapping B) or a new one.  perm_in: B is in the caller's numbering (set_ordering)"""
        B, k, ldb, one = _dev_tensor(B, self.n, self.device, "gram_device")
        if k > self.GRAM_MAX_K:
            raise ValueError(f"gram_device: at most {self.GRAM_MAX_K} columns, got {k}")
        torch = None
        if out is None:
            torch = self._dev_sync()
            out = torch.empty_strided((k, k), (1, max(k, 1)), dtype=torch.float64, device=f"cuda:{self.device}")
        G, kg, ldg, oneg = _dev_tensor(out, k, self.device, "gram_device (out)", writable=True)
        if oneg or kg != k:
            raise ValueError(f"gram_device: out must have shape ({k}, {k}), got {tuple(out.shape)}")
        if k:
            if torch is None:
                self._dev_sync()
            check(lib.sf_chol_plan_gram_device(self._h, 1 if perm_in else 0, k, B.data_ptr(), ldb, G.data_ptr(), ldg),
                  "sf_chol_plan_gram_device")
        return out

    def schur(self, B, D):
        """the Schur complement D - B^T A^-1 B of the bordered matrix [[A, B], [B^T, D]] (B: (n, k), D: (k, k))"""
        Bf, _ = self._block(B, "schur")
        k = Bf.shape[1]
        D = np.asarray(D, dtype=np.float64)
        if D.shape != (k, k):
            raise ValueError(f"schur: D must have shape ({k}, {k}), got {D.shape}")
        return D - self.gram(Bf)

    def solve_bordered(self, B, f, g, C=None):
        """(x, y) with [[A, B], [B^T, -C]] [x; y] = [f; g] (a saddle-point / KKT system; permuted space): B (n, k), f (n,),
        g (k,), C (k, k) symmetric positive semidefinite or None = 0.  One gram of [B f] gives S0 = B^T A^-1 B and
        t = B^T A^-1 f; S = C + S0 is factored on the host, y = S^-1 (t - g), x = solve(f - B y): k + 1 forward sweeps and one
        full solve, no (n, k) block comes back.  A border without full column rank (with C = 0) raises ValueError"""
        Bf, one = self._block(B, "solve_bordered")
        k = Bf.shape[1]
        f = _f64(f)
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        if one or f.shape != (self.n,) or g.shape != (k,):
            raise ValueError(f"solve_bordered: B, f, g must have shapes ({self.n}, k), ({self.n},), (k,), got "
                             f"{np.shape(B)}, {f.shape}, {g.shape}")
        if C is not None:
            C = np.asarray(C, dtype=np.float64)
            if C.shape != (k, k):
                raise ValueError(f"solve_bordered: C must have shape ({k}, {k}), got {C.shape}")
        if k + 1 > self.GRAM_MAX_K:
            raise ValueError(f"solve_bordered: at most {self.GRAM_MAX_K - 1} border columns, got {k}")
        G = self.gram(np.column_stack([Bf, f]))
        S, t = G[:k, :k], G[:k, k]
        if C is not None:
            S = S + C
        y = np.zeros(k)
        if k:
            # a pivot that rounding alone could have produced counts as zero: the factorization of an exactly singular S may run
            # through on a pivot of a few ulps of its diagonal entry, and y would be noise
            try:
                R = np.linalg.cholesky(S)
                singular = bool(np.any(np.diag(R) ** 2 <= 8 * k * np.finfo(np.float64).eps * np.diag(S)))
            except np.linalg.LinAlgError:
                singular = True
            if singular:
                raise ValueError("solve_bordered: C + B^T A^-1 B is not positive definite: a rank-deficient border "
                                 "(dependent columns of B where C does not make up for them)")
            y = np.linalg.solve(R.T, np.linalg.solve(R, t - g))
        x = self.solve(f - Bf @ y)
        return x, y

    def sample(self, k, seed=0, first=0, return_z=False):
        """k samples x ~ N(0, A^-1) as the columns of an (n, k) array (permuted space): x = L^-T z with the standard normals z
        generated on the device.  Column j is sample first + j of the stream `seed`, whatever k is and however a run is cut
        into calls.  return_z: (X, Z) with the normals used"""
        k, ld = int(k), max(self.n, 1)
        if k < 0:
            raise ValueError("sample: k must not be negative")
        X = np.empty((self.n, k), dtype=np.float64, order="F")
        Z = np.empty((self.n, k), dtype=np.float64, order="F") if return_z else None
        if k:
            check(lib.sf_chol_plan_sample(self._h, k, int(seed), int(first), _dp(X), ld, _dp(Z) if return_z else None, ld),
                  "sf_chol_plan_sample")
        return (X, Z) if return_z else X

    def sample_device(self, k, seed=0, first=0, out=None, perm_out=False):
        """sample(k, seed, first) with the samples stored into a device tensor (out, column-major (n, k), or a new one);
        perm_out: in the caller's numbering (set_ordering).  The same stream of samples as sample()"""
        k = int(k)
        if k < 0:
            raise ValueError("sample_device: k must not be negative")
        torch = self._dev_sync()
        if out is None:
            out = self._dev_out(torch, k, False)
        X, kx, ldx, one = _dev_tensor(out, self.n, self.device, "sample_device (out)", writable=True)
        if one or kx != k:
            raise ValueError(f"sample_device: out must have shape ({self.n}, {k}), got {tuple(out.shape)}")
        if k and self.n:
            check(lib.sf_chol_plan_sample_device(self._h, k, int(seed), int(first), 2 if perm_out else 0, X.data_ptr(), ldx),
                  "sf_chol_plan_sample_device")
        return out

    def selinv(self):
        """selected inversion: A^-1 on the pattern of L into a device arena (permuted space), from the resident factor"""
        check(lib.sf_chol_plan_selinv(self._h), "sf_chol_plan_selinv")

    def get_selinv(self, out=None):
        """D2H of the selected inverse in the factor's layout (diagonal blocks full symmetric)"""
        if out is None:
            out = np.zeros(max(self.xsize, 1), dtype=np.float64)
        check(lib.sf_chol_plan_get_selinv_range(self._h, 0, self.xsize, _dp(out)), "sf_chol_plan_get_selinv_range")
        return out[:self.xsize]

    def selinv_diag(self):
        """diag(A^-1), permuted space, gathered on the device"""
        d = np.zeros(max(self.n, 1), dtype=np.float64)
        check(lib.sf_chol_plan_selinv_diag(self._h, _dp(d)), "sf_chol_plan_selinv_diag")
        return d[:self.n]

    def logdet(self):
        """log det A = 2 sum log L_jj of the resident factor"""
        out = np.zeros(1, dtype=np.float64)
        check(lib.sf_chol_plan_logdet(self._h, _dp(out)), "sf_chol_plan_logdet")
        return float(out[0])

    def stat(self, name):
        return float(lib.sf_chol_plan_stat(self._h, name.encode()))

    def set_profiling(self, on=True):
        check(lib.sf_chol_plan_set_profiling(self._h, 1 if on else 0), "sf_chol_plan_set_profiling")

    def close(self):
        if getattr(self, "_h", None):
            lib.sf_chol_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class LUPlan(_ShardedPlanMixin, _ValidateMixin, _ScheduleMixin, _RefineMixin, _CondestMixin, _DeviceIOMixin, _SelinvPatternMixin,
             _AdjointMixin):
    """Device-resident supernodal no-pivot LU (flat ABI, sf_lu_plan_*).  `sym` comes from analyze(..., method='lu').
    phase/load_top/rank/nranks: distributed multi-GPU plan (sf_lu_plan_create_distributed), as CholPlan."""

    def __init__(self, sym, device=0, phase=None, load_top=True, rank=0, nranks=1, owner=None, ooc_group=None, ooc_ngroups=0, ooc_top_mode=0):
        if not sym.lu:
            raise ValueError("LUPlan needs an LU symbolic analysis (method='lu')")
        h = C.c_void_p()
        self._alias = bool(sym.symmetric)
        self._keep = [sym.Super, sym.SuperMap, sym.Lsip, sym.Lsi, sym.Lsxp, sym.Lp, sym.Li]
        if not self._alias:
            self._keep += [sym.Up, sym.Ui]
        args = [_lp(a) for a in self._keep] + ([None, None] if self._alias else [])
        if ooc_group is not None:
            grp = np.ascontiguousarray(ooc_group, dtype=np.int32)
            check(lib.sf_lu_plan_create_ooc(C.byref(h), device, sym.n, sym.nsuper, *args,
                                            grp.ctypes.data_as(C.POINTER(C.c_int32)), int(ooc_ngroups), int(ooc_top_mode)), "sf_lu_plan_create_ooc")
        elif owner is not None:
            owner = np.ascontiguousarray(owner, dtype=np.int32)
            check(lib.sf_lu_plan_create_mapped(C.byref(h), device, sym.n, sym.nsuper, *args,
                                               owner.ctypes.data_as(C.POINTER(C.c_int32)), int(rank), int(nranks)),
                  "sf_lu_plan_create_mapped")
        elif phase is None:
            check(lib.sf_lu_plan_create(C.byref(h), device, sym.n, sym.nsuper, *args), "sf_lu_plan_create")
        else:
            phase = np.ascontiguousarray(phase, dtype=np.int32)
            check(lib.sf_lu_plan_create_distributed(C.byref(h), device, sym.n, sym.nsuper, *args,
                                                    phase.ctypes.data_as(C.POINTER(C.c_int32)), 1 if load_top else 0,
                                                    int(rank), int(nranks)), "sf_lu_plan_create_distributed")
        self.device = device
        self._h = h
        self.xsize = sym.xsize
        self.n = sym.n
        self._nnz = int(self._keep[5][-1]) if len(self._keep[5]) else 0        # Lp[n]
        self._unz = 0 if self._alias or not len(self._keep[7]) else int(self._keep[7][-1])      # Up[n]

    def set_values(self, Lx, Ux=None):
        Lx = _f64(Lx)
        if self._alias:
            check(lib.sf_lu_plan_set_values(self._h, _dp(Lx), None), "sf_lu_plan_set_values")
        else:
            Ux = _f64(Ux)
            check(lib.sf_lu_plan_set_values(self._h, _dp(Lx), _dp(Ux)), "sf_lu_plan_set_values")

    def set_pivoting(self, tol=0.1, perturb=1.4901161193847656e-08):
        """threshold partial pivoting inside the 64 x 64 diagonal blocks (tol in [0, 1]; 0 = none, the reference's behaviour)
        and the perturbation of tiny pivots (relative to max|a_ij|; 0 = a zero pivot is an error).  A new plan has (0, 0): the
        reference never pivots (L:2653)."""
        check(lib.sf_lu_plan_set_pivoting(self._h, float(tol), float(perturb)), "sf_lu_plan_set_pivoting")

    def get_pivots(self):
        """pivpos[g] = row position of original row g after the in-block interchanges (identity where nothing moved)"""
        out = np.arange(max(self.n, 1), dtype=np.int64)
        check(lib.sf_lu_plan_get_pivots(self._h, _lp(out)), "sf_lu_plan_get_pivots")
        return out[:self.n]

    def factorize(self, sync=True):
        check(lib.sf_lu_plan_factorize(self._h, 1 if sync else 0), "sf_lu_plan_factorize")

    def sync(self):
        check(lib.sf_lu_plan_sync(self._h), "sf_lu_plan_sync")

    def get_factor(self, out=None):
        """D2H in the reference's packed layout; a sharded plan returns zeros for the panels of other ranks"""
        if out is None:
            out = np.empty(max(self.xsize, 1), dtype=np.float64)
        check(lib.sf_lu_plan_get_factor(self._h, _dp(out)), "sf_lu_plan_get_factor")
        return out[:self.xsize]

    def factorize_to_host(self, Lx, Ux=None, out=None):
        """as CholPlan.factorize_to_host; the factor arrives in the reference's packed LU layout"""
        Lx = _f64(Lx)
        if out is None:
            out = np.empty(max(self.xsize, 1), dtype=np.float64)
        ux = None if self._alias else _dp(_f64(Ux))
        check(lib.sf_chol_plan_factorize_to_host(self._h, _dp(Lx), ux, _dp(out)), "sf_chol_plan_factorize_to_host")
        return out[:self.xsize]

    def solve(self, b, trans=False):
        """x = A^-1 b, or A^-T b with trans=True (the same resident factor); a 2-D b goes to solve_many"""
        if np.ndim(b) == 2:
            return self.solve_many(b, trans)
        b = _f64(b)
        x = np.empty_like(b)
        if trans:
            check(lib.sf_lu_plan_solve_transposed(self._h, _dp(b), _dp(x)), "sf_lu_plan_solve_transposed")
        else:
            check(lib.sf_lu_plan_solve(self._h, _dp(b), _dp(x)), "sf_lu_plan_solve")
        return x

    def solve_many(self, B, trans=False):
        """X = A^-1 B (trans=True: A^-T B) for an (n, k) block of right-hand sides (any memory order), permuted space, 16 columns
        per device sweep"""
        if trans:
            return _solve_many(lib.sf_lu_plan_solve_many_transposed, "sf_lu_plan_solve_many_transposed", self._h, self.n, B)
        return _solve_many(lib.sf_lu_plan_solve_many, "sf_lu_plan_solve_many", self._h, self.n, B)

    def _block(self, B, what):
        """1-D or (n, k) input in any memory order -> (column-major float64 (n, k), was 1-D)"""
        B = np.asarray(B)
        one = B.ndim == 1
        if one:
            B = B.reshape(-1, 1)
        if B.ndim != 2 or B.shape[0] != self.n:
            raise ValueError(f"{what}: block must have shape ({self.n},) or ({self.n}, k), got {B.shape}")
        return np.asfortranarray(B, dtype=np.float64), one

    _HALVES = {"L": 0, "U": 1, "Ut": 2, "Lt": 3}        # SF_LU_HALF_*
    GRAM_MAX_K = 1024       # SF_GRAM_MAX_K

    def half_solve(self, B, which="L"):
        """one half of a solve with the resident factor (A = L U, permuted space; F = what the forward sweep of solve applies,
        L^-1 with the plan's interchanges): F B (which="L"), U^-1 B ("U"), U^-T B ("Ut") or F^T B ("Lt").  "L" then "U" is
        solve_many, "Ut" then "Lt" is solve_many(trans=True).  B: (n,) or (n, k) in any memory order"""
        if which not in self._HALVES:
            raise ValueError(f"half_solve: which must be one of 'L', 'U', 'Ut', 'Lt', got {which!r}")
        Bf, one = self._block(B, "half_solve")
        k, ld = Bf.shape[1], max(self.n, 1)
        X = np.empty((self.n, k), dtype=np.float64, order="F")
        if k:
            check(lib.sf_lu_plan_solve_half(self._h, self._HALVES[which], k, _dp(Bf), ld, _dp(X), ld), "sf_lu_plan_solve_half")
        return X[:, 0] if one else X

    def cross_gram(self, C, B):
        """G = C^T A^-1 B for the blocks C (n, m) and B (n, k) in any memory order (permuted space): two forward sweeps per pair
        of 16-column chunks and a reduction on the device, only the (m, k) result comes back.  Not symmetric, even for C is B.
        Two 1-D inputs give the float c^T A^-1 b.  m, k <= 1024"""
        Cf, onec = self._block(C, "cross_gram")
        Bf, oneb = self._block(B, "cross_gram")
        m, k = Cf.shape[1], Bf.shape[1]
        if m > self.GRAM_MAX_K or k > self.GRAM_MAX_K:
            raise ValueError(f"cross_gram: at most {self.GRAM_MAX_K} columns a block, got {m} and {k}")
        G = np.zeros((m, k), dtype=np.float64, order="F")
        if m and k:
            ld = max(self.n, 1)
            check(lib.sf_lu_plan_gram(self._h, m, _dp(Cf), ld, k, _dp(Bf), ld, _dp(G), m), "sf_lu_plan_gram")
        return float(G[0, 0]) if (onec and oneb) else G

    def cross_gram_device(self, C, B, out=None, perm_in=False):
        """cross_gram(C, B) for device tensors ((n,) or column-major (n, m) / (n, k)) into a device tensor: out (column-major
        (m, k), overlapping neither input) or a new one.  perm_in: C and B are in the caller's numbering (set_ordering)"""
        C, m, ldc, _ = _dev_tensor(C, self.n, self.device, "cross_gram_device (C)")
        B, k, ldb, _ = _dev_tensor(B, self.n, self.device, "cross_gram_device (B)")
        if m > self.GRAM_MAX_K or k > self.GRAM_MAX_K:
            raise ValueError(f"cross_gram_device: at most {self.GRAM_MAX_K} columns a block, got {m} and {k}")
        torch = None
        if out is None:
            torch = self._dev_sync()
            out = torch.empty_strided((m, k), (1, max(m, 1)), dtype=torch.float64, device=f"cuda:{self.device}")
        G, kg, ldg, oneg = _dev_tensor(out, m, self.device, "cross_gram_device (out)", writable=True)
        if oneg or kg != k:
            raise ValueError(f"cross_gram_device: out must have shape ({m}, {k}), got {tuple(out.shape)}")
        if m and k:
            if torch is None:
                self._dev_sync()
            check(lib.sf_lu_plan_gram_device(self._h, 1 if perm_in else 0, m, C.data_ptr(), ldc, k, B.data_ptr(), ldb, G.data_ptr(), ldg),
                  "sf_lu_plan_gram_device")
        return out

    def schur_complement(self, C, B, D):
        """the Schur complement D - C^T A^-1 B of the bordered matrix [[A, B], [C^T, D]] (C: (n, m), B: (n, k), D: (m, k))"""
        Cf, _ = self._block(C, "schur_complement")
        Bf, _ = self._block(B, "schur_complement")
        D = np.asarray(D, dtype=np.float64)
        if D.shape != (Cf.shape[1], Bf.shape[1]):
            raise ValueError(f"schur_complement: D must have shape ({Cf.shape[1]}, {Bf.shape[1]}), got {D.shape}")
        return D - self.cross_gram(Cf, Bf)

    def solve_saddle(self, B, C, f, g, D=None):
        """(x, y) with [[A, B], [C^T, -D]] [x; y] = [f; g] (an unsymmetric bordered system; permuted space): B, C (n, k), f (n,),
        g (k,), D (k, k) or None = 0.  One cross_gram(C, [B f]) gives S0 = C^T A^-1 B and t = C^T A^-1 f; S = D + S0 is solved on
        the host by LU with partial pivoting, y = S^-1 (t - g), x = solve(f - B y): no (n, k) block comes back.  A singular S --
        exactly, or with a pivot below 8 k eps of the largest entry its column had before the elimination -- raises ValueError"""
        Bf, oneb = self._block(B, "solve_saddle")
        Cf, onec = self._block(C, "solve_saddle")
        k = Bf.shape[1]
        f = _f64(f)
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        if oneb or onec or Cf.shape[1] != k or f.shape != (self.n,) or g.shape != (k,):
            raise ValueError(f"solve_saddle: B, C, f, g must have shapes ({self.n}, k), ({self.n}, k), ({self.n},), (k,), got "
                             f"{np.shape(B)}, {np.shape(C)}, {f.shape}, {g.shape}")
        if D is not None:
            D = np.asarray(D, dtype=np.float64)
            if D.shape != (k, k):
                raise ValueError(f"solve_saddle: D must have shape ({k}, {k}), got {D.shape}")
        if k + 1 > self.GRAM_MAX_K:
            raise ValueError(f"solve_saddle: at most {self.GRAM_MAX_K - 1} border columns, got {k}")
        G = self.cross_gram(Cf, np.column_stack([Bf, f]))
        S, t = G[:, :k], G[:, k]
        if D is not None:
            S = S + D
        y = _lu_solve_guarded(S, t - g, "solve_saddle: D + C^T A^-1 B is singular (a singular Schur complement)") if k else np.zeros(0)
        x = self.solve(f - Bf @ y)
        return x, y

    def selinv(self):
        """selected inversion: A^-1 on the pattern of L + U into a pair of device arenas (permuted space), from the resident
        factor; refused while threshold pivoting is on"""
        check(lib.sf_lu_plan_selinv(self._h), "sf_lu_plan_selinv")

    def get_selinv(self, out=None):
        """D2H of the selected inverse in get_factor's packed layout: per panel the full diagonal block, Sigma(R,C), Sigma(C,R)^T"""
        if out is None:
            out = np.zeros(max(self.xsize, 1), dtype=np.float64)
        check(lib.sf_lu_plan_get_selinv_range(self._h, 0, self.xsize, _dp(out)), "sf_lu_plan_get_selinv_range")
        return out[:self.xsize]

    def selinv_diag(self):
        """diag(A^-1), permuted space, gathered on the device"""
        d = np.zeros(max(self.n, 1), dtype=np.float64)
        check(lib.sf_lu_plan_selinv_diag(self._h, _dp(d)), "sf_lu_plan_selinv_diag")
        return d[:self.n]

    def logdet(self):
        """(log|det A|, sign of det A) from the U diagonal of the resident factor and the parity of its row interchanges"""
        out = np.zeros(1, dtype=np.float64)
        sign = C.c_int(0)
        check(lib.sf_lu_plan_logdet(self._h, _dp(out), C.byref(sign)), "sf_lu_plan_logdet")
        return float(out[0]), int(sign.value)

    def stat(self, name):
        return float(lib.sf_lu_plan_stat(self._h, name.encode()))

    def set_profiling(self, on=True):
        check(lib.sf_lu_plan_set_profiling(self._h, 1 if on else 0), "sf_lu_plan_set_profiling")

    def close(self):
        if getattr(self, "_h", None):
            lib.sf_lu_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


# -------------------------------------------------------------------------------------------------
# struct-based interface (reference names)
# -------------------------------------------------------------------------------------------------
class CommonInfoStruct(C.Structure):       # info.h:12-29
    _fields_ = [("numCPU", C.c_int), ("numGPU", C.c_int), ("numGPU_physical", C.c_int),
                ("minDevMemSize", C.c_size_t), ("minHostMemSize", C.c_size_t),
                ("matrixThreadNum", C.c_int), ("numSparseMatrix", C.c_int),
                ("devSlotSize", C.c_size_t),
                ("allocateTime", C.c_double), ("computeTime", C.c_double), ("freeTime", C.c_double)]


class MatrixInfoStruct(C.Structure):       # info.h:70-150
    _fields_ = [("serial", C.c_int), ("path", C.c_char_p), ("file", C.c_void_p),
                ("factorizeType", C.c_int), ("isSymmetric", C.c_int), ("isComplex", C.c_int),
                ("ncol", C.c_int64), ("nrow", C.c_int64), ("nzmax", C.c_int64),
                ("Tj", c_long_p), ("Ti", c_long_p), ("Tx", c_double_p),
                ("Cp", c_long_p), ("Ci", c_long_p), ("Cx", c_double_p),
                ("Lp", c_long_p), ("Li", c_long_p), ("Lx", c_double_p),
                ("LTp", c_long_p), ("LTi", c_long_p), ("LTx", c_double_p),
                ("permMethod", C.c_int),
                ("Perm", c_long_p), ("Parent", c_long_p), ("Post", c_long_p), ("ColCount", c_long_p),
                ("nsuper", C.c_int64), ("Super", c_long_p), ("SuperMap", c_long_p), ("Sparent", c_long_p),
                ("nsleaf", C.c_int64), ("LeafQueue", c_long_p),
                ("isize", C.c_int64), ("xsize", C.c_int64),
                ("Lsip", c_long_p), ("Lsxp", c_long_p), ("Lsi", c_long_p), ("Lsx", c_double_p),
                ("csize", C.c_int64), ("nstage", C.c_int64),
                ("ST_Map", c_long_p), ("ST_Pointer", c_long_p), ("ST_Index", c_long_p), ("ST_Parent", c_long_p),
                ("Aoffset", C.POINTER(C.c_size_t)), ("Moffset", C.POINTER(C.c_size_t)),
                ("workspace", C.c_void_p), ("workSize", C.c_size_t),
                ("Bx", c_double_p), ("Xx", c_double_p), ("Rx", c_double_p),
                ("residual", C.c_double),
                ("readTime", C.c_double), ("analyzeTime", C.c_double),
                ("factorizeTime", C.c_double), ("solveTime", C.c_double)]


for _name, _args in (("SparseFrame_allocate_gpu", [C.POINTER(CommonInfoStruct), C.POINTER(C.c_void_p)]),
                     ("SparseFrame_free_gpu", [C.POINTER(CommonInfoStruct), C.POINTER(C.c_void_p)]),
                     ("SparseFrame_initialize_matrix", [C.POINTER(MatrixInfoStruct)]),
                     ("SparseFrame_read_matrix", [C.POINTER(MatrixInfoStruct)]),
                     ("SparseFrame_set_matrix_csc", [C.POINTER(MatrixInfoStruct), C.c_int64, C.c_int64,
                                                     c_long_p, c_long_p, c_double_p, C.c_int]),
                     ("SparseFrame_set_perm", [C.POINTER(MatrixInfoStruct), c_long_p]),
                     ("SparseFrame_analyze", [C.POINTER(CommonInfoStruct), C.POINTER(MatrixInfoStruct)]),
                     ("SparseFrame_factorize", [C.POINTER(CommonInfoStruct), C.c_void_p, C.POINTER(MatrixInfoStruct)]),
                     ("SparseFrame_factorize_supernodal", [C.POINTER(CommonInfoStruct), C.c_void_p, C.POINTER(MatrixInfoStruct)]),
                     ("SparseFrame_solve_supernodal", [C.POINTER(MatrixInfoStruct)]),
                     ("SparseFrame_validate", [C.POINTER(MatrixInfoStruct)]),
                     ("SparseFrame_cleanup_matrix", [C.POINTER(MatrixInfoStruct)])):
    _f = getattr(lib, _name)
    _f.argtypes = _args
    _f.restype = C.c_int


class LUMatrixInfoStruct(C.Structure):     # LU/Include/info.h:70-163
    _fields_ = [("serial", C.c_int), ("path", C.c_char_p), ("file", C.c_void_p),
                ("factorizeType", C.c_int), ("isSymmetric", C.c_int), ("isComplex", C.c_int),
                ("ncol", C.c_int64), ("nrow", C.c_int64), ("nzmax", C.c_int64),
                ("Tj", c_long_p), ("Ti", c_long_p), ("Tx", c_double_p),
                ("Cp", c_long_p), ("Ci", c_long_p), ("Cx", c_double_p),
                ("nzCPCT", C.c_int64), ("CPCTp", c_long_p), ("CPCTi", c_long_p),
                ("Lp", c_long_p), ("Li", c_long_p), ("Lx", c_double_p),
                ("LTp", c_long_p), ("LTi", c_long_p), ("LTx", c_double_p),
                ("Up", c_long_p), ("Ui", c_long_p), ("Ux", c_double_p),
                ("UTp", c_long_p), ("UTi", c_long_p), ("UTx", c_double_p),
                ("permMethod", C.c_int), ("PivInv", c_long_p),
                ("Perm", c_long_p), ("Parent", c_long_p), ("Post", c_long_p), ("ColCount", c_long_p),
                ("nsuper", C.c_int64), ("Super", c_long_p), ("SuperMap", c_long_p), ("Sparent", c_long_p),
                ("nsleaf", C.c_int64), ("LeafQueue", c_long_p),
                ("isize", C.c_int64), ("xsize", C.c_int64),
                ("Lsip", c_long_p), ("Lsxp", c_long_p), ("Lsi", c_long_p), ("Lsx", c_double_p),
                ("csize", C.c_int64), ("nstage", C.c_int64),
                ("ST_Map", c_long_p), ("ST_Pointer", c_long_p), ("ST_Index", c_long_p), ("ST_Parent", c_long_p),
                ("Aoffset", C.POINTER(C.c_size_t)), ("Moffset", C.POINTER(C.c_size_t)),
                ("workspace", C.c_void_p), ("workSize", C.c_size_t),
                ("Bx", c_double_p), ("Xx", c_double_p), ("Rx", c_double_p),
                ("residual", C.c_double),
                ("readTime", C.c_double), ("analyzeTime", C.c_double),
                ("factorizeTime", C.c_double), ("solveTime", C.c_double)]


for _name, _args in (("SparseFrame_allocate_gpu", [C.POINTER(CommonInfoStruct), C.POINTER(C.c_void_p)]),
                     ("SparseFrame_free_gpu", [C.POINTER(CommonInfoStruct), C.POINTER(C.c_void_p)]),
                     ("SparseFrame_initialize_matrix", [C.POINTER(LUMatrixInfoStruct)]),
                     ("SparseFrame_read_matrix", [C.POINTER(LUMatrixInfoStruct)]),
                     ("SparseFrame_set_matrix_csc", [C.POINTER(LUMatrixInfoStruct), C.c_int64, C.c_int64,
                                                     c_long_p, c_long_p, c_double_p, C.c_int]),
                     ("SparseFrame_set_perm", [C.POINTER(LUMatrixInfoStruct), c_long_p]),
                     ("SparseFrame_analyze", [C.POINTER(CommonInfoStruct), C.POINTER(LUMatrixInfoStruct)]),
                     ("SparseFrame_factorize", [C.POINTER(CommonInfoStruct), C.c_void_p, C.POINTER(LUMatrixInfoStruct)]),
                     ("SparseFrame_factorize_supernodal", [C.POINTER(CommonInfoStruct), C.c_void_p, C.POINTER(LUMatrixInfoStruct)]),
                     ("SparseFrame_solve_supernodal", [C.POINTER(LUMatrixInfoStruct)]),
                     ("SparseFrame_validate", [C.POINTER(LUMatrixInfoStruct)]),
                     ("SparseFrame_cleanup_matrix", [C.POINTER(LUMatrixInfoStruct)])):
    _f = getattr(lu_lib, _name)
    _f.argtypes = _args
    _f.restype = C.c_int


class CommonInfo:
    """common_info_struct + the opaque gpu_info list (SparseFrame_allocate_gpu / _free_gpu)."""

    def __init__(self, dev_slot_size=None):
        self.c = CommonInfoStruct()
        self.gpu_list = C.c_void_p()
        check(lib.SparseFrame_allocate_gpu(C.byref(self.c), C.byref(self.gpu_list)), "SparseFrame_allocate_gpu")
        if dev_slot_size is not None:
            self.c.devSlotSize = dev_slot_size

    def plan_builds(self):
        """device plans the handlers have built so far (a repeated sparsity pattern must not add to it)"""
        return int(lib.sf_handlers_plan_builds(self.gpu_list, self.c.numGPU))

    def close(self):
        if self.gpu_list:
            lib.SparseFrame_free_gpu(C.byref(self.c), C.byref(self.gpu_list))
            self.gpu_list = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MatrixInfo:
    """matrix_info_struct driven through the reference's stage functions (Cholesky library)."""
    _lib = lib
    _struct = MatrixInfoStruct

    def __init__(self, serial=0):
        self.c = self._struct()
        self.c.serial = serial
        self._lib.SparseFrame_initialize_matrix(C.byref(self.c))

    def set_csc(self, n, Cp, Ci, Cx, symmetric=True):
        """symmetric=True: one triangle (Cholesky, or LU of a symmetric matrix); False: whole matrix (LU only)"""
        Cp, Ci, Cx = _i64(Cp), _i64(Ci), _f64(Cx)
        check(self._lib.SparseFrame_set_matrix_csc(C.byref(self.c), n, len(Ci), _lp(Cp), _lp(Ci), _dp(Cx),
                                             1 if symmetric else 0), "SparseFrame_set_matrix_csc")

    def read(self, path):
        self._path = str(path).encode()
        self.c.path = self._path
        check(self._lib.SparseFrame_read_matrix(C.byref(self.c)), "SparseFrame_read_matrix")

    def set_perm(self, perm):
        """perm[new] = old; None = natural order (explicit opt-in: the default is the built-in nested dissection)"""
        if perm is None:
            check(self._lib.SparseFrame_set_perm(C.byref(self.c), None), "SparseFrame_set_perm")
            return
        perm = _i64(perm)
        check(self._lib.SparseFrame_set_perm(C.byref(self.c), _lp(perm)), "SparseFrame_set_perm")

    def use_builtin_ordering(self):
        """permMethod = PERM_METIS with no Perm supplied (the default after initialize_matrix): SparseFrame_analyze orders
        with the built-in nested dissection"""
        self.c.permMethod = 2

    def analyze(self, common):
        check(self._lib.SparseFrame_analyze(C.byref(common.c), C.byref(self.c)), "SparseFrame_analyze")

    def factorize(self, common):
        check(self._lib.SparseFrame_factorize(C.byref(common.c), common.gpu_list, C.byref(self.c)), "SparseFrame_factorize")

    def validate(self):
        """the struct path's residual |Ax - b|_inf / (|A|_1 |x|_inf + |b|_inf), b_i = 1 + i/n; NaN when any r_i or x_i is not
        finite (the return code stays 0)"""
        check(self._lib.SparseFrame_validate(C.byref(self.c)), "SparseFrame_validate")
        return float(self.c.residual)

    def cleanup(self):
        self._lib.SparseFrame_cleanup_matrix(C.byref(self.c))

    def array(self, name, length):
        p = getattr(self.c, name)
        if not p or length == 0:
            return np.zeros(0, dtype=np.float64 if name.endswith("x") else np.int64)
        return np.ctypeslib.as_array(p, shape=(length,))

    def __del__(self):
        try:
            self.cleanup()
        except Exception:
            pass


class LUMatrixInfo(MatrixInfo):
    """the same stage functions from the LU library (libsparseframe_lu_hip.so, LU struct layout)"""
    _lib = lu_lib
    _struct = LUMatrixInfoStruct

    @staticmethod
    def set_pivoting(tol=0.0, perturb=0.0):
        """process-wide policy of the LU struct entry points (SparseFrame_set_pivoting): (0, 0) = the reference's behaviour"""
        check(lu_lib.SparseFrame_set_pivoting(float(tol), float(perturb)), "SparseFrame_set_pivoting")

    def set_matrix_pivoting(self, tol=0.0, perturb=0.0):
        """this matrix's own policy (SparseFrame_set_matrix_pivoting); overrides the process-wide one for this matrix_info"""
        check(lu_lib.SparseFrame_set_matrix_pivoting(C.byref(self.c), float(tol), float(perturb)), "SparseFrame_set_matrix_pivoting")

    def perturbed_pivots(self):
        return int(lu_lib.SparseFrame_perturbed_pivots(C.byref(self.c)))
