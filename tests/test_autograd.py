"""torch.autograd for plans (the package's autograd module).

Wiring: values.grad and B.grad of a loss that mixes solve, quadform and logdet of ONE Factorization are the manual composition of
solve_device, adjoint_values_device and logdet_grad_values_device bit for bit.  The plans' solves add into x with floating-point
atomics, so two solves of one right-hand side may differ in their last bits (a composition with solves of its own was not
bit-identical in any of the eight cases); the composition therefore takes the results of the solves the graph itself made -- recorded at
plan.solve_device, each checked to be the solve, with bit-identical input, that the composition would make -- and everything after
them is compared bit for bit.  Three contributions meet in values.grad: any of the three orders of adding them is accepted.  Accuracy: against torch.linalg on the CPU in float64, both judged by a
longdouble numpy gradient; the device's relative error may be at most 8 times the CPU's (the margin of DESIGN 8o / 8q), printed as
ADJOINT_RATIO lines.  The guard: a backward against a plan that has moved on raises and leaves values.grad alone."""
import numpy as np
import pytest

import adjoint_ref as ar
from util import sf, gen

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 7                       # 7^3 = 343 <= 512
SHIFT = 0.5


def _problem(kind):
    """(sym, structure for the reference, shifted values (VL, VU)): kind in chol / lu_alias / lu_own"""
    perm = sf.grid_nd_perm(N, N, N)
    if kind == "lu_own":
        n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=3)
        sym = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
        S = (n, np.asarray(sym.Lp), np.asarray(sym.Li), np.asarray(sym.Up), np.asarray(sym.Ui))
        VL, VU = np.array(sym.Lx, dtype=np.float64), np.array(sym.Ux, dtype=np.float64)
        VU[np.asarray(sym.Ui) == ar.columns(sym.Up)] += SHIFT
        return sym, S, perm, VL, VU
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    if kind == "chol":
        sym = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30)
        S = (n, np.asarray(sym.Lp), np.asarray(sym.Li))
    else:
        sym = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", True)
        S = (n, np.asarray(sym.Lp), np.asarray(sym.Li), None, None)
    VL = np.array(sym.Lx, dtype=np.float64)
    VL[np.asarray(sym.Li) == ar.columns(sym.Lp)] += SHIFT
    return sym, S, perm, VL, None


def _plan(kind, sym):
    return (sf.CholPlan if kind == "chol" else sf.LUPlan)(sym, device=0)


def _dev(a, grad=False):
    t = torch.from_numpy(np.asfortranarray(a)).cuda()
    if a.ndim == 2:
        t = t.t().contiguous().t()
    return t.requires_grad_(grad)


def _loss(f, B, W, wq, trans):
    X = f.solve(B, trans=trans) if trans else f.solve(B)
    return (W * X).sum() + (wq * f.quadform(B)).sum() + 0.7 * f.logdet()


@pytest.mark.parametrize("kind,trans,mode", [("chol", False, "plain"), ("chol", False, "perm"), ("chol", False, "mapped"),
                                             ("lu_alias", False, "plain"), ("lu_alias", True, "plain"), ("lu_own", False, "plain"),
                                             ("lu_own", True, "perm"), ("lu_own", False, "mapped")])
def test_wiring_is_the_manual_composition(kind, trans, mode):
    sym, S, perm, VL, VU = _problem(kind)
    n, k = S[0], 3
    rng = np.random.default_rng(1)
    plan = _plan(kind, sym)
    try:
        lu, pm, mapped = kind != "chol", mode == "perm", mode == "mapped"
        if pm:
            plan.set_ordering(perm)
        if mapped:                                          # the caller's layout: the plan's arrays one after the other, reversed
            src = np.concatenate([VL] + ([VU] if VU is not None else []))[::-1].copy()
            nsrc = len(src)
            mapL = nsrc - 1 - np.arange(len(VL))
            mapU = nsrc - 1 - len(VL) - np.arange(len(VU)) if VU is not None else None
            plan.set_value_map(nsrc, mapL, mapU)
            vals = [_dev(src, True)]
        else:
            vals = [_dev(VL, True)] + ([_dev(VU, True)] if VU is not None else [])
        B, W, wq = _dev(rng.uniform(-1, 1, (n, k)), True), _dev(rng.uniform(-1, 1, (n, k))), _dev(rng.uniform(0.5, 1.5, k))
        f = sf.Factorization(plan, vals[0], None if mapped or len(vals) == 1 else vals[1], mapped=mapped)
        assert f.perm == pm
        made = []                                           # every solve the graph makes: (op, its input, its result)
        solve_device = plan.solve_device

        def recording(T, out=None, op="solve", perm_in=False, perm_out=False):
            assert (perm_in, perm_out) == (pm, pm)
            R = solve_device(T, out=out, op=op, perm_in=perm_in, perm_out=perm_out)
            made.append((op, T.clone(), R))
            return R

        plan.solve_device = recording
        loss = _loss(f, B, W, wq, trans)
        if lu:
            assert f.sign in (1, -1)
        loss.backward()
        plan.solve_device = solve_device
        # ---- the same by hand ----
        fwd, oth = (("trans", "solve") if trans else ("solve", "trans")) if lu else ("solve", "solve")
        adj = lambda Y, X_: plan.adjoint_values_device(Y, X_, alpha=-1.0, perm_in=pm, mapped=mapped)
        tup = lambda r: list(r) if isinstance(r, tuple) else [r]
        Bd = B.detach()
        # the solves in the order the graph makes them: forward solve, forward quadform; backward quadform (LU), backward solve
        expect = [(fwd, Bd), ("solve", Bd)] + ([("trans", Bd)] if lu else []) + [(oth, W)]
        assert [m[0] for m in made] == [e[0] for e in expect]
        for (op, T, R), (_, want_in) in zip(made, expect):
            assert torch.equal(T, want_in)
            fresh = solve_device(want_in, op=op, perm_in=pm, perm_out=pm)
            assert torch.allclose(R, fresh, rtol=1e-11, atol=1e-13)
        X, Xq = made[0][2], made[1][2]
        Xt = made[2][2] if lu else Xq
        Lam = made[-1][2]
        g_solve = tup(adj(X, Lam) if trans else adj(Lam, X))
        g_quad = tup(adj(Xt * wq, Xq))
        g_logdet = tup(plan.logdet_grad_values_device(alpha=0.7, mapped=mapped))
        for v, gs, gq, gl in zip(vals, g_solve, g_quad, g_logdet):
            # three contributions meet in values.grad; which two the engine adds first is its business, the bits of each are ours
            wants = ((gl + gq) + gs, (gl + gs) + gq, (gq + gs) + gl)
            assert v.grad is not None and any(torch.equal(v.grad, w) for w in wants)
        dB_quad = (2.0 * Xq * wq) if not lu else ((Xq + Xt) * wq)
        assert torch.equal(B.grad, Lam + dB_quad) and B.grad.stride() == B.stride()
        by_hand = (W * X).sum() + (wq * (Bd * Xq).sum(0)).sum() + 0.7 * float(plan.logdet()[0] if lu else plan.logdet())
        assert torch.allclose(loss.detach(), by_hand, rtol=1e-14, atol=0.0)
    finally:
        plan.close()


def _dense_from_values(S, vals_t):
    """M(V) with torch on the CPU through the reference's marks (differentiable)"""
    n = S[0]
    M = torch.zeros((n, n), dtype=torch.float64)
    for V, (i, j, a, b) in zip(vals_t, ar.marks(S)):
        i, j = torch.from_numpy(i), torch.from_numpy(j)
        a, b = torch.from_numpy(a), torch.from_numpy(b)
        M = M.index_put((i[a], j[a]), V[a]).index_put((j[b], i[b]), V[b])
    return M


def _ld_solve(M, B):
    """longdouble solve: float64 LU solve refined three times with a longdouble residual"""
    M64 = M.astype(np.float64)
    X = np.linalg.solve(M64, B.astype(np.float64)).astype(ar.LD)
    for _ in range(3):
        X = X + np.linalg.solve(M64, (B - M @ X).astype(np.float64)).astype(ar.LD)
    return X


@pytest.mark.parametrize("kind", ["chol", "lu_own"])
def test_gradients_against_cpu_float64_and_longdouble(kind):
    sym, S, perm, VL, VU = _problem(kind)
    n, k = S[0], 2
    rng = np.random.default_rng(2)
    Bh, Wh, wqh = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(0.5, 1.5, k)
    host_vals = [VL] + ([VU] if VU is not None else [])
    # ---- longdouble numpy gradient ----
    M = ar.assemble(S, VL, VU)
    X, Lam = _ld_solve(M, Bh.astype(ar.LD)), _ld_solve(M.T, Wh.astype(ar.LD))
    Xt = _ld_solve(M.T, Bh.astype(ar.LD))
    Sg = _ld_solve(M, np.eye(n, dtype=ar.LD))
    gs, gq, gl = ar.adjoint_values(S, Lam, X, -1.0)[0], ar.adjoint_values(S, Xt * wqh, X, -1.0)[0], ar.logdet_grad_values(S, Sg, 0.7)
    ref_vals = [a + b + c for a, b, c in zip(gs, gq, gl)]
    ref_B = Lam + (X + Xt) * wqh
    # ---- torch on the CPU, float64 ----
    cv = [torch.from_numpy(v.copy()).requires_grad_(True) for v in host_vals]
    cB = torch.from_numpy(Bh.copy()).requires_grad_(True)
    Mt = _dense_from_values(S, cv)
    Xc = torch.linalg.solve(Mt, cB)
    (torch.from_numpy(Wh) * Xc).sum().add((torch.from_numpy(wqh) * (cB * Xc).sum(0)).sum()).add(0.7 * torch.linalg.slogdet(Mt)[1]).backward()
    # ---- the device ----
    plan = _plan(kind, sym)
    try:
        dv = [_dev(v, True) for v in host_vals]
        dB = _dev(Bh, True)
        f = sf.Factorization(plan, dv[0], dv[1] if len(dv) > 1 else None)
        _loss(f, dB, _dev(Wh), _dev(wqh), False).backward()
        rel = lambda got, ref: float(np.max(np.abs(got.astype(ar.LD) - ref)) / np.max(np.abs(ref)))
        pairs = [(f"values{s}", dv[s].grad.cpu().numpy(), cv[s].grad.numpy(), ref_vals[s]) for s in range(len(dv))]
        pairs.append(("B", dB.grad.cpu().numpy(), cB.grad.numpy(), ref_B))
        for name, dev_g, cpu_g, ref in pairs:
            e_dev, e_cpu = rel(dev_g, ref), rel(cpu_g, ref)
            print(f"ADJOINT_RATIO {kind} {name}: device {e_dev:.3e} cpu {e_cpu:.3e} ratio {e_dev / max(e_cpu, 2.0 ** -53):.3f}")
            assert e_dev <= 8 * max(e_cpu, 2.0 ** -53)
    finally:
        plan.close()


@pytest.mark.parametrize("how", ["set_values", "update", "failed"])
def test_a_backward_against_a_moved_plan_raises(how):
    sym, S, perm, VL, _ = _problem("chol")
    n = S[0]
    plan = _plan("chol", sym)
    try:
        vals, B = _dev(VL, True), _dev(np.ones(n))
        f = sf.Factorization(plan, vals)
        loss = f.solve(B).sum() + f.logdet()
        if how == "set_values":
            plan.set_values(2.0 * VL)
            plan.factorize()
        elif how == "update":
            w = np.zeros(n)
            w[n - 1] = 0.5
            plan.update(w)
        else:
            plan.set_values(-VL)
            with pytest.raises(sf.SparseFrameError):
                plan.factorize()
        with pytest.raises(RuntimeError, match="Factorization"):
            loss.backward()
        assert vals.grad is None
        with pytest.raises(RuntimeError, match="Factorization"):
            f.solve(B)
    finally:
        plan.close()
