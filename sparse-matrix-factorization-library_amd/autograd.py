"""torch.autograd for resident factorizations: a solve, a quadratic form or a log-determinant of a plan as a node of
a torch graph whose differentiable inputs are the matrix VALUES (and B).  The only module of the package that imports torch at
import time; the package re-exports it lazily.

    f = Factorization(plan, values)            # set_values_device + factorize, once
    x = f.solve(b)                             # A^-1 b
    nll = 0.5 * f.logdet() + 0.5 * f.quadform(b).sum()
    nll.backward()                             # values.grad, b.grad

Every backward runs on the device through the plan's own entry points: the other-transposition solve for B, and
`adjoint_values_device` / `logdet_grad_values_device` for the values -- no (nnz x k) temporary, no index arithmetic here.
Backward passes are once-differentiable.  A backward whose plan has meanwhile been given other values or another factor raises
RuntimeError instead of returning the gradient of a different matrix.
"""
import torch
from torch.autograd.function import once_differentiable

from .api import LUPlan

__all__ = ["Factorization"]


def _colmajor(T):
    """T with unit stride along the rows and columns that do not overlap (what the plans' device entry points take)"""
    if T.dim() != 2:
        return T.contiguous()
    n, k = T.shape
    if (n > 1 and T.stride(0) != 1) or (k > 1 and T.stride(1) < max(n, 1)):
        return T.t().contiguous().t()
    return T


def _row_major(T):
    """T is a 2-D tensor in row-major order (and not column-major as well)"""
    return T.dim() == 2 and T.is_contiguous() and not T.t().is_contiguous()


def _ordered(G, row_major):
    """G in the memory order its input had (a row-major B gets a row-major result and gradient)"""
    return G.contiguous() if row_major and not G.is_contiguous() else G


class Factorization:
    """A plan factorized at `values`, as the source of differentiable results.

    plan: a whole, resident CholPlan or LUPlan.  values: 1-D float64 device tensor in set_values order (valuesU: the U part of an
    LUPlan with its own U structure), or with mapped=True the caller's own nsrc-entry array (set_value_map).  Right-hand sides and
    results are in the caller's numbering when the plan holds an ordering (set_ordering; the plan's stat "ordering_set"), else in
    permuted space.
    """

    def __init__(self, plan, values, valuesU=None, mapped=False):
        self.plan = plan
        self.lu = isinstance(plan, LUPlan)
        self.values, self.valuesU, self.mapped, self.perm = values, valuesU, bool(mapped), plan.stat("ordering_set") == 1.0
        if mapped and valuesU is not None:
            raise ValueError("Factorization: mapped values are one array (valuesU must be None)")
        with torch.no_grad():
            if mapped:
                plan.set_values_mapped_device(values.detach())
            elif self.lu:
                plan.set_values_device(values.detach(), None if valuesU is None else valuesU.detach())
            else:
                plan.set_values_device(values.detach())
        plan.factorize()
        self._gen = plan.stat("factor_generation")
        self._selinv_done = False
        self.sign = None

    # ---- the guard ----
    def check(self):
        """RuntimeError unless the plan still holds the factorization this object made"""
        now = self.plan.stat("factor_generation")
        if not self.plan.stat("factor_usable"):
            raise RuntimeError("Factorization: the plan's last factorization or update failed; its factor is not the one this "
                               "Factorization computed (a gradient from it would belong to no matrix)")
        if now != self._gen:
            raise RuntimeError(f"Factorization: the plan's values or factor have changed since this Factorization was made (factor "
                               f"generation {int(self._gen)}, now {int(now)}: set_values, factorize, update, rowdel or rowadd); "
                               "make a new Factorization")

    def _value_inputs(self):
        return self.values, self.valuesU

    def _ops(self, trans):
        """(op of the forward solve, op of the other transposition)"""
        if not self.lu:
            return "solve", "solve"
        return ("trans", "solve") if trans else ("solve", "trans")

    def _solve(self, B, op):
        return self.plan.solve_device(_colmajor(B), op=op, perm_in=self.perm, perm_out=self.perm)

    def _adjoint(self, Y, X, alpha):
        """(d values, d valuesU or None)"""
        r = self.plan.adjoint_values_device(Y, X, alpha=alpha, perm_in=self.perm, mapped=self.mapped)
        return r if isinstance(r, tuple) else (r, None)

    # ---- the differentiable results ----
    def solve(self, B, trans=False):
        """X = A^-1 B (trans, LUPlan: A^-T B); B (n,) or (n, k)"""
        if trans and not self.lu:
            raise ValueError("Factorization.solve: trans is for an LUPlan (a Cholesky plan's matrix is symmetric)")
        return _Solve.apply(self, bool(trans), B, *self._value_inputs())

    def quadform(self, B):
        """q[c] = b_c^T A^-1 b_c; B (n,) -> a scalar, (n, k) -> (k,)"""
        return _Quadform.apply(self, B, *self._value_inputs())

    def logdet(self):
        """log det A (LUPlan: log|det A|, and the sign of det A as the attribute .sign of the result and of this object)"""
        out = _Logdet.apply(self, *self._value_inputs())
        if self.lu:
            out.sign = self.sign
        return out


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fact, trans, B, values, valuesU):
        fact.check()
        X = fact._solve(B.detach(), fact._ops(trans)[0])
        ctx.fact, ctx.trans, ctx.row_major = fact, trans, _row_major(B)
        ctx.save_for_backward(X)
        return _ordered(X, ctx.row_major)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        fact = ctx.fact
        fact.check()
        X, = ctx.saved_tensors
        Lam = fact._solve(G, fact._ops(ctx.trans)[1])
        dV = dU = None
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            # X = A^-1 B: <G, dX> = -sum_c lam_c^T dA x_c; X = A^-T B: the roles of Lam and X swap
            Xc = _colmajor(X)
            dV, dU = fact._adjoint(Xc, Lam, -1.0) if ctx.trans else fact._adjoint(Lam, Xc, -1.0)
        dB = _ordered(Lam, ctx.row_major) if ctx.needs_input_grad[2] else None
        return None, None, dB, dV, dU


class _Quadform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fact, B, values, valuesU):
        fact.check()
        Bd = _colmajor(B.detach())
        X = fact._solve(Bd, "solve")
        ctx.fact, ctx.row_major = fact, _row_major(B)
        ctx.save_for_backward(X, Bd)
        return (Bd * X).sum(0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        fact = ctx.fact
        fact.check()
        X, Bd = ctx.saved_tensors
        # q = b^T A^-1 b: dq = 2 x^T db - x^T dA x for a symmetric A; in general db meets x + A^-T b and dA meets (A^-T b) x^T
        Xt = fact._solve(Bd, "trans") if fact.lu else X
        Yg = _colmajor(Xt * g)
        dV = dU = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dV, dU = fact._adjoint(Yg, X, -1.0)
        dB = None
        if ctx.needs_input_grad[1]:
            dB = _ordered((2.0 * X * g) if not fact.lu else ((X + Xt) * g), ctx.row_major)
        return None, dB, dV, dU


class _Logdet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fact, values, valuesU):
        fact.check()
        r = fact.plan.logdet()
        if fact.lu:
            r, fact.sign = r
        ctx.fact = fact
        return torch.tensor(float(r), dtype=torch.float64, device=fact.values.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        fact = ctx.fact
        fact.check()
        if not fact._selinv_done:
            fact.plan.selinv()
            fact._selinv_done = True
        r = fact.plan.logdet_grad_values_device(alpha=float(g), mapped=fact.mapped)
        dV, dU = r if isinstance(r, tuple) else (r, None)
        return None, dV, dU
