"""torch.autograd on top of the least-squares objects of capi.py: ``lstsq`` solves min |A x - b| (LeastSquares) or
min |W (A x - b)|^2 + |D x|^2 with D = diag(sqrt(lam) * d) (DampedLeastSquares) and is differentiable in the values of A on their
pattern, in B, in the row weights w, the column scales d and in lam.  The forward is the object's solve, the backward is
stmmqr_ls_adjoint on the factors that solve left on the device: no second plan, nothing densified.  Imported on request
(``from <package> import autograd``): capi itself does not need torch.

Tensors are float64.  On the plan's device they go to the library by ``data_ptr()`` (solve_dev / adjoint_dev), after torch's current
stream has been waited for (the library works on a stream of its own and waits for it before it returns); CPU tensors go through the
host entry points.  B is [m] or [m, nrhs] and X [n] or [n, nrhs] in torch's row-major layout: the column-major arrays of the C
interface are made here.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .capi import DampedLeastSquares, LeastSquares, StmmqrError


def _cm(t: torch.Tensor, rows: int) -> torch.Tensor:
    """[rows] or [rows, k] -> a contiguous [k, rows] tensor: the column-major rows x k array of the C interface"""
    return t.detach().reshape(rows, -1).t().contiguous()


def _flat(t):
    return None if t is None else t.detach().reshape(-1).contiguous()


def _solve(obj, damped, Ax, B, w, d, lam):
    """one forward solve -> X as a contiguous [nrhs, n] tensor (column-major n x nrhs) on the device of Ax"""
    k, n, m = obj.nrhs, obj.n, obj.m
    Bc = _cm(B, m)
    if Bc.shape[0] != k:
        raise StmmqrError(f"lstsq: B has {Bc.shape[0]} columns, the object was created for {k}")
    axf, wf, df = _flat(Ax), _flat(w), _flat(d)
    if axf.numel() != obj.anz:
        raise StmmqrError("lstsq: Ax must hold one value per entry of A's pattern")
    if Ax.is_cuda:
        X = torch.empty((k, max(n, 1)), dtype=torch.float64, device=Ax.device)
        torch.cuda.current_stream(Ax.device).synchronize()
        ptr = lambda t: None if t is None else t.data_ptr()                                                  # noqa: E731
        if damped:
            obj.solve_dev(Bc.data_ptr(), X.data_ptr(), ax_ptr=axf.data_ptr(), w_ptr=ptr(wf), d_ptr=ptr(df), lam=lam)
        else:
            obj.solve_dev(Bc.data_ptr(), X.data_ptr(), ax_ptr=axf.data_ptr(), resid=False)
        return X[:, :n]
    Bn = Bc.numpy().T
    if damped:
        Xn = obj.solve(Bn, Ax=axf.numpy(), w=None if wf is None else wf.numpy(), d=None if df is None else df.numpy(), lam=lam)[0]
    else:
        Xn = obj.solve(Bn, Ax=axf.numpy())[0]
    return torch.from_numpy(np.ascontiguousarray(np.asarray(Xn).reshape(n, k).T))


class _LstSq(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obj, refine, Ax, B, w, d, lam):
        damped = isinstance(obj, DampedLeastSquares)
        lamv = 0.0 if lam is None else float(lam)
        X = _solve(obj, damped, Ax, B, w, d, lamv)
        ctx.obj, ctx.refine, ctx.damped, ctx.lamv = obj, int(refine), damped, lamv
        ctx.solves = obj.info["solves"]
        ctx.vector = B.dim() == 1
        ctx.save_for_backward(Ax, B, w, d, X)
        out = X.t()
        return out[:, 0].clone() if ctx.vector else out.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, Xbar):
        obj, damped, lamv = ctx.obj, ctx.damped, ctx.lamv
        Ax, B, w, d, X = ctx.saved_tensors
        n, m, k = obj.n, obj.m, obj.nrhs
        if obj.info["solves"] != ctx.solves:
            # the factors on the device belong to another solve: this one's is made again from the saved tensors
            X = _solve(obj, damped, Ax, B, w, d, lamv)
            obj.resolves = getattr(obj, "resolves", 0) + 1
            ctx.solves = obj.info["solves"]
        need_ax, need_b, need_w, need_d, need_lam = ctx.needs_input_grad[2:7]
        need_D = damped and (need_d or need_lam)
        need_w = damped and need_w
        Xc, Xb, wf = X.contiguous(), _cm(Xbar, n), _flat(w)
        if Ax.is_cuda:
            dev = Ax.device
            new = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)                                 # noqa: E731
            gA = new(max(obj.anz, 1)) if need_ax else None
            gB = new(k, max(m, 1)) if need_b else None
            gw = new(max(m, 1)) if need_w else None
            gD = new(max(n, 1)) if need_D else None
            ptr = lambda t: None if t is None else t.data_ptr()                                              # noqa: E731
            torch.cuda.current_stream(dev).synchronize()
            if damped:
                obj.adjoint_dev(Xc.data_ptr(), Xb.data_ptr(), w_ptr=ptr(wf), axbar_ptr=ptr(gA), bbar_ptr=ptr(gB), wbar_ptr=ptr(gw),
                                dbar_ptr=ptr(gD), refine=ctx.refine)
            else:
                obj.adjoint_dev(Xc.data_ptr(), Xb.data_ptr(), axbar_ptr=ptr(gA), bbar_ptr=ptr(gB), refine=ctx.refine)
            Z = None
            if need_lam:
                Z = new(k, max(n, 1))
                obj.adjoint_z(dev_ptr=Z.data_ptr())
                Z = Z[:, :n]
            gA = None if gA is None else gA[:obj.anz]
            gB = None if gB is None else gB[:, :m]
            gw = None if gw is None else gw[:m]
            gD = None if gD is None else gD[:n]
        else:
            xn, xbn = Xc.numpy().T, Xb.numpy().T
            if damped:
                a, b, wb, Db, _ = obj.adjoint(xn, xbn, w=None if wf is None else wf.numpy(), refine=ctx.refine)
            else:
                (a, b, _), wb, Db = obj.adjoint(xn, xbn, refine=ctx.refine), None, None
            t = lambda v: torch.from_numpy(np.ascontiguousarray(v))                                          # noqa: E731
            gA = t(a) if need_ax else None
            gB = t(np.asarray(b).reshape(m, k).T) if need_b else None
            gw = t(wb) if need_w else None
            gD = t(Db) if need_D else None
            Z = t(obj.adjoint_z().T) if need_lam else None
        gd = glam = None
        if damped and need_d:
            gd = (math.sqrt(lamv) * gD).reshape(d.shape)
        if damped and need_lam:
            # lambdabar = -sum_j s_j^2 sum_k x[j,k] z[j,k]: finite at lam = 0, where Dbar / (2 sqrt(lam)) is not
            q = (Xc * Z).sum(dim=0)
            s2 = q.new_ones(n) if d is None else _flat(d) ** 2
            glam = -(s2 * q).sum().reshape(())
        if gA is not None:
            gA = gA.reshape(Ax.shape)
        if gB is not None:
            gB = gB.t().reshape(B.shape)
        if gw is not None:
            gw = gw.reshape(w.shape)
        return None, None, gA, gB, gw, gd, glam


def lstsq(obj, Ax, B, w=None, d=None, lam=None, refine=1, scale=0):
    """X = argmin |A x - B| for a LeastSquares ``obj`` or argmin |W (A x - B)|^2 + lam |diag(d) x|^2 for a DampedLeastSquares one,
    differentiable in Ax [anz], B ([m] or [m, nrhs]), w [m], d [n] and lam (a float or a 0-dim tensor); None = all 1 / 0.  All
    tensors float64 and on one device: the plan's, or the CPU.  refine: the refinement steps of the adjoint's normal solve
    (stmmqr_ls_adjoint).  Rank-deficient A: the gradient of the basic solution with the dead set held fixed.

    Two forwards through one object before a backward are allowed: the backward that finds another solve's factors on the device
    repeats its own solve first and counts it in ``obj.resolves``."""
    if scale != 0:
        raise StmmqrError("lstsq: scale = 1 is not offered: the column scales would depend on W A, and the adjoint does not go through them")
    if not isinstance(obj, LeastSquares):
        raise StmmqrError("lstsq: obj must be a LeastSquares or a DampedLeastSquares object")
    damped = isinstance(obj, DampedLeastSquares)
    if not damped and (w is not None or d is not None or lam is not None):
        raise StmmqrError("lstsq: w, d and lam need a DampedLeastSquares object")
    tensors = [t for t in (Ax, B, w, d, lam) if isinstance(t, torch.Tensor)]
    if not isinstance(Ax, torch.Tensor) or not isinstance(B, torch.Tensor):
        raise StmmqrError("lstsq: Ax and B must be tensors")
    for t in tensors:
        if t.dtype != torch.float64:
            raise StmmqrError("lstsq: tensors must be float64")
        if t.device != Ax.device:
            raise StmmqrError("lstsq: all tensors must be on one device")
    if lam is not None and not isinstance(lam, torch.Tensor):
        lam = float(lam)
    if isinstance(lam, torch.Tensor) and lam.dim() != 0:
        raise StmmqrError("lstsq: lam must be a float or a 0-dim tensor")
    if not hasattr(obj, "resolves"):
        obj.resolves = 0
    return _LstSq.apply(obj, refine, Ax, B, w, d, lam)
