"""Closed-form fit of the gmp backbone.

gmp is the one registry backbone that is linear in its parameters (495 real weights on complex basis terms, backbones/gmp.py), so
the optimum of the L2 loss that `train_pa --PA_backbone gmp` descends is one symmetric solve:
  gmp_gram    the 496 x 496 normal equations [A | b]^T [A | b] in fp64, on the device (csrc/gmp_ls.hip: the basis is formed inside
              the kernel and accumulated on the fp64 matrix pipe — the Gram matrix of these columns is numerically singular, fp32
              accumulation loses the fit);
  solve_ridge the ridge-regularised solution, on the host in fp64 (a 495 x 495 symmetric eigendecomposition: milliseconds);
  fit_gmp     both, as an ordinary CoreModel("gmp") for every existing kernel and entry point.
A gmp predistorter through a frozen PA model is no longer linear, but its basis still never changes, so the same Gram matrix
preconditions the loss train_dpd descends (docs/design/gmp_ls.md, "Direct learning"):
  factor_ridge    solve_ridge's eigendecomposition kept for many right-hand sides;
  refine_steps    preconditioned gradient steps with a line search whose candidates are evaluated together, over callables;
  refine_gmp_dpd  that loop on the existing kernels (no kernel of its own).
No CPU path: the samples must be on a HIP device."""
import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

N_WEIGHTS = 495          # memory_length 11, degree 5 (the configuration the registry builds)
N_COLS = N_WEIGHTS + 1   # + the target column


def _desc():
    return _lib.ModelDesc(_lib.BACKBONE_IDS["gmp"], 11, 0.0, 0.0, 0, 0, 0)


def _sequences(t, name):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t), dtype=torch.float32)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[-1] != 2:
        raise ValueError(f"{name}: expected (B, T, 2) or (T, 2) I/Q samples, got {tuple(t.shape)}")
    return t


def gmp_gram(x, target):
    """G = [A | b]^T [A | b] (496, 496) torch.float64 on the device of `x`, for sequences x, target (B, T, 2) (or one sequence (T, 2)),
    each with the reference's zero history.  A has two rows per output sample (real, imaginary part) and one column per gmp weight in
    the order of `backbone.Weight`; b is the target.  G[:495, :495] is the normal matrix, G[:495, 495] the right-hand side,
    G[495, 495] the target's energy.  Deterministic: two calls give the same bits."""
    x, target = _sequences(x, "x"), _sequences(target, "target")
    if not x.is_cuda:
        raise RuntimeError("opendpd_amd kernels need tensors on a HIP device (no CPU fallback)")
    target = target.to(x.device)
    if x.shape != target.shape:
        raise ValueError(f"x {tuple(x.shape)} and target {tuple(target.shape)} differ in shape")
    x, target = x.detach().float().contiguous(), target.detach().float().contiguous()
    B, T = int(x.shape[0]), int(x.shape[1])
    lib, d = _lib.load(), _desc()
    nbytes = int(lib.odpd_gmp_gram_workspace_bytes(C.byref(d), B, T))
    if nbytes <= 0:
        _lib.check(nbytes, "odpd_gmp_gram_workspace_bytes")
    with torch.cuda.device(x.device):
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        gram = torch.empty(N_COLS, N_COLS, dtype=torch.float64, device=x.device)
        _lib.check(lib.odpd_gmp_gram(_lib.stream_ptr(), C.byref(d), _lib.ptr(x), _lib.ptr(target), B, T, _lib.ptr(gram), _lib.ptr(ws)),
                   "odpd_gmp_gram")
    return gram


class RidgeSolution(NamedTuple):
    w: np.ndarray        # (495,) float64
    residual: float      # ||A w - b||^2 = G_yy - 2 w^T r + w^T G w
    e_min: float         # smallest / largest eigenvalue of the normal matrix
    e_max: float


def _host_gram(gram):
    G = gram.detach().cpu().numpy() if isinstance(gram, torch.Tensor) else np.asarray(gram)
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 2:
        raise ValueError(f"gram: expected a square matrix of [A | b], got {G.shape}")
    return G


class RidgeFactor:
    """The eigendecomposition G[:n, :n] = V diag(e) V^T of an (n + 1, n + 1) Gram matrix of [A | b] with its ridge, kept for more than one
    right-hand side: `solve(r) = V diag(1 / (e + ridge * e_max)) V^T r`, solve_ridge's rule (directions whose regularised eigenvalue is not
    positive get no weight).  A numpy `r` is solved on the host; a torch `r` on its own device in fp64 (V is copied there once), so a loop
    that keeps its vectors on the device needs no host round trip."""

    def __init__(self, gram, ridge=1e-6):
        G = _host_gram(gram)
        n = G.shape[0] - 1
        N = G[:n, :n]
        self.e, self.V = np.linalg.eigh(0.5 * (N + N.T))
        self.ridge, self.e_min, self.e_max = ridge, float(self.e[0]), float(self.e[-1])
        d = self.e + ridge * max(self.e_max, 0.0)
        self.inv = np.zeros_like(d)
        np.divide(1.0, d, out=self.inv, where=d > 0.0)
        self._on = {}      # device -> (V, inv) as torch.float64

    def solve(self, r):
        if not isinstance(r, torch.Tensor):
            return self.V @ (self.inv * (self.V.T @ np.asarray(r, dtype=np.float64)))
        if r.device not in self._on:
            self._on[r.device] = (torch.from_numpy(self.V).to(r.device), torch.from_numpy(self.inv).to(r.device))
        V, inv = self._on[r.device]
        return V @ (inv * (V.T @ r.double()))


def factor_ridge(gram, ridge=1e-6):
    """-> RidgeFactor of the (n + 1, n + 1) Gram matrix of [A | b] (only G[:n, :n] is read): V, e, e_min, e_max and `.solve(r)`."""
    return RidgeFactor(gram, ridge)


def solve_ridge(gram, ridge=1e-6):
    """w = argmin ||A w - b||^2 + ridge * e_max * ||w||^2 from the (n + 1, n + 1) Gram matrix of [A | b], on the host in fp64:
    G[:n, :n] = V diag(e) V^T, w = V diag(1 / (e + ridge * e_max)) V^T r.  The ridge is relative to the largest eigenvalue, so it means
    the same whatever the signal's scale; directions whose regularised eigenvalue is not positive (ridge = 0 on a singular matrix) get
    no weight.  -> RidgeSolution(w, residual, e_min, e_max)."""
    G = _host_gram(gram)
    n = G.shape[0] - 1
    N, r, gyy = G[:n, :n], G[:n, n], float(G[n, n])
    F = RidgeFactor(G, ridge)
    w = F.solve(r)
    residual = gyy - 2.0 * float(w @ r) + float(w @ (N @ w))
    return RidgeSolution(w, residual, F.e_min, F.e_max)


def fit_gmp(x, target, ridge=1e-6, net=None):
    """The ridge least-squares gmp model of target ~ gmp(x): a CoreModel("gmp") on the device of `x` with `backbone.Weight` set (fp32).
    `net`: an existing gmp CoreModel to fill instead of a new one.  The solution's numbers stay on the model as `net.gmp_fit`
    (a dict of the RidgeSolution fields and `n_samples`)."""
    from .models import CoreModel
    x = _sequences(x, "x")
    sol = solve_ridge(gmp_gram(x, target), ridge)
    if net is None:
        net = CoreModel(2, 11, 1, "gmp")
    if getattr(net, "backbone_type", None) != "gmp" or net.backbone.Weight.numel() != N_WEIGHTS:
        raise ValueError("fit_gmp fills a CoreModel('gmp')")
    net = net.to(x.device)
    with torch.no_grad():
        net.backbone.Weight.copy_(torch.from_numpy(sol.w).to(torch.float32).view(1, N_WEIGHTS))
    net.gmp_fit = dict(sol._asdict(), n_samples=int(x.shape[0] * x.shape[1]))
    return net


def refine_steps(w, loss_and_grad, losses, factor, scale, iterations=8, halvings=6, tol=1e-4, accepted=None):
    """The loop of refine_gmp_dpd on any device and in any precision its callables work in: preconditioned gradient steps with a
    backtracking line search whose candidates are evaluated together.
      w              (n,) start; the master copy is torch.float64 on w's device
      loss_and_grad  w -> (loss, dloss/dw (n,)) as tensors on that device
      losses         W (K, n) -> the K losses of the rows of W, one tensor
      factor         RidgeFactor of the preconditioner; the direction is d = -scale * factor.solve(grad)
      accepted       called as accepted(k, w, loss) for the start (k = 0) and after every accepted step
    Per iteration the candidates w + 2^-k d, k = 0 .. halvings, are evaluated in one `losses` call and the largest step whose loss is below
    the current one is taken; the current loss and the candidates' come to the host in one transfer, the only synchronisation of the
    iteration.  The current loss is `loss_and_grad`'s at the start and the accepted candidate's from then on (the same quantity at the same
    w), so the recorded losses fall strictly by construction.  Stops: "no_descent" when no candidate is lower (w stays), "converged" when
    an accepted step lowered the loss by less than `tol` of it, "iterations" after `iterations` accepted steps.
    -> (w, dict(losses, steps, stopped))"""
    w = w.detach().double().reshape(-1)
    shrink = 0.5 ** torch.arange(halvings + 1, dtype=torch.float64, device=w.device)
    hist, steps, stopped = [], [], "iterations"
    L, grad = loss_and_grad(w)

    def record_start(value):
        hist.append(value)
        if accepted is not None:
            accepted(0, w, value)

    for it in range(iterations):
        d = -scale * factor.solve(grad.detach().double().reshape(-1))
        W = w[None, :] + shrink[:, None] * d[None, :]
        vals = torch.cat([L.detach().double().reshape(1), losses(W).detach().double().reshape(-1)]).cpu().tolist()
        if not hist:
            record_start(vals[0])
        base = hist[-1]
        k = next((k for k, v in enumerate(vals[1:]) if v < base), None)      # (a NaN candidate is never below)
        if k is None:
            stopped = "no_descent"
            break
        w = W[k].clone()
        hist.append(vals[1 + k])
        steps.append(0.5 ** k)
        if accepted is not None:
            accepted(len(steps), w, hist[-1])
        if (base - hist[-1]) / base < tol:
            stopped = "converged"
            break
        if it + 1 < iterations:
            L, grad = loss_and_grad(w)
    if not hist:
        record_start(float(L))
    return w, dict(losses=hist, steps=steps, stopped=stopped)


def candidate_losses(dpd, pa, x, target, W):
    """mean((PA(DPD_w(x)) - target)^2) for every row w of W (K, 495) -> (K,) on x's device, without a host synchronisation: one gmp forward
    per candidate (the kernel takes one weight vector per launch), the K outputs stacked along the batch for ONE PA forward of K * B
    sequences, then per candidate the reduction a single cascade's loss runs (so a feed-forward PA, whose sequences are independent, gives
    the bits of K separate evaluations).  Leaves the last row in `dpd.backbone.Weight`."""
    B, T = int(x.shape[0]), int(x.shape[1])
    with torch.no_grad():
        u = []
        for w in W:
            dpd.backbone.Weight.copy_(w.to(torch.float32).view(1, N_WEIGHTS))
            u.append(dpd(x))
        y = pa(torch.cat(u, dim=0)).view(len(u), B, T, 2)
        return torch.stack([torch.nn.functional.mse_loss(yk, target) for yk in y])


def refine_gmp_dpd(dpd, pa, x, gain, iterations=8, ridge=1e-6, halvings=6, tol=1e-4, accepted=None):
    """Direct learning of a gmp predistorter through a frozen PA model: lowers what train_dpd descends, mean((PA(DPD(x)) - gain x)^2), from
    the weights `dpd` holds, by `refine_steps`.  The DPD's output is A(x) w with a basis that never changes, so N = A^T A (gmp_gram, fp64,
    factored once) preconditions every step: with a PA close to gain * identity the Gauss-Newton Hessian is (2 gain^2 / n) N, n = 2 B T,
    and the direction is d = -(n / (2 gain^2)) (N + ridge e_max I)^-1 dL/dw.
      dpd   CoreModel("gmp"); its `backbone.Weight` is the start and receives the fp32 cast of the fp64 result
      pa    any CoreModel; its parameters are not written (a kernel-backed PA returns dL/du from its backward kernel with no weight
            gradient, an ATen-route PA goes through autograd)
      x     (B, T, 2) on a HIP device, every sequence with zero history
    Per iteration: one cascade forward + backward on x (loss and dL/dw, the kernels train_dpd runs), then the halvings + 1 candidates in
    one line-search forward — one gmp forward per candidate weight vector, their outputs stacked along the batch for ONE PA forward of
    (halvings + 1) * B sequences, the per-candidate means by torch — and one host synchronisation.
    -> dpd; the run stays on it as `dpd.gmp_refine`: losses (accepted steps + 1), steps, stopped, n_samples, e_min, e_max, w (fp64)."""
    from .models import CascadedModel
    if getattr(dpd, "backbone_type", None) != "gmp" or dpd.backbone.Weight.numel() != N_WEIGHTS:
        raise ValueError("refine_gmp_dpd refines a CoreModel('gmp')")
    if not ridge >= 0.0:
        raise ValueError(f"ridge={ridge!r}: expected a number >= 0")
    if iterations < 0 or halvings < 0:
        raise ValueError(f"iterations={iterations!r}, halvings={halvings!r}: expected non-negative counts")
    x = _sequences(x, "x")
    if not x.is_cuda:
        raise RuntimeError("opendpd_amd kernels need tensors on a HIP device (no CPU fallback)")
    x = x.detach().float().contiguous()
    B, T = int(x.shape[0]), int(x.shape[1])
    gain = float(gain)
    target = gain * x
    dpd, pa = dpd.to(x.device), pa.to(x.device)
    net = CascadedModel(dpd, pa)
    weight = dpd.backbone.Weight
    factor = factor_ridge(gmp_gram(x, x), ridge)
    mse = torch.nn.functional.mse_loss

    def put(w):
        with torch.no_grad():
            weight.copy_(w.to(torch.float32).view(1, N_WEIGHTS))

    def loss_and_grad(w):
        put(w)
        loss = mse(net(x), target)
        return loss.detach(), torch.autograd.grad(loss, weight)[0].reshape(-1)

    def losses(W):
        return candidate_losses(dpd, pa, x, target, W)

    def on_accept(k, w, loss):
        put(w)
        if accepted is not None:
            accepted(k, w, loss)

    state = [(p, p.requires_grad) for p in list(pa.parameters()) + [weight]]
    try:
        for p in pa.parameters():
            p.requires_grad_(False)
        weight.requires_grad_(True)
        w, run = refine_steps(weight.detach().double().reshape(-1), loss_and_grad, losses, factor, B * T / (gain * gain),
                              iterations, halvings, tol, on_accept)
    finally:
        for p, flag in state:
            p.requires_grad_(flag)
    put(w)
    dpd.gmp_refine = dict(run, n_samples=B * T, e_min=factor.e_min, e_max=factor.e_max, w=w.cpu().numpy())
    return dpd
