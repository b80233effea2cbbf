"""Closed-form fit of the gmp backbone.

gmp is the one registry backbone that is linear in its parameters (495 real weights on complex basis terms, backbones/gmp.py), so
the optimum of the L2 loss that `train_pa --PA_backbone gmp` descends is one symmetric solve:
  gmp_gram    the 496 x 496 normal equations [A | b]^T [A | b] in fp64, on the device (csrc/gmp_ls.hip: the basis is formed inside
              the kernel and accumulated on the fp64 matrix pipe — the Gram matrix of these columns is numerically singular, fp32
              accumulation loses the fit);
  solve_ridge the ridge-regularised solution, on the host in fp64 (a 495 x 495 symmetric eigendecomposition: milliseconds);
  fit_gmp     both, as an ordinary CoreModel("gmp") for every existing kernel and entry point.
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


def solve_ridge(gram, ridge=1e-6):
    """w = argmin ||A w - b||^2 + ridge * e_max * ||w||^2 from the (n + 1, n + 1) Gram matrix of [A | b], on the host in fp64:
    G[:n, :n] = V diag(e) V^T, w = V diag(1 / (e + ridge * e_max)) V^T r.  The ridge is relative to the largest eigenvalue, so it means
    the same whatever the signal's scale; directions whose regularised eigenvalue is not positive (ridge = 0 on a singular matrix) get
    no weight.  -> RidgeSolution(w, residual, e_min, e_max)."""
    G = gram.detach().cpu().numpy() if isinstance(gram, torch.Tensor) else np.asarray(gram)
    G = np.asarray(G, dtype=np.float64)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 2:
        raise ValueError(f"gram: expected a square matrix of [A | b], got {G.shape}")
    n = G.shape[0] - 1
    N, r, gyy = G[:n, :n], G[:n, n], float(G[n, n])
    e, V = np.linalg.eigh(0.5 * (N + N.T))
    e_min, e_max = float(e[0]), float(e[-1])
    d = e + ridge * max(e_max, 0.0)
    inv = np.zeros_like(d)
    np.divide(1.0, d, out=inv, where=d > 0.0)
    w = V @ (inv * (V.T @ r))
    residual = gyy - 2.0 * float(w @ r) + float(w @ (N @ w))
    return RidgeSolution(w, residual, e_min, e_max)


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
