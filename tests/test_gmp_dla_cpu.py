"""Direct learning of a gmp predistorter through a PA model (opendpd_amd/fit.py: factor_ridge, refine_steps, refine_gmp_dpd; fit_dpd_direct
at the API), the parts that need no GPU: the device-agnostic loop run in fp64 on a torch restatement of the gmp basis (the comparator,
pinned on the reference's recorded output) against numbers recorded from a CPU fp64 run, the factorisation against solve_ridge, the
loop's three stops, the exports and the argument errors."""
import functools

import numpy as np
import pytest
import torch

from tests.golden_util import Fixture, rel_err
from tests.test_gmp_ls_cpu import M, NP, P, basis, dataset, gram, train_design

RIDGE = 1e-6
RECORDED_LOSSES = [1.274e-3, 3.043e-4, 1.378e-4, 9.080e-5, 7.101e-5, 6.165e-5, 5.675e-5, 5.394e-5, 5.331e-5]
RECORDED_STEPS = [0.5, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.5]


# ---- the comparator (not the code under test) -----------------------------------------------------------------------------------------
def torch_basis(x):
    """(B, T, 2) float64 I/Q samples -> complex (B, T, 495): tests/test_gmp_ls_cpu.py::basis in torch, differentiable in x"""
    B, T = x.shape[0], x.shape[1]
    u = torch.cat([x.new_zeros(B, M - 1, dtype=torch.complex128), torch.complex(x[..., 0], x[..., 1])], 1)      # gmp.py:26-27
    # (the envelope's gradient at a zero sample is taken as 0, as the kernels take it: sqrt alone would give NaN)
    sq = x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]
    amp = torch.where(sq > 0, torch.sqrt(torch.where(sq > 0, sq, torch.ones_like(sq))), torch.zeros_like(sq))
    a = torch.cat([x.new_zeros(B, 2 * (M - 1)), amp], 1)                                                         # gmp.py:33
    pw = [a, a * a, a * a * a, (a * a) * (a * a)]
    t = torch.arange(T)
    cols = [u[:, t + m] for m in range(M)]
    cols += [u[:, t + m] * pw[d][:, t + i + m] for d in range(NP) for i in range(M) for m in range(M)]
    return torch.stack(cols, dim=2)


def torch_gmp(x, w):
    """the gmp model of weights w (495,) on sequences x (B, T, 2), each with zero history -> (B, T, 2)"""
    y = torch_basis(x) @ w.to(torch.complex128)
    return torch.stack([y.real, y.imag], -1)


def frames_gram(x, target):
    return gram(np.asarray(x), np.asarray(target))


@functools.lru_cache(maxsize=None)
def golden_case(n_frames, frame_length):
    """the issue's experiment: PA = the ridge-1e-6 gmp fit of the whole golden training stream, x = its first n_frames * frame_length
    samples as frames, start = the indirect fit x ~ gmp(y / gain) on those frames -> (x, gain, w_pa, w_start) in fp64"""
    from opendpd_amd import data as D
    from opendpd_amd.fit import solve_ridge
    d = dataset()
    w_pa = solve_ridge(train_design()[1], RIDGE).w
    gain = float(D.set_target_gain(d["train_input"], d["train_output"]))
    n = n_frames * frame_length
    x = d["train_input"][:n].reshape(n_frames, frame_length, 2)
    y = d["train_output"][:n].reshape(n_frames, frame_length, 2)
    w_start = solve_ridge(frames_gram((y / gain).astype(np.float32), x), RIDGE).w
    return x.astype(np.float64), gain, w_pa, w_start


def comparator_run(n_frames, frame_length, iterations=8, **kw):
    """refine_steps in fp64 on the comparator -> (w, run)"""
    from opendpd_amd.fit import factor_ridge, refine_steps
    x, gain, w_pa, w_start = golden_case(n_frames, frame_length)
    xt, wp = torch.from_numpy(x), torch.from_numpy(w_pa)
    target = gain * xt
    A = torch_basis(xt)                                    # the DPD's basis never changes

    def cascade(w):
        u = A @ w.to(torch.complex128)
        return torch_gmp(torch.stack([u.real, u.imag], -1), wp)

    def loss_and_grad(w):
        w = w.clone().requires_grad_(True)
        loss = torch.mean((cascade(w) - target) ** 2)
        return loss.detach(), torch.autograd.grad(loss, w)[0]

    def losses(W):
        with torch.no_grad():
            return torch.stack([torch.mean((cascade(w) - target) ** 2) for w in W])

    factor = factor_ridge(frames_gram(x, x), RIDGE)
    n = 2 * n_frames * frame_length
    return refine_steps(torch.from_numpy(w_start), loss_and_grad, losses, factor, n / (2.0 * gain * gain), iterations, **kw)


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_the_torch_comparator_reproduces_the_reference_output_and_the_numpy_basis():
    fx = Fixture("gmp_m11")
    w = torch.from_numpy(fx["sd/backbone.Weight"].astype(np.float64).reshape(-1))
    for xk, yk in (("x", "y"), ("xa", "ya")):
        x = torch.from_numpy(fx[xk].astype(np.float64))
        assert rel_err(torch_gmp(x, w).numpy(), fx[yk]) < 1e-5, xk
        phi = torch_basis(x).numpy()
        ref = np.stack([basis(xs) for xs in fx[xk]])
        assert np.max(np.abs(phi - ref)) <= 1e-14 * np.max(np.abs(ref)), xk


def test_the_loop_reproduces_the_recorded_run():
    w, run = comparator_run(7, 64)
    print("losses", " ".join(f"{v:.4e}" for v in run["losses"]), "steps", run["steps"], run["stopped"],
          f"ratio {run['losses'][0] / run['losses'][-1]:.5f}")
    assert run["steps"] == RECORDED_STEPS
    assert len(run["losses"]) == len(RECORDED_LOSSES)
    for got, ref in zip(run["losses"], RECORDED_LOSSES):
        assert abs(got - ref) <= 0.01 * ref, (got, ref)
    assert run["stopped"] == "iterations"
    assert w.dtype == torch.float64 and tuple(w.shape) == (P,)


def test_factor_ridge_solves_what_solve_ridge_solves():
    from opendpd_amd.fit import factor_ridge, solve_ridge
    x = np.tile(np.array([[0.3, -0.4]], dtype=np.float32), (64, 1))[None]
    for name, G in (("training stream", train_design()[1]), ("constant sequence", gram(x, 2.0 * x))):
        sol, F = solve_ridge(G, RIDGE), factor_ridge(G, RIDGE)
        scale = np.max(np.abs(sol.w))
        assert np.max(np.abs(F.solve(G[:P, P]) - sol.w)) <= 1e-12 * scale, name
        # the same products through torch's matvecs, which sum in another order: 495 roundings of 2^-53, amplified by at most 1 / ridge
        on_torch = F.solve(torch.from_numpy(np.ascontiguousarray(G[:P, P])))
        assert on_torch.dtype == torch.float64 and np.max(np.abs(on_torch.numpy() - sol.w)) <= P * 2.0 ** -53 / RIDGE * scale, name
        assert (F.e_min, F.e_max) == (sol.e_min, sol.e_max) and F.V.shape == (P, P) and F.e.shape == (P,)
    assert np.linalg.matrix_rank(gram(x, 2.0 * x)[:P, :P]) < P


class _Identity:
    e_min = e_max = 1.0

    @staticmethod
    def solve(r):
        return r


def _quadratic(w):
    return (w * w).sum(), 2.0 * w


def test_a_direction_that_cannot_descend_stops_and_leaves_w():
    from opendpd_amd.fit import refine_steps
    w0 = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    seen = []
    w, run = refine_steps(w0, _quadratic, lambda W: (w0 * w0).sum() + 0.25 + 0 * W[:, 0], _Identity, 0.25, iterations=5,
                          accepted=lambda k, w, loss: seen.append(k))
    assert run["stopped"] == "no_descent" and run["steps"] == [] and run["losses"] == [float((w0 * w0).sum())]
    assert torch.equal(w, w0) and seen == [0]


def test_tol_above_one_stops_after_one_accepted_step():
    from opendpd_amd.fit import refine_steps
    w0 = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    w, run = refine_steps(w0, _quadratic, lambda W: (W * W).sum(1), _Identity, 0.25, iterations=5, tol=1.5)
    assert run["stopped"] == "converged" and run["steps"] == [1.0] and len(run["losses"]) == 2
    assert torch.equal(w, 0.5 * w0)                      # d = -0.25 * 2 w: the full step halves w


def test_zero_iterations_return_the_start():
    from opendpd_amd.fit import refine_steps
    w0 = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    w, run = refine_steps(w0, _quadratic, lambda W: (W * W).sum(1), _Identity, 0.25, iterations=0)
    assert torch.equal(w, w0) and run == dict(losses=[5.25], steps=[], stopped="iterations")


def test_exports():
    import opendpd_amd
    from opendpd_amd import api
    assert opendpd_amd.fit_dpd_direct is api.fit_dpd_direct and callable(api.fit_dpd_direct)
    for name in ("fit_dpd_direct", "factor_ridge", "refine_gmp_dpd"):
        assert name in opendpd_amd.__all__ and callable(getattr(opendpd_amd, name)), name
    from opendpd_amd.project import run_fit_dpd_direct      # noqa: F401
    # (no OpenDPDTrainer method: the class keeps exactly the reference's public names, tests/test_api_cpu.py — as fit_pa / fit_dpd have none)

def test_argument_errors(tmp_path, monkeypatch):
    import opendpd_amd as od
    from opendpd_amd.fit import refine_gmp_dpd
    monkeypatch.chdir(tmp_path)
    kw = dict(dataset_name="DPA_200MHz", PA_backbone="gmp", PA_hidden_size=11)
    with pytest.raises(ValueError):
        od.fit_dpd_direct(DPD_backbone="dgru", **kw)
    with pytest.raises(ValueError):
        od.fit_dpd_direct(DPD_hidden_size=12, **kw)
    with pytest.raises(ValueError):
        od.fit_dpd_direct(ridge=-1e-6, **kw)
    with pytest.raises(ValueError):
        od.fit_dpd_direct(start="somewhere/that/does/not/exist.pt", **kw)
    with pytest.raises(ValueError):
        od.fit_dpd_direct(iterations=-1, **kw)
    x = torch.zeros(1, 32, 2)
    gmp, dgru = od.CoreModel(2, 11, 1, "gmp"), od.CoreModel(2, 8, 1, "dgru")
    with pytest.raises(ValueError):
        refine_gmp_dpd(dgru, gmp, x, 2.5)
    with pytest.raises(ValueError):
        refine_gmp_dpd(gmp, gmp, x, 2.5, ridge=-1.0)
    assert not list(tmp_path.iterdir())                  # refused before a directory was made
