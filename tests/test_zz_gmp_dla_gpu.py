"""Direct learning of a gmp predistorter through a PA model on the device (opendpd_amd/fit.py: refine_gmp_dpd, candidate_losses;
fit_dpd_direct at the API).  No kernel of its own: every launch is an existing one (odpd_gmp_gram, the gmp forward and weight gradient, the
PA's forward and dL/du), so what is held here is the loop — its invariants at every shape, a decrease it must reach, the one-forward line
search against candidates evaluated alone, and the files of the project flow.

Shapes: frames of the golden training stream.  (7, 64) and (20, 200) carry the decrease (a frame barely above the 20-sample look-back;
4 000 samples across the 512-sample Gram chunks); (3, 21) and (1, 513) the invariants alone (one sample past the look-back, one past a
chunk).  Kernel routes of the recurrent PA (dgru, 8 units; csrc/gru_family.hip gru_plan, 256 CUs): a forward without checkpoints goes to
gru_eval_kernel, one sequence per wave, up to 512 sequences, and to the row-rotated kernel, four sequences per wave, beyond — so B = 20
alone and 7 * 20 = 140 stacked both run gru_eval_kernel, B = 80 alone runs it and 7 * 80 = 560 stacked the row-rotated one.  The gmp
kernel has one route.

Measured on an MI355X: see docs/design/gmp_ls.md ("Direct learning")."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests.test_gmp_ls_cpu import P, dataset
from tests.test_zz_gmp_ls_gpu import workdir  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

RIDGE = 1e-6
STEPS = {2.0 ** -k for k in range(7)}
# the fp64 comparator's runs (tests/test_gmp_dla_cpu.py::comparator_run), 8 iterations from the indirect start
COMPARATOR = {(7, 64): [1.2742089e-03, 3.0430698e-04, 1.3776296e-04, 9.0797682e-05, 7.1013728e-05, 6.1653941e-05, 5.6750177e-05,
                        5.3942583e-05, 5.3308007e-05],
              (20, 200): [4.4895058e-04, 2.9488498e-04, 1.8741942e-04, 4.4237563e-05, 3.3207432e-05, 3.3155894e-05, 3.1312568e-05,
                          3.1224402e-05, 3.0791442e-05]}


@functools.lru_cache(maxsize=None)
def gain():
    from opendpd_amd import data as D
    d = dataset()
    return float(D.set_target_gain(d["train_input"], d["train_output"]))


@functools.lru_cache(maxsize=None)
def gmp_pa():
    """the ridge-1e-6 gmp fit of the whole training stream (never written to)"""
    from opendpd_amd import fit_gmp
    d = dataset()
    return fit_gmp(torch.from_numpy(d["train_input"][None]).cuda(), torch.from_numpy(d["train_output"][None]).cuda(), ridge=RIDGE)


def dgru_pa():
    from opendpd_amd import CoreModel
    torch.manual_seed(1)
    return CoreModel(2, 8, 1, "dgru").cuda()


def frames(B, T):
    d = dataset()
    cut = lambda s: torch.from_numpy(np.ascontiguousarray(s[:B * T].reshape(B, T, 2))).cuda()
    return cut(d["train_input"]), cut(d["train_output"])


def indirect_start(B, T):
    """a fresh gmp DPD holding the one-shot indirect fit x ~ gmp(y / gain) on the frames"""
    from opendpd_amd import fit_gmp
    x, y = frames(B, T)
    return fit_gmp(y / gain(), x, ridge=RIDGE), x


def refine_and_check(B, T, pa, iterations=8):
    """refine_gmp_dpd from the indirect start, with everything that holds by construction -> the run"""
    from opendpd_amd import refine_gmp_dpd
    before = [p.detach().clone() for p in pa.parameters()]
    flags = [p.requires_grad for p in pa.parameters()]
    dpd, x = indirect_start(B, T)
    w_start = dpd.backbone.Weight.detach().clone()
    run = refine_gmp_dpd(dpd, pa, x, gain(), iterations=iterations, ridge=RIDGE).gmp_refine
    L, steps = run["losses"], run["steps"]
    print(f"({B}, {T}) {pa.backbone_type} PA: losses {' '.join(f'{v:.6e}' for v in L)}; steps {steps}; {run['stopped']}; "
          f"ratio {L[0] / L[-1]:.5f}")
    assert all(b < a for a, b in zip(L, L[1:])), L                       # strictly decreasing
    assert len(steps) == len(L) - 1 <= iterations and set(steps) <= STEPS
    assert run["stopped"] in ("iterations", "converged", "no_descent") and (run["stopped"] != "iterations" or len(steps) == iterations)
    assert run["n_samples"] == B * T and run["e_max"] > 0 and run["e_min"] <= run["e_max"]
    for p, q, f in zip(pa.parameters(), before, flags):
        assert torch.equal(p.detach(), q) and p.requires_grad == f       # the PA is bit-identical, and trainable if it was
    w = run["w"]
    assert w.dtype == np.float64 and w.shape == (P,)
    assert torch.equal(dpd.backbone.Weight.detach().cpu().view(-1), torch.from_numpy(w).to(torch.float32))
    if not steps:
        assert torch.equal(dpd.backbone.Weight.detach(), w_start)
    # a second call from the same start: the same bits
    again, _ = indirect_start(B, T)
    assert torch.equal(again.backbone.Weight.detach(), w_start)
    rerun = refine_gmp_dpd(again, pa, x, gain(), iterations=iterations, ridge=RIDGE).gmp_refine
    assert rerun["losses"] == L and rerun["steps"] == steps and np.array_equal(rerun["w"], w)
    assert torch.equal(again.backbone.Weight.detach(), dpd.backbone.Weight.detach())
    return run


@pytest.mark.parametrize("B,T", [(7, 64), (20, 200)], ids=["7x64", "20x200"])
def test_the_loss_falls_sixfold_through_the_gmp_pa(B, T):
    """Condition: losses[-1] <= losses[0] / 6 after 8 iterations.  The fp64 comparator reaches 23.90277 x and 14.58037 x; measured on an
    MI355X 23.90253 x and 14.58034 x, the same steps, every loss within 1e-5 of the comparator's."""
    L = refine_and_check(B, T, gmp_pa())["losses"]
    ref = COMPARATOR[(B, T)]
    print(f"({B}, {T}): measured ratio {L[0] / L[-1]:.5f}, comparator {ref[0] / ref[-1]:.5f}; per iteration, loss / comparator's - 1: "
          + " ".join(f"{a / b - 1:+.2e}" for a, b in zip(L, ref)))
    assert L[-1] <= L[0] / 6.0, (L[0], L[-1])


@pytest.mark.parametrize("B,T", [(3, 21), (1, 513)], ids=["3x21", "1x513"])
def test_the_invariants_at_the_edges_of_the_look_back_and_the_gram_chunk(B, T):
    refine_and_check(B, T, gmp_pa())


def test_the_invariants_through_a_recurrent_pa():
    """dgru, 8 units, seeded random weights, (20, 200): nothing like gain * identity, so only what holds by construction is asserted;
    the decrease is printed."""
    refine_and_check(20, 200, dgru_pa())


def test_the_invariants_through_a_pa_on_the_aten_route():
    """gru of 80 units is beyond the kernels' envelope: CoreModel runs its ATen restatement, and dL/du comes from autograd"""
    import warnings
    from opendpd_amd import CoreModel
    torch.manual_seed(2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (the restatement announces itself)
        pa = CoreModel(2, 80, 1, "gru").cuda()
    assert not pa.backbone.native
    refine_and_check(3, 21, pa, iterations=2)


def _stacked_and_alone(B, T, pa):
    from opendpd_amd.fit import candidate_losses
    dpd, x = indirect_start(B, T)
    target = gain() * x
    w = dpd.backbone.Weight.detach().double().view(-1)
    g = torch.Generator().manual_seed(B * 1000 + T)
    d = (0.05 * float(w.abs().max()) * torch.randn(P, generator=g, dtype=torch.float64)).cuda()
    W = w[None, :] + (0.5 ** torch.arange(7, dtype=torch.float64, device="cuda"))[:, None] * d[None, :]
    stacked = candidate_losses(dpd, pa, x, target, W)
    alone = torch.cat([candidate_losses(dpd, pa, x, target, W[k:k + 1]) for k in range(7)])
    assert tuple(stacked.shape) == (7,) and stacked.dtype == torch.float32 and len(set(stacked.tolist())) == 7
    return stacked, alone


@pytest.mark.parametrize("B,T", [(7, 64), (20, 200)], ids=["7x64", "20x200"])
def test_the_stacked_line_search_equals_the_candidates_alone_bit_for_bit_through_the_gmp_pa(B, T):
    stacked, alone = _stacked_and_alone(B, T, gmp_pa())
    assert torch.equal(stacked, alone), (stacked.tolist(), alone.tolist())


@pytest.mark.parametrize("B,T", [(20, 200), (80, 25)], ids=["20x200-eval-eval", "80x25-eval-rotated"])
def test_the_stacked_line_search_equals_the_candidates_alone_through_the_dgru_pa(B, T):
    """within 1e-6 relative; (80, 25): the stacked forward of 560 sequences runs another kernel than the 80 alone (module docstring)"""
    stacked, alone = _stacked_and_alone(B, T, dgru_pa())
    rel = ((stacked.double() - alone.double()).abs() / alone.double()).max().item()
    print(f"dgru PA ({B}, {T}): stacked against alone, largest relative difference {rel:.3g}")
    assert rel <= 1e-6, rel


def test_fit_dpd_direct_writes_what_run_dpd_loads(workdir):  # noqa: F811
    import opendpd_amd as od
    from opendpd_amd import data as D
    kw = dict(dataset_name="DPA_200MHz", PA_backbone="gmp", PA_hidden_size=11, frame_length=50, accelerator="cuda")
    od.fit_pa(dataset_name="DPA_200MHz", frame_length=50)
    r = od.fit_dpd_direct(iterations=3, **kw)
    dpd_id = "DPD_S_0_M_GMP_H_11_F_50_P_495"
    sub = os.path.join("DPA_200MHz", "train_dpd", "PA_S_0_M_GMP_H_11_F_50")
    assert r["status"] == "completed" and os.path.normpath(r["model_path"]) == os.path.join("save", sub, dpd_id + ".pt")
    assert os.path.normpath(r["log_path"]) == os.path.join("log", sub, "best", dpd_id + ".csv")
    hist = pd.read_csv(os.path.join("log", sub, "history", dpd_id + ".csv"))
    print(hist[["EPOCH", "TRAIN_LOSS", "VAL_NMSE", "VAL_ACLR_AVG", "TEST_LOSS", "TEST_NMSE", "TEST_ACLR_AVG"]].to_string())
    assert 2 <= len(hist) <= 4 and list(hist["EPOCH"]) == list(range(len(hist)))      # row 0 = the start, then one per accepted step
    assert all(b <= a for a, b in zip(hist["TRAIN_LOSS"], hist["TRAIN_LOSS"][1:]))
    assert set(hist["N_PARAM"]) == {495} and set(hist["BACKBONE"]) == {"gmp"} and set(hist["N_EPOCH"]) == {4}
    best = pd.read_csv(r["log_path"])
    assert len(best) == 1 and best["VAL_ACLR_AVG"].iloc[0] == hist["VAL_ACLR_AVG"].min()
    sd = torch.load(r["model_path"], map_location="cpu")
    assert list(sd) == ["backbone.Weight"] and sd["backbone.Weight"].dtype == torch.float32 and tuple(sd["backbone.Weight"].shape) == (1, P)
    # run_dpd loads it
    d = dataset()
    out = od.run_dpd(DPD_backbone="gmp", DPD_hidden_size=11, **kw)
    csv = pd.read_csv(out["output_path"])
    assert list(csv.columns) == ["I", "Q", "I_dpd", "Q_dpd"] and len(csv) == len(d["test_input"]) and np.all(np.isfinite(csv.to_numpy()))
    # the saved model through the saved PA on the test split, against gain * x: below the indirect start's own row 0
    dpd, pa = od.CoreModel(2, 11, 1, "gmp"), od.CoreModel(2, 11, 1, "gmp")
    dpd.load_state_dict(sd)
    pa.load_state_dict(torch.load(os.path.join("save", "DPA_200MHz", "train_pa", "PA_S_0_M_GMP_H_11_F_50_P_495.pt"), map_location="cpu"))
    seg = D.segments(d["test_input"], D.load_spec("DPA_200MHz", None)["nperseg"]).cuda()
    with torch.no_grad():
        mse = float(torch.mean((pa.cuda()(dpd.cuda()(seg)) - gain() * seg) ** 2))
    print(f"test split: cascade MSE {mse:.6e} after direct learning, {hist['TEST_LOSS'].iloc[0]:.6e} at the indirect start")
    assert mse < hist["TEST_LOSS"].iloc[0]
    # the other starts: the identity, and a saved model (here the one just written)
    saved = hist["TRAIN_LOSS"].iloc[int(hist["VAL_ACLR_AVG"].idxmin())]      # the row whose model the file holds
    r2 = od.fit_dpd_direct(iterations=1, start=r["model_path"], **kw)
    h2 = pd.read_csv(os.path.join("log", sub, "history", dpd_id + ".csv"))
    assert r2["model_path"] == r["model_path"] and abs(h2["TRAIN_LOSS"].iloc[0] - saved) <= 1e-8 + 1e-5 * saved, (h2["TRAIN_LOSS"].iloc[0], saved)      # (the log keeps 8 decimals)
    od.fit_dpd_direct(iterations=1, start="identity", **kw)
    h3 = pd.read_csv(os.path.join("log", sub, "history", dpd_id + ".csv"))
    assert h3["TRAIN_LOSS"].iloc[0] > 10 * hist["TRAIN_LOSS"].iloc[0]      # DPD(x) = x leaves the PA's whole distortion
