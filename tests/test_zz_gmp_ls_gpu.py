"""The closed-form fit of gmp on the device: odpd_gmp_gram (csrc/gmp_ls.hip: fp64 basis formed in the kernel, v_mfma_f64_16x16x4_f64) against the
numpy fp64 comparator of tests/test_gmp_ls_cpu.py, the fitted model through the kernels that already exist, and fit_pa / fit_dpd at the API.

Measured on an MI355X (largest ratio of an entry's error to its bound, per shape): see docs/design/gmp_ls.md.
(The file name sorts behind the older suites: in a collected run their tests keep the positions they had.)"""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests.golden_util import GOLDEN, rel_err
from tests.test_gmp_ls_cpu import P, basis, dataset, gram, reference_solution, train_design

pytestmark = pytest.mark.gpu

TC = 512                 # csrc/gmp_ls.hip kTC: samples of a staged chunk
RIDGE = 1e-6
SHAPES = [(1, 1), (1, 2), (1, 10), (1, 11), (1, 12), (1, 20), (1, 21), (1, 22), (3, 37), (5, 200), (2, 513), (1, 1031), (64, 50),
          (1, TC - 1), (1, TC), (1, TC + 1), (1, TC + 21)]


def _signal(B, T):
    rng = np.random.RandomState(B * 7 + T)
    amp, ph = 0.05 + 0.85 * rng.rand(B, T, 1), 2 * np.pi * rng.rand(B, T, 1)
    x = np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)
    return x, (0.5 * rng.randn(B, T, 2)).astype(np.float32)


def _bound(G_ref, rows):
    d = np.sqrt(np.diag(G_ref))
    return (rows + 64) * 2.0 ** -53 * np.outer(d, d)


def _worst_ratio(G, G_ref, rows):
    """largest |G - G_ref| / bound over the entries; an entry whose bound is 0 (a column of zeros: history terms of a short sequence) must be 0"""
    err, bound = np.abs(G - G_ref), _bound(G_ref, rows)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0]))


def _check_gram(x, t, G_ref):
    from opendpd_amd import gmp_gram
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    g1 = gmp_gram(xd, td)
    g2 = gmp_gram(xd, td)
    assert g1.dtype == torch.float64 and tuple(g1.shape) == (P + 1, P + 1) and g1.is_cuda
    assert torch.equal(g1, g2)                       # two calls, the same bits
    G = g1.cpu().numpy()
    assert np.all(np.isfinite(G)) and np.array_equal(G, G.T)      # symmetric bit for bit
    ratio = _worst_ratio(G, G_ref, 2 * x.shape[0] * x.shape[1])
    print(f"gram ({x.shape[0]}, {x.shape[1]}): worst error / bound = {ratio:.3g}")
    assert ratio <= 1.0, ratio
    return G


@pytest.mark.parametrize("B,T", SHAPES, ids=[f"{b}x{t}" for b, t in SHAPES])
def test_gram_equals_the_comparator(B, T):
    x, t = _signal(B, T)
    _check_gram(x, t, gram(x, t))


def test_gram_of_the_training_stream():
    d = dataset()
    _check_gram(d["train_input"][None], d["train_output"][None], train_design()[1])


def test_history_restarts_at_each_sequence():
    from opendpd_amd import gmp_gram
    x, t = _signal(3, 37)
    whole = gmp_gram(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()).cpu().numpy()
    parts = sum(gmp_gram(torch.from_numpy(x[b:b + 1]).cuda(), torch.from_numpy(t[b:b + 1]).cuda()).cpu().numpy() for b in range(3))
    assert _worst_ratio(whole, parts, 2 * 3 * 37) <= 1.0
    assert _worst_ratio(parts, gram(x, t), 2 * 3 * 37) <= 1.0


@pytest.fixture(scope="module")
def fitted():
    """fit_gmp on the dataset's training stream, the comparator's solution, and the stream on the device"""
    from opendpd_amd import fit_gmp
    d = dataset()
    x, y = torch.from_numpy(d["train_input"][None]).cuda(), torch.from_numpy(d["train_output"][None]).cuda()
    net = fit_gmp(x, y, ridge=RIDGE)
    w_ref, e_max = reference_solution(train_design()[1], RIDGE)
    return net, w_ref, e_max, x, y


def test_fit_equals_the_comparators_solution(fitted):
    net, w_ref, e_max, x, _ = fitted
    w = net.backbone.Weight.detach().cpu().numpy().reshape(-1)
    assert net.backbone.Weight.dtype == torch.float32 and net.backbone_type == "gmp" and net.backbone.native
    err = float(np.max(np.abs(w - w_ref)) / np.max(np.abs(w_ref)))
    print(f"fit: max|w| {np.max(np.abs(w_ref)):.4f}, weight error / max|w| = {err:.3g}")
    assert err < 1e-4
    assert abs(net.gmp_fit["e_max"] - e_max) < 1e-9 * e_max
    with torch.no_grad():
        out = net(x)[0].cpu().numpy()
    pred = train_design()[0][:, :P] @ w_ref
    ref = np.stack([pred[:len(out)], pred[len(out):]], -1)
    print(f"fit: forward through gmp_fwd_kernel vs comparator: {rel_err(out, ref):.3g}")
    assert rel_err(out, ref) < 2e-5


def test_the_fit_minimises_the_regularised_loss_as_the_existing_forward_sees_it(fitted):
    net, _, e_max, x, y = fitted
    w_fit = net.backbone.Weight.detach().clone()

    def J(w):
        with torch.no_grad():
            net.backbone.Weight.copy_(w.view(1, P))
            e = (net(x) - y).double()
            return float((e * e).sum()) + RIDGE * e_max * float((w.double() ** 2).sum())

    try:
        j_fit = J(w_fit)
        w_trained = torch.from_numpy(np.load(os.path.join(GOLDEN, "ref_runs_gmp_model.npz"))["backbone.Weight"]).cuda().view(1, P)
        j_trained = J(w_trained)
        print(f"J(fit) = {j_fit:.6f}, J(reference's trained weights) = {j_trained:.6f}")
        assert j_fit <= j_trained + 1e-5 * j_fit
        g = torch.Generator().manual_seed(0)
        for k in range(5):
            delta = torch.randn(1, P, generator=g).cuda()
            delta *= 1e-2 * w_fit.norm() / delta.norm()
            j = J(w_fit + delta)
            print(f"J(fit + delta_{k}) - J(fit) = {j - j_fit:.6g}")
            assert j_fit <= j + 1e-5 * j_fit
    finally:
        with torch.no_grad():
            net.backbone.Weight.copy_(w_fit)


@pytest.fixture()
def workdir(tmp_path):
    d = dict(np.load(os.path.join(GOLDEN, "dpa200_dataset.npz")))
    ds = tmp_path / "datasets" / "DPA_200MHz"
    ds.mkdir(parents=True)
    (ds / "spec.json").write_text(str(d.pop("spec")))
    for k, v in d.items():
        pd.DataFrame(v, columns=["I", "Q"]).to_csv(ds / f"{k}.csv", index=False)
    old = os.getcwd()
    os.chdir(tmp_path)
    os.environ["OPENDPD_DATASETS"] = str(tmp_path / "datasets")
    yield tmp_path
    os.chdir(old)


def test_fit_pa_and_fit_dpd_write_what_the_training_steps_load(workdir):
    import json
    import opendpd_amd as od
    from opendpd_amd import data as D, metrics
    # ---- fit_pa: the files of train_pa --PA_backbone gmp
    r = od.fit_pa(dataset_name="DPA_200MHz", frame_length=50)
    pa_id = "PA_S_0_M_GMP_H_11_F_50_P_495"
    assert r["status"] == "completed"
    assert os.path.normpath(r["model_path"]) == os.path.join("save", "DPA_200MHz", "train_pa", pa_id + ".pt")
    assert os.path.normpath(r["log_path"]) == os.path.join("log", "DPA_200MHz", "train_pa", "best", pa_id + ".csv")
    hist = pd.read_csv(os.path.join("log", "DPA_200MHz", "train_pa", "history", pa_id + ".csv"))
    best = pd.read_csv(r["log_path"])
    ref_cols = list(json.load(open(os.path.join(GOLDEN, "ref_runs_gmp.json")))["train_pa_hist"])
    assert list(hist.columns) == ref_cols == list(best.columns) and len(hist) == len(best) == 1
    row = hist.iloc[0]
    assert (row["EPOCH"], row["N_EPOCH"], row["N_PARAM"], row["BACKBONE"], row["HIDDEN_SIZE"], row["FRAME_LENGTH"]) == (0, 1, 495, "gmp", 11, 50)
    # the logged numbers against the comparator's own solution on the same segments
    d = dataset()
    A, G = train_design()
    w_ref, _ = reference_solution(G, RIDGE)
    mse = float(np.mean((A[:, :P] @ w_ref - A[:, P]) ** 2))
    assert abs(row["TRAIN_LOSS"] - mse) < 1e-4 * mse, (row["TRAIN_LOSS"], mse)
    nperseg = D.load_spec("DPA_200MHz", None)["nperseg"]
    seg_x, seg_y = D.segments(d["val_input"], nperseg).numpy(), D.segments(d["val_output"], nperseg).numpy()
    pred = np.stack([basis(s) @ w_ref for s in seg_x])
    nmse_ref = metrics.NMSE(np.stack([pred.real, pred.imag], -1), seg_y)
    print(f"fit_pa: VAL_NMSE {row['VAL_NMSE']:.4f} dB (comparator {nmse_ref:.4f} dB; the reference after two AdamW epochs -18.0770 dB), "
          f"TEST_NMSE {row['TEST_NMSE']:.4f} dB, TRAIN_LOSS {row['TRAIN_LOSS']:.8f}")
    assert row["VAL_NMSE"] < -18.08
    assert abs(row["VAL_NMSE"] - nmse_ref) < 0.1
    sd = torch.load(r["model_path"], map_location="cpu")
    assert list(sd) == ["backbone.Weight"] and sd["backbone.Weight"].dtype == torch.float32
    assert float(np.max(np.abs(sd["backbone.Weight"].numpy().reshape(-1) - w_ref))) < 1e-4 * np.max(np.abs(w_ref))
    # ---- train_dpd finds and loads the fitted PA with no further step
    kw = dict(dataset_name="DPA_200MHz", PA_backbone="gmp", PA_hidden_size=11, frame_length=50, accelerator="cuda")
    t = od.train_dpd(DPD_backbone="dgru", DPD_hidden_size=8, n_epochs=1, batch_size=64, **kw)
    loss = pd.read_csv(t["log_path"])["TRAIN_LOSS"].iloc[0]
    assert np.isfinite(loss), loss
    # ---- fit_dpd: the post-inverse of the measured PA, where train_dpd --DPD_backbone gmp saves its model
    f = od.fit_dpd(**kw)
    dpd_id = "DPD_S_0_M_GMP_H_11_F_50_P_495"
    assert os.path.normpath(f["model_path"]) == os.path.join("save", "DPA_200MHz", "train_dpd", "PA_S_0_M_GMP_H_11_F_50", dpd_id + ".pt")
    assert len(pd.read_csv(f["log_path"])) == 1
    raw = np.load(os.path.join(GOLDEN, "dpa200_dataset.npz"))
    gain = D.set_target_gain(raw["train_input"], raw["train_output"])
    u = (raw["train_output"] / gain).astype(np.float32)
    w_inv, _ = reference_solution(gram(u[None], d["train_input"][None]), RIDGE)
    w = torch.load(f["model_path"], map_location="cpu")["backbone.Weight"].numpy().reshape(-1)
    err = float(np.max(np.abs(w - w_inv)) / np.max(np.abs(w_inv)))
    print(f"fit_dpd: max|w| {np.max(np.abs(w_inv)):.4f}, weight error / max|w| = {err:.3g}")
    assert err < 1e-4
    # ---- run_dpd loads it
    out = od.run_dpd(DPD_backbone="gmp", DPD_hidden_size=11, **kw)
    csv = pd.read_csv(out["output_path"])
    assert list(csv.columns) == ["I", "Q", "I_dpd", "Q_dpd"] and len(csv) == len(d["test_input"]) and np.all(np.isfinite(csv.to_numpy()))
