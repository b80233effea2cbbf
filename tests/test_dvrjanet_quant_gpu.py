"""`--quant` on dvrjanet on the HIP kernels (csrc/dvrjanet_q.hip: nine INT_Linear inside the cell, selected by ODPD_FLAG_QUANT_CELL) against

* the two fixtures the REFERENCE produced (quant_dvrjanet_h12_w8a8, quant_dvrjanet_h10_w16a16, both with three DVR units): state dict and RNG
  after the surgery, train / eval outputs, gradients, three clip + AdamW steps, four 200-sample frames in eval mode;
* the ATen route (`opendpd_amd.quant._quantise_aten` on a CPU copy of the same state dict, float32 — itself pinned to the same fixtures by
  tests/test_quant_partial_cpu.py) on ragged shapes, with weights beyond their grids and activation ranges narrowed.

The quantised layers sit INSIDE the recurrence and sin / cos / sigmoid / tanh are float: where the kernel's value (1e-7 from torch's) lies that
close to a rounding boundary of one of a step's roundings, the state rounds the other way and THAT sequence follows another trajectory from there
on (the ATen route in float32 against itself in float64 does the same).  Hence `grid_close` on the 8-bit fixture and, on the ragged shapes: a
required share of sequences that agree over their whole length ('clean'), gradients compared on those, boundedness for the others.  The required
shares are conditions, not measurements — the comparator alone (ATen float32 against ATen float64) measured 1.000 on seven of the 8-bit cases,
0.984 at (6, 4, 64, 50), 0.999 at (16, 4, 700, 20), 0.997 at (8, 2, 1000, 16), 0.969 at (10, 3, 256, 200).  On 16-bit grids no share is required
(the comparator alone: 0.56 / 0.44 / 0.02), only a bound on the largest deviation: 4 x the comparator's own, which the test computes.

Measured on the MI355X (printed by the tests, recorded in docs/design/quantised.md): W8A8 fixture outputs equal in every sample; W16A16 113 of
370 and 1 247 of 1 600 samples beyond 2e-6, largest deviation 1.40e-4 / 2.07e-4; ragged 8-bit shares 1.000 (largest deviation 0) except 0.999 at
(16, 4, 700, 20) and 0.977 at (10, 3, 256, 200); 16-bit shares 0.562 / 0.594 / 0.281 with largest deviation 3.04e-4 / 3.97e-4 / 5.64e-4 against the
comparator's own 3.53e-4 / 3.97e-4 / 6.87e-4; gradients on the agreeing sequences within 8.1e-6 everywhere."""
import warnings

import numpy as np
import pytest
import torch

from tests.golden_util import Fixture, rel_err
from tests.test_oracle_golden import grid_close

pytestmark = pytest.mark.gpu

FIXTURES = [("quant_dvrjanet_h12_w8a8", 8), ("quant_dvrjanet_h10_w16a16", 16)]
ATEN_NOTE = "ATen restatement of the quantised model"
# W16A16: no cap on the number of moved samples (the comparator alone — the same model in float64 against the fixture — moves 83 of 370 and
# 1 187 of 1 600), a bound on the largest deviation only: 4 x the comparator's 8.43e-5 (y, y_eval) and 1.72e-4 (ya_eval), because the kernel's
# transcendental functions differ from torch's in more places than float64 differs from float32
Y16_BOUND, YA16_BOUND = 4 * 8.43e-5, 4 * 1.72e-4


class _Proj:
    quant = True
    pretrained_model = ""


def _surgery(fx, bits):
    """tests/test_quant_partial_cpu.py::_surgery from a model on the HIP device: no ATen warning, a kernel-backed module"""
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import QuantDVRJANET, get_quant_model
    net = CoreModel(2, fx.meta["hidden"], 1, "dvrjanet", num_dvr_units=fx.meta["num_dvr_units"])
    net.load_state_dict({k: torch.from_numpy(fx["fsd/" + k]) for k in fx.keys("fsd")})
    net = net.cuda()
    _Proj.n_bits_w = _Proj.n_bits_a = bits
    torch.manual_seed(123)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        q = get_quant_model(_Proj, net)
    assert not any(ATEN_NOTE in str(x.message) for x in w)
    assert q is not net and q.backbone.native and isinstance(q.backbone, QuantDVRJANET)
    return q


def _aten_twin(q, bits, device="cpu"):
    """the ATen route holding the same state dict (float32)"""
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import _quantise_aten
    rng = torch.get_rng_state()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = CoreModel(2, q.hidden_size, 1, "dvrjanet", num_dvr_units=q.num_dvr_units)
        if device != "cpu":
            net = net.cuda()
        a = _quantise_aten(net, bits, bits, "", torch.device(device))
    torch.set_rng_state(rng)
    a.load_state_dict({k: v.detach().cpu() for k, v in q.state_dict().items()})
    assert not a.backbone.native
    return a


@pytest.mark.parametrize("name,bits", FIXTURES)
def test_surgery_on_the_device_state_dict_rng_and_routing(name, bits):
    fx = Fixture(name)
    q = _surgery(fx, bits)
    rng_after = torch.rand(4).numpy()
    sd = q.state_dict()
    assert list(sd.keys()) == fx.keys("sd")
    for k in fx.keys("sd"):
        assert sd[k].is_cuda and np.array_equal(sd[k].cpu().numpy(), fx["sd/" + k]), k
    assert np.array_equal(rng_after, fx["rng_after"])
    assert sum(p.numel() for p in q.parameters()) == fx.meta["n_param"]
    import types
    from opendpd_amd.project import Project
    from opendpd_amd.train_funcs import FusedAdamW
    ns = types.SimpleNamespace(opt_type="adamw", lr=fx.meta["lr"], decay_factor=0.5, patience=10, lr_end=1e-6, world=1)
    opt, _ = Project.build_optimizer(ns, q)                # the fused HIP optimiser, not the torch one of the ATen route
    assert isinstance(opt, FusedAdamW)
    with pytest.raises(NotImplementedError):      # h_0 stays refused for quantised models
        q(torch.from_numpy(fx["x"]).cuda(), torch.ones(1, fx["x"].shape[0], fx.meta["hidden"], device="cuda"))


@pytest.mark.parametrize("name,bits", FIXTURES)
def test_forward_matches_the_reference(name, bits):
    """measured on the MI355X — W8A8: 0 of 370 (y, y_eval) and 0 of 1 600 (ya_eval) samples beyond 2e-6; W16A16: see docs/design/quantised.md"""
    fx = Fixture(name)
    q = _surgery(fx, bits)
    step = 2.0 ** (2 - bits) * 4
    x = torch.from_numpy(fx["x"]).cuda()
    q.train()
    with torch.no_grad():
        yt = q(x).cpu().numpy()
    q.eval()
    with torch.no_grad():
        ye = q(x).cpu().numpy()
        ya = q(torch.from_numpy(fx["xa"]).cuda()).cpu().numpy()
    assert np.array_equal(yt, ye)                      # no module is named fc_out: no output quantiser in either mode
    for got, ref in ((yt, "y"), (ye, "y_eval"), (ya, "ya_eval")):
        d = np.abs(got - fx[ref])
        print(f"[dvrjanet q {name}] {ref}: {int((d > 2e-6).sum())} of {d.size} samples beyond 2e-6, largest deviation {d.max():.2e}")
    if bits == 8:
        assert grid_close(yt, fx["y"], step, 2)
        assert grid_close(ye, fx["y_eval"], step, 2)
        assert grid_close(ya, fx["ya_eval"], step, 2)
    else:
        assert np.isfinite(yt).all() and np.abs(yt - fx["y"]).max() <= Y16_BOUND
        assert np.isfinite(ye).all() and np.abs(ye - fx["y_eval"]).max() <= Y16_BOUND
        assert np.isfinite(ya).all() and np.abs(ya - fx["ya_eval"]).max() <= YA16_BOUND


@pytest.mark.parametrize("name,bits", FIXTURES)
def test_gradients_match_the_reference(name, bits):
    fx = Fixture(name)
    q = _surgery(fx, bits)
    q.train()
    xg = torch.from_numpy(fx["x"]).cuda().requires_grad_(True)
    t = torch.from_numpy(fx["tgt"]).cuda()
    loss = torch.nn.functional.mse_loss(q(xg), t)
    loss.backward()
    ref = float(fx["losses"][0])
    print(f"[dvrjanet q {name}] loss {loss.item():.8f} (reference {ref:.8f}), dL/dx rel {rel_err(xg.grad.cpu().numpy(), fx['gx']):.2e}")
    assert abs(loss.item() - ref) < 1e-5 * max(1.0, ref)
    assert rel_err(xg.grad.cpu().numpy(), fx["gx"]) < 2e-3
    worst = 0.0
    for k, p in q.named_parameters():
        if ("g/" + k) in fx:
            g = fx["g/" + k]
            assert p.grad is not None, k
            if np.abs(g).max() == 0:
                assert float(p.grad.abs().max()) == 0.0, k         # the 18 weight / activation scales: the round of the exponent kills them
            else:
                worst = max(worst, rel_err(p.grad.cpu().numpy(), g))
                assert rel_err(p.grad.cpu().numpy(), g) < 2e-3, k
        else:
            assert "out_quantizer" in k and p.grad is None, k     # outside the graph
    print(f"[dvrjanet q {name}] worst weight-gradient rel {worst:.2e}")


@pytest.mark.parametrize("name,bits", FIXTURES)
def test_three_fused_train_steps_follow_the_reference(name, bits):
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    fx = Fixture(name)
    q = _surgery(fx, bits)
    q.train()
    x, t = torch.from_numpy(fx["x"]).cuda(), torch.from_numpy(fx["tgt"]).cuda()
    opt = FusedAdamW(q, lr=fx.meta["lr"])
    assert not opt.has_fused(x.shape[0], x.shape[1])      # forward, loss, backward chained: there is no one-launch step for this model
    before = {k: p.detach().clone() for k, p in q.named_parameters()}
    for s in range(1, 4):
        l = fused_train_step(opt, x, t, "l2", fx.meta["clip"])
        ref = float(fx["losses"][s - 1])
        assert abs(l.item() - ref) < 2e-4 * max(1.0, ref), s
        worst = 0.0
        for k, p in q.named_parameters():
            worst = max(worst, rel_err(p.detach().cpu().numpy(), fx[f"p{s}/{k}"]))
            assert rel_err(p.detach().cpu().numpy(), fx[f"p{s}/{k}"]) < 1e-3, (s, k)
        print(f"[dvrjanet q {name}] step {s}: loss {l.item():.8f} (reference {ref:.8f}), worst parameter rel {worst:.2e}")
    for k, p in q.named_parameters():
        if "out_quantizer" in k:
            assert torch.equal(p.detach(), before[k]), k                                   # AdamW skips them (grad is None in the reference)
        elif "scale" in k:
            now = float(p.detach())
            assert now < float(before[k]), k                                                # zero gradient, but decayed
            assert abs(now - float(fx["sd3/" + k][0])) <= 1e-6 * float(before[k]), k


SPIKED = ("W_f", "W_ccos", "W_ah")


def _prepared(H, K, bits):
    """a quantised dvrjanet on the device with every kind of mask in play: biases off zero; W_pθ and W_o2 weights partly beyond the weight grid's
    range (max |w| = 2.6); two single entries each of W_f, W_ccos, W_ah beyond it (+2.5 / -2.5: a whole recurrent matrix scaled beyond its grid
    makes dL/dx overflow fp32 within 200 steps in the ATen route itself); the activation ranges of W_ah, W_o1, W_ax narrowed; W_ax's weights
    widened; cs conditioned as the float test conditions it (sum |c| <= 1.5)"""
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import get_quant_model
    _Proj.n_bits_w = _Proj.n_bits_a = bits
    q = get_quant_model(_Proj, CoreModel(2, H, 1, "dvrjanet", num_dvr_units=K).cuda())
    bb = q.backbone
    assert bb.native
    with torch.no_grad():
        g = torch.Generator().manual_seed(H)
        for lay in (bb.W_f, bb.W_ccos, bb.W_csin, bb.W_o1, bb.W_o2):
            lay.bias.copy_(((torch.rand(lay.bias.shape, generator=g) - 0.5) * 0.4).cuda())
        for n in ("W_pθ", "W_o2"):
            lay = getattr(bb, n)
            lay.weight.mul_(2.6 / float(lay.weight.abs().max()))
        for n in SPIKED:
            w = getattr(bb, n).weight
            w[0, 0] = 2.5
            w[-1, -1] = -2.5
        for n in ("W_ah", "W_o1", "W_ax"):
            getattr(bb, n).act_quantizer.scale.mul_(0.25)
        bb.W_ax.weight.mul_(1.5)
        bb.cs.mul_(min(1.0, 1.5 / float(bb.cs.abs().sum())))
    return q


def _aten_forward_backward(a, x, dy):
    xt = torch.from_numpy(x).to(next(a.parameters()).dtype).requires_grad_(True)
    a.zero_grad()
    y = a(xt)
    y.backward(torch.from_numpy(dy).to(y.dtype))
    return y.detach().numpy(), xt.grad.numpy()


CASES = [(3, 8, 3, 1, 8), (5, 2, 2, 65, 8), (16, 8, 5, 200, 8), (12, 3, 40, 16, 8), (1, 1, 8, 17, 8), (16, 8, 24, 16, 8), (13, 5, 3, 130, 8),
         (6, 4, 64, 50, 8), (16, 4, 700, 20, 8), (8, 2, 1000, 16, 8), (10, 3, 256, 200, 8), (9, 3, 16, 20, 16), (7, 4, 32, 40, 16), (16, 8, 64, 64, 16)]


@pytest.mark.parametrize("H,K,B,T,bits", CASES)
def test_matches_the_aten_route_on_ragged_sizes(H, K, B, T, bits):
    """(8, 2, 1000, 16, 8 bits): more sequences than the backward launch has workgroups, so every workgroup runs several and carries its weight
    gradients from one to the next"""
    import copy
    torch.manual_seed(H + B + T)
    q = _prepared(H, K, bits)
    a = _aten_twin(q, bits)
    g = torch.Generator().manual_seed(B + T)
    x = (0.3 * torch.randn(B, T, 2, generator=g) + 0.1).numpy()
    dy = torch.randn(B, T, 2, generator=g).numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yo, dxo_all = _aten_forward_backward(a, x, dy)
    assert np.isfinite(dxo_all).all()
    # at least one sample of the case is clamped by W_pθ's activation grid ([-2, 2 - step] against theta in [-pi, pi])
    th = np.arctan2(x[..., 1], x[..., 0])
    s_a = 2.0 ** (2 - bits)
    assert ((th < -2.0 ** (bits - 1) * s_a) | (th > (2.0 ** (bits - 1) - 1) * s_a)).any()
    bb = q.backbone
    # what the read-outs can produce: |y| <= sum |q(w)| + |b| (the states stay in (-1, 1))
    s_w, lo, hi = 2.0 ** (2 - bits), -2.0 ** (bits - 1), 2.0 ** (bits - 1) - 1
    reach = [float((torch.clamp(l.weight.detach() / s_w, lo, hi).round() * s_w).abs().sum() + l.bias.detach().abs().sum()) for l in (bb.W_o1, bb.W_o2)]
    ys = []
    for mode in (q.eval, q.train):
        mode()
        with torch.no_grad():
            y = q(torch.from_numpy(x).cuda()).cpu().numpy()
        ys.append(y)
        assert np.isfinite(y).all() and np.abs(y[..., 0]).max() <= reach[0] and np.abs(y[..., 1]).max() <= reach[1]
    assert np.array_equal(ys[0], ys[1])
    d = np.abs(ys[1] - yo).reshape(B, -1).max(1)
    clean = d <= 4e-6
    print(f"[dvrjanet q H{H} K{K} B{B} T{T} W{bits}] sequences on the ATen route's trajectory: {clean.mean():.3f}, largest deviation {d.max():.2e}")
    if bits == 8:
        assert clean.mean() >= (0.8 if T == 200 and B == 256 else 0.9), (clean.mean(), d.max())
    else:      # the comparator alone: the ATen twin in float64 against the ATen twin in float32
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            y64, _ = _aten_forward_backward(copy.deepcopy(a).double(), x, dy)
        own = np.abs(yo - y64).max()
        print(f"[dvrjanet q H{H} K{K} B{B} T{T} W{bits}] comparator alone (float32 against float64): largest deviation {own:.2e}")
        assert d.max() <= 4 * own, (d.max(), own)
    tol = 2e-4 if bits == 8 else 2e-3
    if clean.any():
        dyk = dy * clean[:, None, None]                       # the other sequences contribute nothing to either side
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        q(xt).backward(torch.from_numpy(dyk).cuda())
        dx = xt.grad.cpu().numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, dxo = _aten_forward_backward(a, x, dyk)
        assert np.isfinite(dx).all()
        print(f"[dvrjanet q H{H} K{K} B{B} T{T} W{bits}] dL/dx rel {rel_err(dx[clean], dxo[clean]):.2e}")
        assert rel_err(dx[clean], dxo[clean]) < tol
        assert np.abs(dx[~clean]).max(initial=0.0) == 0.0
        ref = dict(a.named_parameters())
        worst = 0.0
        for k, v in q.named_parameters():
            r = ref[k].grad
            if "out_quantizer" in k:
                assert v.grad is None and r is None, k
            elif "scale" in k:
                assert float(v.grad.abs().max()) == 0.0 and float(r.abs().max()) == 0.0, k
            elif float(r.abs().max()) == 0.0:      # (T = 1: the state is 0, so is every gradient of the matrices that read it)
                assert float(v.grad.abs().max()) == 0.0, k
            else:
                worst = max(worst, rel_err(v.grad.cpu().numpy(), r.numpy()))
                assert rel_err(v.grad.cpu().numpy(), r.numpy()) < tol, k
        print(f"[dvrjanet q H{H} K{K} B{B} T{T} W{bits}] worst weight-gradient rel {worst:.2e}")
        # the spiked weights lie beyond the weight grid: gradient exactly 0; their neighbours inside it: not.  (T = 1: the state every recurrent
        # matrix reads is 0 and so is its whole gradient, in the ATen route too; of W_ccos's other half the last row's is 0 there as well in
        # this case — unit H - 1 leaves W_o1's narrowed activation range in all three samples: the neighbours are then held to the ATen route's
        # zero / non-zero pattern)
        for n in SPIKED:
            gw, gr = getattr(bb, n).weight.grad.cpu().numpy(), ref["backbone." + n + ".weight"].grad.numpy()
            assert gw[0, 0] == 0.0 and gw[-1, -1] == 0.0 and gr[0, 0] == 0.0 and gr[-1, -1] == 0.0, n
            if H > 1:
                assert (gw[0, 1] != 0.0) == (gr[0, 1] != 0.0) and (gw[-1, -2] != 0.0) == (gr[-1, -2] != 0.0), n
                if T > 1:
                    assert gw[0, 1] != 0.0 and gw[-1, -2] != 0.0, n
        # dL/dx alone (the frozen-PA role): the same values
        for v in q.parameters():
            v.requires_grad_(False)
        xt2 = torch.from_numpy(x).cuda().requires_grad_(True)
        q(xt2).backward(torch.from_numpy(dyk).cuda())
        assert np.array_equal(xt2.grad.cpu().numpy(), dx)
    else:
        assert bits == 16


def test_cascade_with_a_frozen_float_pa():
    """a quantised dvrjanet DPD (H 12, K 3, W8A8) in front of a frozen float dgru PA (H 13): one fused_train_step — forward, PA forward + loss +
    dL/du, backward, chained — against the same composition with the ATen-route DPD, on the sequences both DPDs agree on"""
    from opendpd_amd import CascadedModel, CoreModel
    from opendpd_amd.quant import get_quant_model
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    rng = np.random.RandomState(0)
    x = (rng.uniform(0.05, 0.7, (9, 41, 2)) * rng.choice([-1.0, 1.0], (9, 41, 2))).astype(np.float32)
    torch.manual_seed(3)
    _Proj.n_bits_w = _Proj.n_bits_a = 8
    dpd = get_quant_model(_Proj, CoreModel(2, 12, 1, "dvrjanet", num_dvr_units=3).cuda())
    assert dpd.backbone.native
    casc = CascadedModel(dpd_model=dpd, pa_model=CoreModel(2, 13, 1, "dgru"))
    casc.freeze_pa_model()
    casc = casc.cuda()
    a = _aten_twin(casc.dpd_model, 8, "cuda").cuda()
    xt = torch.from_numpy(x).cuda()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d = (casc.dpd_model(xt) - a(xt)).abs().reshape(x.shape[0], -1).max(1).values.cpu().numpy()
    clean = d <= 4e-6
    print(f"[dvrjanet q cascade] sequences on the ATen route's trajectory: {clean.mean():.3f}")
    assert clean.mean() >= 0.9
    xc = xt[torch.from_numpy(clean).cuda()].contiguous()
    pa_before = [p.detach().clone() for p in casc.pa_model.parameters()]
    opt = FusedAdamW(casc, lr=0.0, weight_decay=0.0)
    loss = fused_train_step(opt, xc, xc.clone(), "l2", 0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lo = torch.nn.functional.mse_loss(casc.pa_model(a(xc)), xc)
        lo.backward()
    assert np.isfinite(loss.item()) and abs(loss.item() - lo.item()) < 2e-5 * max(1.0, lo.item())
    got = opt.grad[:-4].cpu().numpy()
    off = 0
    for k, v in a.named_parameters():
        n = v.numel()
        gk = got[off:off + n]
        off += n
        if v.grad is None or float(v.grad.abs().max()) == 0.0:
            assert np.abs(gk).max() == 0.0, k
        else:
            assert rel_err(gk, v.grad.cpu().numpy().reshape(-1)) < 2e-4, k
    # a step with a learning rate: the DPD's parameters move, the frozen PA's do not
    dpd_before = [p.detach().clone() for p in casc.dpd_model.parameters()]
    opt2 = FusedAdamW(casc, lr=1e-3)
    assert np.isfinite(fused_train_step(opt2, xc, xc.clone(), "l2", 200.0).item())
    assert any(not torch.equal(p.detach(), b) for p, b in zip(casc.dpd_model.parameters(), dpd_before))
    assert all(torch.equal(p.detach(), b) for p, b in zip(casc.pa_model.parameters(), pa_before))


def test_a_long_evaluation_sequence_runs_and_its_head_equals_a_short_run():
    torch.manual_seed(11)
    _Proj.n_bits_w = _Proj.n_bits_a = 8
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import get_quant_model
    q = get_quant_model(_Proj, CoreModel(2, 12, 1, "dvrjanet", num_dvr_units=3).cuda())
    q.eval()
    g = torch.Generator().manual_seed(1)
    x = (0.3 * torch.randn(1, 19662, 2, generator=g) + 0.1).cuda()
    with torch.no_grad():
        y = q(x)
        ys = q(x[:, :200].contiguous())
    assert y.shape == (1, 19662, 2) and bool(torch.isfinite(y).all())
    assert torch.equal(y[:, :200], ys)


def test_a_single_step_frame():
    """T = 1: the state every recurrent matrix reads is 0; the output is the read-outs of (1 - f) g from the input columns alone"""
    torch.manual_seed(2)
    _Proj.n_bits_w = _Proj.n_bits_a = 8
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import get_quant_model
    q = get_quant_model(_Proj, CoreModel(2, 7, 1, "dvrjanet", num_dvr_units=4).cuda())
    a = _aten_twin(q, 8)
    x = (0.3 * torch.randn(6, 1, 2) + 0.1)
    xt = x.cuda().requires_grad_(True)
    y = q(xt)
    y.sum().backward()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xo = x.clone().requires_grad_(True)
        yo = a(xo)
        yo.sum().backward()
    assert y.shape == (6, 1, 2) and np.abs(y.detach().cpu().numpy() - yo.detach().numpy()).max() <= 4e-6
    assert rel_err(xt.grad.cpu().numpy(), xo.grad.numpy()) < 2e-4


def test_train_dpd_with_quant_runs_on_the_kernels_and_saves_the_references_keys(tmp_path):
    """train_pa (float dgru), then `train_dpd --quant --DPD_backbone dvrjanet` through the Project flow: the DPD is quantised while it is still on
    the CPU and must come out on the kernel route of the project's device (no ATen announcement: warnings are errors), one epoch completes, the
    saved state dict has the reference's keys (the fixture's, in its order)"""
    import os
    import pandas as pd
    import opendpd_amd as od
    from opendpd_amd.project import Project, run_train_dpd
    from opendpd_amd.quant import QuantDVRJANET
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    d = dict(np.load(os.path.join(golden, "dpa200_dataset.npz")))
    ds = tmp_path / "datasets" / "DPA_200MHz"
    ds.mkdir(parents=True)
    (ds / "spec.json").write_text(str(d.pop("spec")))
    for k, v in d.items():
        pd.DataFrame(v, columns=["I", "Q"]).to_csv(ds / f"{k}.csv", index=False)
    old, old_ds = os.getcwd(), os.environ.get("OPENDPD_DATASETS")
    os.chdir(tmp_path)
    os.environ["OPENDPD_DATASETS"] = str(tmp_path / "datasets")
    try:
        kw = dict(dataset_name="DPA_200MHz", PA_backbone="dgru", PA_hidden_size=8, frame_length=50, batch_size=64, lr=2e-3, seed=0, accelerator="cuda")
        with warnings.catch_warnings():
            warnings.simplefilter("error", UserWarning)
            assert od.train_pa(n_epochs=1, **kw)["status"] == "completed"
            proj = Project(step="train_dpd", DPD_backbone="dvrjanet", DPD_hidden_size=12, num_dvr_units=3, quant=True, n_bits_w=8, n_bits_a=8,
                           quant_dir_label="w8a8", n_epochs=1, **kw)
            net = run_train_dpd(proj)
        bb = net.dpd_model.backbone
        assert isinstance(bb, QuantDVRJANET) and bb.native and next(bb.parameters()).is_cuda
        hist = pd.read_csv(proj.path_log_file_hist)
        assert len(hist) == 1 and np.isfinite(hist["TRAIN_LOSS"]).all()
        saved = torch.load(proj.path_save_file_best, map_location="cpu")
        assert list(saved.keys()) == Fixture("quant_dvrjanet_h12_w8a8").keys("sd")
        assert all(bool(torch.isfinite(v).all()) for v in saved.values())
    finally:
        os.chdir(old)
        if old_ds is not None:
            os.environ["OPENDPD_DATASETS"] = old_ds
        else:
            os.environ.pop("OPENDPD_DATASETS", None)
