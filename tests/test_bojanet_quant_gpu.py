"""`--quant` on bojanet on the HIP kernels (csrc/bojanet_q.hip: eight INT_Linear inside the cell, selected by ODPD_FLAG_QUANT_CELL) against

* the two fixtures the REFERENCE produced (oracle/gen_golden_quant_more.py: quant_bojanet_h12_w8a8, quant_bojanet_h16_w16a16): state dict and RNG
  after the surgery, train / eval outputs, gradients, three clip + AdamW steps, four 200-sample frames in eval mode;
* the ATen route (`opendpd_amd.quant._quantise_aten` on a CPU copy of the same state dict, float32 — itself pinned to the same fixtures by
  tests/test_quant_partial_cpu.py) on ragged shapes, with weights beyond their grids and activation ranges narrowed.

The quantised layers sit INSIDE the recurrence and the gates are float sigmoid / tanh: where the kernel's value (1e-7 from torch's) lies that
close to a rounding boundary of one of a step's roundings, the state rounds the other way and THAT sequence follows another trajectory from there
on (the ATen route in float32 against itself in float64 does the same).  Hence `grid_close` on the fixtures and, on the ragged shapes: a required
share of sequences that agree over their whole length ('clean'), gradients compared on those, boundedness for the others.  The required shares
are conditions, not measurements — the comparator alone (ATen float32 against ATen float64) measured 1.000 on the 8-bit cases up to T = 130,
0.980 at 256 x 200, 0.69 .. 0.875 at (9, 16, 20, 16 bits) and 0.34 at (7, 32, 40, 16 bits).

With inputs on a grid a filter output of exactly 0 + 0j is no measure-zero event; the reference's gradient is NaN there (0 * inf through sqrt),
the kernels drop the term (as csrc/bojanet_s16.hip does).  A sequence whose comparator dL/dx is not finite is 'singular' and left out of the
gradient comparison on both sides."""
import warnings

import numpy as np
import pytest
import torch

from tests.golden_util import Fixture, rel_err
from tests.test_oracle_golden import grid_close

pytestmark = pytest.mark.gpu

FIXTURES = [("quant_bojanet_h12_w8a8", 8), ("quant_bojanet_h16_w16a16", 16)]
ATEN_NOTE = "ATen restatement of the quantised model"
# W16A16 on 200-step frames: no cap on the number of moved samples (a flipped state travels on), a bound on the largest deviation only — 4 x what
# the comparator alone shows (the same model in float64 against the fixture: 1.6e-4), because the kernel's sigmoid / tanh differ from torch's in
# more places than float64 differs from float32.  Measured on the MI355X: largest deviation 7.9e-6, 2 of 1 600 samples beyond 2e-6
# (docs/design/quantised.md).
YA16_BOUND = 4 * 1.6e-4


class _Proj:
    quant = True
    pretrained_model = ""


def _surgery(fx, bits):
    """tests/test_quant_partial_cpu.py::_surgery from a model on the HIP device: no ATen warning, a kernel-backed module"""
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import QuantBOJANET, get_quant_model
    net = CoreModel(2, fx.meta["hidden"], 1, "bojanet")
    net.load_state_dict({k: torch.from_numpy(fx["fsd/" + k]) for k in fx.keys("fsd")})
    net = net.cuda()
    _Proj.n_bits_w = _Proj.n_bits_a = bits
    torch.manual_seed(123)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        q = get_quant_model(_Proj, net)
    assert not any(ATEN_NOTE in str(x.message) for x in w)
    assert q is not net and q.backbone.native and isinstance(q.backbone, QuantBOJANET)
    return q


def _aten_twin(q, bits, device="cpu"):
    """the ATen route holding the same state dict (float32)"""
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import _quantise_aten
    rng = torch.get_rng_state()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = CoreModel(2, q.hidden_size, 1, "bojanet")
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
        print(f"[bojanet q {name}] {ref}: {int((d > 2e-6).sum())} of {d.size} samples beyond 2e-6, largest deviation {d.max():.2e}")
    flips = 2 if bits == 8 else yt.size // 5
    assert grid_close(yt, fx["y"], step, flips)
    assert grid_close(ye, fx["y_eval"], step, flips)
    if bits == 8:
        assert grid_close(ya, fx["ya_eval"], step, 2)
    else:
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
    print(f"[bojanet q {name}] loss {loss.item():.8f} (reference {ref:.8f}), dL/dx rel {rel_err(xg.grad.cpu().numpy(), fx['gx']):.2e}")
    assert abs(loss.item() - ref) < 1e-5 * max(1.0, ref)
    assert rel_err(xg.grad.cpu().numpy(), fx["gx"]) < 2e-3
    worst = 0.0
    for k, p in q.named_parameters():
        if ("g/" + k) in fx:
            g = fx["g/" + k]
            assert p.grad is not None, k
            if np.abs(g).max() == 0:
                assert float(p.grad.abs().max()) == 0.0, k         # the 16 weight / activation scales: the round of the exponent kills them
            else:
                worst = max(worst, rel_err(p.grad.cpu().numpy(), g))
                assert rel_err(p.grad.cpu().numpy(), g) < 2e-3, k
        else:
            assert "out_quantizer" in k and p.grad is None, k     # outside the graph
    print(f"[bojanet q {name}] worst weight-gradient rel {worst:.2e}")


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
        print(f"[bojanet q {name}] step {s}: loss {l.item():.8f} (reference {ref:.8f}), worst parameter rel {worst:.2e}")
    for k, p in q.named_parameters():
        if "out_quantizer" in k:
            assert torch.equal(p.detach(), before[k]), k                                   # AdamW skips them (grad is None in the reference)
        elif "scale" in k:
            now = float(p.detach())
            assert now < float(before[k]), k                                                # zero gradient, but decayed
            assert abs(now - float(fx["sd3/" + k][0])) <= 1e-6 * float(before[k]), k


def _prepared(H, bits):
    """a quantised bojanet on the device with every kind of mask in play: biases off zero, W_fh / W_gh / W_fi weights partly beyond the weight
    grid's range (max |w| = 2.6), W_fh's and W_out_I's activation ranges narrowed, the last FIR tap of both banks kept off zero (so that a zero
    filter output is not a property of the model)"""
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import get_quant_model
    _Proj.n_bits_w = _Proj.n_bits_a = bits
    q = get_quant_model(_Proj, CoreModel(2, H, 1, "bojanet").cuda())
    bb = q.backbone
    assert bb.native
    with torch.no_grad():
        g = torch.Generator().manual_seed(H)
        for lay in (bb.W_fi, bb.W_gi, bb.W_out_I, bb.W_out_Q):
            lay.bias.copy_(((torch.rand(lay.bias.shape, generator=g) - 0.5) * 0.4).cuda())
        for lay in (bb.W_fh, bb.W_gh, bb.W_fi):
            lay.weight.mul_(2.6 / float(lay.weight.abs().max()))
        bb.W_fh.act_quantizer.scale.mul_(0.25)
        bb.W_out_I.act_quantizer.scale.mul_(0.25)
        for lay in (bb.fir_I, bb.fir_Q):
            w = lay.weight[:, 15]
            lay.weight[:, 15] = torch.where(w < 0, -1.0, 1.0) * w.abs().clamp_min(0.02)
    return q


def _aten_forward_backward(a, x, dy):
    xt = torch.from_numpy(x).requires_grad_(True)
    a.zero_grad()
    y = a(xt)
    y.backward(torch.from_numpy(dy))
    return y.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize("H,B,T,bits", [(12, 40, 16, 8), (1, 8, 17, 8), (6, 64, 50, 8), (16, 24, 16, 8), (13, 3, 130, 8), (16, 700, 20, 8),
                                         (10, 256, 200, 8), (9, 16, 20, 16), (7, 32, 40, 16), (8, 1000, 16, 8)])
def test_matches_the_aten_route_on_ragged_sizes(H, B, T, bits):
    """(8, 1000, 16, 8 bits): more sequences than the backward launch has workgroups, so every workgroup runs several and carries its weight
    gradients from one to the next; comparator alone at this shape: clean share 0.998, no singular sequence)"""
    torch.manual_seed(H + B + T)
    q = _prepared(H, bits)
    a = _aten_twin(q, bits)
    g = torch.Generator().manual_seed(B + T)
    x = (0.3 * torch.randn(B, T, 2, generator=g) + 0.1).numpy()
    dy = torch.randn(B, T, 2, generator=g).numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yo, dxo_all = _aten_forward_backward(a, x, dy)
    singular = ~np.isfinite(dxo_all.reshape(B, -1)).all(1)
    clean = None
    ys = []
    for mode in (q.eval, q.train):
        mode()
        with torch.no_grad():
            y = q(torch.from_numpy(x).cuda()).cpu().numpy()
        ys.append(y)
        d = np.abs(y - yo).reshape(B, -1).max(1)
        assert np.isfinite(y).all() and d.max() < 2.0
        clean = d <= 4e-6
    assert np.array_equal(ys[0], ys[1])
    print(f"[bojanet q H{H} B{B} T{T} W{bits}] sequences on the ATen route's trajectory: {clean.mean():.3f}, largest deviation {d.max():.2e}, "
          f"singular {int(singular.sum())} of {B}")
    need = (0.8 if T == 200 else 0.9) if bits == 8 else (0.4 if T <= 20 else 0.0)
    assert clean.mean() >= need, (clean.mean(), d.max())
    assert singular.mean() <= 0.02
    keep = clean & ~singular
    if not keep.any():
        return
    dyk = dy * keep[:, None, None]                       # the other sequences contribute nothing to either side
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    q(xt).backward(torch.from_numpy(dyk).cuda())
    dx = xt.grad.cpu().numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, dxo = _aten_forward_backward(a, x[keep], dy[keep])      # (a singular sequence would turn the weight gradients to NaN even with dy = 0)
    tol = 2e-4 if bits == 8 else 2e-3
    assert np.isfinite(dx).all()
    assert rel_err(dx[keep], dxo) < tol
    assert np.abs(dx[~keep]).max(initial=0.0) == 0.0
    ref = dict(a.named_parameters())
    for k, v in q.named_parameters():
        r = ref[k].grad
        if "out_quantizer" in k:
            assert v.grad is None and r is None, k
        elif "scale" in k:
            assert float(v.grad.abs().max()) == 0.0 and float(r.abs().max()) == 0.0, k
        else:
            assert rel_err(v.grad.cpu().numpy(), r.numpy()) < tol, k
    if H > 1:
        bb = q.backbone
        for lay in (bb.W_fh, bb.W_fi):
            w, gw = lay.weight.detach().cpu().numpy(), lay.weight.grad.cpu().numpy()
            v = w / 2.0 ** (2 - bits)
            beyond = (v < -2.0 ** (bits - 1)) | (v > 2.0 ** (bits - 1) - 1)
            assert beyond.any() and np.all(gw[beyond] == 0.0) and np.abs(gw[~beyond]).max() > 0
    # dL/dx alone (the frozen-PA role): the same values
    for v in q.parameters():
        v.requires_grad_(False)
    xt2 = torch.from_numpy(x).cuda().requires_grad_(True)
    q(xt2).backward(torch.from_numpy(dyk).cuda())
    assert np.array_equal(xt2.grad.cpu().numpy(), dx)


def test_a_zero_filter_output_is_finite_here_and_not_in_the_aten_route():
    """a frame whose first three samples are exactly 0: every filter output of steps 0 .. 2 is 0 + 0j (cos = sin = 0, mag = 1e-8)"""
    H, B, T, bits = 12, 4, 20, 8
    torch.manual_seed(5)
    q = _prepared(H, bits)
    a = _aten_twin(q, bits)
    g = torch.Generator().manual_seed(7)
    x = (0.3 * torch.randn(B, T, 2, generator=g) + 0.1).numpy()
    x[:, :3] = 0.0
    dy = torch.randn(B, T, 2, generator=g).numpy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yo, dxo = _aten_forward_backward(a, x, dy)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    y = q(xt)
    y.backward(torch.from_numpy(dy).cuda())
    yk = y.detach().cpu().numpy()
    assert np.array_equal(yk[:, :3], yo[:, :3])
    assert np.abs(yk - yo).max() <= 4e-6
    assert np.isfinite(xt.grad.cpu().numpy()).all()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in q.parameters())
    assert not np.isfinite(dxo).all() or any(p.grad is not None and not bool(torch.isfinite(p.grad).all()) for p in a.parameters())


def test_cascade_with_a_frozen_float_pa():
    """a quantised bojanet DPD (H 12, W8A8) in front of a frozen float dgru PA (H 13): one fused_train_step — forward, PA forward + loss + dL/du,
    backward, chained — against the same composition with the ATen-route DPD, on the sequences both DPDs agree on"""
    from opendpd_amd import CascadedModel, CoreModel
    from opendpd_amd.quant import get_quant_model
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    rng = np.random.RandomState(0)
    x = (rng.uniform(0.05, 0.7, (9, 41, 2)) * rng.choice([-1.0, 1.0], (9, 41, 2))).astype(np.float32)
    torch.manual_seed(3)
    _Proj.n_bits_w = _Proj.n_bits_a = 8
    dpd = get_quant_model(_Proj, CoreModel(2, 12, 1, "bojanet").cuda())
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
    print(f"[bojanet q cascade] sequences on the ATen route's trajectory: {clean.mean():.3f}")
    assert clean.mean() >= 0.9
    xc = xt[torch.from_numpy(clean).cuda()].contiguous()
    opt = FusedAdamW(casc, lr=0.0, weight_decay=0.0)
    loss = fused_train_step(opt, xc, xc.clone(), "l2", 0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lo = torch.nn.functional.mse_loss(casc.pa_model(a(xc)), xc)
        lo.backward()
    assert abs(loss.item() - lo.item()) < 2e-5 * max(1.0, lo.item())
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


def test_a_long_evaluation_sequence_runs_and_its_head_equals_a_short_run():
    torch.manual_seed(11)
    _Proj.n_bits_w = _Proj.n_bits_a = 8
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import get_quant_model
    q = get_quant_model(_Proj, CoreModel(2, 12, 1, "bojanet").cuda())
    q.eval()
    g = torch.Generator().manual_seed(1)
    x = (0.3 * torch.randn(1, 19662, 2, generator=g) + 0.1).cuda()
    with torch.no_grad():
        y = q(x)
        ys = q(x[:, :200].contiguous())
    assert y.shape == (1, 19662, 2) and bool(torch.isfinite(y).all())
    assert torch.equal(y[:, :200], ys)


def test_frames_shorter_than_the_window_are_refused():
    """the reference cannot frame T < 15 (bojanet.py:72-77); the quantised kernels answer as the float ones do"""
    _Proj.n_bits_w = _Proj.n_bits_a = 8
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import get_quant_model
    q = get_quant_model(_Proj, CoreModel(2, 8, 1, "bojanet").cuda())
    with pytest.raises(RuntimeError):
        q(torch.randn(2, 14, 2, device="cuda") * 0.3)
    assert q(torch.randn(2, 15, 2, device="cuda") * 0.3).shape == (2, 15, 2)
