"""GPU parity of the MCLDNN kernels (csrc/mcldnn.hip; reference backbones/mcldnn.py:9-134) against vectors produced by the reference
(tests/golden/mcldnn_c{8,3}.npz, extra_mcldnn_h8.npz) and against the CPU oracle on ragged shapes: outputs, the gradients of all 14
parameter tensors (the three convolutions through the composed front end, W_ih, the LSTM, the two linear layers), dL/dx incl. the
circular window's wrap onto the frame's last four samples and across chunk boundaries, trajectory, both cascade roles."""
import warnings

import numpy as np
import pytest
import torch

from tests.golden_util import Fixture, assert_grad_blocks, net_grad_blocks, rel_err

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = 2e-5, 3e-4


def _net(C, fx=None, prefix="sd", device="cuda"):
    from opendpd_amd import CoreModel
    net = CoreModel(2, C, 1, "mcldnn")
    if fx is not None:
        net.load_state_dict({k: torch.from_numpy(fx[f"{prefix}/" + k]) for k in fx.keys(prefix)})
    return net.to(device)


def _iq(rng, B, T):
    amp, ph = 0.05 + 0.85 * rng.rand(B, T, 1), 2 * np.pi * rng.rand(B, T, 1)
    return np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)


@pytest.mark.parametrize("name", ["mcldnn_c8", "mcldnn_c3"])
def test_golden_forward_backward(name):
    fx = Fixture(name)
    net = _net(fx.meta["hidden"], fx)
    assert net.backbone.native and sum(p.numel() for p in net.parameters()) == fx.meta["n_param"]
    x = torch.from_numpy(fx["x"]).cuda().requires_grad_(True)
    y = net(x)
    assert rel_err(y.detach().cpu().numpy(), fx["y"]) < FWD_TOL
    loss = torch.nn.functional.mse_loss(y, torch.from_numpy(fx["tgt"]).cuda())
    assert abs(loss.item() - fx["losses"][0]) < 1e-5 * max(1.0, fx["losses"][0])
    loss.backward()
    for k, p in net.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), fx["g/" + k]) < GRAD_TOL, k
    assert rel_err(x.grad.cpu().numpy(), fx["gx"]) < GRAD_TOL
    with torch.no_grad():
        ya = net(torch.from_numpy(fx["xa"]).cuda())
    assert rel_err(ya.cpu().numpy(), fx["ya"]) < FWD_TOL


def test_second_reference_vector():
    fx = Fixture("extra_mcldnn_h8")
    net = _net(8, fx, "sdu")
    x = torch.from_numpy(fx["x"]).cuda().requires_grad_(True)
    y = net(x)
    assert rel_err(y.detach().cpu().numpy(), fx["y"]) < FWD_TOL
    torch.nn.functional.mse_loss(y, torch.from_numpy(fx["tgt"]).cuda()).backward()
    for k, p in net.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), fx["g/" + k]) < GRAD_TOL, k
    assert rel_err(x.grad.cpu().numpy(), fx["gx"]) < GRAD_TOL


RAGGED_CHANNELS = [1, 2, 3, 5, 8, 11, 16]
RAGGED_SHAPES = [(1, 4), (3, 5), (17, 32), (7, 33), (5, 200), (66, 63), (2, 36)]
# input seeds of the (C, B, T) on which B * 17 + T draws a dL/dy whose convolution gradients (conv2d_*.bias: one sum over every sample of
# the batch per element) cancel so far that the serial fp32 oracle's own rounding on such a block exceeds GRAD_TOL / 16 of the fp64 oracle
# (tests/test_grad_blocks_cpu.py; 1.9e-5 .. 8.1e-5 there): the first of B * 17 + T + 1000 k on which it does not
RAGGED_RESEEDED = {(1, 1, 4): 1021, (3, 5, 200): 1285, (3, 66, 63): 2185, (5, 5, 200): 1285, (5, 66, 63): 2185, (11, 66, 63): 2185,
                   (16, 5, 200): 3285, (16, 66, 63): 4185}


def ragged_case(C, B, T, device="cuda"):
    """model, input and output gradient of test_against_oracle_ragged (tests/test_grad_blocks_cpu.py holds the fp32 oracle to the
    fp64 one on the same cases, `device` "cpu")"""
    torch.manual_seed(C * 100 + B + T)
    net = _net(C, device=device)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
    rng = np.random.RandomState(RAGGED_RESEEDED.get((C, B, T), B * 17 + T))
    x = _iq(rng, B, T)
    dy = rng.randn(B, T, 2).astype(np.float32)
    return net, x, dy


@pytest.mark.parametrize("C", RAGGED_CHANNELS)
@pytest.mark.parametrize("B,T", RAGGED_SHAPES)
def test_against_oracle_ragged(C, B, T):
    from oracle.oracle import Oracle, make_model
    net, x, dy = ragged_case(C, B, T)
    o = Oracle("f32")
    m = make_model("mcldnn", C)
    p = np.concatenate([q.detach().cpu().numpy().reshape(-1) for q in net.parameters()])
    assert o.param_count(m) == p.size == net.backbone.n_flat
    yo, _ = o.forward(m, p, x)
    go, dxo = o.backward(m, p, x, dy)
    # weight gradients alone, then with dL/dx, then dL/dx of the frozen model
    y = net(torch.from_numpy(x).cuda())
    y.backward(torch.from_numpy(dy).cuda())
    assert rel_err(y.detach().cpu().numpy(), yo) < FWD_TOL
    blocks = net_grad_blocks(net)
    g = np.concatenate([q.grad.cpu().numpy().reshape(-1) for q in net.parameters()])
    assert_grad_blocks(g, go, blocks, GRAD_TOL, exact_zeros=True)                  # every tensor on its own scale
    for q in net.parameters():
        q.grad = None
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    net(xt).backward(torch.from_numpy(dy).cuda())
    g = np.concatenate([q.grad.cpu().numpy().reshape(-1) for q in net.parameters()])
    assert_grad_blocks(g, go, blocks, GRAD_TOL)
    assert rel_err(xt.grad.cpu().numpy(), dxo) < GRAD_TOL
    for q in net.parameters():
        q.requires_grad_(False)
    xt2 = torch.from_numpy(x).cuda().requires_grad_(True)
    net(xt2).backward(torch.from_numpy(dy).cuda())
    assert rel_err(xt2.grad.cpu().numpy(), dxo) < GRAD_TOL


@pytest.mark.parametrize("C", [1, 2, 3, 5, 8, 11, 16])
@pytest.mark.parametrize("B,T", [(1, 4), (3, 5), (7, 63), (5, 64), (2, 65), (64, 50), (9, 200), (300, 200), (5, 130), (3, 260)])
def test_gate_parallel_train_kernel(C, B, T):
    """the reference's own batch sizes run mcl_gp_train_kernel (one sequence per four-wave workgroup: wave 0 the LSTM(8) recurrences gate-
    parallel, the feature table, gates_in, the read-out and dA | db over all 256 threads, composition / chain rule as the S16 kernels): loss
    and gradient — every tensor on its own scale — against the oracle (L2 and L1), and against the split S16 chain (gp_max_batch = 0)"""
    import ctypes as C_
    from opendpd_amd import _lib
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    from oracle.oracle import Oracle, make_model
    lib = _lib.load()
    torch.manual_seed(C * 100 + B + T)
    net = _net(C)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
    rng = np.random.RandomState(B * 13 + T)
    x = _iq(rng, B, T)
    tgt = (0.4 * rng.randn(B, T, 2)).astype(np.float32)
    xt, tt = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    p = np.concatenate([q.detach().cpu().numpy().reshape(-1) for q in net.parameters()])
    o, m = Oracle("f32"), make_model("mcldnn", C)
    yo, _ = o.forward(m, p, x)
    blocks = net_grad_blocks(net)
    opt = FusedAdamW(net, lr=0.0, weight_decay=0.0)
    assert opt.has_fused(B, T)
    try:
        for kind in ("l2", "l1"):
            d = yo - tgt
            lo = float((d * d).mean()) if kind == "l2" else float(np.abs(d).mean())
            dy = (2 * d / d.size if kind == "l2" else np.sign(d) / d.size).astype(np.float32)
            go, _ = o.backward(m, p, x, dy, need_dx=False)
            loss = fused_train_step(opt, xt, tt, kind, 0.0)
            got = opt.grad[:-4].cpu().numpy().copy()
            assert abs(float(loss) - lo) < 2e-5 * max(1.0, lo)
            assert_grad_blocks(got, go, blocks, GRAD_TOL, exact_zeros=True)
            lib.odpd_set_tuning(b"gp_max_batch", C_.c_int64(0))
            opt2 = FusedAdamW(net, lr=0.0, weight_decay=0.0)
            assert not opt2.has_fused(B, T)
            for q in net.parameters():
                q.grad = None
            y = net(xt)
            l2 = torch.nn.functional.mse_loss(y, tt) if kind == "l2" else torch.nn.functional.l1_loss(y, tt)
            l2.backward()
            gs = torch.cat([q.grad.reshape(-1) for q in net.parameters()]).cpu().numpy()
            assert abs(float(loss) - l2.item()) < 1e-5 * max(1.0, lo) and rel_err(got, gs) < 1e-4
            lib.odpd_set_tuning(b"gp_max_batch", C_.c_int64(-1))
    finally:
        lib.odpd_set_tuning(b"gp_max_batch", C_.c_int64(-1))


def test_gate_parallel_envelope():
    """frames whose state does not fit a CU's LDS, and batches past a few rounds of workgroups, stay on the split S16 chain"""
    from opendpd_amd.train_funcs import FusedAdamW
    opt = FusedAdamW(_net(8), lr=0.0)
    assert opt.has_fused(256, 200) and opt.has_fused(64, 50)
    assert not opt.has_fused(4, 400) and not opt.has_fused(20000, 50)


def test_large_batch_every_wave_slot():
    from oracle.oracle import Oracle, make_model
    torch.manual_seed(5)
    C, B, T = 8, 16 * 256 * 8 + 19, 9
    net = _net(C)
    rng = np.random.RandomState(1)
    x = _iq(rng, B, T)
    dy = rng.randn(B, T, 2).astype(np.float32)
    o = Oracle("f32")
    m = make_model("mcldnn", C)
    p = np.concatenate([q.detach().cpu().numpy().reshape(-1) for q in net.parameters()])
    yo, _ = o.forward(m, p, x)
    go, dxo = o.backward(m, p, x, dy)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    y = net(xt)
    y.backward(torch.from_numpy(dy).cuda())
    assert rel_err(y.detach().cpu().numpy(), yo) < FWD_TOL
    g = np.concatenate([q.grad.cpu().numpy().reshape(-1) for q in net.parameters()])
    assert_grad_blocks(g, go, net_grad_blocks(net), GRAD_TOL)
    assert rel_err(xt.grad.cpu().numpy(), dxo) < GRAD_TOL


@pytest.mark.parametrize("name", ["mcldnn_c8", "mcldnn_c3"])
def test_train_steps_follow_reference(name):
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    fx = Fixture(name)
    net = _net(fx.meta["hidden"], fx)
    opt = FusedAdamW(net, lr=fx.meta["lr"])
    x = torch.from_numpy(fx["x"]).cuda()
    t = torch.from_numpy(fx["tgt"]).cuda()
    names = fx.keys("sd")
    for s in range(1, 4):
        loss = fused_train_step(opt, x, t, "l2", fx.meta["clip"])
        assert abs(loss.item() - fx["losses"][s - 1]) < 2e-5 * max(1.0, fx["losses"][s - 1])
        assert rel_err(net.backbone.flat_params().detach().cpu().numpy(), fx.flat(f"p{s}", names)) < 3e-5, s


def test_cascade_roles():
    """mcldnn as the DPD in front of a frozen DGRU PA and as the frozen PA behind a GRU DPD, against the oracle composition"""
    from opendpd_amd import CascadedModel, CoreModel
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    from oracle.oracle import Oracle, make_model
    o = Oracle("f32")
    rng = np.random.RandomState(0)
    x = (rng.uniform(0.05, 0.7, (9, 41, 2)) * rng.choice([-1.0, 1.0], (9, 41, 2))).astype(np.float32)
    for dpd_bb, dH, pa_bb, pH in (("mcldnn", 8, "dgru", 13), ("gru", 11, "mcldnn", 5)):
        torch.manual_seed(3)
        casc = CascadedModel(dpd_model=CoreModel(2, dH, 1, dpd_bb), pa_model=CoreModel(2, pH, 1, pa_bb))
        casc.freeze_pa_model()
        casc = casc.cuda()
        pd = torch.cat([q.detach().reshape(-1) for q in casc.dpd_model.parameters()]).cpu().numpy()
        pp = torch.cat([q.detach().reshape(-1) for q in casc.pa_model.parameters()]).cpu().numpy()
        md, mp = make_model(dpd_bb, dH), make_model(pa_bb, pH)
        u, _ = o.forward(md, pd, x)
        y, _ = o.forward(mp, pp, u)
        lo, dy = o.loss("l2", y, x)
        _, du = o.backward(mp, pp, u, dy)
        gd, _ = o.backward(md, pd, x, du, need_dx=False)
        opt = FusedAdamW(casc, lr=0.0, weight_decay=0.0)
        xt = torch.from_numpy(x).cuda()
        loss = fused_train_step(opt, xt, xt.clone(), "l2", 0.0)
        assert abs(loss.item() - lo) < 1e-5 * max(1.0, lo), (dpd_bb, pa_bb)
        assert rel_err(opt.grad[:-4].cpu().numpy(), gd) < GRAD_TOL, (dpd_bb, pa_bb)


def test_outside_the_envelope_runs_the_restatement():
    """more than 16 channels: the torch restatement, announced"""
    from opendpd_amd import CoreModel
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        net = CoreModel(2, 20, 1, "mcldnn").cuda()
    assert not net.backbone.native and any("envelope" in str(i.message) for i in w)
    y = net(torch.randn(3, 20, 2, device="cuda") * 0.3)
    assert y.shape == (3, 20, 2) and bool(torch.isfinite(y).all())


def test_frames_shorter_than_the_window_are_refused():
    """the circular window takes the frame's own last four samples (mcldnn.py:115-118): T < 4 cannot be framed"""
    net = _net(8)
    with pytest.raises(RuntimeError):
        net(torch.randn(2, 3, 2, device="cuda") * 0.3)
    assert net(torch.randn(2, 4, 2, device="cuda") * 0.3).shape == (2, 4, 2)
