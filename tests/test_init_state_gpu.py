"""CoreModel.forward(x, h_0) with a given initial state on the kernels (ODPD_FLAG_INIT_STATE: the lane-per-unit state route of
csrc/gru_wide.hip / lstm_wide.hip, hidden 1 .. 64): the reference's vectors (tests/golden/h0_*.npz), a grid against the fp64 ATen
restatement (backbones/wide.py) under every grad mode, zero states, a carried state, the backbones that ignore h_0, the refusals, the knob
guard, the raw C ABI and a learned initial state."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from tests.golden_util import Fixture, rel_err

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = 2e-5, 2e-4
STATE_BACKBONES = ("gru", "dgru", "qgru", "qgru_amp1", "lstm")


def _data(B, T, seed):
    rng = np.random.RandomState(seed)
    amp = 0.05 + 0.85 * rng.rand(B, T, 1)
    ph = 2 * np.pi * rng.rand(B, T, 1)
    x = np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)
    return x, rng.randn(B, T, 2).astype(np.float32)


def _net(bb, H, seed, **kw):
    from opendpd_amd import CoreModel
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = CoreModel(2, H, 1, bb, **kw).cuda()
    with torch.no_grad():      # biases are zero after init: make them count
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
    return net


def _restatement(net):
    """fp64 ATen restatement (backbones/wide.py) of a kernel-backed model, same parameters, on the CPU"""
    from opendpd_amd.backbones import wide as W
    mod = W.build(net.backbone_type, 2, net.hidden_size, 1).double()
    mod.load_state_dict({k: v.detach().cpu().double() for k, v in net.backbone.state_dict().items()})
    return mod


def _ref(net, x, h0, dy):
    """fp64: y, dL/dx, dL/dh0 and the parameter gradients (state-dict order) for the loss sum(y * dy)"""
    mod = _restatement(net)
    xd = torch.from_numpy(x).double().requires_grad_(True)
    hd = torch.from_numpy(h0).double().requires_grad_(True)
    y = mod(xd, hd)
    (y * torch.from_numpy(dy).double()).sum().backward()
    return y.detach().numpy(), xd.grad.numpy(), hd.grad.numpy(), {k: p.grad.numpy() for k, p in mod.named_parameters()}


@pytest.mark.parametrize("name", ["h0_gru_h8", "h0_dgru_h13", "h0_qgru_h10", "h0_qgru_amp1_h16", "h0_lstm_h9", "h0_gru_h40", "h0_lstm_h48"])
def test_reference_fixtures_with_h0(name):
    from opendpd_amd import CoreModel
    fx = Fixture(name)
    m = fx.meta
    net = CoreModel(2, m["hidden"], 1, m["backbone"])
    net.load_state_dict({k: torch.from_numpy(fx["sd/" + k]) for k in fx.keys("sd")})
    net = net.cuda()
    x = torch.from_numpy(fx["x"]).cuda().requires_grad_(True)
    h0 = torch.from_numpy(fx["h0"]).cuda().requires_grad_(True)
    y = net(x, h0)
    assert rel_err(y.detach().cpu().numpy(), fx["y"]) < FWD_TOL
    loss = torch.nn.functional.mse_loss(y, torch.from_numpy(fx["tgt"]).cuda())
    assert abs(loss.item() - fx["loss"][0]) < 1e-5 * max(1.0, fx["loss"][0])
    loss.backward()
    for k, p in net.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), fx["g/" + k]) < GRAD_TOL, k
    assert rel_err(x.grad.cpu().numpy(), fx["gx"]) < GRAD_TOL
    assert h0.grad.shape == h0.shape and rel_err(h0.grad.cpu().numpy(), fx["gh0"]) < GRAD_TOL


@pytest.mark.parametrize("bb", STATE_BACKBONES)
@pytest.mark.parametrize("H", [1, 5, 8, 13, 16, 17, 23, 32, 33, 64])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 50), (7, 129), (300, 64), (1100, 5)])
def test_grid_against_the_fp64_restatement(bb, H, B, T):
    """(1100, 5): more sequences than gru_wide_rows' grid of 4 x CUs — every workgroup walks several, each with its own state"""
    net = _net(bb, H, H * 1000 + B * 10 + T)
    x, dy = _data(B, T, B * 7 + T)
    h0 = (0.6 * np.random.RandomState(H + B).randn(1, B, H)).astype(np.float32)
    yo, dxo, dho, go = _ref(net, x, h0, dy)
    xc, hc, dyc = torch.from_numpy(x).cuda(), torch.from_numpy(h0).cuda(), torch.from_numpy(dy).cuda()
    with torch.no_grad():                                                   # inference: no records written
        assert rel_err(net(xc, hc).cpu().numpy(), yo) < FWD_TOL
    # the parameters only
    y = net(xc, hc)
    y.backward(dyc)
    assert rel_err(y.detach().cpu().numpy(), yo) < FWD_TOL
    for k, p in net.backbone.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), go[k]) < GRAD_TOL, k
    for p in net.parameters():
        p.requires_grad_(False)
    # h_0 only
    h = hc.clone().requires_grad_(True)
    net(xc, h).backward(dyc)
    assert rel_err(h.grad.cpu().numpy(), dho) < GRAD_TOL
    # x and h_0
    xg, h = xc.clone().requires_grad_(True), hc.clone().requires_grad_(True)
    net(xg, h).backward(dyc)
    assert rel_err(xg.grad.cpu().numpy(), dxo) < GRAD_TOL and rel_err(h.grad.cpu().numpy(), dho) < GRAD_TOL


@pytest.mark.parametrize("bb,H", [("gru", 8), ("dgru", 13), ("lstm", 20), ("qgru", 40), ("lstm", 64)])
def test_zero_h0(bb, H):
    """without grad: today's path, bit for bit; requiring grad: the state route, and h_0.grad is the fp64 dL/dh_0"""
    net = _net(bb, H, 3)
    x, dy = _data(6, 70, 4)
    xc = torch.from_numpy(x).cuda()
    z = torch.zeros(1, 6, H, device="cuda")
    with torch.no_grad():
        assert torch.equal(net(xc, z), net(xc))
    assert torch.equal(net(xc, z).detach(), net(xc).detach())
    _, _, dho, _ = _ref(net, x, np.zeros((1, 6, H), np.float32), dy)
    zg = z.clone().requires_grad_(True)
    net(xc, zg).backward(torch.from_numpy(dy).cuda())
    assert zg.grad is not None and rel_err(zg.grad.cpu().numpy(), dho) < GRAD_TOL


@pytest.mark.parametrize("bb,H", [("gru", 12), ("dgru", 40), ("qgru", 5), ("qgru_amp1", 33)])
def test_carried_state(bb, H):
    """a sequence run in one pass equals its tail run from the state the fp64 restatement's rnn reaches over the head"""
    from opendpd_amd.backbones import wide as W
    net = _net(bb, H, 5)
    B, T, k = 4, 200, 77
    x, _ = _data(B, T, 6)
    h0 = (0.5 * np.random.RandomState(1).randn(1, B, H)).astype(np.float32)
    mod = _restatement(net)
    xd = torch.from_numpy(x[:, :k]).double()
    f = W._feat_polar6(xd) if bb == "dgru" else mod.features(xd)
    with torch.no_grad():
        _, hk = mod.rnn(f, torch.from_numpy(h0).double())
        y_full = net(torch.from_numpy(x).cuda(), torch.from_numpy(h0).cuda()).cpu().numpy()
        y_tail = net(torch.from_numpy(np.ascontiguousarray(x[:, k:])).cuda(), hk.float().cuda()).cpu().numpy()
    assert rel_err(y_tail, y_full[:, k:]) < FWD_TOL


@pytest.mark.parametrize("bb,H,kw", [("deltagru", 10, {}), ("deltajanet", 10, {}), ("deltagru_tcnskip", 15, {}), ("vdlstm", 10, {}),
                                     ("apnrru", 10, {}), ("mcldnn", 10, {}), ("gmp", 11, {}), ("tcnn", 10, {}), ("rvtdcnn", 10, {}),
                                     ("neuraltx", 10, {})])
def test_backbones_that_ignore_h0(bb, H, kw):
    net = _net(bb, H, 7, **kw)
    x = torch.from_numpy(_data(3, 40, 8)[0]).cuda()
    h0 = torch.randn(1, 3, H, device="cuda")
    assert net.backbone.native
    with torch.no_grad():
        assert torch.equal(net(x, h_0=h0), net(x))
    assert torch.equal(net(x, h_0=h0.requires_grad_(True)).detach(), net(x).detach())


def test_out_of_scope_models_still_refuse_a_state():
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import QuantGRUCellModel
    x = torch.from_numpy(_data(2, 10, 9)[0]).cuda()
    nets = [_net("pgjanet", 10, 1), _net("bojanet", 10, 1), _net("dvrjanet", 8, 1, num_dvr_units=4), CoreModel(2, 8, 2, "gru").cuda(),
            CoreModel(2, 8, 2, "lstm").cuda()]
    q = _net("gru", 10, 1)
    q.backbone = QuantGRUCellModel("gru", 10, 8, 8).cuda()
    nets.append(q)
    for net in nets:
        H = net.hidden_size
        with pytest.raises(NotImplementedError, match="it runs on float gru / dgru / qgru / qgru_amp1 / lstm of one layer"):
            net(x, torch.ones(1, 2, H, device="cuda"))
        with pytest.raises(NotImplementedError, match="requiring grad"):      # (its gradient could not be returned)
            net(x, torch.zeros(1, 2, H, device="cuda", requires_grad=True))


def test_knob_change_between_forward_and_backward_is_refused():
    from opendpd_amd import _lib
    lib = _lib.load()
    net = _net("gru", 20, 2)
    x = torch.from_numpy(_data(4, 30, 3)[0]).cuda()
    h0 = torch.randn(1, 4, 20, device="cuda", requires_grad=True)
    y = net(x, h0)
    in_force = int(os.environ.get("ODPD_S16_MIN_BATCH", -1))      # (the knob's value: set again, the generation still moves)
    assert lib.odpd_set_tuning(b"s16_min_batch", in_force) == 0
    with pytest.raises(RuntimeError, match="kernel-selection knobs"):
        y.sum().backward()
    assert not net.backbone.desc.flags & _lib.FLAG_INIT_STATE
    net(x, h0).sum().backward()
    assert h0.grad is not None


def test_raw_c_abi():
    from opendpd_amd import _lib
    lib = _lib.load()
    net = _net("gru", 16, 4)
    d = net.backbone.desc
    B, T, H = 4, 20, 16
    x = torch.from_numpy(_data(B, T, 5)[0]).cuda()
    h0 = torch.randn(B, H, device="cuda")
    y = torch.empty_like(x)
    flat = net.backbone.flat_params()
    assert lib.odpd_backbone_fwd_state(_lib.stream_ptr(), C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(h0), _lib.ptr(y), None) == -1
    d.flags |= _lib.FLAG_INIT_STATE
    try:
        assert lib.odpd_backbone_fwd_state(_lib.stream_ptr(), C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(h0), _lib.ptr(y), None) == 0
        assert lib.odpd_backbone_fwd(_lib.stream_ptr(), C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(y), None, None) == -1
        assert lib.odpd_partial_rows(C.byref(d), B, T, 1) == -2 and lib.odpd_partial_rows(C.byref(d), B, T, 0) == B
        assert lib.odpd_ckpt_floats(C.byref(d), B, T) == B * T * 5 * 64
        part = torch.empty(8, net.backbone.n_flat + _lib.LOSS_COLS, device="cuda")
        rc = lib.odpd_train_fwd_bwd(_lib.stream_ptr(), C.byref(d), 0, B, T, B * T * 2, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(x), _lib.ptr(part), None)
        assert rc == -2
        assert lib.odpd_train_workspace_floats(C.byref(d), B, T) == -2 and lib.odpd_frozen_loss_rows(C.byref(d), B, T) == -2
        assert lib.odpd_framed_train_supported_shape(C.byref(d), B, T) == 0 and lib.odpd_sweep_fwd_supported(C.byref(d), B, T) == 0
    finally:
        d.flags &= ~_lib.FLAG_INIT_STATE
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(y, net(x, h0.unsqueeze(0)))
    boj = _net("bojanet", 10, 1).backbone
    bd = _lib.ModelDesc(boj.desc.backbone, boj.desc.hidden, 0, 0, 0, 0, _lib.FLAG_INIT_STATE)
    yb, hb = torch.empty_like(x), torch.zeros(B, 10, device="cuda")
    assert lib.odpd_backbone_fwd_state(_lib.stream_ptr(), C.byref(bd), B, T, _lib.ptr(boj.flat_params()), _lib.ptr(x), _lib.ptr(hb), _lib.ptr(yb),
                                       None) == -2
    assert lib.odpd_ckpt_floats(C.byref(bd), B, T) == -2 and lib.odpd_param_count(C.byref(bd)) == -2
    for bb, H, flags in (("gru", 8, _lib.FLAG_TWO_LAYERS), ("vdlstm", 8, 0), ("gru", 65, 0)):
        dd = _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, 0, 0, 0, 0, flags | _lib.FLAG_INIT_STATE)
        assert lib.odpd_partial_rows(C.byref(dd), B, T, 0) == -2, bb


def test_learned_initial_state_moves_under_adamw():
    net = _net("dgru", 13, 6)
    x, t = _data(8, 50, 7)
    xc, tc = torch.from_numpy(x).cuda(), torch.from_numpy(0.3 * t).cuda()
    h0 = torch.nn.Parameter(torch.zeros(1, 8, 13, device="cuda"))
    opt = torch.optim.AdamW(list(net.parameters()) + [h0], lr=1e-2)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(net(xc, h0), tc)
        loss.backward()
        assert h0.grad is not None and torch.isfinite(h0.grad).all()
        opt.step()
        losses.append(loss.item())
    assert h0.detach().abs().max().item() > 1e-3 and np.isfinite(losses).all()
