"""No call writes the module's descriptor (backbones/native.py: `desc` / `call_desc`): after an autograd forward, its backward, a refused
backward, a state-route call, an eval() pass and a fused train step `bytes(backbone.desc)` in train mode is what it was before them — and the
last call computes, bit for bit, what a fresh module with the same weights computes that made only that call: nothing an earlier call
selected (ODPD_FLAG_NEED_DX, ODPD_FLAG_INIT_STATE, ODPD_FLAG_EVAL) reaches the next one."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEVER = 1 << 30
REFUSED = "kernel-selection knobs .* changed between forward and backward"


@pytest.fixture
def lib():
    from opendpd_amd import _lib
    lib = _lib.load()
    yield lib
    lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1))


def _signal(B, T, seed):
    rng = np.random.RandomState(seed)
    amp, ph = 0.05 + 0.85 * rng.rand(B, T, 1), 2 * np.pi * rng.rand(B, T, 1)
    x = np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(rng.randn(B, T, 2).astype(np.float32)).cuda()


def _core(bb, H, thx=0.0, thh=0.0, seed=0):
    from opendpd_amd import CoreModel
    torch.manual_seed(seed)
    net = CoreModel(2, H, 1, bb, thx=thx, thh=thh).cuda()
    with torch.no_grad():      # biases are zero after init: make them count
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
    return net


def _flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])


def _fused_step(net, x, t):
    """one fused train step of a new optimiser -> (loss, the updated parameters)"""
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    loss = fused_train_step(FusedAdamW(net, lr=1e-2), x, t, "l2", 1.0)
    return loss.clone(), _flat(net).clone()


def test_delta_autograd_refusal_then_fused_step(lib):
    from opendpd_amd import _lib
    bb, H, thx, thh, B, T = "deltagru", 15, 0.01, 0.05, 19, 65
    net, fresh = _core(bb, H, thx, thh, seed=5), _core(bb, H, thx, thh, seed=5)
    x, t = _signal(B, T, 3)
    net.train()
    before = bytes(net.backbone.desc)
    xr = x.clone().requires_grad_(True)
    y = net(xr)      # (dL/dx asked for: this call alone takes the 16-sequences-per-wave kernels)
    assert bytes(net.backbone.desc) == before
    y.backward(t)
    assert bytes(net.backbone.desc) == before and xr.grad is not None
    _lib.check(lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(NEVER)), "odpd_set_tuning")
    y = net(x.clone().requires_grad_(True))
    _lib.check(lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(0)), "odpd_set_tuning")
    with pytest.raises(RuntimeError, match=REFUSED):
        y.backward(t)
    assert bytes(net.backbone.desc) == before
    _lib.check(lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1)), "odpd_set_tuning")
    loss, params = _fused_step(net, x, t)
    assert bytes(net.backbone.desc) == before
    want_loss, want_params = _fused_step(fresh, x, t)
    assert torch.equal(loss, want_loss) and torch.equal(params, want_params)


def test_state_route_then_plain_forward(lib):
    bb, H, B, T = "gru", 20, 4, 30
    net, fresh = _core(bb, H, seed=7), _core(bb, H, seed=7)
    x, t = _signal(B, T, 11)
    net.train()
    before = bytes(net.backbone.desc)
    h0 = (0.2 * torch.randn(1, B, H, device="cuda")).requires_grad_(True)
    y = net.backbone.forward_state(x, h0)
    assert bytes(net.backbone.desc) == before
    y.backward(t)
    assert bytes(net.backbone.desc) == before and h0.grad is not None and h0.grad.shape == h0.shape
    y = net.backbone(x)
    assert bytes(net.backbone.desc) == before
    assert torch.equal(y, fresh.backbone(x))


def _cascade(seed):
    from opendpd_amd import CascadedModel
    net = CascadedModel(dpd_model=_core("dgru", 8, seed=seed), pa_model=_core("deltagru", 15, 0.01, 0.05, seed=seed + 1))
    net.freeze_pa_model()
    return net.cuda()


def test_autograd_on_the_frozen_pa_then_cascade_step(lib):
    B, T = 5, 40
    net, fresh = _cascade(21), _cascade(21)
    x, t = _signal(B, T, 13)
    net.train()
    dpd, pa = net.dpd_model.backbone, net.pa_model.backbone
    before = bytes(dpd.desc), bytes(pa.desc)
    xr = x.clone().requires_grad_(True)
    y = net.pa_model(xr)      # the PA alone, asked for dL/dx
    assert (bytes(dpd.desc), bytes(pa.desc)) == before
    y.backward(t)
    assert (bytes(dpd.desc), bytes(pa.desc)) == before and xr.grad is not None
    with torch.no_grad():
        net.pa_model(x)      # .. and NOT asked for it (an evaluation pass): the step below still asks its PA for dL/du
    assert (bytes(dpd.desc), bytes(pa.desc)) == before
    loss, params = _fused_step(net, x, t)
    assert (bytes(dpd.desc), bytes(pa.desc)) == before
    want_loss, want_params = _fused_step(fresh, x, t)
    assert torch.equal(loss, want_loss) and torch.equal(params, want_params)


@pytest.mark.parametrize("bb,H,B,T", [("qgru", 10, 37, 41), ("dgru", 8, 37, 41)])
def test_w8a8_eval_forward_then_fused_step(lib, bb, H, B, T):
    from tests.test_quant_more_gpu import _w8a8_model
    q, x, dy = _w8a8_model(bb, H, B, T)
    fresh, _, _ = _w8a8_model(bb, H, B, T)
    x, t = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    q.train()
    fresh.train()
    before = bytes(q.backbone.desc)
    q.eval()
    with torch.no_grad():
        q(x)
    q.train()      # (the call above ran with ODPD_FLAG_EVAL; the module's own descriptor follows the mode back)
    assert bytes(q.backbone.desc) == before
    loss, params = _fused_step(q, x, t)
    assert bytes(q.backbone.desc) == before
    want_loss, want_params = _fused_step(fresh, x, t)
    assert torch.equal(loss, want_loss) and torch.equal(params, want_params)
