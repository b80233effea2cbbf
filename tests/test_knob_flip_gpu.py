"""A kernel-selection knob (odpd_set_tuning) changed between an autograd forward and its backward.

The forward sizes and writes the checkpoints in the layout of the kernel the live knobs choose; the backward picks its kernel again from the
knobs at its own call.  backbones/native.py (_BackboneFn) records odpd_tuning_generation at the forward and refuses the backward when it moved:
a RuntimeError, and no gradient written.  Per row (ragged shapes: partial 16-sequence groups, odd T):
  control — the knob set before the forward, once per value: each run matches the oracle at the family's ragged-test bounds, and the two
            values really select different kernels at this shape (different checkpoint sizes, or gradients that are not bit-equal);
  flip    — forward under one value, backward under the other: refused (knobs inside the generation), or bit-identical gradients (the two
            knobs outside it);
  after   — the next ordinary forward / backward on the same module, under the new value, matches the oracle again.
The `samesize` rows flip a knob that keeps every buffer size (the layout inside the checkpoint records changes): without the guard their
backward would silently write wrong gradients instead of raising."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden_util import assert_grad_blocks, net_grad_blocks, rel_err

pytestmark = pytest.mark.gpu

NEVER = 1 << 30          # s16_min_batch / gp_max_batch: a batch no test reaches
DEFAULTS = {"s16_min_batch": -1, "s16_occupancy": 0, "gp_max_batch": -1}     # (knobs whose built-in value is not 1)
UNSIZED = ("xchg_fused", "lstm_pack")       # outside odpd_tuning_generation
TOLS = {"gru": (2e-5, 2e-4), "dgru": (2e-5, 2e-4), "lstm": (2e-5, 3e-4), "vdlstm": (2e-5, 3e-4), "deltagru": (2e-5, 3e-4),
        "pgjanet": (2e-5, 3e-4)}      # forward / gradient bounds of each family's test_against_oracle_ragged
REFUSED = "kernel-selection knobs .* changed between forward and backward"

# (backbone, hidden, thx, thh, B, T, knob, (value before, value after), knobs held fixed, dL/dx asked for).  Two flips select the same kernels
# on the autograd path and so have no row of their own: "s16_occupancy" only reaches the fused train step (the split S16 forward / backward
# keep their launch shape), and a delta backbone asked for dL/dx takes the 16-sequences-per-wave kernels whatever "s16_min_batch" says
# (test_refused_delta_backward_leaves_no_dx_flag_behind covers that forward's refusal).
FLOAT_ROWS = [
    pytest.param("gru", 11, 0.0, 0.0, 3, 65, "s16_min_batch", (0, NEVER), {}, True, id="s16_min_batch-gru11-B3"),
    pytest.param("dgru", 13, 0.0, 0.0, 37, 65, "s16_min_batch", (0, NEVER), {}, True, id="s16_min_batch-dgru13"),
    pytest.param("deltagru", 15, 0.01, 0.05, 19, 65, "s16_min_batch", (0, NEVER), {}, False, id="s16_min_batch-deltagru15"),
    pytest.param("pgjanet", 11, 0.0, 0.0, 19, 65, "s16_min_batch", (0, NEVER), {}, True, id="s16_min_batch-pgjanet11"),
    pytest.param("gru", 11, 0.0, 0.0, 3, 65, "gp_max_batch", (0, NEVER), {"s16_min_batch": NEVER}, True, id="gp_max_batch-gru11"),
    pytest.param("dgru", 23, 0.0, 0.0, 37, 70, "s16x", (1, 0), {"s16_min_batch": 0}, True, id="s16x-dgru23"),
    pytest.param("dgru", 23, 0.0, 0.0, 37, 70, "s16x_train", (1, 0), {"s16_min_batch": 0}, True, id="samesize-s16x_train-dgru23"),
    pytest.param("gru", 17, 0.0, 0.0, 37, 70, "s16x_train", (1, 0), {"s16_min_batch": 0}, True, id="samesize-s16x_train-gru17"),
    pytest.param("lstm", 9, 0.0, 0.0, 37, 65, "lstm_pack", (1, 0), {"s16_min_batch": 0}, True, id="lstm_pack-lstm9"),
    pytest.param("vdlstm", 13, 0.0, 0.0, 37, 65, "xchg_fused", (1, 0), {"s16_min_batch": 0}, True, id="xchg_fused-vdlstm13"),
]
# (backbone, hidden, B, T): quantisation-aware GRUCell kinds on the 16-sequences-per-wave kernels, three (two at hidden <= 8) or four unit slots
W8A8_ROWS = [pytest.param("qgru", 10, 37, 41, id="samesize-qat_u3-qgru10"), pytest.param("dgru", 8, 37, 41, id="samesize-qat_u3-dgru8")]


@pytest.fixture
def lib():
    from opendpd_amd import _lib
    lib = _lib.load()
    yield lib
    for k in ("s16_min_batch", "s16_occupancy", "gp_max_batch", "s16x", "s16x_train", "lstm_pack", "xchg_fused", "qat_u3"):
        lib.odpd_set_tuning(k.encode(), C.c_int64(DEFAULTS.get(k, 1)))


def _set(lib, key, value):
    from opendpd_amd import _lib
    _lib.check(lib.odpd_set_tuning(key.encode(), C.c_int64(value)), f"odpd_set_tuning({key})")


def _net(bb, H, thx, thh, B, T):
    from opendpd_amd import CoreModel
    torch.manual_seed(H * 100 + B + T)
    net = CoreModel(2, H, 1, bb, thx=thx, thh=thh).cuda()
    with torch.no_grad():      # biases are zero after init: make them count
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
    rng = np.random.RandomState(B * 7 + T)
    amp = 0.05 + 0.85 * rng.rand(B, T, 1)
    ph = 2 * np.pi * rng.rand(B, T, 1)
    x = np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)
    return net, x, rng.randn(B, T, 2).astype(np.float32)


def _step(net, x, dy, need_dx):
    """one ordinary forward / backward -> (y, flat parameter gradient, dL/dx or None)"""
    for p in net.parameters():
        p.grad = None
    if getattr(net.backbone, "debug", 0):
        net.backbone.set_debug(1)      # (the delta sparsity counters accumulate: this step's alone)
    xt = torch.from_numpy(x).cuda().requires_grad_(need_dx)
    y = net(xt)
    y.backward(torch.from_numpy(dy).cuda())
    g = np.concatenate([p.grad.cpu().numpy().reshape(-1) for p in net.parameters()])
    return y.detach().cpu().numpy(), g, (xt.grad.cpu().numpy() if need_dx else None)


def _against_the_oracle(bb, H, thx, thh, net, x, dy, out):
    from oracle.oracle import Oracle, make_model
    y, g, dx = out
    o = Oracle("f64")
    m = make_model(bb, H, thx, thh)
    p = np.concatenate([q.detach().cpu().numpy().reshape(-1) for q in net.parameters()]).astype(np.float64)
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    yo, so = o.forward(m, p, x64)
    go, dxo = o.backward(m, p, x64, dy64, need_dx=dx is not None)
    tol_f, tol_g = TOLS[bb]
    if thx or thh:      # (test_delta_family_gpu: a rounding-level difference may flip a threshold decision or two)
        st = net.backbone.statistics
        assert abs(st["num_dx_zeros"] - so[0]) <= 2 and abs(st["num_dh_zeros"] - so[2]) <= 2
        if not (st["num_dx_zeros"] == so[0] and st["num_dh_zeros"] == so[2]):
            tol_f, tol_g = 5e-3, 5e-2
    assert rel_err(y, yo) < tol_f
    assert_grad_blocks(g, go, net_grad_blocks(net), tol_g)
    if dx is not None:
        assert rel_err(dx, dxo) < tol_g


def _ckpt_floats(lib, net, B, T):
    return int(lib.odpd_ckpt_floats(C.byref(net.backbone.desc), B, T))


@pytest.mark.parametrize("bb,H,thx,thh,B,T,knob,values,held,need_dx", FLOAT_ROWS)
def test_knob_flip_between_forward_and_backward(lib, bb, H, thx, thh, B, T, knob, values, held, need_dx):
    for k, v in held.items():
        _set(lib, k, v)
    net, x, dy = _net(bb, H, thx, thh, B, T)
    if thx or thh:
        net.backbone.set_debug(1)      # (the sparsity counters the oracle comparison reads)
    control, sizes = [], []
    for v in values:
        _set(lib, knob, v)
        control.append(_step(net, x, dy, need_dx))
        _against_the_oracle(bb, H, thx, thh, net, x, dy, control[-1])
        sizes.append(_ckpt_floats(lib, net, B, T))
    if knob in UNSIZED:
        # outside the generation: the autograd path does not see the knob at all
        assert sizes[0] == sizes[1] and all(np.array_equal(a, b) for a, b in zip(control[0], control[1]) if a is not None)
    else:
        assert sizes[0] != sizes[1] or not np.array_equal(control[0][1], control[1][1]), "both values select the same kernel here"

    before, after = values
    _set(lib, knob, before)
    for p in net.parameters():
        p.grad = None
    xt = torch.from_numpy(x).cuda().requires_grad_(need_dx)
    y = net(xt)
    _set(lib, knob, after)
    if knob in UNSIZED:
        y.backward(torch.from_numpy(dy).cuda())
        g = np.concatenate([p.grad.cpu().numpy().reshape(-1) for p in net.parameters()])
        assert np.array_equal(g, control[0][1])
        if need_dx:
            assert np.array_equal(xt.grad.cpu().numpy(), control[0][2])
    else:
        with pytest.raises(RuntimeError, match=REFUSED):
            y.backward(torch.from_numpy(dy).cuda())
        assert all(p.grad is None for p in net.parameters()) and xt.grad is None

    # the module stays usable: the next step runs under the new value and matches the oracle
    _against_the_oracle(bb, H, thx, thh, net, x, dy, _step(net, x, dy, need_dx))


@pytest.mark.parametrize("bb,H,B,T", W8A8_ROWS)
def test_qat_u3_flip_between_forward_and_backward(lib, bb, H, B, T):
    """the quantised rows against the oracle the way tests/test_quant_more_gpu.py holds them (grids bit for bit); the slot count changes no
    buffer size, only where each unit sits inside a checkpoint record"""
    from tests.test_quant_more_gpu import _w8a8_against_the_oracle, _w8a8_model
    _set(lib, "s16_min_batch", 0)
    control = []
    for v in (1, 0):
        _set(lib, "qat_u3", v)
        control.append(_w8a8_against_the_oracle(bb, H, B, T))
    assert not np.array_equal(control[0][2], control[1][2]), "three and four unit slots give bit-equal gradients here"

    q, x, dy = _w8a8_model(bb, H, B, T)
    q.train()
    _set(lib, "qat_u3", 1)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    y = q(xt)
    _set(lib, "qat_u3", 0)
    with pytest.raises(RuntimeError, match=REFUSED):
        y.backward(torch.from_numpy(dy).cuda())
    assert all(p.grad is None for p in q.parameters()) and xt.grad is None
    # the same module, under the new value
    after = _w8a8_against_the_oracle(bb, H, B, T, q=q)
    assert np.array_equal(after[2], control[1][2])


def test_refused_delta_backward_leaves_no_dx_flag_behind(lib):
    """delta backbones with x.requires_grad route the forward through ODPD_FLAG_NEED_DX, carried by the descriptor of that one call
    (NativeBackbone.call_desc) and never by the module's own: it is absent there between forward and backward and after a refused backward,
    and the next weight-only step takes the kernels a fresh module would"""
    from opendpd_amd import _lib
    bb, H, thx, thh, B, T = "deltagru", 15, 0.01, 0.05, 19, 65
    net, x, dy = _net(bb, H, thx, thh, B, T)
    net.backbone.set_debug(1)
    _set(lib, "s16_min_batch", NEVER)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    y = net(xt)
    assert not net.backbone.desc.flags & _lib.FLAG_NEED_DX
    _set(lib, "s16_min_batch", 0)
    with pytest.raises(RuntimeError, match=REFUSED):
        y.backward(torch.from_numpy(dy).cuda())
    assert not net.backbone.desc.flags & _lib.FLAG_NEED_DX
    assert all(p.grad is None for p in net.parameters()) and xt.grad is None
    _against_the_oracle(bb, H, thx, thh, net, x, dy, _step(net, x, dy, False))
    _against_the_oracle(bb, H, thx, thh, net, x, dy, _step(net, x, dy, True))
