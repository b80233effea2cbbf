"""Block, chunk and tail edges of the 16-sequences-per-wave GRU kernels (csrc/gru_s16.hip): the fused train step whose forward pass
stops at the last checkpoint and whose L2 loss is its own instantiation, the frozen loss + dL/du launch, and the split kernels on the
batched frame staging.  The fused kernel is forced for every shape as in test_gru_s16_gpu.py (`s16_min_batch` = 0), at one and at two
waves per SIMD; both knobs are restored afterwards.

Shapes.  Frame lengths 1, 2, 3, 4, 5 (below, at and one past the block lengths 2 and 4: no checkpoint at all, a forward pass of zero
steps, a one-step tail block), 31, 32, 33, 34 (the 32-step staging chunk and its neighbours) and 65 (two chunks and a tail); batches
1, 15, 16, 17, 33 (one lane, a ragged group, a full one, one row into a second group, three groups); dgru of 13 (K-packed), 14 and 16
units, gru 11, qgru 10.  Every (model, length, batch) runs once per occupancy; the loss kind and the frame format follow the position in
the grid — kind (iT + iB) % 2, format (iT + 2 iB + iM) % 3 — so that every length and every batch meets both kinds and all three formats
(fp32 (B, T, 2) tensors, frames addressed in place in fp32 streams, the same in bf16 storage) under every model.

Reference and bounds: the CPU oracle's train step, once per case and shared by the two occupancies.  The bounds are those of the existing
S16 oracle tests: 2e-5 on the loss and 2e-5 scale-relative on the flat gradient (test_gru_s16_staging_gpu.py), then every tensor and gate
block on its own maximum at the split tests' 2e-4 (test_gru_family_gpu.py GRAD_TOL, golden_util.assert_grad_blocks); forward 2e-5 and
dL/dx 2e-4 for the split and frozen launches."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden_util import assert_grad_blocks, net_grad_blocks, rel_err

pytestmark = pytest.mark.gpu

MODELS = [("dgru", 13), ("dgru", 14), ("dgru", 16), ("gru", 11), ("qgru", 10)]
LENGTHS = [1, 2, 3, 4, 5, 31, 32, 33, 34, 65]
BATCHES = [1, 15, 16, 17, 33]
KINDS = ["l2", "l1"]
FORMS = ["tensor", "framed", "bf16"]
LOSS_TOL, FLAT_TOL, FWD_TOL, GRAD_TOL = 2e-5, 2e-5, 2e-5, 2e-4


@pytest.fixture(params=[1, 2], ids=["occ1", "occ2"])
def force_s16(request):
    from opendpd_amd import _lib
    lib = _lib.load()
    try:
        assert lib.odpd_set_tuning(b"s16_min_batch", 0) == 0
        assert lib.odpd_set_tuning(b"s16_occupancy", request.param) == 0
        yield request.param
    finally:
        lib.odpd_set_tuning(b"s16_min_batch", -1)
        lib.odpd_set_tuning(b"s16_occupancy", 0)


def _net(bb, H):
    from opendpd_amd import CoreModel
    torch.manual_seed(7)
    net = CoreModel(2, H, 1, bb).cuda()
    with torch.no_grad():      # biases are zero after init: make them count
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
    return net


def _streams(B, T, bf16):
    """I/Q streams and B frame starts (stride 1, shuffled, one frame at sample 0 and one ending on the last sample); bf16: values a bf16 holds"""
    rng = np.random.default_rng(1000 * B + T)
    M = 0 if B == 1 else B + 5
    n = M + T
    x = (rng.uniform(0.05, 0.8, (n, 2)) * rng.choice([-1, 1], (n, 2))).astype(np.float32)
    y = rng.normal(0, 0.3, (n, 2)).astype(np.float32)
    if bf16:
        x, y = (torch.from_numpy(a).to(torch.bfloat16).float().numpy() for a in (x, y))
    order = rng.permutation(M + 1)[:B].astype(np.int64)
    if B > 1:
        order[0], order[1] = M, 0
    return x, y, order, order[:, None] + np.arange(T)[None, :]


_ORACLE = {}


def _oracle_step(bb, H, p0, fx, fy, kind, bf16=False):
    """(loss, gradient) of the oracle's train step at lr 0 without clip on the frames of _streams(B, T, bf16); one computation per case,
    read-only afterwards"""
    from oracle.oracle import Oracle, make_model
    key = (bb, H, fx.shape, kind, bf16)
    if key not in _ORACLE:
        p, ea, eas = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
        scratch = (np.empty_like(fx), np.empty_like(fx), np.empty(p.size, dtype=np.float32))
        lo = Oracle("f32").train_step(make_model(bb, H), p, fx, fy, ea, eas, 1, 0.0, 0.0, kind, scratch)
        g = scratch[2].copy()
        g.setflags(write=False)
        _ORACLE[key] = (lo, g)
    return _ORACLE[key]


def _fused(net, x, t, B, T, kind):
    """one fused step without clip or update: (loss, gradient)"""
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    opt = FusedAdamW(net, lr=0.0, weight_decay=0.0)
    assert opt.train_workspace(B, T, torch.device("cuda", 0)) is not None      # the S16 kernel is the one that runs
    loss = fused_train_step(opt, x, t, kind, 0.0)
    return loss.item(), opt.grad[:-4].cpu().numpy()


def _grid_case(iM, iT, iB):
    return KINDS[(iT + iB) % 2], FORMS[(iT + 2 * iB + iM) % 3]


@pytest.mark.parametrize("iM", range(len(MODELS)), ids=[f"{bb}{H}" for bb, H in MODELS])
def test_fused_step_at_block_chunk_and_tail_edges(force_s16, iM):
    from opendpd_amd.train_funcs import FrameBatch
    bb, H = MODELS[iM]
    net = _net(bb, H)
    blocks = net_grad_blocks(net)
    p0 = net.backbone.flat_params().detach().cpu().numpy().copy()
    seen = set()
    for iT, T in enumerate(LENGTHS):
        for iB, B in enumerate(BATCHES):
            kind, form = _grid_case(iM, iT, iB)
            seen |= {(T, kind), (T, form), (B, kind), (B, form), (kind, form)}
            x, y, order, idx = _streams(B, T, form == "bf16")
            fx, fy = np.ascontiguousarray(x[idx]), np.ascontiguousarray(y[idx])
            lo, go = _oracle_step(bb, H, p0, fx, fy, kind, form == "bf16")
            if form == "tensor":
                lf, gf = _fused(net, torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda(), B, T, kind)
            else:
                xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
                if form == "bf16":
                    xs, ys = xs.to(torch.bfloat16), ys.to(torch.bfloat16)
                lf, gf = _fused(net, FrameBatch(xs, ys, torch.from_numpy(order).cuda(), T, 1), None, B, T, kind)
            el, eg = abs(lf - lo) / max(1.0, lo), rel_err(gf, go)
            print(f"{bb} H{H} T{T} B{B} {kind} {form}: loss err {el:.2e}, flat gradient err {eg:.2e}")
            assert el < LOSS_TOL and eg < FLAT_TOL, (T, B, kind, form, el, eg)
            assert_grad_blocks(gf, go, blocks, GRAD_TOL)
    for v in LENGTHS + BATCHES:
        assert all((v, k) in seen for k in KINDS + FORMS), v
    assert all((k, f) in seen for k in KINDS for f in FORMS)


def _case(bb, H, B, T):
    net = _net(bb, H)
    x, y, _, idx = _streams(B, T, False)
    return net, np.ascontiguousarray(x[idx]), np.ascontiguousarray(y[idx])


@pytest.mark.parametrize("T", [3, 33])
@pytest.mark.parametrize("bb,H", MODELS)
def test_split_path_on_the_same_inputs(force_s16, bb, H, T):
    """odpd_backbone_fwd, loss, odpd_backbone_bwd through autograd: with parameter gradients (and dL/dx), then dL/dx only"""
    from oracle.oracle import Oracle, make_model
    B = 17
    net, fx, fy = _case(bb, H, B, T)
    orc, m = Oracle("f32"), make_model(bb, H)
    p = net.backbone.flat_params().detach().cpu().numpy().copy()
    yo, _ = orc.forward(m, p, fx)
    for kind in KINDS:
        _, dyo = orc.loss(kind, yo, fy)
        go, dxo = orc.backward(m, p, fx, dyo)
        for with_params in (True, False):
            for q in net.parameters():
                q.requires_grad_(with_params)
                q.grad = None
            xt = torch.from_numpy(fx).cuda().requires_grad_(True)
            yt = net(xt)
            loss = (torch.nn.functional.mse_loss if kind == "l2" else torch.nn.functional.l1_loss)(yt, torch.from_numpy(fy).cuda())
            loss.backward()
            ey, ex = rel_err(yt.detach().cpu().numpy(), yo), rel_err(xt.grad.cpu().numpy(), dxo)
            print(f"{bb} H{H} T{T} {kind} params={with_params}: y err {ey:.2e}, dL/dx err {ex:.2e}")
            assert ey < FWD_TOL and ex < GRAD_TOL
            if with_params:
                g = np.concatenate([q.grad.cpu().numpy().reshape(-1) for q in net.parameters()])
                assert_grad_blocks(g, go, net_grad_blocks(net), GRAD_TOL)
            else:
                assert all(q.grad is None for q in net.parameters())


@pytest.mark.parametrize("T", [3, 33])
@pytest.mark.parametrize("bb,H", MODELS)
def test_frozen_loss_and_du_launch(force_s16, bb, H, T):
    from opendpd_amd import _lib
    from oracle.oracle import Oracle, make_model
    lib, B = _lib.load(), 17
    net, fx, fy = _case(bb, H, B, T)
    d, flat = net.backbone.desc, net.backbone.flat_params()
    orc, m = Oracle("f32"), make_model(bb, H)
    p = flat.detach().cpu().numpy().copy()
    yo, _ = orc.forward(m, p, fx)
    rows = int(lib.odpd_frozen_loss_rows(C.byref(d), B, T))
    assert rows > 0
    u, t = torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda()
    ws = torch.empty(max(int(lib.odpd_ckpt_floats(C.byref(d), B, T)), 1), device="cuda")
    for kind in KINDS:
        lo, dyo = orc.loss(kind, yo, fy)
        _, dxo = orc.backward(m, p, fx, dyo)
        du = torch.full_like(u, float("nan"))
        lrows = torch.full((rows, _lib.LOSS_COLS), float("nan"), device="cuda")
        _lib.check(lib.odpd_frozen_loss_dx(_lib.stream_ptr(), C.byref(d), _lib.LOSS_IDS[kind], B, T, B * T * 2, _lib.ptr(flat), _lib.ptr(u),
                                           _lib.ptr(t), _lib.ptr(du), _lib.ptr(lrows), _lib.ptr(ws)), "frozen loss + dL/du")
        lf = lrows[:, 0].double().sum().item() / (B * T * 2)
        el, ex = abs(lf - lo) / max(1.0, lo), rel_err(du.cpu().numpy(), dxo)
        print(f"{bb} H{H} T{T} {kind}: loss err {el:.2e}, dL/du err {ex:.2e}")
        assert el < LOSS_TOL and ex < GRAD_TOL


def test_workspace_of_exactly_the_answered_size(force_s16):
    """odpd_train_fwd_bwd on a workspace of exactly odpd_train_workspace_floats floats inside a larger sentinel-filled tensor: nothing
    is written in front of it or beyond the answered size, and the step is the oracle's"""
    from opendpd_amd import _lib
    lib, (bb, H), B, T = _lib.load(), MODELS[0], 33, 34
    net, fx, fy = _case(bb, H, B, T)
    d, flat = net.backbone.desc, net.backbone.flat_params()
    P = flat.numel()
    n, rows = int(lib.odpd_train_workspace_floats(C.byref(d), B, T)), int(lib.odpd_partial_rows(C.byref(d), B, T, 1))
    assert n > 0 and rows > 0
    pad, sentinel = 1024, -7.25
    big = torch.full((pad + n + pad,), sentinel, device="cuda")
    part = torch.empty(rows, P + _lib.LOSS_COLS, device="cuda")
    grad = torch.empty(P + _lib.LOSS_COLS, device="cuda")
    x, t = torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda()
    st = _lib.stream_ptr()
    _lib.check(lib.odpd_train_fwd_bwd(st, C.byref(d), _lib.LOSS_IDS["l2"], B, T, B * T * 2, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(t),
                                      _lib.ptr(part), _lib.ptr(big[pad:])), "fused step")
    _lib.check(lib.odpd_reduce_partials(st, rows, P, _lib.ptr(part), _lib.ptr(grad), 0), "reduce")
    torch.cuda.synchronize()
    assert bool((big[:pad] == sentinel).all()) and bool((big[pad + n:] == sentinel).all())
    lo, go = _oracle_step(bb, H, flat.detach().cpu().numpy().copy(), fx, fy, "l2")
    lf, gf = grad[P].item() / (B * T * 2), grad[:P].cpu().numpy()
    assert abs(lf - lo) / max(1.0, lo) < LOSS_TOL and rel_err(gf, go) < FLAT_TOL
    assert_grad_blocks(gf, go, net_grad_blocks(net), GRAD_TOL)
