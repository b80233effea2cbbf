"""Frame staging of the 16-sequences-per-wave fused GRU train kernel (csrc/gru_s16.hip, gru16_train_body; csrc/odpd_seq.h stage_rows /
stage_issue / stage_commit): the row offsets of a wave's 16 frames are fetched once per group and the samples of a chunk — x and the target
together in the backward pass — are loaded as one batch.  The kernel is forced for every shape as in test_gru_s16_gpu.py (`s16_min_batch`),
at one and at two waves per SIMD.

Shapes: batches that are not a multiple of 16 (1, 17, 33: one lane, one row into the second group, three groups) and frame lengths below, at
and above the 4-step checkpoint block and the 32-step chunk (1, 5, 31, 32, 33, 65, 200).  Frames are windows of a resident stream in a
shuffled order that repeats one index, with frame strides 1 and 3; one frame starts at sample 0 and one ends on the stream's last sample.
The bound is the project's fp32 one (2e-5 on the loss, 2e-5 scale-relative on the gradient: sums in a different order than the oracle)."""
import numpy as np
import pytest
import torch

from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu

MODELS = [("dgru", 13), ("gru", 11)]
BATCHES = [1, 17, 33]
LENGTHS = [1, 5, 31, 32, 33, 65, 200]


@pytest.fixture(params=[1, 2], ids=["occ1", "occ2"])
def force_s16(request):
    from opendpd_amd import _lib
    lib = _lib.load()
    assert lib.odpd_set_tuning(b"s16_min_batch", 0) == 0
    assert lib.odpd_set_tuning(b"s16_occupancy", request.param) == 0
    yield request.param
    lib.odpd_set_tuning(b"s16_min_batch", -1)
    lib.odpd_set_tuning(b"s16_occupancy", 0)


def _frames(B, T, stride, seed=0):
    """streams of exactly (M * stride + T) samples and B frame starts out of 0 .. M: shuffled, with start 0, start M (that frame ends on the
    last sample) and — from three frames on — one index twice"""
    rng = np.random.default_rng(seed + 1000 * B + T)
    M = 0 if B == 1 else B + 5
    n = M * stride + T
    x = (rng.uniform(0.05, 0.8, (n, 2)) * rng.choice([-1, 1], (n, 2))).astype(np.float32)
    y = rng.normal(0, 0.3, (n, 2)).astype(np.float32)
    order = rng.permutation(M + 1)[:B].astype(np.int64)
    if B > 1:
        pos = rng.permutation(B)
        order[pos[0]], order[pos[1]] = 0, M
        order[pos[2]] = order[pos[3]]
        assert len(set(order.tolist())) < B
    idx = order[:, None] * stride + np.arange(T)[None, :]
    assert idx.min() == 0 and idx.max() == n - 1
    return x, y, order, idx


def _net(bb, H):
    from opendpd_amd import CoreModel
    torch.manual_seed(7)
    net = CoreModel(2, H, 1, bb).cuda()
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
    return net


def _step(net, x, t, B, T, prefill=None):
    """one fused step without clip or update: (loss, gradient) as device tensors"""
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    opt = FusedAdamW(net, lr=0.0, weight_decay=0.0)
    assert opt.train_workspace(B, T, torch.device("cuda", 0)) is not None      # the S16 kernel is the one that runs
    if prefill is not None:
        opt.partials(B, T, torch.device("cuda", 0)).fill_(prefill)
        opt.grad.fill_(prefill)
    loss = fused_train_step(opt, x, t, "l2", 0.0)
    return loss.clone(), opt.grad[:-4].clone()


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("bb,H", MODELS)
def test_framed_step_against_oracle_and_materialised_frames(force_s16, bb, H, B, stride):
    """Every frame length: the step on a FrameBatch against the CPU oracle's train step (loss, gradient), and torch.equal to the same frames
    given as (B, T, 2) tensors."""
    from opendpd_amd.train_funcs import FrameBatch
    from oracle.oracle import Oracle, make_model
    net = _net(bb, H)
    orc, m = Oracle("f32"), make_model(bb, H)
    p0 = net.backbone.flat_params().detach().cpu().numpy().copy()
    for T in LENGTHS:
        x, y, order, idx = _frames(B, T, stride)
        xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        lf, gf = _step(net, FrameBatch(xs, ys, torch.from_numpy(order).cuda(), T, stride), None, B, T)
        fx, fy = np.ascontiguousarray(x[idx]), np.ascontiguousarray(y[idx])
        p, ea, eas = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
        scratch = (np.empty_like(fx), np.empty_like(fx), np.empty(p.size, dtype=np.float32))
        lo = orc.train_step(m, p, fx, fy, ea, eas, 1, 0.0, 0.0, "l2", scratch)      # lr 0, no clip: scratch[2] is the gradient
        el, eg = abs(lf.item() - lo) / max(1.0, lo), rel_err(gf.cpu().numpy(), scratch[2])
        print(f"{bb} H{H} B{B} T{T} stride{stride}: loss err {el:.2e}, gradient err {eg:.2e}")
        assert el < 2e-5 and eg < 2e-5, (T, el, eg)
        lm, gm = _step(net, torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda(), B, T)
        assert torch.equal(lf, lm) and torch.equal(gf, gm), T


@pytest.mark.parametrize("B,T,stride", [(1, 1, 1), (17, 33, 3), (33, 65, 1), (33, 200, 3)])
@pytest.mark.parametrize("bb,H", MODELS)
def test_bf16_streams_equal_the_fp32_step_on_the_widened_values(force_s16, bb, H, B, T, stride):
    from opendpd_amd.train_funcs import FrameBatch
    net = _net(bb, H)
    x, y, order, _ = _frames(B, T, stride, seed=1)
    xb, yb = torch.from_numpy(x).cuda().to(torch.bfloat16), torch.from_numpy(y).cuda().to(torch.bfloat16)
    od = torch.from_numpy(order).cuda()
    lb, gb = _step(net, FrameBatch(xb, yb, od, T, stride), None, B, T)
    lw, gw = _step(net, FrameBatch(xb.float(), yb.float(), od, T, stride), None, B, T)
    assert torch.isfinite(gb).all() and torch.equal(lb, lw) and torch.equal(gb, gw)


@pytest.mark.parametrize("B,T", [(1, 5), (17, 32), (33, 200)])
@pytest.mark.parametrize("bb,H", MODELS)
def test_partials_and_gradient_are_overwritten(force_s16, bb, H, B, T):
    """partial rows and the gradient buffer pre-filled with NaN come back finite and equal to a clean run"""
    from opendpd_amd.train_funcs import FrameBatch
    net = _net(bb, H)
    x, y, order, _ = _frames(B, T, 1, seed=2)
    fb = FrameBatch(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(order).cuda(), T, 1)
    l0, g0 = _step(net, fb, None, B, T)
    l1, g1 = _step(net, fb, None, B, T, prefill=float("nan"))
    assert torch.isfinite(l1) and torch.isfinite(g1).all()
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
