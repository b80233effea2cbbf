"""Block, chunk, tail and group-loop edges of the two siblings of csrc/gru_s16.hip, against the fp64 build of the CPU oracle:
csrc/lstm_s16.hip (lstm16_train_kernel<VD, NT, PK>: lstm and vdlstm of <= 32 units, fused step on tensors) and csrc/gru_s16n.hip (GRU family
of 17 .. 32 units: the fused step, mode 0, and the frozen loss + dL/du launch, mode 3).  Modelled on test_sweeps_s16_blocks_gpu.py, whose
parameters and inputs it uses (seed 7, biases moved to uniform(-0.3, 0.3), |x| in 0.05 .. 0.8 with random sign, targets N(0, 0.3)).

Kernel selection.  `s16_min_batch` = 0 forces the 16-sequences-per-wave kernels for every shape; hidden 17 .. 24 of the GRU family would train on
the bf16 kernels of gru_s16x.hip, so those models run with `s16x` = `s16x_train` = 0; lstm 9 runs K-packed and again with `lstm_pack` = 0.  The
`tune` fixture sets the knobs and restores all four.  Every case asserts has_fused and a workspace (the HBM checkpoints only these kernels use).

Shapes.  lstm and GRU lengths 1, 2, 3, 4, 5 (below, at and one past the checkpoint stride 4: no checkpoint at all, a one-step tail block), 31,
32, 33, 34 (the 32-step staging chunk and its neighbours) and 65 (two chunks and a tail).  vdlstm (stride 2, 3-sample circular halo, T >= 3):
3 (the halo wraps over the whole frame), 4, 5, 6, 7, 31, 32, 33, 35, 64, 65, 67 (35 and 67: a chunk plus the halo).  Batches 1, 15, 16, 17, 33
and 129 (lstm: nine groups, a second eight-wave workgroup with one busy wave) or 65 (GRU: five groups, a second four-wave workgroup).  The loss
kind follows the grid position, (iT + iB) % 2, and for the GRU family the frame format too, (iT + 2 iB + iM) % 3: fp32 tensors, frames addressed
in place in fp32 streams (shuffled starts, one frame at sample 0, one ending on the last sample; stride 3 at T = 33, else 1), the same streams
in bf16 storage with the oracle fed the rounded values.  A wave's second pass over the group loop needs more groups than the chip has waves:
B = 16 * W * CUs + 17 (W = 8 waves per workgroup for lstm / vdlstm of <= 16 units, else 4), at T = 5 (vdlstm 3).

Reference and bounds.  Oracle("f64").train_step at lr 0 without clip (frozen launch: forward + loss + backward), once per case and shared by
the knob settings.  Bounds of the existing S16 oracle tests: 2e-5 on the loss relative to max(1, loss), 2e-5 scale-relative on the flat gradient,
2e-4 on every tensor and gate block on its own maximum (golden_util.assert_grad_blocks; a block whose reference is identically zero stays on the
flat scale), 2e-4 on dL/du.  The fp32 oracle stays below 8e-8 / 2.6e-6 / 3.2e-6 of the fp64 one over these grids; at the second-pass batch its
sequential fp32 sum leaves fc_out.bias under L1 by 1.5e-4, which is why the reference is the fp64 build."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.golden_util import assert_grad_blocks, grad_block_errors, net_grad_blocks, rel_err
from tests.test_sweeps_s16_blocks_gpu import _net      # seed 7, biases moved to uniform(-0.3, 0.3)

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 31, 32, 33, 34, 65]
VD_LENGTHS = [3, 4, 5, 6, 7, 31, 32, 33, 35, 64, 65, 67]
LSTM_BATCHES = [1, 15, 16, 17, 33, 129]
GRU_BATCHES = [1, 15, 16, 17, 33, 65]
KINDS = ["l2", "l1"]
FORMS = ["tensor", "framed", "bf16"]
LOSS_TOL, FLAT_TOL, GRAD_TOL = 2e-5, 2e-5, 2e-4
STRIDE3_AT = 33      # the one length whose framed cases address their streams with stride 3

# (backbone, hidden, lstm_pack): one per instantiation of lstm16_train_kernel<VD, NT, PK> and boundary of its hidden range
LSTM_MODELS = [("lstm", 9, 1), ("lstm", 13, 1), ("lstm", 9, 0), ("lstm", 14, 1), ("lstm", 16, 1), ("lstm", 17, 1), ("lstm", 32, 1),
               ("vdlstm", 8, 1), ("vdlstm", 13, 1), ("vdlstm", 16, 1), ("vdlstm", 20, 1), ("vdlstm", 32, 1)]
# (backbone, hidden, s16x = s16x_train): hidden 17 .. 24 with the bf16 kernels switched off, 25 .. 32 at the defaults
GRU_MODELS = [("gru", 17, 0), ("dgru", 24, 0), ("qgru", 20, 0), ("qgru_amp1", 21, 0), ("dgru", 25, 1), ("qgru_amp1", 29, 1), ("gru", 32, 1),
              ("dgru", 32, 1)]
SECOND_PASS = [("lstm", 9, 1), ("lstm", 9, 0), ("lstm", 14, 1), ("vdlstm", 13, 1), ("vdlstm", 16, 1), ("lstm", 23, 1), ("vdlstm", 20, 1),
               ("dgru", 29, 1), ("gru", 32, 1)]
EXACT_SIZE = [("lstm", 9), ("vdlstm", 16), ("lstm", 23), ("dgru", 29)]
_KNOB_DEFAULTS = {"s16_min_batch": -1, "s16x": 1, "s16x_train": 1, "lstm_pack": 1}


def _ids(models):
    return [f"{bb}{H}" + ("" if k else "-knob0") for bb, H, k in models]


@pytest.fixture
def tune():
    """forces the S16 kernels; yields a setter for the four knobs this module may touch; restores all of them"""
    from opendpd_amd import _lib
    lib = _lib.load()

    def set_knobs(**knobs):
        for k, v in knobs.items():
            assert k in _KNOB_DEFAULTS and lib.odpd_set_tuning(k.encode(), v) == 0
    try:
        set_knobs(s16_min_batch=0)
        yield set_knobs
    finally:
        for k, v in _KNOB_DEFAULTS.items():
            lib.odpd_set_tuning(k.encode(), v)


def _streams(B, T, bf16=False, stride=1):
    """I/Q streams and the indices of B frames (frame f = samples [f stride, f stride + T); shuffled, one frame at sample 0 and one ending on
    the last sample); bf16: values a bf16 holds.  Returns x, y, the frame indices and the (B, T) sample indices of the frames.  At stride 1
    these are the streams of test_sweeps_s16_blocks_gpu.py."""
    rng = np.random.default_rng(1000 * B + T)
    M = 0 if B == 1 else B + 5
    n = M * stride + T
    x = (rng.uniform(0.05, 0.8, (n, 2)) * rng.choice([-1, 1], (n, 2))).astype(np.float32)
    y = rng.normal(0, 0.3, (n, 2)).astype(np.float32)
    if bf16:
        x, y = (torch.from_numpy(a).to(torch.bfloat16).float().numpy() for a in (x, y))
    order = rng.permutation(M + 1)[:B].astype(np.int64)
    if B > 1:
        order[0], order[1] = M, 0
    return x, y, order, stride * order[:, None] + np.arange(T)[None, :]


def _frames(B, T, bf16=False, stride=1):
    x, y, _, idx = _streams(B, T, bf16, stride)
    return np.ascontiguousarray(x[idx]), np.ascontiguousarray(y[idx])


_ORACLE = {}


def _oracle_step(bb, H, p0, fx, fy, kind, tag=()):
    """(loss, gradient) of the fp64 oracle's train step at lr 0 without clip on the frames (fx, fy) — `tag` tells apart inputs of one shape —;
    one computation per case, read-only afterwards"""
    from oracle.oracle import Oracle, make_model
    key = (bb, H, fx.shape, kind, tag)
    if key not in _ORACLE:
        p = p0.astype(np.float64)
        x, y = fx.astype(np.float64), fy.astype(np.float64)
        scratch = (np.empty_like(x), np.empty_like(x), np.empty(p.size, dtype=np.float64))
        lo = Oracle("f64").train_step(make_model(bb, H), p, x, y, np.zeros_like(p), np.zeros_like(p), 1, 0.0, 0.0, kind, scratch)
        assert np.array_equal(p, p0.astype(np.float64))      # lr 0: the step moved nothing
        g = scratch[2].copy()
        g.setflags(write=False)
        _ORACLE[key] = (lo, g)
    return _ORACLE[key]


def _fused(net, x, t, B, T, kind):
    """one fused step without clip or update: (loss, gradient)"""
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    opt = FusedAdamW(net, lr=0.0, weight_decay=0.0)
    assert opt.has_fused(B, T)
    assert opt.train_workspace(B, T, torch.device("cuda", 0)) is not None      # the S16 kernel is the one that runs
    loss = fused_train_step(opt, x, t, kind, 0.0)
    return loss.item(), opt.grad[:-4].cpu().numpy()


class _Worst:
    """the largest loss, flat and per-block error of one test, printed as the baseline of the kernel it ran"""

    def __init__(self, what):
        self.what, self.loss, self.flat, self.block = what, (0.0, "-"), (0.0, "-"), (0.0, "-")

    def check(self, case, lf, gf, lo, go, blocks):
        """prints the case's figures, keeps the largest, then holds the case to the bounds"""
        el, eg = abs(lf - lo) / max(1.0, lo), rel_err(gf, go)
        own = [(e, label) for label, e, _, _ in grad_block_errors(gf, go, blocks) if e is not None]
        eb, label = max(own) if own else (0.0, "-")
        print(f"{self.what} {case}: loss err {el:.2e}, flat gradient err {eg:.2e}, worst block {label} {eb:.2e}")
        self.loss, self.flat, self.block = max(self.loss, (el, case)), max(self.flat, (eg, case)), max(self.block, (eb, f"{label} at {case}"))
        assert el < LOSS_TOL and eg < FLAT_TOL, (self.what, case, el, eg)
        assert_grad_blocks(gf, go, blocks, GRAD_TOL)

    def report(self):
        print(f"WORST {self.what}: loss {self.loss[0]:.2e} ({self.loss[1]}), flat {self.flat[0]:.2e} ({self.flat[1]}), "
              f"block {self.block[0]:.2e} ({self.block[1]})")


def _lstm_instantiation(bb, H, pack):
    return f"lstm16_train_kernel<VD={int(bb == 'vdlstm')}, NT={(H + 15) // 16}, PK={int(H <= 13 and pack != 0)}> {bb} H{H}"


# ---- 1. csrc/lstm_s16.hip: the fused step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iM", range(len(LSTM_MODELS)), ids=_ids(LSTM_MODELS))
def test_lstm_fused_step_at_block_chunk_and_tail_edges(tune, iM):
    bb, H, pack = LSTM_MODELS[iM]
    tune(lstm_pack=pack)
    net = _net(bb, H)
    blocks = net_grad_blocks(net)
    p0 = net.backbone.flat_params().detach().cpu().numpy().copy()
    lengths = VD_LENGTHS if bb == "vdlstm" else LENGTHS
    worst, seen = _Worst(_lstm_instantiation(bb, H, pack)), set()
    for iT, T in enumerate(lengths):
        for iB, B in enumerate(LSTM_BATCHES):
            kind = KINDS[(iT + iB) % 2]
            seen |= {(T, kind), (B, kind)}
            fx, fy = _frames(B, T)
            lo, go = _oracle_step(bb, H, p0, fx, fy, kind)
            lf, gf = _fused(net, torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda(), B, T, kind)
            worst.check(f"T{T} B{B} {kind}", lf, gf, lo, go, blocks)
    worst.report()
    for v in lengths + LSTM_BATCHES:
        assert all((v, k) in seen for k in KINDS), v


# ---- 2. csrc/gru_s16n.hip: the fused step and the frozen loss + dL/du launch --------------------------------------------------------------
@pytest.mark.parametrize("iM", range(len(GRU_MODELS)), ids=_ids(GRU_MODELS))
def test_gru_s16n_fused_step_at_block_chunk_and_tail_edges(tune, iM):
    from opendpd_amd.train_funcs import FrameBatch
    bb, H, x3 = GRU_MODELS[iM]
    tune(s16x=x3, s16x_train=x3)
    net = _net(bb, H)
    blocks = net_grad_blocks(net)
    p0 = net.backbone.flat_params().detach().cpu().numpy().copy()
    worst, seen = _Worst(f"gru16n_kernel fused {bb} H{H}"), set()
    for iT, T in enumerate(LENGTHS):
        for iB, B in enumerate(GRU_BATCHES):
            kind, form = KINDS[(iT + iB) % 2], FORMS[(iT + 2 * iB + iM) % 3]
            seen |= {(T, kind), (T, form), (B, kind), (B, form), (kind, form)}
            stride = 3 if form != "tensor" and T == STRIDE3_AT else 1
            x, y, order, idx = _streams(B, T, form == "bf16", stride)
            fx, fy = np.ascontiguousarray(x[idx]), np.ascontiguousarray(y[idx])
            lo, go = _oracle_step(bb, H, p0, fx, fy, kind, (form == "bf16", stride))
            if form == "tensor":
                lf, gf = _fused(net, torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda(), B, T, kind)
            else:
                xs, ys = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
                if form == "bf16":
                    xs, ys = xs.to(torch.bfloat16), ys.to(torch.bfloat16)
                lf, gf = _fused(net, FrameBatch(xs, ys, torch.from_numpy(order).cuda(), T, stride), None, B, T, kind)
            worst.check(f"T{T} B{B} {kind} {form}" + (" stride 3" if stride == 3 else ""), lf, gf, lo, go, blocks)
    worst.report()
    for v in LENGTHS + GRU_BATCHES:
        assert all((v, k) in seen for k in KINDS + FORMS), v
    assert all((k, f) in seen for k in KINDS for f in FORMS)


@pytest.mark.parametrize("T", [3, 33])
@pytest.mark.parametrize("bb,H,x3", GRU_MODELS, ids=_ids(GRU_MODELS))
def test_gru_s16n_frozen_loss_and_du_launch(tune, bb, H, x3, T):
    from opendpd_amd import _lib
    from oracle.oracle import Oracle, make_model
    tune(s16x=x3, s16x_train=x3)
    lib, B = _lib.load(), 17
    net = _net(bb, H)
    fx, fy = _frames(B, T)
    d, flat = net.backbone.desc, net.backbone.flat_params()
    orc, m = Oracle("f64"), make_model(bb, H)
    p = flat.detach().cpu().numpy().astype(np.float64)
    yo, _ = orc.forward(m, p, fx)
    rows = int(lib.odpd_frozen_loss_rows(C.byref(d), B, T))
    assert rows == 1      # two 16-sequence groups: one workgroup
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
        print(f"gru16n_kernel frozen {bb} H{H} T{T} B{B} {kind}: loss err {el:.2e}, dL/du err {ex:.2e}")
        assert el < LOSS_TOL and ex < GRAD_TOL


# ---- 3. a wave's second pass over the group loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bb,H,pack", SECOND_PASS, ids=_ids(SECOND_PASS))
def test_second_group_of_a_wave(tune, bb, H, pack, kind):
    """the smallest batch at which the grid-stride loop over 16-sequence groups runs twice in a wave: every workgroup the chip takes, each
    wave busy, and two groups more — a full one and one of a single sequence, for waves 0 and 1 of the first workgroup.  The accumulators and
    the two transpose tiles zeroed in front of that loop carry over; T = 5 (vdlstm 3) gives one full block and a one-step tail per group."""
    from opendpd_amd import _lib
    tune(lstm_pack=pack)
    lstm = bb in ("lstm", "vdlstm")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, T = 16 * (8 if lstm and H <= 16 else 4) * cus + 17, 3 if bb == "vdlstm" else 5
    net = _net(bb, H)
    assert int(_lib.load().odpd_partial_rows(C.byref(net.backbone.desc), B, T, 1)) == cus
    p0 = net.backbone.flat_params().detach().cpu().numpy().copy()
    fx, fy = _frames(B, T)
    lo, go = _oracle_step(bb, H, p0, fx, fy, kind)
    lf, gf = _fused(net, torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda(), B, T, kind)
    worst = _Worst(f"second pass {_lstm_instantiation(bb, H, pack) if lstm else f'gru16n_kernel fused {bb} H{H}'}")
    try:
        worst.check(f"T{T} B{B} {kind}", lf, gf, lo, go, net_grad_blocks(net))
    finally:
        worst.report()


# ---- 4. buffers of exactly the answered sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bb,H", EXACT_SIZE)
def test_workspace_and_rows_of_exactly_the_answered_sizes(tune, bb, H):
    """odpd_train_fwd_bwd on a workspace of exactly odpd_train_workspace_floats floats and on exactly odpd_partial_rows rows (pre-filled with
    NaN), each inside a larger sentinel-filled tensor: nothing is written in front of or beyond either, every element of the rows is
    written, and the reduced step is the oracle's"""
    from opendpd_amd import _lib
    lib, B, T = _lib.load(), 33, 34
    net = _net(bb, H)
    fx, fy = _frames(B, T)
    d, flat = net.backbone.desc, net.backbone.flat_params()
    P = flat.numel()
    n, rows = int(lib.odpd_train_workspace_floats(C.byref(d), B, T)), int(lib.odpd_partial_rows(C.byref(d), B, T, 1))
    assert n > 0 and rows > 0
    pad, sentinel, nrow = 1024, -7.25, rows * (P + _lib.LOSS_COLS)
    x, t = torch.from_numpy(fx).cuda(), torch.from_numpy(fy).cuda()
    st = _lib.stream_ptr()
    for kind in KINDS:
        big = torch.full((pad + n + pad,), sentinel, device="cuda")
        rbig = torch.full((pad + nrow + pad,), sentinel, device="cuda")
        part = rbig[pad:pad + nrow]
        part.fill_(float("nan"))
        grad = torch.empty(P + _lib.LOSS_COLS, device="cuda")
        _lib.check(lib.odpd_train_fwd_bwd(st, C.byref(d), _lib.LOSS_IDS[kind], B, T, B * T * 2, _lib.ptr(flat), _lib.ptr(x), _lib.ptr(t),
                                          _lib.ptr(part), _lib.ptr(big[pad:])), "fused step")
        torch.cuda.synchronize()
        assert bool((big[:pad] == sentinel).all()) and bool((big[pad + n:] == sentinel).all())
        assert bool((rbig[:pad] == sentinel).all()) and bool((rbig[pad + nrow:] == sentinel).all())
        assert bool(torch.isfinite(part).all())
        _lib.check(lib.odpd_reduce_partials(st, rows, P, _lib.ptr(part), _lib.ptr(grad), 0), "reduce")
        lo, go = _oracle_step(bb, H, flat.detach().cpu().numpy().copy(), fx, fy, kind)
        lf, gf = grad[P].item() / (B * T * 2), grad[:P].cpu().numpy()
        _Worst(f"exact-size buffers {bb} H{H}").check(f"T{T} B{B} {kind}", lf, gf, lo, go, net_grad_blocks(net))
