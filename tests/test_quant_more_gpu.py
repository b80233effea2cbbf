"""GPU parity of the general quantisation-aware kernels (csrc/qat_s16.hip): gru / dgru through the GRU swap, qgru beyond 16 hidden
units, deltagru_tcnskip (the OpenDPDv2 QAT stage) — against vectors produced by RUNNING the reference's surgery
(oracle/gen_golden_quant_more.py) and against the oracle on ragged shapes.  8-bit grids: bit-exact (deltagru_tcnskip adds its
float skip path to the grid-valued fc_out result: 1 ulp of that sum, three orders below one grid step); 16-bit grids: one LSB."""
import numpy as np
import pytest
import torch

from tests.golden_util import Fixture, assert_grad_blocks, net_grad_blocks, rel_err
from tests.test_oracle_golden import QAT_MORE, qat_param_names

pytestmark = pytest.mark.gpu


class _Proj:
    quant = True
    pretrained_model = ""


def _fresh(bb, H, bits, thx=0.0, thh=0.0):
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import get_quant_model
    _Proj.n_bits_w = _Proj.n_bits_a = bits
    return get_quant_model(_Proj, CoreModel(2, H, 1, bb, thx=thx, thh=thh))


def _qmodel(fx, bb, bits, prefix="sd"):
    q = _fresh(bb, fx.meta["hidden"], bits, fx.meta["thx"], fx.meta["thh"])
    q.load_state_dict({k: torch.from_numpy(fx[f"{prefix}/" + k]) for k in fx.keys(prefix)})
    return q.cuda()


def _stats(q):
    s = q.backbone.statistics
    return np.array([s["num_dx_zeros"], s["num_dx_numel"], s["num_dh_zeros"], s["num_dh_numel"]])


@pytest.mark.parametrize("name,bb,bits", QAT_MORE)
def test_forward_train_eval_match_the_reference(name, bb, bits):
    fx = Fixture(name)
    tres = bb == "deltagru_tcnskip"
    tol = (2.5e-7 if tres else 0.0) if bits == 8 else 2.0 ** -12
    x = torch.from_numpy(fx["x"]).cuda()
    for prefix, ytr, yev in (("sd", "y", "y_eval"), ("sd3", "y_p3_train", "y_p3_eval")):
        q = _qmodel(fx, bb, bits, prefix)
        q.train()
        if tres:
            q.backbone.set_debug(1)
        with torch.no_grad():
            yt = q(x).cpu().numpy()
        if tres and prefix == "sd":      # exact sparsity counters of the train-mode forward
            assert np.abs(_stats(q) - fx["stats"]).max() <= (0 if bits == 8 else 2), (_stats(q), fx["stats"])
        q.eval()
        with torch.no_grad():
            ye = q(x).cpu().numpy()
        assert np.abs(yt - fx[ytr]).max() <= tol, (prefix, np.abs(yt - fx[ytr]).max())
        assert np.abs(ye - fx[yev]).max() <= tol, (prefix, np.abs(ye - fx[yev]).max())
    # config-shaped frames (T = 200), eval mode
    q = _qmodel(fx, bb, bits)
    q.eval()
    if tres:
        q.backbone.set_debug(1)
    with torch.no_grad():
        ya = q(torch.from_numpy(fx["xa"]).cuda()).cpu().numpy()
    if bits == 8:
        assert np.abs(ya - fx["ya_eval"]).max() <= tol
        if tres:
            assert np.array_equal(_stats(q), fx["stats_a"])
    else:   # 16-bit grids: a flipped threshold decision sends THAT sequence onto another trajectory (as between two reference builds)
        bad = np.abs(ya - fx["ya_eval"]).reshape(ya.shape[0], -1).max(1) > 2.0 ** -11
        flips = np.abs(_stats(q) - fx["stats_a"]).max() if tres else 0
        assert bad.sum() <= flips, (bad, flips)


@pytest.mark.parametrize("name,bb,bits", QAT_MORE)
def test_gradients_and_trajectory(name, bb, bits):
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    fx = Fixture(name)
    q = _qmodel(fx, bb, bits)
    q.train()
    x = torch.from_numpy(fx["x"]).cuda().requires_grad_(True)
    t = torch.from_numpy(fx["tgt"]).cuda()
    loss = torch.nn.functional.mse_loss(q(x), t)
    loss.backward()
    assert abs(loss.item() - fx["losses"][0]) < (2e-6 if bits == 8 else 1e-4)
    tol = 2e-5 if bits == 8 else 3e-3
    for k, p in q.named_parameters():
        if ("g/" + k) in fx:
            assert rel_err(p.grad.cpu().numpy(), fx["g/" + k]) < tol or np.abs(fx["g/" + k]).max() == 0, k
            if "scale" in k:
                assert float(p.grad.abs().max()) == 0.0
    assert rel_err(x.grad.cpu().numpy(), fx["gx"]) < tol
    names = qat_param_names(fx)
    opt = FusedAdamW(q, lr=fx.meta["lr"])
    xd = x.detach()
    for s in range(1, 4):
        l = fused_train_step(opt, xd, t, "l2", fx.meta["clip"])
        assert abs(l.item() - fx["losses"][s - 1]) < (2e-6 if bits == 8 else 1e-4)
        got = np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in q.parameters()])
        assert rel_err(got, fx.flat(f"p{s}", names)) < (3e-6 if bits == 8 else 1e-4), s


def _signal(B, T, seed):
    rng = np.random.RandomState(seed)
    amp = 0.05 + 0.85 * rng.rand(B, T, 1)
    ph = 2 * np.pi * rng.rand(B, T, 1)
    # a slowly varying component so that thresholded deltas see both kept and dropped samples
    amp = 0.5 * amp + 0.5 * np.repeat(amp[:, ::4], 4, axis=1)[:, :T]
    x = np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)
    return x, rng.randn(B, T, 2).astype(np.float32)


RAGGED = [("gru", 11, 3, 5), ("gru", 16, 7, 33), ("gru", 23, 17, 40), ("gru", 32, 5, 66),
          ("dgru", 13, 5, 37), ("dgru", 8, 33, 21), ("dgru", 23, 18, 35), ("dgru", 30, 3, 70),
          ("qgru", 10, 19, 63), ("qgru", 20, 6, 33), ("qgru", 30, 35, 17), ("qgru_amp1", 20, 7, 50), ("qgru_amp1", 17, 16, 9),
          ("deltagru_tcnskip", 15, 5, 37), ("deltagru_tcnskip", 9, 34, 50), ("deltagru_tcnskip", 16, 3, 130),
          ("deltagru_tcnskip", 24, 7, 45), ("deltagru_tcnskip", 30, 19, 33)]


@pytest.mark.parametrize("bb,H,B,T", RAGGED)
def test_w8a8_matches_the_oracle_on_ragged_sizes(bb, H, B, T):
    """Forward bit for bit (train and eval mode), weight gradients and dL/dx — together, and dL/dx alone (frozen model = the PA of a
    cascade) — against the oracle, at hidden sizes on both sides of the 16-unit tile boundary."""
    _w8a8_against_the_oracle(bb, H, B, T)


# hidden <= 12 on the 16-sequences-per-wave kernels: THREE unit slots per lane (csrc/qat_s16.hip q16_unit; hidden 10 = the reference's QGRU,
# quant_mp_dpd.sh:43; 6 and 9 from quant_qgru_dpd_regr.sh:74; dgru 8 = every script's PA size)
U3 = [("qgru", 10, 35, 63), ("qgru", 8, 17, 40), ("qgru_amp1", 5, 33, 21), ("qgru", 6, 7, 33), ("qgru", 9, 16, 50), ("qgru", 12, 3, 21), ("qgru_amp1", 12, 19, 40), ("qgru_amp1", 1, 5, 9),
      ("gru", 11, 21, 37), ("gru", 4, 5, 9), ("dgru", 8, 33, 21), ("dgru", 12, 18, 35), ("dgru", 3, 2, 70)]


@pytest.mark.parametrize("bb,H,B,T", U3)
def test_three_unit_slots_per_lane_match_the_oracle_and_the_four_slot_kernels(bb, H, B, T):
    """The three-slot kernels (default) and the four-slot ones they replace at hidden <= 12 (knob "qat_u3" = 0), both forced onto the S16 mapping
    at a ragged batch: each against the oracle (forward bit for bit, gradients and dL/dx at the ragged test's bounds), and the two forwards
    against each other bit for bit (the gradients differ by the order of the unit sums of the data-gradient mat-vecs)."""
    import ctypes as C
    from opendpd_amd import _lib
    lib = _lib.load()
    got = []
    try:
        _lib.check(lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(0)), "set_tuning")
        for knob in (1, 0):
            _lib.check(lib.odpd_set_tuning(b"qat_u3", C.c_int64(knob)), "set_tuning")
            got.append(_w8a8_against_the_oracle(bb, H, B, T))
    finally:
        lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1))
        lib.odpd_set_tuning(b"qat_u3", C.c_int64(1))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert rel_err(got[0][2], got[1][2]) < 2e-5 and rel_err(got[0][3], got[1][3]) < 2e-5


@pytest.mark.parametrize("bb,H", [("qgru", 10), ("dgru", 8), ("gru", 11), ("qgru_amp1", 6)])
def test_three_unit_slots_on_16_bit_grids_agree_with_four_to_the_summation_order(bb, H):
    """W16A16 (the table-free build: fp32 MFMAs, fp32 gates): the unit sums of the mat-vecs run in a different order on the three-slot layout,
    visible at one LSB of the 16-bit grids — the bound the fixtures of the reference itself are held to (2^-12, test_forward_train_eval_...)."""
    import ctypes as C
    from opendpd_amd import _lib
    lib = _lib.load()
    torch.manual_seed(H)
    q = _fresh(bb, H, 16).cuda()
    x, dy = _signal(37, 41, 9)
    outs = []
    try:
        _lib.check(lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(0)), "set_tuning")
        for knob in (1, 0):
            _lib.check(lib.odpd_set_tuning(b"qat_u3", C.c_int64(knob)), "set_tuning")
            for v in q.parameters():
                v.grad = None
            q.train()
            xt = torch.from_numpy(x).cuda().requires_grad_(True)
            y = q(xt)
            y.backward(torch.from_numpy(dy).cuda())
            outs.append((y.detach().cpu().numpy(), np.concatenate([(v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy().reshape(-1)
                                                                   for v in q.parameters()]), xt.grad.cpu().numpy()))
    finally:
        lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1))
        lib.odpd_set_tuning(b"qat_u3", C.c_int64(1))
    assert np.abs(outs[0][0] - outs[1][0]).max() <= 2.0 ** -12
    assert rel_err(outs[0][1], outs[1][1]) < 1e-3 and rel_err(outs[0][2], outs[1][2]) < 1e-3


def _w8a8_model(bb, H, B, T):
    """the seeded W8A8 model of _w8a8_against_the_oracle and its (x, dy)"""
    tres = bb == "deltagru_tcnskip"
    thx, thh = (0.01, 0.05) if tres else (0.0, 0.0)
    torch.manual_seed(H + B + T)
    q = _fresh(bb, H, 8, thx, thh).cuda()
    with torch.no_grad():      # biases and scales off their defaults: clamps and pass masks get exercised
        g = torch.Generator().manual_seed(H)
        for k, p in q.named_parameters():
            if k.endswith("bias"):
                p.copy_(((torch.rand(p.shape, generator=g) - 0.5) * 0.6).cuda())
            elif k.endswith("weight") and p.dim() == 2:
                p.mul_(1.7)
    x, dy = _signal(B, T, B + T)
    return q, x, dy


def _w8a8_against_the_oracle(bb, H, B, T, q=None):
    """`q`: a model _w8a8_model made for these arguments (default: a fresh one); its parameters come out frozen"""
    from oracle.oracle import Oracle, make_model
    tres = bb == "deltagru_tcnskip"
    thx, thh = (0.01, 0.05) if tres else (0.0, 0.0)
    if q is None:
        q, x, dy = _w8a8_model(bb, H, B, T)
    else:
        x, dy = _signal(B, T, B + T)
    o = Oracle("f32")
    m = make_model(bb, H, thx, thh, bits_w=8, bits_a=8)
    p = np.concatenate([v.detach().cpu().numpy().reshape(-1) for v in q.parameters()])
    assert o.param_count(m) == p.size
    tol = 2.5e-7 if tres else 0.0
    q.eval()
    with torch.no_grad():
        ye = q(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.abs(ye - o.qat_forward(m, p, x, eval_mode=True)).max() <= tol
    q.train()
    if tres:
        q.backbone.set_debug(1)
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    y = q(xt)
    st = np.zeros(4)
    yo = o.qat_forward(m, p, x, stats=st)
    assert np.abs(y.detach().cpu().numpy() - yo).max() <= tol
    if tres:
        assert np.array_equal(_stats(q), st)
    y.backward(torch.from_numpy(dy).cuda())
    go, dxo = o.qat_backward(m, p, x, dy, need_dx=True)
    g = np.concatenate([(v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy().reshape(-1) for v in q.parameters()])
    assert_grad_blocks(g, go, net_grad_blocks(q, H), 3e-5, exact_zeros=True)      # every parameter tensor and gate on its own scale
    assert rel_err(xt.grad.cpu().numpy(), dxo) < 3e-5
    for v in q.parameters():
        v.requires_grad_(False)
    xt2 = torch.from_numpy(x).cuda().requires_grad_(True)
    q(xt2).backward(torch.from_numpy(dy).cuda())
    assert rel_err(xt2.grad.cpu().numpy(), dxo) < 3e-5
    return ye, y.detach().cpu().numpy(), g, xt.grad.cpu().numpy()


@pytest.mark.parametrize("bb,H", [("qgru", 10), ("qgru_amp1", 16)])
def test_both_kernel_mappings_agree_bitwise(bb, H):
    """qgru / qgru_amp1 at hidden <= 16 are served by the row-rotated kernels at small batches and by the 16-sequences-per-wave
    kernels at large ones: same outputs bit for bit, same gradients up to summation order."""
    import ctypes as C
    from opendpd_amd import _lib
    lib = _lib.load()
    torch.manual_seed(3)
    q = _fresh(bb, H, 8).cuda()
    x, dy = _signal(37, 41, 9)
    outs = []
    try:
        for min_batch in (1 << 30, 0):
            _lib.check(lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(min_batch)), "set_tuning")
            for v in q.parameters():
                v.grad = None
            q.train()
            y = q(torch.from_numpy(x).cuda())
            y.backward(torch.from_numpy(dy).cuda())
            outs.append((y.detach().cpu().numpy(), np.concatenate([(v.grad if v.grad is not None else torch.zeros_like(v)).cpu().numpy().reshape(-1)
                                                                   for v in q.parameters()])))
    finally:
        lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert rel_err(outs[0][1], outs[1][1]) < 2e-5


def test_openDPDv2_quantisation_stage_from_a_float_checkpoint(tmp_path):
    """bash_scripts/OpenDPDv2.sh:84-117 in small: a float deltagru_tcnskip checkpoint -> `--quant --n_bits_w 16 --n_bits_a 16
    --pretrained_model ...` -> the quantised model's outputs equal the reference's (to one 2^-14 LSB of its output grid)."""
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import get_quant_model
    fx = Fixture("quant_tres_h15_w16a16_pre")
    pre = tmp_path / "float.pt"
    torch.save({k: torch.from_numpy(fx["pre/" + k]) for k in fx.keys("pre")}, pre)

    class P:
        quant = True
        n_bits_w = n_bits_a = 16
        pretrained_model = str(pre)
    torch.manual_seed(0)
    fnet = CoreModel(2, 15, 1, "deltagru_tcnskip", thx=fx.meta["thx"], thh=fx.meta["thh"])
    torch.manual_seed(123)
    q = get_quant_model(P, fnet).cuda()
    q.eval()
    with torch.no_grad():
        y = q(torch.from_numpy(fx["x"]).cuda()).cpu().numpy()
    assert np.abs(y - fx["y_eval"]).max() <= 2.0 ** -12


def _fused_equals_split(bb, H, bits, B, T, expect_one_launch):
    import ctypes as C
    from opendpd_amd import _lib
    from opendpd_amd.train_funcs import FrameBatch, FusedAdamW, fused_train_step
    lib = _lib.load()
    tres = bb == "deltagru_tcnskip"
    torch.manual_seed(B)
    q = _fresh(bb, H, bits, *((0.01, 0.05) if tres else (0.0, 0.0))).cuda()
    q.train()
    g = torch.Generator(device="cuda").manual_seed(B + T)
    xs = (torch.rand(B + T - 1, 2, device="cuda", generator=g) - 0.5) * 1.4
    xs = (xs + 0.05 * torch.sign(xs)).contiguous()
    ys = (torch.rand(B + T - 1, 2, device="cuda", generator=g) - 0.5).contiguous()
    order = torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()
    x = torch.stack([xs[int(o):int(o) + T] for o in order]).contiguous()
    t = torch.stack([ys[int(o):int(o) + T] for o in order]).contiguous()
    q.eval()      # an evaluation pass first (net_eval between the epochs): the mode flag it leaves on the descriptor must not pick the step's kernels
    with torch.no_grad():
        q(x)
    q.train()
    opt = FusedAdamW(q, lr=0.0, weight_decay=0.0)
    assert opt.has_fused(B, T)
    one_launch = int(lib.odpd_train_workspace_floats(C.byref(q.backbone.desc), B, T)) == 0
    assert one_launch == expect_one_launch
    if one_launch:
        assert int(lib.odpd_partial_rows(C.byref(q.backbone.desc), B, T, 1)) == B      # one frame per single-wave workgroup
    for kind, fn in (("l2", torch.nn.functional.mse_loss), ("l1", torch.nn.functional.l1_loss)):
        for p in q.parameters():
            p.grad = None
        if tres:
            q.backbone.set_debug(1)
        loss = fn(q(x), t)
        loss.backward()
        st_ref = _stats(q) if tres else None
        gref = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in q.parameters()]).cpu().numpy()
        for inp, tgt in ((x, t), (FrameBatch(xs, ys, order, T, 1), None)):
            if tres:
                q.backbone.set_debug(1)
            lf = fused_train_step(opt, inp, tgt, kind, 0.0)
            assert abs(lf.item() - loss.item()) < 2e-6 * max(1.0, abs(loss.item())), kind
            assert rel_err(opt.grad[:-4].cpu().numpy(), gref) < 2e-5, kind
            if tres and one_launch:      # the one-launch step counts the forward pass's delta statistics as the module's forward does
                assert np.array_equal(_stats(q), st_ref)


@pytest.mark.parametrize("bb,H,bits,B,T", [("qgru", 20, 8, 37, 41), ("gru", 11, 8, 5, 66), ("dgru", 13, 8, 19, 33), ("deltagru_tcnskip", 15, 8, 21, 50),
                                            ("deltagru_tcnskip", 24, 16, 7, 35), ("qgru_amp1", 10, 16, 33, 20)])
def test_fused_train_step_equals_the_split_chain(bb, H, bits, B, T):
    """odpd_train_fwd_bwd on a quantised model (sixteen sequences per wave) = forward-with-checkpoints launch + backward launch that forms the
    output, the loss and dL/dy inside (no y / dy round trip, no loss kernel): same loss and gradients as autograd through the split kernels
    (L2 and L1), also with the batch given as frames of resident streams."""
    import ctypes as C
    from opendpd_amd import _lib
    lib = _lib.load()
    lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(0))
    try:
        _fused_equals_split(bb, H, bits, B, T, False)
    finally:
        lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1))


@pytest.mark.parametrize("bb,H,bits,B,T", [("qgru", 10, 8, 64, 50), ("qgru", 20, 8, 37, 41), ("gru", 11, 8, 5, 66), ("gru", 30, 16, 9, 40),
                                            ("qgru_amp1", 16, 16, 33, 20), ("qgru_amp1", 10, 8, 256, 200),
                                            ("deltagru_tcnskip", 15, 8, 64, 200), ("deltagru_tcnskip", 9, 16, 7, 35), ("deltagru_tcnskip", 16, 8, 300, 33),
                                            ("dgru", 13, 8, 19, 33), ("dgru", 13, 8, 256, 200), ("dgru", 23, 8, 64, 50), ("dgru", 16, 16, 33, 20), ("dgru", 32, 8, 7, 70),
                                            ("dgru", 1, 8, 3, 5), ("dgru", 17, 16, 5, 131)])
def test_one_launch_train_step_at_the_reference_batch_sizes(bb, H, bits, B, T):
    """train_pa --quant at the reference's batch sizes: the whole step body (forward, loss, backward) of a quantised model is ONE launch with
    one frame per wave (csrc/qat_cascade.hip qat_gp_train_kernel; no checkpoint scratch) — same loss, gradients and sparsity counters as
    autograd through the split kernels.  dgru (r04): its fc_hid + relu + cat + fc_out head runs with lane = time step inside the engine
    (odpd_qatseq.h dg_head / dg_reduce)."""
    _fused_equals_split(bb, H, bits, B, T, True)


@pytest.mark.parametrize("H,bits,B,T", [(13, 8, 64, 50), (8, 8, 33, 21), (23, 8, 18, 35), (30, 8, 3, 70), (16, 8, 256, 200), (21, 16, 9, 40)])
def test_dgru_one_launch_step_matches_the_oracle(H, bits, B, T):
    """The quantised dgru engine's train step (loss + gradients of one launch) against the ORACLE, with biases, weights and scales moved off
    their defaults so that clamps, relu and every pass mask of the fc_hid / fc_out head are exercised; then an evaluation pass on the same
    engine (bit for bit on 8-bit grids)."""
    import ctypes as C
    from opendpd_amd import _lib
    from opendpd_amd.train_funcs import FusedAdamW, fused_train_step
    from oracle.oracle import Oracle, make_model
    torch.manual_seed(H + B + T)
    q = _fresh("dgru", H, bits).cuda()
    with torch.no_grad():
        g = torch.Generator().manual_seed(H)
        for k, p in q.named_parameters():
            if k.endswith("bias"):
                p.copy_(((torch.rand(p.shape, generator=g) - 0.5) * 0.6).cuda())
            elif k.endswith("weight") and p.dim() == 2:
                p.mul_(1.7)
        q.backbone.fc_hid.act_quantizer.scale.mul_(0.5)         # states beyond fc_hid's activation range
        q.backbone.fc_out.act_quantizer.scale.mul_(0.5)
    x, t = _signal(B, T, B + T)
    o = Oracle("f32")
    m = make_model("dgru", H, bits_w=bits, bits_a=bits)
    p = np.concatenate([v.detach().cpu().numpy().reshape(-1) for v in q.parameters()])
    q.train()
    assert int(_lib.load().odpd_train_workspace_floats(C.byref(q.backbone.desc), B, T)) == 0      # the one-launch step
    yo = o.qat_forward(m, p, x)
    lo, dy = o.loss("l2", yo, t)
    go, _ = o.qat_backward(m, p, x, dy, need_dx=False)
    opt = FusedAdamW(q, lr=0.0, weight_decay=0.0)
    lf = fused_train_step(opt, torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), "l2", 0.0)
    assert abs(lf.item() - lo) < (2e-6 if bits == 8 else 2e-4) * max(1.0, abs(lo))
    got = opt.grad[:-4].cpu().numpy()
    off = 0
    for k, v in q.named_parameters():
        n = v.numel()
        ref = go[off:off + n]
        if np.abs(ref).max() > 0:
            assert rel_err(got[off:off + n], ref) < (3e-5 if bits == 8 else 2e-3), k
        else:
            assert np.abs(got[off:off + n]).max() == 0, k
        off += n
    whid = q.backbone.fc_hid.weight.detach().cpu().numpy()
    names = [k for k, _ in q.named_parameters()]
    sizes = [v.numel() for v in q.parameters()]
    o_hid = int(np.sum(sizes[:names.index("backbone.fc_hid.weight")]))
    ghid = got[o_hid:o_hid + whid.size].reshape(whid.shape)
    lim = 2.0 ** (bits - 1) * 2.0 ** (2 - bits)
    assert np.all(ghid[np.abs(whid) > lim] == 0.0) and np.abs(ghid).max() > 0
    q.eval()
    with torch.no_grad():
        ye = q(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = o.qat_forward(m, p, x, eval_mode=True)
    # (16-bit grids: 32-bit products summed in fp32 — the summation order decides single roundings, and with the scales moved as above a few of
    # them travel through fc_hid and fc_out: measured 6.1e-4 at most, the same for the sixteen-sequences-per-wave kernels, which the engine
    # matches bit for bit)
    assert np.abs(ye - ref).max() <= (0.0 if bits == 8 else 2.0 ** -10)
    lib = _lib.load()
    lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(0))
    try:
        with torch.no_grad():
            ys = q(torch.from_numpy(x).cuda()).cpu().numpy()
    finally:
        lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1))
    assert np.array_equal(ye, ys)


def test_quantised_dgru_beyond_one_frame_per_simd_keeps_the_two_launch_step():
    _fused_equals_split("dgru", 13, 8, 600, 9, False)
