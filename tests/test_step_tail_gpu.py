"""The tail every training step ends in (csrc/optim.hip) at the edges of its kernels: the loss (odpd_loss_fwd_bwd: vector body, 1..3
element tail, single-launch / two-launch threshold, the 256-block cap, a second grid-stride pass, dy == NULL, count != n), the row
reduction (odpd_reduce_partials: both sides of the unrolled loop's entry, the remainder loop, the column tail, accumulate, P = 0) and
clip + optimiser (odpd_clip_optim_step, odpd_clip_adamw_step, odpd_clip_adamw_step_masked: one and several trips of the 1024-stride
loops, the clip boundary, zero and non-finite gradients).

References are numpy float64 / int64 and torch on the CPU.  The exact cases use inputs on a grid on which every fp32 operation of the
kernel is exact in any summation order, and each test asserts that condition itself; their assertions are bit-equality.  Every
tolerance is one the suite already asserts for the same quantity (test_gru_family_gpu.py, test_optim_gpu.py) or the order-independent
a-priori summation bound rows * 2^-24 * sum |x|.  Every output buffer carries sentinels behind its end that must survive."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu

EINVAL = -1
_SENT_BITS = 0xDEADBEEF         # a finite float no kernel here produces
_SENT = np.array([_SENT_BITS], np.uint32).view(np.float32)[0]
KINDS = ["adamw", "adam", "sgd", "rmsprop"]
STEP_BOUND = {"adamw": 6e-7, "adam": 6e-7, "sgd": 2e-7, "rmsprop": 2e-7}     # test_optim_gpu.py: |p| up to 1.6, one / a few ulp


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _guarded(values, guard):
    """device buffer: `values` followed by `guard` sentinel floats"""
    buf = np.empty(len(values) + guard, np.float32)
    buf[:len(values)] = values
    buf[len(values):] = _SENT
    return torch.from_numpy(buf).cuda()


def _guard_intact(t, n):
    return bool((_bits(t[n:]) == _SENT_BITS).all())


# ---- loss ---------------------------------------------------------------------------------------------------------------------------
# tails of 1, 2, 3 elements; the 4096-element stride of the single-workgroup kernel; the last n of the single-launch route and the first
# of the two-launch route with a tail; the 256-block cap (256 blocks x 256 lanes x 4 = 262 144) from both sides; a second grid-stride pass
LOSS_N = [1, 2, 3, 4, 6, 7, 4094, 4098, 32766, 32768, 32770, 65538, 262142, 262146, 524294]


@functools.lru_cache(maxsize=None)
def _grid_case(n):
    """t a multiple of 0.5 in [-4, 4], y = t + d with d a multiple of 0.5 in [-2, 2] (a third of them 0): y - t, d^2 (a multiple of 0.25,
    <= 4) and |d| (a multiple of 0.5, <= 2) are exact in fp32, and so is every partial sum below 2^24 of those units."""
    rng = np.random.RandomState(1000 + n % 997)
    t = rng.randint(-8, 9, n).astype(np.float32) * np.float32(0.5)
    d = rng.randint(-4, 5, n).astype(np.float32) * np.float32(0.5)
    d[rng.rand(n) < 0.3] = 0.0
    y = t + d
    assert np.array_equal(y - t, d)
    yt, tt = torch.from_numpy(y).cuda(), torch.from_numpy(t).cuda()
    for a in (y, t, d):
        a.setflags(write=False)
    return y, t, d, yt, tt


def _call_loss(lib, _lib, kind, n, count, yt, tt, with_dy):
    dy = _guarded(np.full(n, np.nan, np.float32), 8) if with_dy else None
    out = _guarded(np.zeros(_lib.LOSS_WS, np.float32), 8)
    rc = lib.odpd_loss_fwd_bwd(_lib.stream_ptr(), _lib.LOSS_IDS[kind], n, count, _lib.ptr(yt), _lib.ptr(tt), _lib.ptr(dy), _lib.ptr(out))
    assert rc == 0
    out = out.cpu().numpy()
    assert _guard_intact(out, _lib.LOSS_WS)
    if with_dy:
        dy = dy.cpu().numpy()
        assert _guard_intact(dy, n), "dy written behind its n elements"
        assert not np.isnan(dy[:n]).any(), "dy not written everywhere"
        dy = dy[:n]
    return out[0], dy


@pytest.mark.parametrize("count_mul", [1, 3])
@pytest.mark.parametrize("with_dy", [True, False])
@pytest.mark.parametrize("kind", ["l2", "l1"])
def test_loss_exact_on_a_grid(kind, with_dy, count_mul):
    from opendpd_amd import _lib
    lib = _lib.load()
    for n in LOSS_N:
        y, t, d, yt, tt = _grid_case(n)
        count = count_mul * n
        d64 = d.astype(np.float64)
        S, unit = (float(np.sum(d64 * d64)), 0.25) if kind == "l2" else (float(np.sum(np.abs(d64))), 0.5)
        assert S / unit == int(S / unit) and S / unit < 2 ** 24         # the exactness condition: any partial sum is an exact fp32 number
        inv = np.float32(1.0 / count)
        loss, dy = _call_loss(lib, _lib, kind, n, count, yt, tt, with_dy)
        assert _same_bits(loss, np.float32(S) * inv), (n, loss, S, count)
        if with_dy:
            want = (y - t) * np.float32(2) * inv if kind == "l2" else np.sign(y - t) * inv
            assert want.dtype == np.float32
            bad = np.flatnonzero(_bits(dy) != _bits(want))
            assert bad.size == 0, (n, bad[:8], dy[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("n", [3700, 32770, 524294])
@pytest.mark.parametrize("kind", ["l2", "l1"])
def test_loss_generic(kind, n):
    from opendpd_amd import _lib
    lib = _lib.load()
    rng = np.random.RandomState(n)
    y, t = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    d = y.astype(np.float64) - t.astype(np.float64)
    want = float(np.mean(d * d if kind == "l2" else np.abs(d)))
    want_dy = 2.0 * d / n if kind == "l2" else np.sign(d) / n
    yt, tt = torch.from_numpy(y).cuda(), torch.from_numpy(t).cuda()
    loss, dy = _call_loss(lib, _lib, kind, n, n, yt, tt, True)
    assert abs(float(loss) - want) < 1e-5 * max(1.0, abs(want))       # the bound of test_loss_and_adamw_kernels_match_oracle
    assert rel_err(dy, want_dy) < 1e-6
    loss2, dy2 = _call_loss(lib, _lib, kind, n, n, yt, tt, True)
    assert _same_bits(loss, loss2) and _same_bits(dy, dy2)


def test_loss_bad_arguments():
    from opendpd_amd import _lib
    lib = _lib.load()
    t = torch.zeros(16, device="cuda")
    out = torch.zeros(_lib.LOSS_WS, device="cuda")
    s, p = _lib.stream_ptr(), _lib.ptr
    assert lib.odpd_loss_fwd_bwd(s, 0, 0, 16, p(t), p(t), None, p(out)) == EINVAL
    assert lib.odpd_loss_fwd_bwd(s, 0, 16, 0, p(t), p(t), None, p(out)) == EINVAL
    assert lib.odpd_loss_fwd_bwd(s, 2, 16, 16, p(t), p(t), None, p(out)) == EINVAL
    assert lib.odpd_loss_fwd_bwd(s, 0, 16, 16, None, p(t), None, p(out)) == EINVAL
    assert lib.odpd_loss_fwd_bwd(s, 0, 16, 16, p(t), None, None, p(out)) == EINVAL
    assert lib.odpd_loss_fwd_bwd(s, 0, 16, 16, p(t), p(t), None, None) == EINVAL


# ---- row reduction ------------------------------------------------------------------------------------------------------------------
# wave w enters the unrolled loop (8 rows, 16 apart) when w + 112 < rows: 113 is the first row count at which wave 0 does, 128 the first
# at which wave 15 does, 240 / 241 the same for a second trip; everything else goes through the remainder loop
REDUCE_ROWS = [1, 2, 15, 16, 17, 112, 113, 127, 128, 129, 240, 241, 1000]
REDUCE_P = [0, 1, 59, 60, 61, 124, 1041]      # cols = P + 4: 4, 5, 63, 64, 65, 128, 1045


@functools.lru_cache(maxsize=None)
def _int_partials(rows, P):
    cols = P + 4
    rng = np.random.RandomState(rows * 2003 + P)
    part = rng.randint(-32, 33, (rows, cols))
    pre = rng.randint(-1000, 1001, cols)
    col_sum = part.astype(np.int64).sum(0)
    assert np.abs(part).astype(np.int64).sum(0).max() + 1000 < 2 ** 24       # every partial sum, in any order, is an exact fp32 integer
    for a in (part, pre, col_sum):
        a.setflags(write=False)
    return part.astype(np.float32), pre, col_sum


@pytest.mark.parametrize("P", REDUCE_P)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_reduce_partials_exact_on_integers(accumulate, P):
    from opendpd_amd import _lib
    lib = _lib.load()
    cols = P + 4
    for rows in REDUCE_ROWS:
        part, pre, col_sum = _int_partials(rows, P)
        pt = torch.from_numpy(part).cuda()
        grad = _guarded(pre.astype(np.float32) if accumulate else np.full(cols, np.nan, np.float32), 64)
        assert lib.odpd_reduce_partials(_lib.stream_ptr(), rows, P, _lib.ptr(pt), _lib.ptr(grad), accumulate) == 0
        got = grad.cpu().numpy()
        assert _guard_intact(got, cols), f"rows {rows}: grad written behind its P + 4 columns"
        want = (col_sum + pre if accumulate else col_sum).astype(np.float32)
        bad = np.flatnonzero(_bits(got[:cols]) != _bits(want))
        assert bad.size == 0, (rows, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("rows,P", [(129, 61), (1000, 1041)])
def test_reduce_partials_generic(rows, P):
    from opendpd_amd import _lib
    lib = _lib.load()
    cols = P + 4
    part = np.random.RandomState(rows + P).randn(rows, cols).astype(np.float32)
    p64 = part.astype(np.float64)
    pt = torch.from_numpy(part).cuda()
    got = []
    for _ in range(2):
        grad = _guarded(np.full(cols, np.nan, np.float32), 64)
        assert lib.odpd_reduce_partials(_lib.stream_ptr(), rows, P, _lib.ptr(pt), _lib.ptr(grad), 0) == 0
        got.append(grad.cpu().numpy())
        assert _guard_intact(got[-1], cols)
    # any order of fp32 additions of `rows` numbers stays within (rows - 1) u sum |x| + O(u^2) of the true sum, u = 2^-24
    bound = rows * 2.0 ** -24 * np.abs(p64).sum(0)
    err = np.abs(got[0][:cols].astype(np.float64) - p64.sum(0))
    assert (err <= bound).all(), (int(np.argmax(err - bound)), float((err / bound).max()))
    assert _same_bits(got[0], got[1])


def test_reduce_partials_bad_arguments():
    from opendpd_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, device="cuda")
    s, p = _lib.stream_ptr(), _lib.ptr
    assert lib.odpd_reduce_partials(s, 0, 4, p(t), p(t), 0) == EINVAL
    assert lib.odpd_reduce_partials(s, 2, -1, p(t), p(t), 0) == EINVAL
    assert lib.odpd_reduce_partials(s, 2, 4, None, p(t), 0) == EINVAL
    assert lib.odpd_reduce_partials(s, 2, 4, p(t), None, 0) == EINVAL


# ---- clip + optimiser ---------------------------------------------------------------------------------------------------------------
_LOSS_COLS = np.array([0.75, -2.5, 1e-3, 7.0], np.float32)       # grad[P .. P+4): the reduced loss columns, not the step's to touch
ENTRIES = [("optim", k) for k in KINDS] + [("adamw_step", "adamw"), ("adamw_masked", "adamw")]


def _torch_opt(kind, params, lr):
    return {"adamw": lambda: torch.optim.AdamW(params, lr=lr), "adam": lambda: torch.optim.Adam(params, lr=lr),
            "sgd": lambda: torch.optim.SGD(params, lr=lr, momentum=0.9), "rmsprop": lambda: torch.optim.RMSprop(params, lr=lr)}[kind]()


class _Dev:
    """flat parameters and both state buffers of P floats on the device, each with 8 sentinels behind it"""

    def __init__(self, p0):
        self.P = len(p0)
        self.p = _guarded(np.asarray(p0, np.float32), 8)
        self.s1 = _guarded(np.zeros(self.P, np.float32), 8)
        self.s2 = _guarded(np.zeros(self.P, np.float32), 8)
        self.norm = torch.zeros(1, device="cuda")

    def step(self, entry, kind, grad, step, lr, max_norm, skip=None):
        """one call; returns (grad[0..P) as the call left it, norm_out) after checking the loss columns and every sentinel"""
        from opendpd_amd import _lib
        lib, P = _lib.load(), self.P
        g = _guarded(np.concatenate([np.asarray(grad, np.float32), _LOSS_COLS]), 8)
        sk = None if skip is None else torch.from_numpy(np.asarray(skip, np.uint8)).cuda()
        a = (_lib.ptr(self.p), _lib.ptr(g), _lib.ptr(self.s1), _lib.ptr(self.s2))
        if entry == "optim":
            rc = lib.odpd_clip_optim_step(_lib.stream_ptr(), _lib.OPTIMIZER_IDS[kind], P, *a, step, float(lr), float(max_norm), _lib.ptr(self.norm),
                                          _lib.ptr(sk))
        elif entry == "adamw_step":
            assert sk is None
            rc = lib.odpd_clip_adamw_step(_lib.stream_ptr(), P, *a, step, float(lr), 0.9, 0.999, 1e-8, 0.01, float(max_norm), _lib.ptr(self.norm))
        else:
            rc = lib.odpd_clip_adamw_step_masked(_lib.stream_ptr(), P, *a, step, float(lr), 0.9, 0.999, 1e-8, 0.01, float(max_norm),
                                                 _lib.ptr(self.norm), _lib.ptr(sk))
        assert rc == 0
        g = g.cpu().numpy()
        assert _same_bits(g[P:P + 4], _LOSS_COLS), "the step touched the loss columns grad[P .. P+4)"
        assert _guard_intact(g, P + 4)
        for t in (self.p, self.s1, self.s2):
            assert _guard_intact(t.cpu().numpy(), P), "written behind P"
        return g[:P], self.norm.cpu().numpy()[0]

    def params(self):
        return self.p.cpu().numpy()[:self.P]

    def state(self):
        return self.s1.cpu().numpy()[:self.P], self.s2.cpu().numpy()[:self.P]


def _torch_step(ref, opt, grad, max_norm):
    """clip_grad_norm_ + opt.step() on the CPU; returns the gradient as the clip left it"""
    ref.grad = torch.from_numpy(np.array(grad, np.float32))
    if max_norm:
        torch.nn.utils.clip_grad_norm_([ref], max_norm)
    opt.step()
    return ref.grad.numpy().copy()


@pytest.mark.parametrize("max_norm", [0.0, 0.5])
@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_kinds_at_loop_boundaries(kind, max_norm):
    """test_optim_gpu.py::test_fused_optimizer_kinds_match_torch (same generator scales, same bounds) with no, exactly one, and up to
    three trips of the 1024-stride loops; three steps"""
    lr = 3e-3
    for P in (1, 63, 1023, 1024, 1025, 3001):
        gen = torch.Generator().manual_seed(7)
        p0 = torch.randn(P, generator=gen) * 0.4
        ref = torch.nn.Parameter(p0.clone())
        opt = _torch_opt(kind, [ref], lr)
        dev = _Dev(p0.numpy())
        for step in range(1, 4):
            grad = (torch.randn(P, generator=gen) * (0.05 if step % 2 else 0.01)).numpy()
            want_norm = float(np.sqrt(np.sum(grad.astype(np.float64) ** 2)))
            want_g = _torch_step(ref, opt, grad, max_norm)
            g, norm = dev.step("optim", kind, grad, step, lr, max_norm)
            assert abs(float(norm) - want_norm) < 1e-5 * want_norm, (P, step)
            if max_norm:
                assert rel_err(g, want_g) < 1e-5, (P, step)    # the bound of test_loss_and_adamw_kernels_match_oracle on the clipped gradient
            else:
                assert _same_bits(g, grad), (P, step)
            err = float(np.abs(dev.params() - ref.detach().numpy()).max())
            assert err < STEP_BOUND[kind], (kind, P, step, err)


def test_adamw_entry_points_agree():
    """odpd_clip_adamw_step, odpd_clip_adamw_step_masked (no mask, an all-zero mask) and odpd_clip_optim_step(ADAMW) with the
    reference's hyper-parameters run the same kernel with the same arguments: every output is the same bits"""
    P, lr = 1025, 3e-3
    rng = np.random.RandomState(3)
    p0 = (rng.randn(P) * 0.4).astype(np.float32)
    grads = [(rng.randn(P) * s).astype(np.float32) for s in (0.05, 0.01)]
    outs = []
    for entry, skip in (("adamw_step", None), ("adamw_masked", None), ("adamw_masked", np.zeros(P, np.uint8)), ("optim", None)):
        dev = _Dev(p0)
        trace = []
        for step, grad in enumerate(grads, 1):
            trace += list(dev.step(entry, "adamw", grad, step, lr, 0.5, skip))
        outs.append(trace + [dev.params(), *dev.state()])
    for o in outs[1:]:
        assert all(_same_bits(a, b) for a, b in zip(outs[0], o))


@pytest.mark.parametrize("max_norm", [5.0, 5.00001, 2.5])
@pytest.mark.parametrize("where", [(5, 700), (1500, 2900), (1023, 1024)])
def test_clip_boundary_exact(where, max_norm):
    """a gradient of zeros, 3 and 4: its squared norm 25 is exact in any summation order, the norm is exactly 5.  The gradient the call
    leaves is the same bits as the one clip_grad_norm_ leaves on the CPU: total_norm + 1e-6 in fp32, its reciprocal times max_norm (what
    `max_norm / tensor` is in torch), a clamp at 1 and one multiplication.  At max_norm = 5.00001 the coefficient is 1."""
    P = 3001
    grad = np.zeros(P, np.float32)
    grad[list(where)] = (3.0, 4.0)
    ref = torch.nn.Parameter(torch.zeros(P))
    ref.grad = torch.from_numpy(grad.copy())
    assert float(torch.nn.utils.clip_grad_norm_([ref], max_norm)) == 5.0
    want = ref.grad.numpy()
    for entry in ("adamw_step", "optim"):
        g, norm = _Dev(np.zeros(P, np.float32)).step(entry, "adamw", grad, 1, 1e-3, max_norm)
        assert _same_bits(norm, np.float32(5.0))
        assert _same_bits(g, want), (entry, g[list(where)], want[list(where)])
    if max_norm > 5.000002:
        assert _same_bits(want, grad)
    else:
        assert (want[list(where)] < grad[list(where)]).all()


@pytest.mark.parametrize("entry,kind", ENTRIES)
def test_zero_gradient(entry, kind):
    """norm 0, coefficient 1 (max_norm / 1e-6 clamps), no NaN; AdamW decays the parameters, the other kinds leave them as they are"""
    P, lr = 1025, 3e-3
    p0 = (np.random.RandomState(5).randn(P) * 0.4).astype(np.float32)
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = _torch_opt(kind, [ref], lr)
    dev = _Dev(p0)
    for step in (1, 2):
        _torch_step(ref, opt, np.zeros(P, np.float32), 0.5)
        g, norm = dev.step(entry, kind, np.zeros(P, np.float32), step, lr, 0.5)
        assert _same_bits(norm, np.float32(0)) and _same_bits(g, np.zeros(P, np.float32))
        assert _same_bits(dev.params(), ref.detach().numpy())
        assert all(_same_bits(s, np.zeros(P, np.float32)) for s in dev.state())
    if kind == "adamw":
        assert _same_bits(dev.params(), p0 * np.float32(1.0 - lr * 0.01) * np.float32(1.0 - lr * 0.01))
    else:
        assert _same_bits(dev.params(), p0)


def _nonfinite_setup(kind, P, lr, seed):
    """one ordinary step on both sides, so that the non-finite gradient meets non-zero optimiser state"""
    rng = np.random.RandomState(seed)
    p0 = (rng.randn(P) * 0.4).astype(np.float32)
    g1 = (rng.randn(P) * 0.05).astype(np.float32)
    g2 = (rng.randn(P) * 0.05).astype(np.float32)
    ref = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = _torch_opt(kind, [ref], lr)
    return p0, g1, g2, ref, opt


@pytest.mark.parametrize("at", [7, 1024])
@pytest.mark.parametrize("entry,kind", ENTRIES)
def test_nan_gradient_poisons_the_step_like_torch(entry, kind, at):
    """clip_grad_norm_ with a NaN entry: NaN norm, NaN coefficient, an all-NaN gradient and all-NaN parameters — in torch, in the
    oracle and here (max_norm = 200, the reference's default)"""
    P, lr = 1025, 3e-3
    p0, g1, g2, ref, opt = _nonfinite_setup(kind, P, lr, 11)
    dev = _Dev(p0)
    _torch_step(ref, opt, g1, 200.0)
    dev.step(entry, kind, g1, 1, lr, 200.0)
    g2[at] = np.nan
    want_g = _torch_step(ref, opt, g2, 200.0)
    assert np.isnan(want_g).all() and np.isnan(ref.detach().numpy()).all()        # the reference's behaviour
    g, norm = dev.step(entry, kind, g2, 2, lr, 200.0)
    assert math.isnan(float(norm))
    assert np.isnan(g).all(), f"{int((~np.isnan(g)).sum())} of {P} gradients stayed finite"
    assert np.isnan(dev.params()).all(), f"{int((~np.isnan(dev.params())).sum())} of {P} parameters were stepped with a finite gradient"


@pytest.mark.parametrize("at", [7, 1024])
@pytest.mark.parametrize("entry,kind", ENTRIES)
def test_inf_gradient_zeroes_the_others_like_torch(entry, kind, at):
    """one +inf entry: norm inf, coefficient 0; inf * 0 = NaN at that entry (gradient and parameter), every other gradient becomes 0
    and every other parameter takes the zero-gradient step torch takes"""
    P, lr = 1025, 3e-3
    p0, g1, g2, ref, opt = _nonfinite_setup(kind, P, lr, 12)
    dev = _Dev(p0)
    _torch_step(ref, opt, g1, 200.0)
    dev.step(entry, kind, g1, 1, lr, 200.0)
    g2[at] = np.inf
    want_g = _torch_step(ref, opt, g2, 200.0)
    g, norm = dev.step(entry, kind, g2, 2, lr, 200.0)
    others = np.arange(P) != at
    assert float(norm) == math.inf
    assert np.isnan(want_g[at]) and (want_g[others] == 0).all()                   # the reference's behaviour
    assert np.isnan(g[at]) and (g[others] == 0).all()
    want_p, got_p = ref.detach().numpy(), dev.params()
    assert np.isnan(want_p[at]) and np.isnan(got_p[at]) and not np.isnan(got_p[others]).any()
    err = float(np.abs(got_p[others] - want_p[others]).max())
    assert err < STEP_BOUND[kind], (kind, err)


@pytest.mark.parametrize("entry,kind", [e for e in ENTRIES if e[0] != "adamw_step"])
def test_nan_under_the_skip_mask_poisons_nothing(entry, kind):
    """a parameter whose .grad is None is outside the norm and the update, whatever its slot of the flat gradient holds"""
    P, lr, at = 1025, 3e-3, 1024
    p0, g1, g2, _, _ = _nonfinite_setup(kind, P, lr, 13)
    skip = (np.random.RandomState(14).rand(P) < 0.1).astype(np.uint8)
    skip[at] = 1
    g2[at] = 0.25
    g2_nan = g2.copy()
    g2_nan[at] = np.nan
    runs = []
    for second in (g2, g2_nan):
        dev = _Dev(p0)
        dev.step(entry, kind, g1 * 100, 1, lr, 0.5, skip)           # the first step clips, the second does not
        g, norm = dev.step(entry, kind, second, 2, lr, 200.0, skip)
        assert _same_bits(g[at], second[at])                        # untouched
        runs.append((np.delete(g, at), norm, dev.params(), *dev.state()))
    assert not math.isnan(float(runs[1][1])) and all(not np.isnan(a).any() for a in runs[1])
    assert all(_same_bits(a, b) for a, b in zip(*runs))
    masked = skip != 0
    p, s1, s2 = runs[1][2:]
    assert _same_bits(p[masked], p0[masked]) and _same_bits(s1[masked], np.zeros(int(masked.sum()))) and _same_bits(s2[masked], np.zeros(int(masked.sum())))
