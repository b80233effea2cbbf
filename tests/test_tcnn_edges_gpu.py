"""Tile, threshold, channel-split and group-loop edges of csrc/tcnn.hip — tcnn_fwd_kernel<R, NTX>, tcnn_bwd_kernel<R, NTX> and
tcnn_dx_kernel<R, NTX>, the kernels of the tcnn and neuraltx (NTX) backbones — against the fp64 build of the CPU oracle.  Modelled on
test_sweeps_s16_edges_gpu.py; models and inputs follow the recipe of test_janet_tcnn_gpu.ragged_case (biases moved to uniform(-0.3, 0.3), NeuralTX
FIR taps to uniform(-0.6, 0.6), amplitude 0.05 .. 0.9 with uniform phase — no sample at the origin —, dy ~ N(0, 1)).

What selects the code.  tcnn_geom: R = 4 / 8 / 13 / 16 at T <= 64 / 128 / 208 / 256 (one tile holds the frame), above that R = 16 tiles
with a halo: 30 (tile 196) for tcnn's forward and backward, 32 (192) for neuraltx's, 60 (136) for tcnn's dL/dx, 64 (128) for neuraltx's.
tcnn_split: `ncw` waves share a tile's channels, the smallest power of two with ngroups * ncw >= 8 CUs, at most 4 (forward, dL/dx: LDS sum
of the waves' shares) or 32 (backward).  tcnn_bwd_shape: at most 2 blocks per CU, beyond which a wave walks several tile groups.  Four
16-lane rows per wave, item = group * 4 + row, sequence = item / ntiles.  `_geom`, `_split` and `_bwd_shape` restate these in Python;
every case asserts that odpd_partial_rows answers the grid they give, the regime cases also that they run the regime they were written for.

Shapes.  Lengths 1, 2, 3 (shorter than a 5-tap kernel), 16, 17 (the outer tap of the dilation-8 stage enters the frame), both sides of every
R threshold, and tiled 257, 272 | 273 (tcnn dL/dx: two full tiles | one owned sample in the third), 384 | 385 (neuraltx), 392 | 393 (tcnn),
589; batches 1, 3, 4, 5, 9 (a partly filled wave, rows of one wave holding tiles of different sequences, one row in a second wave).  The
width follows the grid position (`_width`): tcnn 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, neuraltx 1, 3, 5, 33, 64 (below the split, one past it,
around the backward cap of 32, the largest); `test_the_grid_covers_what_it_claims` holds the grid to its coverage conditions.  Channel-split
regimes at T = 3 (R = 4) and 70 (R = 8), widths 5 and 33: B = 4 (8 CUs / n) + 3 for n = 16 .. 1 (backward ncw = n, forward and dL/dx ncw
4, 4, 4, 2, 1; the capped backward grid holds 8 CUs / n groups, so the first n waves take the one group more as their second), at T = 3 also
B = 4 (8 CUs / n) - 1 (the same splits, one group per wave), and B = 16 CUs + 5, 32 CUs + 5 (two groups more than the capped grid's stride,
at ncw 2 and 1).

Every case compares (1) the inference forward under torch.no_grad(), (2) forward and backward with weights and input requiring grad, (3)
weights alone, (4) dL/dx alone with frozen parameters (the PA of a cascade) with one Oracle("f64") forward / backward of the fp32 parameters
and inputs.  Bounds of test_janet_tcnn_gpu.py: 2e-5 scale-relative on y, 3e-4 on the flat gradient, on every parameter tensor on its own
maximum and on dL/dx.  The fp32 oracle stays within 2.4e-7 / 4.3e-6 / 7.2e-6 / 1.8e-7 of the fp64 one on this grid
(tests/test_grad_blocks_cpu.py holds it to 2e-6 / 2e-5 / 2e-5 / 2e-6).  The autograd wrapper allocates y and dx with torch.empty, where an
unwritten sample can hold the right value of the previous call: `test_every_owned_sample_is_written` calls the C ABI on NaN-filled buffers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.golden_util import assert_grad_blocks, grad_block_errors, net_grad_blocks, rel_err
from tests.test_janet_tcnn_gpu import FWD_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

SINGLE = [1, 2, 3, 16, 17, 63, 64, 65, 127, 128, 129, 207, 208, 209, 255, 256]
TILED = [257, 272, 273, 384, 385, 392, 393, 589]
LENGTHS = SINGLE + TILED
BATCHES = [1, 3, 4, 5, 9]
WIDTHS = {"tcnn": [1, 2, 3, 4, 5, 31, 32, 33, 63, 64], "neuraltx": [1, 3, 5, 33, 64]}
STRIDE = {"tcnn": 3, "neuraltx": 1}      # the width index advances by this per length and by one per batch
REGIME_LENGTHS, REGIME_WIDTHS, REGIME_N = [3, 70], [5, 33], [16, 8, 4, 2, 1]
WRITTEN_WIDTH = {"tcnn": 33, "neuraltx": 3}
WRITTEN_LENGTHS = [129, 209, 256, 257, 273, 385, 393]
FALLBACK_CUS = 256      # collection without a device (the CPU twin, --collect-only): ids only, the tests themselves ask the device


# input seeds of the (backbone, C, B, T) on which B * 17 + T draws a frame that leaves the one channel of a C = 1 neuraltx stack nearly dead
# (its bias gradient, one sum over every sample, is 1e-5 of the flat maximum and the serial fp32 oracle's own rounding on it exceeds 2e-5 of
# the fp64 oracle's: tests/test_grad_blocks_cpu.py): the first of B * 17 + T + 1000 k on which it does not
RESEEDED = {("neuraltx", 1, 4, 16): 1084, ("neuraltx", 1, 5, 208): 1293, ("neuraltx", 1, 4, 273): 1341}


def edge_case(bb, C, B, T, device="cuda"):
    """model, input and output gradient of one case, by the recipe of test_janet_tcnn_gpu.ragged_case: biases to uniform(-0.3, 0.3), NeuralTX
    FIR taps to uniform(-0.6, 0.6), amplitude 0.05 .. 0.9 with uniform phase, dy ~ N(0, 1).  Every draw comes from the CPU generators, so
    that the CPU twin (tests/test_grad_blocks_cpu.py, `device` "cpu") judges the very parameters and inputs the kernels get."""
    from opendpd_amd import CoreModel
    torch.manual_seed(C * 100 + B + T)
    net = CoreModel(2, C, 1, bb)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "bias" in k:
                p.uniform_(-0.3, 0.3)
            if k.startswith("backbone.conv_"):
                p.uniform_(-0.6, 0.6)
    rng = np.random.RandomState(RESEEDED.get((bb, C, B, T), B * 17 + T))
    amp = 0.05 + 0.85 * rng.rand(B, T, 1)
    ph = 2 * np.pi * rng.rand(B, T, 1)
    x = np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)
    dy = rng.randn(B, T, 2).astype(np.float32)
    return net.to(device), x, dy


# ---- tcnn_geom, tcnn_split, tcnn_bwd_shape (csrc/tcnn.hip), written out ---------------------------------------------------------------------
def _halo(bb, dx):
    return (60 if dx else 30) + ((4 if dx else 2) if bb == "neuraltx" else 0)


def _geom(bb, B, T, dx=False):
    """(R, tiled, ntiles, ngroups) of the forward / backward (dx: the dL/dx) launch"""
    if T <= 256:
        return (4 if T <= 64 else 8 if T <= 128 else 13 if T <= 208 else 16), False, 1, (B + 3) // 4
    tile = 256 - 2 * _halo(bb, dx)
    ntiles = (T + tile - 1) // tile
    return 16, True, ntiles, (B * ntiles + 3) // 4


def _split(ngroups, cap, cus):
    ncw = 1
    while ncw < cap and ngroups * ncw < 8 * cus:
        ncw *= 2
    return ncw


def _bwd_shape(ngroups, cus):
    """(ncw, grid, groups the busiest wave walks) of the backward launch"""
    ncw = _split(ngroups, 32, cus)
    grid = min((ngroups * ncw + 3) // 4, 2 * cus)
    grid = (grid + 7) // 8 * 8
    gstep = grid * 4 // ncw
    return ncw, grid, (ngroups + gstep - 1) // gstep


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else FALLBACK_CUS


def _regime(bb, B, T, cus):
    """the launch of every kernel of a case: what its test id names and its WORST line is keyed by"""
    R, tiled, _, ng = _geom(bb, B, T)
    ncw_b, grid, passes = _bwd_shape(ng, cus)
    return {"R": R, "tiled": tiled, "fwd": _split(ng, 4, cus), "dx": _split(_geom(bb, B, T, True)[3], 4, cus), "bwd": ncw_b, "grid": grid,
            "passes": passes}


def _instantiation(bb, R, tiled):
    return f"<R={R}{' tiled' if tiled else ''}, NTX={int(bb == 'neuraltx')}>"


def _case_id(bb, C, B, T):
    r = _regime(bb, B, T, _cus())
    return (f"{bb}-fwd+bwd+dx{_instantiation(bb, r['R'], r['tiled'])}-C{C}-B{B}-T{T}-fwd_ncw{r['fwd']}-dx_ncw{r['dx']}-bwd_ncw{r['bwd']}"
            + ("-second_group" if r["passes"] > 1 else ""))


# ---- the grid -----------------------------------------------------------------------------------------------------------------------------
def _width(bb, iT, iB):
    w = WIDTHS[bb]
    return w[(STRIDE[bb] * iT + iB) % len(w)]


def grid_cases():
    """(backbone, width, batch, length) of the length x batch grid, the width chosen by the position"""
    return [(bb, _width(bb, iT, iB), B, T) for bb in WIDTHS for iT, T in enumerate(LENGTHS) for iB, B in enumerate(BATCHES)]


def regime_batches(cus):
    """[(batch, backward ncw, forward / dL/dx ncw, groups of the busiest backward wave, lengths)] the channel-split cases are written for.
    8 CUs / n + 1 groups at ncw = n are n waves more than the capped grid of 2 blocks per CU holds, so the first n waves of that grid take
    the last group as their second; one sequence short of 8 CUs / n full groups fills the capped grid exactly, one group per wave."""
    return ([(4 * (8 * cus // n) - 1, n, min(n, 4), 1, REGIME_LENGTHS[:1]) for n in REGIME_N]
            + [(4 * (8 * cus // n) + 3, n, min(n, 4), 2, REGIME_LENGTHS) for n in REGIME_N]
            + [(16 * cus + 5, 2, 2, 2, REGIME_LENGTHS), (32 * cus + 5, 1, 1, 2, REGIME_LENGTHS)])


def regime_cases(cus):
    return [(bb, Cw, T, i) for bb in WIDTHS for T in REGIME_LENGTHS for Cw in REGIME_WIDTHS for i, b in enumerate(regime_batches(cus))
            if T in b[4]]


def _r_class(T):
    R, tiled, _, _ = _geom("tcnn", 1, T)
    return (R, tiled)


def test_the_grid_covers_what_it_claims():
    """the coverage conditions over the generated parameter lists, so that an edit cannot thin the grid silently"""
    cases = grid_cases()
    classes = {_r_class(T) for T in LENGTHS}
    assert classes == {(4, False), (8, False), (13, False), (16, False), (16, True)}
    assert len(cases) == 2 * len(LENGTHS) * len(BATCHES) and len(set(cases)) == len(cases)
    for bb, widths in WIDTHS.items():
        mine = [c for c in cases if c[0] == bb]
        for T in LENGTHS:       # every length meets at least two widths, and every batch
            assert len({c[1] for c in mine if c[3] == T}) >= 2, (bb, T)
            assert {c[2] for c in mine if c[3] == T} == set(BATCHES), (bb, T)
        for Cw in widths:       # every width meets a length of each R
            assert {_r_class(c[3]) for c in mine if c[1] == Cw} == classes, (bb, Cw)
        for cl in classes:      # every instantiation of the three kernels (each case runs all three) meets C = 1, 33 and 64
            assert {1, 33, 64} <= {c[1] for c in mine if _r_class(c[3]) == cl}, (bb, cl)
    # both sides of every threshold and of every exact tile fill
    for a in (64, 128, 208, 256, 272, 384, 392):
        assert a in LENGTHS and a + 1 in LENGTHS
    assert _geom("tcnn", 1, 392)[2] == 2 and _geom("tcnn", 1, 393)[2] == 3 and _geom("neuraltx", 1, 384)[2] == 2
    assert _geom("neuraltx", 1, 385)[2] == 3 and _geom("tcnn", 1, 272, True)[2] == 2 and _geom("tcnn", 1, 273, True)[2] == 3
    assert _geom("neuraltx", 1, 256, True)[2] == 1 and _geom("neuraltx", 1, 257, True)[2] == 3
    # the names the test ids carry: every instantiation, every ncw of every kernel, the second group
    cus = _cus()
    ids = [_case_id(*c) for c in cases] + [_case_id(bb, Cw, regime_batches(cus)[i][0], T) for bb, Cw, T, i in regime_cases(cus)]
    for bb in WIDTHS:
        for R, tiled in classes:
            assert any(_instantiation(bb, R, tiled) in i and i.startswith(bb) for i in ids)
    for k, ns in (("fwd", (1, 2, 4)), ("dx", (1, 2, 4)), ("bwd", (1, 2, 4, 8, 16, 32))):
        for n in ns:
            assert any(f"-{k}_ncw{n}-" in i + "-" for i in ids), (k, n)
    assert any(i.endswith("second_group") for i in ids)


# ---- reference, comparison, record --------------------------------------------------------------------------------------------------------
def _flat(net):
    return np.concatenate([q.detach().cpu().numpy().reshape(-1) for q in net.parameters()])


def _oracle(bb, Cw, net, x, dy):
    """y, weight gradient and dL/dx of the fp64 oracle at the fp32 parameters and inputs: once per case, read-only"""
    from oracle.oracle import Oracle, make_model
    o, m, p = Oracle("f64"), make_model(bb, Cw), _flat(net).astype(np.float64)
    x64, dy64 = x.astype(np.float64), dy.astype(np.float64)
    yo, _ = o.forward(m, p, x64)
    go, dxo = o.backward(m, p, x64, dy64, need_dx=True)
    for a in (yo, go, dxo):
        a.setflags(write=False)
    return yo, go, dxo


_WORST = {}


def _larger(a, b):
    """max(a, b) that keeps a NaN (Python's max drops one in second place)"""
    return b if np.isnan(b) or b > a else a


class _Figures:
    """the figures of one case; `check` prints them, folds them into the record of the case's (backbone, regime) and holds them to the bounds"""

    def __init__(self, key, case, ref, blocks):
        self.key, self.case, (self.yo, self.go, self.dxo), self.blocks = key, case, ref, blocks
        self.y = self.flat = self.block = self.dx = 0.0
        self.label, self.grads = "-", []

    def fwd(self, y):
        self.y = _larger(self.y, rel_err(y, self.yo))

    def grad(self, g):
        self.flat = _larger(self.flat, rel_err(g, self.go))
        for label, e, _, _ in grad_block_errors(g, self.go, self.blocks):
            if e is not None and _larger(self.block, e) != self.block:
                self.block, self.label = e, label
        self.grads.append(g)

    def dldx(self, dx):
        self.dx = _larger(self.dx, rel_err(dx, self.dxo))

    def check(self):
        print(f"{self.key} {self.case}: y err {self.y:.2e}, flat gradient err {self.flat:.2e}, worst tensor {self.label} {self.block:.2e}, "
              f"dL/dx err {self.dx:.2e}")
        w = _WORST.setdefault(self.key, {"y": (0.0, "-"), "flat": (0.0, "-"), "block": (0.0, "-"), "dx": (0.0, "-")})
        for k, v, at in (("y", self.y, self.case), ("flat", self.flat, self.case), ("block", self.block, f"{self.label} at {self.case}"),
                         ("dx", self.dx, self.case)):
            if _larger(w[k][0], v) != w[k][0]:
                w[k] = (v, at)
        assert self.y < FWD_TOL, (self.case, "y", self.y)
        for g in self.grads:
            assert_grad_blocks(g, self.go, self.blocks, GRAD_TOL, exact_zeros=True)
        assert self.dx < GRAD_TOL, (self.case, "dL/dx", self.dx)


@pytest.fixture(scope="module", autouse=True)
def worst_report():
    """one WORST line per (backbone, kernel regime) when the module is through: the baseline of docs/design/parity.md"""
    yield
    for key in sorted(_WORST):
        w = _WORST[key]
        print(f"WORST {key}: y {w['y'][0]:.2e} ({w['y'][1]}), flat {w['flat'][0]:.2e} ({w['flat'][1]}), tensor {w['block'][0]:.2e} "
              f"({w['block'][1]}), dL/dx {w['dx'][0]:.2e} ({w['dx'][1]})")


def _rows_answer_the_grid(net, bb, B, T, cus):
    from opendpd_amd import _lib
    r = _regime(bb, B, T, cus)
    assert int(_lib.load().odpd_partial_rows(C.byref(net.backbone.desc), B, T, 0)) == r["grid"]
    return r


def _compare(bb, Cw, net, x, dy, key):
    """the four comparisons of one case through the autograd wrapper"""
    fig = _Figures(key, f"C{Cw} B{x.shape[0]} T{x.shape[1]}", _oracle(bb, Cw, net, x, dy), net_grad_blocks(net))
    xc, dyc = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()

    def grads():
        return np.concatenate([q.grad.cpu().numpy().reshape(-1) for q in net.parameters()])

    with torch.no_grad():                                       # 1. inference
        fig.fwd(net(xc).cpu().numpy())
    xt = xc.clone().requires_grad_(True)                        # 2. weights and input
    y = net(xt)
    y.backward(dyc)
    fig.fwd(y.detach().cpu().numpy())
    fig.grad(grads())
    fig.dldx(xt.grad.cpu().numpy())
    for q in net.parameters():                                  # 3. weights alone
        q.grad = None
    y = net(xc)
    y.backward(dyc)
    fig.fwd(y.detach().cpu().numpy())
    fig.grad(grads())
    for q in net.parameters():                                  # 4. dL/dx alone, frozen parameters
        q.requires_grad_(False)
        q.grad = None
    xt = xc.clone().requires_grad_(True)
    y = net(xt)
    y.backward(dyc)
    fig.fwd(y.detach().cpu().numpy())
    fig.dldx(xt.grad.cpu().numpy())
    fig.check()


# ---- 1. lengths x batches, the width by the grid position -----------------------------------------------------------------------------------
@pytest.mark.parametrize("bb,Cw,B,T", grid_cases(), ids=[_case_id(*c) for c in grid_cases()])
def test_tile_and_threshold_edges(bb, Cw, B, T):
    cus = _cus()
    net, x, dy = edge_case(bb, Cw, B, T)
    r = _rows_answer_the_grid(net, bb, B, T, cus)
    assert r["bwd"] == 32 and r["fwd"] == r["dx"] == 4 and r["passes"] == 1      # small batches: the caps of the channel split
    _compare(bb, Cw, net, x, dy, f"{bb} {_instantiation(bb, r['R'], r['tiled'])} fwd ncw 4, dx ncw 4, bwd ncw 32")


# ---- 2. the channel-split regimes and the backward group loop -------------------------------------------------------------------------------
@pytest.mark.parametrize("bb,Cw,T,i", regime_cases(_cus()),
                         ids=[_case_id(bb, Cw, regime_batches(_cus())[i][0], T) for bb, Cw, T, i in regime_cases(_cus())])
def test_channel_split_regimes_and_group_loop(bb, Cw, T, i):
    cus = _cus()
    B, ncw_bwd, ncw_fwd, passes, _ = regime_batches(cus)[i]
    net, x, dy = edge_case(bb, Cw, B, T)
    r = _rows_answer_the_grid(net, bb, B, T, cus)
    assert (r["bwd"], r["fwd"], r["dx"], r["passes"]) == (ncw_bwd, ncw_fwd, ncw_fwd, passes), r      # the regime the case was written for
    _compare(bb, Cw, net, x, dy, f"{bb} {_instantiation(bb, r['R'], False)} fwd ncw {ncw_fwd}, dx ncw {ncw_fwd}, bwd ncw {ncw_bwd}"
             + (", second group" if passes > 1 else ""))


# ---- 3. every owned sample is written -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", WRITTEN_LENGTHS)
@pytest.mark.parametrize("bb", list(WIDTHS))
def test_every_owned_sample_is_written(bb, T):
    """odpd_backbone_fwd / odpd_backbone_bwd the way the autograd wrapper calls them (backbones/native.py), on y, dx and exactly the answered
    number of partial rows filled with NaN: weights and dL/dx in one call, weights alone, dL/dx alone.  No NaN may remain in y, dx or the
    gradient the product's row reduction gives, and all of them are the oracle's."""
    from opendpd_amd import _lib
    from opendpd_amd.train_funcs import ckpt_buffer
    lib, cus, Cw, B = _lib.load(), _cus(), WRITTEN_WIDTH[bb], 3
    net, x, dy = edge_case(bb, Cw, B, T)
    r = _rows_answer_the_grid(net, bb, B, T, cus)
    fig = _Figures(f"{bb} {_instantiation(bb, r['R'], r['tiled'])} NaN-filled buffers", f"C{Cw} B{B} T{T}", _oracle(bb, Cw, net, x, dy),
                   net_grad_blocks(net))
    mod = net.backbone
    d, flat, P, st = mod.call_desc(need_dx=True), mod.flat_params(), mod.n_flat, _lib.stream_ptr()
    xc, dyc = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    ckpt = ckpt_buffer(d, B, T, xc.device)
    rows = int(lib.odpd_partial_rows(C.byref(d), B, T, 0))
    nan = float("nan")
    y = torch.full_like(xc, nan)
    _lib.check(lib.odpd_backbone_fwd(st, C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(xc), _lib.ptr(y), _lib.ptr(ckpt), None), "forward")
    assert not bool(torch.isnan(y).any())
    fig.fwd(y.cpu().numpy())
    for need_w, need_dx in ((True, True), (True, False), (False, True)):
        part = torch.full((rows, P + _lib.LOSS_COLS), nan, device="cuda") if need_w else None
        dx = torch.full_like(xc, nan) if need_dx else None
        _lib.check(lib.odpd_backbone_bwd(st, C.byref(d), B, T, _lib.ptr(flat), _lib.ptr(xc), _lib.ptr(dyc), _lib.ptr(ckpt), _lib.ptr(part),
                                         _lib.ptr(dx)), "backward")
        if need_w:
            grad = torch.full((P + _lib.LOSS_COLS,), nan, device="cuda")
            _lib.check(lib.odpd_reduce_partials(st, rows, P, _lib.ptr(part), _lib.ptr(grad), 0), "reduce")
            assert not bool(torch.isnan(grad[:P]).any()), (need_w, need_dx)
            fig.grad(grad[:P].cpu().numpy())
        if need_dx:
            assert not bool(torch.isnan(dx).any()), (need_w, need_dx)
            fig.dldx(dx.cpu().numpy())
    fig.check()
