"""The per-block weight-gradient comparison of the GPU parity tests (tests/golden_util.py: grad_blocks, assert_grad_blocks), on the CPU.

layout     the blocks tile the flat parameter vector of every registry backbone the converted tests use, gates split where the issue is
           a gate's own scale (3 / 4 / 2 blocks for the gru / lstm / deltajanet recurrent tensors, two-layer models included);
reference  on the cases of every converted test_against_oracle_ragged — its own parameter lists, its own model / input builder run on the
           CPU (same seeds and initialisation recipe; the bias and tap draws come from torch's CPU generator here and from the device's on
           the GPU) — the fp32 oracle's gradient passes assert_grad_blocks against the fp64 oracle's at GRAD_TOL / 16: a block that fails on
           the GPU at GRAD_TOL is 16x beyond what the reference's own rounding does to that block.  Observed maxima (docs/design/
           numerics.md): 6.7e-6 on the gru / lstm / janet / tcnn / delta / wide grids, 1.4e-5 on deltajanet's one-element weight_hh gate
           at H = 1 and on mcldnn, eight of whose cases draw their input from another seed for this condition (RAGGED_RESEEDED there);
tcnn edges on the grid of tests/test_tcnn_edges_gpu.py (its own builder, every draw from the CPU generators; 8200 x 3 in place of the batches
           it derives from the device's CU count) the fp32 oracle's y, flat gradient, every tensor and dL/dx stay within 2e-6 / 2e-5 / 2e-5 /
           2e-6 of the fp64 oracle's; observed 2.4e-7 / 4.3e-6 / 7.2e-6 / 1.8e-7;
bite       four faults planted in the oracle's gradient that the flat rel_err lets through at the family's GRAD_TOL fail by block; a block
           whose reference is identically zero stays on the flat scale."""
import functools
import warnings

import numpy as np
import pytest

from tests import test_delta_family_gpu as DELTA
from tests import test_deltajanet_gpu as DJANET
from tests import test_gru_family_gpu as GRU
from tests import test_gru_wide_gpu as WIDE
from tests import test_janet_tcnn_gpu as JANET
from tests import test_lstm_family_gpu as LSTM
from tests import test_mcldnn_gpu as MCLDNN
from tests import test_tcnn_edges_gpu as TCNN_EDGES
from tests.golden_util import assert_grad_blocks, grad_block_errors, grad_blocks, net_grad_blocks, rel_err

GATES = {"gru": 3, "dgru": 3, "qgru": 3, "qgru_amp1": 3, "deltagru": 3, "deltagru_tcnskip": 3, "lstm": 4, "vdlstm": 4, "deltajanet": 2}
GATED = ("weight_ih_l", "weight_hh_l", "bias_ih_l", "bias_hh_l", "x2h.weight", "h2h.weight")


def _cases(mod, models, build):
    """(id, family GRAD_TOL, oracle backbone, hidden, thx, thh, builder of (net, x, dy) on the CPU) per case of a converted test"""
    out = []
    for m in models:
        m = m if isinstance(m, tuple) else (m,)
        for B, T in mod.RAGGED_SHAPES:
            bb, H, thx, thh = build(*m)
            ident = "-".join(str(v) for v in (mod.__name__.split(".")[-1][5:-4], *m, B, T))
            out.append(pytest.param(mod.GRAD_TOL, bb, H, thx, thh, functools.partial(mod.ragged_case, *m, B, T, device="cpu"), id=ident))
    return out


RAGGED = (_cases(GRU, GRU.RAGGED_MODELS, lambda bb, H: (bb, H, 0.0, 0.0))
          + _cases(LSTM, LSTM.RAGGED_MODELS, lambda bb, H: (bb, H, 0.0, 0.0))
          + _cases(JANET, JANET.RAGGED_MODELS, lambda bb, H: (bb, H, 0.0, 0.0))
          + _cases(DELTA, DELTA.RAGGED_MODELS, lambda bb, H, thx, thh: (bb, H, thx, thh))
          + _cases(DJANET, DJANET.RAGGED_HIDDEN, lambda H: ("deltajanet", H, 0.0, 0.0))
          + _cases(WIDE, WIDE.RAGGED_MODELS, lambda bb, H: (bb, H, 0.0, 0.0))
          + _cases(MCLDNN, MCLDNN.RAGGED_CHANNELS, lambda C: ("mcldnn", C, 0.0, 0.0)))
LAYOUT = sorted({(p.values[1], p.values[2], 1) for p in RAGGED}
                | {(bb, H, 2) for bb, H in (("gru", 8), ("gru", 17), ("qgru", 10), ("qgru_amp1", 23), ("lstm", 9), ("lstm", 32), ("dgru", 7), ("dgru", 24))})


def _flat(net):
    return np.concatenate([q.detach().numpy().reshape(-1) for q in net.parameters()])


def _oracle_grads(bb, H, thx, thh, net, x, dy):
    """weight gradient of the fp32 and of the fp64 oracle at the same fp32 parameters and inputs.  On one thread: the oracle adds its
    threads' partial gradients in the order they finish, so only the serial sum is the same on every machine and in every run."""
    from oracle.oracle import Oracle, make_model
    m, p = make_model(bb, H, thx, thh), _flat(net)
    o32, o64 = Oracle("f32"), Oracle("f64")
    threads = o32.max_threads()
    o32.set_threads(1)      # (one OpenMP runtime under both libraries)
    try:
        g32, _ = o32.backward(m, p, x, dy, need_dx=False)
        g64, _ = o64.backward(m, p.astype(np.float64), x.astype(np.float64), dy.astype(np.float64), need_dx=False)
    finally:
        o32.set_threads(threads)
    return g32, g64


@pytest.mark.parametrize("bb,H,layers", LAYOUT)
def test_blocks_tile_the_flat_parameter_vector(bb, H, layers):
    from opendpd_amd import CoreModel
    from oracle.oracle import Oracle, make_model
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # a kernel-backed module, not an ATen restatement with other tensors
        net = CoreModel(2, H, layers, bb)
    named = [(k, tuple(q.shape)) for k, q in net.named_parameters()]
    blocks = grad_blocks(named, H)
    assert blocks == net_grad_blocks(net)
    P = sum(q.numel() for q in net.parameters())
    if layers == 1:      # (the C oracle has no second layer)
        assert P == Oracle("f32").param_count(make_model(bb, H))
    assert blocks[0][1] == 0 and blocks[-1][2] == P
    assert all(a[2] == b[1] for a, b in zip(blocks, blocks[1:])) and all(a < b for _, a, b in blocks)
    off = 0
    for k, shape in named:
        n = int(np.prod(shape))
        mine = [b for b in blocks if off <= b[1] < off + n]
        gated = ".rnn." in k and k.split(".rnn.")[1].rstrip("0123456789") in GATED
        want = GATES[bb] if gated and H > 0 and shape[0] == GATES.get(bb, 1) * H else 1
        assert len(mine) == want, (k, [b[0] for b in mine])
        if want == 1:
            assert mine == [(k, off, off + n)]
        else:
            assert [b[0] for b in mine] == [f"{k}[{i}]" for i in range(want)] and {b[2] - b[1] for b in mine} == {n // want}
        off += n
    n_gated = sum(1 for k, _ in named if ".rnn." in k)
    assert n_gated == (0 if bb not in GATES else (2 if bb == "deltagru_tcnskip" else 4 * layers))


@pytest.mark.parametrize("tol,bb,H,thx,thh,case", RAGGED)
def test_fp32_oracle_earns_the_tolerance_block_by_block(tol, bb, H, thx, thh, case):
    net, x, dy = case()
    g32, g64 = _oracle_grads(bb, H, thx, thh, net, x, dy)
    assert g32.size == net_grad_blocks(net)[-1][2]
    worst = assert_grad_blocks(g32, g64, net_grad_blocks(net), tol / 16)
    print(f"fp32 oracle against fp64: flat {rel_err(g32, g64):.2e}, worst block {worst}")


# the grid of tests/test_tcnn_edges_gpu.py; the batches that module derives from the device's CU count are stood in for by 8200 x 3
TCNN_EDGE_CASES = TCNN_EDGES.grid_cases() + [(bb, Cw, 8200, 3) for bb in TCNN_EDGES.WIDTHS for Cw in TCNN_EDGES.REGIME_WIDTHS]


@pytest.mark.parametrize("bb,Cw,B,T", TCNN_EDGE_CASES, ids=["-".join(str(v) for v in c) for c in TCNN_EDGE_CASES])
def test_fp32_oracle_stays_at_rounding_level_on_the_tcnn_edge_grid(bb, Cw, B, T):
    """the inputs of the tcnn / neuraltx edge grid are well conditioned: the fp32 oracle stays within 2e-6 (y), 2e-5 (flat gradient), 2e-5
    (every tensor on its own maximum) and 2e-6 (dL/dx) of the fp64 one, 10 to 150 times below the bounds the kernels are held to there"""
    from oracle.oracle import Oracle, make_model
    net, x, dy = TCNN_EDGES.edge_case(bb, Cw, B, T, device="cpu")
    assert float(np.min(np.hypot(x[..., 0], x[..., 1]))) > 0.049      # no sample at the origin, where the reference divides by zero
    m, p = make_model(bb, Cw), _flat(net)
    o32, o64 = Oracle("f32"), Oracle("f64")
    threads = o32.max_threads()
    o32.set_threads(1)      # (as _oracle_grads: the serial sum is the same on every machine)
    try:
        y32, _ = o32.forward(m, p, x)
        g32, dx32 = o32.backward(m, p, x, dy, need_dx=True)
        y64, _ = o64.forward(m, p.astype(np.float64), x.astype(np.float64))
        g64, dx64 = o64.backward(m, p.astype(np.float64), x.astype(np.float64), dy.astype(np.float64), need_dx=True)
    finally:
        o32.set_threads(threads)
    worst = assert_grad_blocks(g32, g64, net_grad_blocks(net), 2e-5, exact_zeros=True)
    print(f"fp32 oracle against fp64: y {rel_err(y32, y64):.2e}, flat {rel_err(g32, g64):.2e}, worst tensor {worst}, dL/dx {rel_err(dx32, dx64):.2e}")
    assert rel_err(y32, y64) < 2e-6 and rel_err(dx32, dx64) < 2e-6


# (family file, its ragged case, the faulty tensor, its gate or None, factor): pass the flat assertion, fail by block.  (gru's z gate is
# not among them: with the biases torch's CPU generator draws for this case its weight_hh block is 2.3 % of the flat maximum, and a 2 %
# fault there is beyond the flat tolerance as well.)
FAULTS = [pytest.param(GRU, ("gru", 11, 3, 5), "rnn.weight_hh_l0", 0, 1.02, id="gru11-weight_hh-r"),
          pytest.param(LSTM, ("lstm", 12, 3, 5), "rnn.weight_hh_l0", 0, 1.02, id="lstm12-weight_hh-i"),
          pytest.param(LSTM, ("lstm", 12, 3, 5), "rnn.weight_hh_l0", 1, 1.02, id="lstm12-weight_hh-f"),
          pytest.param(LSTM, ("lstm", 12, 3, 5), "rnn.weight_hh_l0", 3, 1.02, id="lstm12-weight_hh-o"),
          pytest.param(JANET, ("pgjanet", 11, 5, 200), "W_f.weight", None, 1.10, id="pgjanet11-W_f"),
          pytest.param(JANET, ("neuraltx", 36, 3, 5), "network.", None, 1.30, id="neuraltx36-tcn-stack")]


@pytest.mark.parametrize("mod,args,tensor,gate,factor", FAULTS)
def test_planted_fault_passes_flat_and_fails_by_block(mod, args, tensor, gate, factor):
    net, x, dy = mod.ragged_case(*args, device="cpu")
    ref, _ = _oracle_grads(args[0], args[1], 0.0, 0.0, net, x, dy)
    blocks = net_grad_blocks(net)
    hit = [b for b in blocks if ("backbone." + tensor) in b[0] and (gate is None or b[0].endswith(f"[{gate}]"))]
    assert hit and (gate is None or len(hit) == 1)
    got = ref.copy()
    for _, a, b in hit:
        got[a:b] *= factor
    assert rel_err(got, ref) < mod.GRAD_TOL                                  # the gap: the flat scale lets the fault through
    assert_grad_blocks(ref, ref, blocks, mod.GRAD_TOL)
    with pytest.raises(AssertionError, match="worst block") as e:
        assert_grad_blocks(got, ref, blocks, mod.GRAD_TOL)
    assert any(b[0] in str(e.value) for b in hit) and "of the flat maximum" in str(e.value)
    errs = {label: own for label, own, _, _ in grad_block_errors(got, ref, blocks)}
    assert all(abs(errs[b[0]] - (factor - 1)) < 1e-6 for b in hit)


def test_zero_reference_block_stays_on_the_flat_scale():
    blocks = grad_blocks([("backbone.rnn.weight_ih_l0", (6, 2)), ("backbone.rnn.weight_hh_l0", (6, 2)), ("backbone.fc_out.bias", (2,))], 2)
    assert [b[0] for b in blocks][3:6] == [f"backbone.rnn.weight_hh_l0[{i}]" for i in range(3)]
    ref = np.zeros(26)
    ref[:12] = np.linspace(0.01, 0.02, 12)
    ref[24:] = (4.0, -3.0)                  # weight_hh (T = 1: no previous state) has no gradient at all
    tol = 1e-4
    got = ref.copy()
    got[14] = 0.9 * tol * 4.0
    assert_grad_blocks(got, ref, blocks, tol)
    with pytest.raises(AssertionError, match=r"weight_hh_l0\[0\] \(zero reference\)"):
        assert_grad_blocks(got, ref, blocks, tol, exact_zeros=True)
    got[14] = 1.1 * tol * 4.0
    with pytest.raises(AssertionError):
        assert_grad_blocks(got, ref, blocks, tol)
    got[14] = 0.0
    assert_grad_blocks(got, ref, blocks, tol, exact_zeros=True)
    got[0] += 0.9 * tol * 4.0               # inside the flat tolerance, 90 times this block's own
    assert rel_err(got, ref) < tol
    with pytest.raises(AssertionError, match=r"worst block backbone.rnn.weight_ih_l0\[0\]"):
        assert_grad_blocks(got, ref, blocks, tol)
