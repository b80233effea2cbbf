"""Helpers shared by the parity tests: load a golden fixture and flatten its state dict."""
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Fixture:
    """One tests/golden/<name>.npz produced by oracle/gen_golden.py from the reference."""

    def __init__(self, name):
        self.name = name
        self.d = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
        self.meta = json.loads(str(self.d["meta"]))

    def keys(self, prefix):
        """Parameter names (state-dict order) stored under '<prefix>/'."""
        return [k[len(prefix) + 1:] for k in self.d if k.startswith(prefix + "/")]

    def param_names(self, sub=""):
        """State-dict keys that are parameters (have a gradient or are frozen weights), optional sub-model."""
        return [k for k in self.keys("sd") if k.startswith(sub)]

    def flat(self, prefix, names=None, strip=""):
        names = names if names is not None else self.keys(prefix)
        return np.concatenate([self.d[f"{prefix}/{strip}{k}"].reshape(-1) for k in names]).astype(np.float32)

    def sizes(self, names, prefix="sd", strip=""):
        return [int(self.d[f"{prefix}/{strip}{k}"].size) for k in names]

    def __getitem__(self, k):
        return self.d[k]

    def __contains__(self, k):
        return k in self.d


def rel_err(a, b):
    """max |a-b| / max(|b|) — scale-relative max error."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


_GATED = re.compile(r"(^|\.)rnn\.(rnn_cell_list\.\d+\.)?(weight_ih_l\d+|weight_hh_l\d+|bias_ih_l\d+|bias_hh_l\d+|x2h\.weight|h2h\.weight)$")


def grad_blocks(named_shapes, hidden):
    """(label, start, stop) of every block of a flat weight gradient.  `named_shapes`: the (name, shape) pairs of net.named_parameters() in
    flat-parameter order.  Every tensor is one block, except a tensor of the recurrent cell (rnn.weight_ih_l*, weight_hh_l*, bias_ih_l*,
    bias_hh_l*, x2h.weight, h2h.weight) whose first dimension is k * hidden with k > 1: its k gate blocks, labelled name[i]."""
    blocks, off = [], 0
    for name, shape in named_shapes:
        n = int(np.prod(shape, dtype=np.int64))
        k = shape[0] // hidden if len(shape) and hidden > 0 and shape[0] % hidden == 0 else 1
        if k > 1 and _GATED.search(name):
            for i in range(k):
                blocks.append((f"{name}[{i}]", off + i * (n // k), off + (i + 1) * (n // k)))
        else:
            blocks.append((name, off, off + n))
        off += n
    return blocks


def net_grad_blocks(net, hidden=None):
    """grad_blocks of a CoreModel (or a quantised one wrapping it)"""
    return grad_blocks([(k, tuple(p.shape)) for k, p in net.named_parameters()], net.hidden_size if hidden is None else hidden)


def grad_block_errors(got_flat, ref_flat, blocks):
    """per block: (label, max |got - ref| over the block / the block's own max |ref| — None where that is 0 —, the block's max |ref| /
    the flat max |ref|, max |got - ref| over the block / the flat max |ref|)"""
    got = np.asarray(got_flat, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref_flat, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape and blocks[0][1] == 0 and blocks[-1][2] == ref.size
    flat = max(float(np.max(np.abs(ref))), 1e-30)
    out = []
    for label, a, b in blocks:
        err, scale = float(np.max(np.abs(got[a:b] - ref[a:b]))), float(np.max(np.abs(ref[a:b])))
        out.append((label, err / scale if scale > 0 else None, scale / flat, err / flat))
    return out


def assert_grad_blocks(got_flat, ref_flat, blocks, tol, exact_zeros=False):
    """rel_err(got, ref) < tol on the flat vector, then max |got - ref| < tol * max |ref| over every block of `blocks` on the block's own
    scale.  A block whose reference is identically zero (weight_hh at T = 1) stays on the flat scale — with `exact_zeros` (the tests that
    held every tensor to its own scale before this helper did) it must be identically zero too.  Returns the worst block as
    (label, error on its own scale, its scale relative to the flat maximum)."""
    assert rel_err(got_flat, ref_flat) < tol, f"flat gradient error {rel_err(got_flat, ref_flat):.3g} >= {tol:g}"
    worst = None
    for label, own, scale, on_flat in grad_block_errors(got_flat, ref_flat, blocks):
        if own is None:
            assert (on_flat == 0.0) if exact_zeros else (on_flat < tol), f"block {label} (zero reference): error {on_flat:.3g} of the flat maximum"
        elif worst is None or own > worst[1]:
            worst = (label, own, scale)
    assert worst is None or worst[1] < tol, (f"worst block {worst[0]}: error {worst[1]:.3g} of its own scale >= {tol:g}; "
                                             f"the block's scale is {worst[2]:.3g} of the flat maximum")
    return worst


def apnrru_noise_mask(hidden):
    """APNRRU (apnrru.py:77-99) feeds its cell the raw sample rotated by its own conjugate phase: the imaginary part of that
    feature is 0 up to rounding (~1e-9), so the gradient of W_u's column 7 is rounding noise (~1e-10) and AdamW — which normalises
    every gradient by its own magnitude — turns that noise into full-size steps.  Returns the flat-parameter mask of everything
    BUT that column: optimiser trajectories are compared on it."""
    n = 2 * hidden + 3
    m = np.ones(343 + 70 * hidden, dtype=bool)
    o_wu = 96 + 1 + n
    m[o_wu + 7:o_wu + 16 * (8 + n):8 + n] = False
    return m
