#!/usr/bin/env python3
"""Reference vectors for CoreModel.forward(x, h_0) with a non-zero initial state (tests/test_init_state_*.py).

Runs the reference's own CoreModel (models.py:150-160) on the CPU with a seeded non-zero h_0 of shape (1, B, H) and an MSE loss, and
writes tests/golden/h0_<backbone>_h<H>.npz: the state dict (sd/<key>), x, h0, the target, y, the loss, dL/dx (gx), every parameter's
gradient (g/<key>) and dL/dh_0 (gh0).  For deltagru_tcnskip and vdlstm, whose backbones ignore h_0, it records y with h_0 (y) and without
(y_none) instead.  Only the vectors are committed; the reference is needed to regenerate them, never to test.

Usage:  python tools/gen_golden_h0.py /path/to/reference      (writes tests/golden/h0_*.npz)
"""
import json
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

# (backbone, hidden, B, T, seed): the state route's backbones, and two that ignore h_0
CASES = [("gru", 8, 3, 37, 1), ("dgru", 13, 4, 50, 2), ("qgru", 10, 5, 41, 3), ("qgru_amp1", 16, 3, 64, 4), ("lstm", 9, 4, 70, 5),
         ("gru", 40, 3, 65, 6), ("lstm", 48, 5, 38, 7)]
IGNORING = [("deltagru_tcnskip", 15, 3, 40, 8), ("vdlstm", 8, 4, 45, 9)]


def frames(B, T, rng):
    amp = 0.05 + 0.85 * rng.rand(B, T, 1)
    ph = 2 * np.pi * rng.rand(B, T, 1)
    return np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)


def main(ref):
    sys.path.insert(0, ref)
    sys.dont_write_bytecode = True
    import torch
    torch.set_num_threads(1)
    import quant      # (the reference's quant/__init__ does not export Sqrt / Pow, which backbones/qgru.py imports from it)
    from quant.modules.ops import Sqrt, Pow
    quant.Sqrt, quant.Pow = Sqrt, Pow
    import models as ref_models

    def build(bb, H, seed):
        torch.manual_seed(seed)
        net = ref_models.CoreModel(input_size=2, hidden_size=H, num_layers=1, backbone_type=bb)
        with torch.no_grad():      # the registry initialises the biases to 0: make them count
            for k, p in net.named_parameters():
                if "bias" in k:
                    p.uniform_(-0.3, 0.3)
        return net

    for bb, H, B, T, seed in CASES + IGNORING:
        net = build(bb, H, seed)
        rng = np.random.RandomState(100 + seed)
        x = frames(B, T, rng)
        h0 = (0.6 * rng.randn(1, B, H)).astype(np.float32)
        tgt = (0.3 * rng.randn(B, T, 2)).astype(np.float32)
        out = {f"sd/{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()}
        out.update(x=x, h0=h0, tgt=tgt)
        xt = torch.from_numpy(x).clone().requires_grad_(True)
        ht = torch.from_numpy(h0).clone().requires_grad_(True)
        y = net(xt, ht)
        if (bb, H, B, T, seed) in IGNORING:
            with torch.no_grad():
                out["y_none"] = net(torch.from_numpy(x)).numpy().copy()
            out["y"] = y.detach().numpy().copy()
        else:
            loss = torch.nn.functional.mse_loss(y, torch.from_numpy(tgt))
            loss.backward()
            out.update(y=y.detach().numpy().copy(), loss=np.array([loss.item()]), gx=xt.grad.numpy().copy(), gh0=ht.grad.numpy().copy())
            for k, p in net.named_parameters():
                out[f"g/{k}"] = p.grad.detach().numpy().copy()
        out["meta"] = np.array(json.dumps({"backbone": bb, "hidden": H, "B": B, "T": T, "seed": seed, "num_layers": 1}))
        path = os.path.join(OUT, f"h0_{bb}_h{H}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("OPENDPD_REFERENCE", "../reference"))
