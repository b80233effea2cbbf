#!/usr/bin/env python3
"""Train-step time of `--quant` bojanet (H 12, W8A8) or dvrjanet (H 12, K 3, W8A8) on its kernels (csrc/bojanet_q.hip, csrc/dvrjanet_q.hip, through
fused_train_step: forward, loss, backward, reduction, clip + AdamW) next to the ATen route on the same GPU (opendpd_amd.quant._quantise_aten
called directly: one torch op per gate per time step, torch.optim.AdamW) and next to the float step of the same backbone.  Median and span of
device-event timings after warm-up, the three alternating per round in one process.
usage (GPU box): PYTHONPATH=. python tools/qcell_time.py --backbone {bojanet,dvrjanet} [--out FILE] [--rounds N]"""
import argparse
import json
import warnings

import torch

from opendpd_amd import CoreModel
from opendpd_amd.quant import _quantise_aten, get_quant_model
from opendpd_amd.train_funcs import FusedAdamW, fused_train_step

H, BITS, CLIP, LR = 12, 8, 200.0, 5e-4
MODEL_ARGS = {"bojanet": {}, "dvrjanet": {"num_dvr_units": 3}}


class _Proj:
    quant = True
    n_bits_w = n_bits_a = BITS
    pretrained_model = ""


def one(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", choices=sorted(MODEL_ARGS), required=True)
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qcell_time.py measures on a HIP device; none found")
    bb, kw = a.backbone, MODEL_ARGS[a.backbone]
    rows = []
    print(f"| B x T | kernels ({bb}_q.hip): step ms, median (min .. max) | ATen route: step ms | float {bb}: step ms | ATen / kernels | "
          "kernels / float |\n|---|---|---|---|---|---|")
    for B, T in ((256, 200), (4096, 200)):
        g = torch.Generator(device="cuda").manual_seed(B)
        x = 0.3 * torch.randn(B, T, 2, device="cuda", generator=g) + 0.1
        t = 0.3 * torch.randn(B, T, 2, device="cuda", generator=g)
        torch.manual_seed(0)
        fnet = CoreModel(2, H, 1, bb, **kw).cuda()
        sd = {k: v.clone() for k, v in fnet.state_dict().items()}
        q = get_quant_model(_Proj, fnet)
        assert q.backbone.native
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            src = CoreModel(2, H, 1, bb, **kw).cuda()
            src.load_state_dict(sd)
            at = _quantise_aten(src, BITS, BITS, "", torch.device("cuda"))
        assert not at.backbone.native
        at.load_state_dict(q.state_dict())
        fl = CoreModel(2, H, 1, bb, **kw).cuda()
        fl.load_state_dict(sd)
        qopt, fopt = FusedAdamW(q, lr=LR), FusedAdamW(fl, lr=LR)
        topt = torch.optim.AdamW(at.parameters(), lr=LR)

        def aten_step():
            topt.zero_grad()
            loss = torch.nn.functional.mse_loss(at(x), t)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(at.parameters(), CLIP)
            topt.step()

        steps = {"kernels": lambda: fused_train_step(qopt, x, t, "l2", CLIP), "aten": aten_step, "float": lambda: fused_train_step(fopt, x, t, "l2", CLIP)}
        for name, fn in steps.items():      # warm-up of every shape the timed window uses
            for _ in range(1 if name == "aten" else 3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in steps}
        for _ in range(a.rounds):
            for name, fn in steps.items():
                n = 1 if name == "aten" else 20      # (the kernel steps are a fraction of a millisecond: time twenty of them per sample)
                ms[name].append(one(lambda: [fn() for _ in range(n)]) / n)
        med = {k: median(v) for k, v in ms.items()}
        spread = {k: (min(v), max(v)) for k, v in ms.items()}
        rows.append(dict(backbone=bb, B=B, T=T, H=H, **kw, bits=BITS, median_ms=med, min_max_ms=spread, samples_ms=ms))
        span = {k: f"{med[k]:.3f} ({spread[k][0]:.3f} .. {spread[k][1]:.3f})" for k in med}
        print(f"| {B} x {T} | {span['kernels']} | {span['aten']} | {span['float']} | {med['aten'] / med['kernels']:.0f} x | "
              f"{med['kernels'] / med['float']:.2f} x |", flush=True)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
