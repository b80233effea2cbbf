#!/usr/bin/env python3
"""Train-step time of the lane-per-unit kernels (csrc/gru_wide.hip, lstm_wide.hip: 33 .. 64 hidden units; gru_layers2.hip: two layers) at the reference's batch
shapes, next to the ATen restatement they replaced (backbones/wide.py + torch.optim.AdamW).  usage (GPU box): PYTHONPATH=. python tools/wide_bench.py
--kernels-only [--json FILE]: the kernel column alone, plus one forward + backward of the state route (gru H 40 from a non-zero h_0), the
medians also as JSON — one visit of a comparison between two builds of the library ($OPENDPD_HIP_LIB; profiles/wide_refactor.md)."""
import json
import sys
import warnings

import torch

from opendpd_amd import CoreModel
from opendpd_amd.backbones import wide as W
from opendpd_amd.train_funcs import FusedAdamW, fused_train_step


def timeit(fn, n=10, w=2):
    for _ in range(w):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return ts[len(ts) // 2]


KERNELS_ONLY = "--kernels-only" in sys.argv
JSON_OUT = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else ""
medians = {}
print("| model | B x T | kernels: step ms | ATen restatement: step ms |\n|---|---|---|---|")
for bb, H, NL in (("gru", 48, 1), ("dgru", 40, 1), ("dgru", 64, 1), ("qgru", 36, 1), ("lstm", 48, 1), ("vdlstm", 40, 1), ("deltagru", 40, 1), ("deltagru_tcnskip", 48, 1), ("pgjanet", 24, 1), ("gru", 8, 2), ("gru", 23, 2), ("qgru", 32, 2)):
    for B, T in ((64, 50), (256, 200), (2048, 200)):
        g = torch.Generator(device="cuda").manual_seed(B)
        x = (torch.rand(B, T, 2, device="cuda", generator=g) - 0.5) * 1.6
        x = x + 0.05 * torch.sign(x)
        t = torch.randn(B, T, 2, device="cuda", generator=g) * 0.3
        torch.manual_seed(0)
        net = CoreModel(2, H, NL, bb, **({"thx": 0.01, "thh": 0.05} if "delta" in bb else {})).cuda()
        opt = FusedAdamW(net, lr=1e-4)
        ms = timeit(lambda: fused_train_step(opt, x, t, "l2", 200.0))
        medians[f"{bb} H{H} x{NL} {B}x{T}"] = ms
        if KERNELS_ONLY:
            print(f"| {bb} H{H}{' x 2 layers' if NL == 2 else ''} | {B} x {T} | {ms:.3f} | |", flush=True)
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            old = dict(W.KERNEL_HIDDEN_LIMIT)
            W.KERNEL_HIDDEN_LIMIT.update(gru=32, dgru=32, qgru=32, qgru_amp1=32, lstm=32, vdlstm=32, deltagru=32, deltagru_tcnskip=32, pgjanet=16)
            old2, W.TWO_LAYER_KERNELS = W.TWO_LAYER_KERNELS, ()
            ref = CoreModel(2, H, NL, bb, **({"thx": 0.01, "thh": 0.05} if "delta" in bb else {})).cuda()
            W.KERNEL_HIDDEN_LIMIT.update(old)
            W.TWO_LAYER_KERNELS = old2
        topt = torch.optim.AdamW(ref.parameters(), lr=1e-4)

        def aten_step():
            topt.zero_grad()
            loss = torch.nn.functional.mse_loss(ref(x), t)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), 200.0)
            topt.step()
        msa = timeit(aten_step, n=5, w=1)
        print(f"| {bb} H{H}{' x 2 layers' if NL == 2 else ''} | {B} x {T} | {ms:.3f} | {msa:.2f} |", flush=True)
if KERNELS_ONLY:
    for B, T in ((64, 50), (256, 200), (2048, 200)):      # the state route: CoreModel.forward(x, h_0) and its backward, gru H 40
        g = torch.Generator(device="cuda").manual_seed(B)
        x = (torch.rand(B, T, 2, device="cuda", generator=g) - 0.5) * 1.6
        x = x + 0.05 * torch.sign(x)
        h0 = (torch.rand(1, B, 40, device="cuda", generator=g) - 0.5).requires_grad_()
        torch.manual_seed(0)
        net = CoreModel(2, 40, 1, "gru").cuda()

        def state_step():
            net.zero_grad(set_to_none=True)
            net(x, h0).square().mean().backward()
        ms = timeit(state_step)
        medians[f"gru H40 state fwd+bwd {B}x{T}"] = ms
        print(f"| gru H40, h_0 given: forward + backward | {B} x {T} | {ms:.3f} | |", flush=True)
    if JSON_OUT:
        json.dump(medians, open(JSON_OUT, "w"), indent=1)
