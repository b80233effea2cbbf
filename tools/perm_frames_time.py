#!/usr/bin/env python3
"""Times the bench workload's fused DGRU-H13 train step (65 536 x 200, frames addressed in place) with the frame order real training uses:
a random permutation of the stream's frame starts instead of bench.py's 0, 1, 2, ... — consecutive rows of a wave then start anywhere in the
stream, so the row loads of a staged chunk do not share cache lines.  One child process per library ($OPENDPD_HIP_LIB) and order, as
tools/exp_time.py.   python tools/perm_frames_time.py [lib.so ...]   (no argument: the in-tree library; $EXP_STEPS steps, default 100)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r"""
import sys, json, os, torch
sys.path.insert(0, %r)
import bench
from opendpd_amd import CoreModel
from opendpd_amd.train_funcs import FusedAdamW, FrameBatch
B, T, H = 65536, 200, 13
dev = torch.device("cuda:0")
torch.manual_seed(0)
net = CoreModel(2, H, 1, "dgru").to(dev)
opt = FusedAdamW(net, lr=5e-4)
xs, ys = bench.synth_frames(B, T, 0, dev, materialize=False)        # B + T - 1 samples: exactly B distinct frame starts
order = torch.arange(B, device=dev, dtype=torch.int64)
if sys.argv[1] == "perm":
    order = torch.randperm(B, generator=torch.Generator().manual_seed(11)).to(dev)
NS = int(os.environ.get("EXP_STEPS", "100"))
dt, kern_ms, loss = bench.run_steps(opt, FrameBatch(xs, ys, order, T, 1), None, NS, 3, B * T * 2, None, events=True)
print(json.dumps({"order": sys.argv[1], "ms_per_step": dt / NS * 1e3, "kernel_ms_mean": kern_ms, "loss": loss}))
""" % ROOT


def main():
    for lib in sys.argv[1:] or [""]:
        env = dict(os.environ)
        if lib:
            env["OPENDPD_HIP_LIB"] = os.path.abspath(lib)
        for order in ("arange", "perm"):
            out = subprocess.run([sys.executable, "-c", CHILD, order], env=env, capture_output=True, text=True)
            line = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else out.stderr[-600:]
            print(f"{os.path.relpath(lib, ROOT) if lib else 'in-tree'}: {line}", flush=True)
            if out.returncode != 0:      # a failed child: nothing more is started on the device
                sys.exit(out.returncode if out.returncode > 0 else 1)


if __name__ == "__main__":
    main()
