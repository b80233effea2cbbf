#!/usr/bin/env python3
"""bench.py — throughput of the OpenDPD train step on MI355X.

Metric (BASELINE.json): IQ samples/s in the train step (forward + MSE + BPTT + clip_grad_norm_(200)
+ AdamW, modules/train_funcs.py:33-44) for the ~1k-parameter DGRU (hidden 13, 1041 params) on
APA_200MHz-shaped frames (T = 200, fp32 I/Q), data-parallel over N GPUs (one process per GPU, one
RCCL all-reduce of P+4 floats per step).  Synthetic band-limited frames, random-init weights.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
           --master-port 29500 bench.py --gpus 8 --steps 20 --warmup 3

Prints ONE JSON line on rank 0.  `value` = whole-job IQ samples/s with inputs resident in HBM, `ms_per_step` = one
timed step.  `--dump-outputs DIR` also writes what the last timed step left its caller (loss, parameters, gradient,
AdamW moments) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared array for array.
`roofline` prices the dominant kernel (the fused fwd+loss+bwd launch).  The step is compute bound
(~360 flop per algorithmic byte): the bound that binds is the exact-fp32 MFMA / vector rate (157.3
TFLOP/s, the two are the same rate on gfx950), priced with ALGORITHMIC flops = 2 x 3 x 948 MACs per IQ
sample (forward, data gradient, weight gradient of the DGRU-H13 cell + head; recompute and padding not
counted).  The HBM figures (algorithmic bytes = 16 B per IQ sample: fp32 I,Q input + fp32 I,Q target,
SURVEY §8d) are reported next to it under `roofline.hbm`, and `traffic` is the measured HBM bytes.
`cpu_baseline` times the CPU oracle (a port of the reference step, oracle/odpd_oracle.c) on the host
cores of the same box, on a bounded sample (rank 0, N = 1 only).
"""
import argparse
import json
import os
import sys
import time

# Multi-process GPU work on this image needs dmabuf IPC (the host driver has no legacy IPC: without this RCCL and hipIpc handle
# exchange fail with `hipIpcGetMemHandle: invalid argument`).  The GPU boxes export it already; it is set HERE, before anything
# touches the GPU, so that the driver's own `python -m torch.distributed.run ... bench.py` line needs nothing from its caller.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: 8 TB/s spec
VALU_FP32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32 vector peak = exact-fp32 (f32-input) MFMA peak
ALGO_BYTES_PER_SAMPLE = 16.0


def dgru_macs(H):
    """forward multiply-accumulates of one IQ sample through DGRU(H): W_ih (3H x 6), W_hh (3H x H), fc_hid (H x H), fc_out (2 x (H + 6))"""
    return 3 * H * 6 + 3 * H * H + H * H + 2 * (H + 6)


def flops_train_pa_dgru(H):
    """algorithmic flops of the train_pa step per IQ sample: forward + data gradient + weight gradient = 2 x 3 x MACs, MINUS the data
    gradient through the input projection and through fc_out's feature columns (2 x (3H x 6 + 2 x 6)): train_pa never needs dL/dx."""
    return 2 * 3 * dgru_macs(H) - 2 * (3 * H * 6 + 2 * 6)


def flops_frozen_dgru(H):
    """frozen PA inside train_dpd: forward + full data gradient (down to dL/du), no weight gradient"""
    return 2 * 2 * dgru_macs(H)


def vdlstm_macs(H):
    """forward multiply-accumulates of one IQ sample through VDLSTM(H): W_ih (4H x 4), W_hh (4H x H), the two lambda heads (4 x H each), fc_out (2 x 8)"""
    return 4 * H * 4 + 4 * H * H + 2 * 4 * H + 2 * 8


def flops_train_pa_vdlstm(H):
    """train_pa step: forward + data gradient + weight gradient, minus the data gradient through the input projection (never formed)"""
    return 2 * 3 * vdlstm_macs(H) - 2 * (4 * H * 4)


TRES15_MACS = 3 * 15 * 6 + 3 * 15 * 15 + 2 * 15 + (2 * 3 * 3 + 3 * 2)      # x2h, h2h, fc_out, TCN skip = 999 (= its parameter count)
FLOPS_TRAIN_TRES15 = 2 * 3 * TRES15_MACS - 2 * (3 * 15 * 6 + 2 * 3 * 3)         # trained DPD: no dL/dx through x2h / the first conv
QGRU10_MACS = 3 * 10 * 4 + 3 * 10 * 10 + 2 * 10
FLOPS_TRAIN_QGRU10 = 2 * 3 * QGRU10_MACS - 2 * (3 * 10 * 4)
FLOP_PER_SAMPLE = {13: flops_train_pa_dgru(13)}     # 5 196 (r01 / r02 counted 5 688: with the input data gradient train_pa does not compute)


def synth_frames(n_frames, T, seed, device, materialize=True):
    """APA_200MHz-shaped synthetic frames: band-limited complex Gaussian stream (occupied bandwidth
    200/983.04 of fs), peak-normalised to 0.914, no sample with |x| < 1e-3, framed at stride 1 exactly as
    IQFrameDataset does (data_collector.py:239-247); target = memory-polynomial PA-like map of x.
    materialize=False returns the two (N,2) streams instead of the (n_frames,T,2) frame tensors."""
    g = torch.Generator(device=device).manual_seed(seed)
    n = n_frames + T - 1
    nfft = 1 << (n - 1).bit_length()
    spec = torch.complex(torch.randn(nfft, generator=g, device=device), torch.randn(nfft, generator=g, device=device))
    f = torch.fft.fftfreq(nfft, device=device).abs()
    spec = spec * (f <= 0.5 * 200.0 / 983.04)
    x = torch.fft.ifft(spec)[:n]
    x = x / x.abs().max() * 0.914
    small = x.abs() < 1e-3
    x = torch.where(small, torch.full_like(x, 1e-3), x)
    a2 = (x.real ** 2 + x.imag ** 2)
    xm1 = torch.roll(x, 1)
    y = x * (1.0 - 0.25 * a2 + 0.05 * a2 * a2) + 0.08 * xm1 * (1.0 - 0.3 * a2)
    xs = torch.view_as_real(x).float()
    ys = torch.view_as_real(y).float()
    if not materialize:
        return xs.contiguous(), ys.contiguous()
    fx = xs.unfold(0, T, 1).permute(0, 2, 1).contiguous()   # (n_frames, T, 2)
    fy = ys.unfold(0, T, 1).permute(0, 2, 1).contiguous()
    return fx, fy


def cascade_spans(opt, x, t, count, n=5):
    """mean HIP-event time (ms) of every launch group of the cascade step (train_funcs._cascade_train_step), over n steps"""
    from opendpd_amd.train_funcs import fused_train_step
    spans = []
    for _ in range(n):
        fused_train_step(opt, x, t, "l2", 200.0, count, timing=spans)
    torch.cuda.synchronize()
    out = {}
    for name, a, b in spans:
        out.setdefault(name, []).append(a.elapsed_time(b))
    return {k: float(np.mean(v)) for k, v in out.items()}


def run_steps(opt, x, t, steps, warmup, count, dist, events=False):
    from opendpd_amd.train_funcs import fused_train_step
    for _ in range(warmup):
        fused_train_step(opt, x, t, "l2", 200.0, count)
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] if events else None
    t0 = time.perf_counter()
    loss = None
    for i in range(steps):
        loss = fused_train_step(opt, x, t, "l2", 200.0, count, timing=evs[i] if events else None)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in evs])) if events else None
    return el, kern_ms, float(loss.item())


def dump_outputs(out_dir, net, opt, loss):
    """What the timed steps left their caller after the last one, as out_dir/<name>.npy (float32): the step's loss, every parameter of
    the trained model under its state-dict name, and the optimiser state the next step starts from (the last step's gradient, the
    AdamW moments).  The inputs are seeded, so two builds run with the same arguments can be compared array for array."""
    os.makedirs(out_dir, exist_ok=True)
    P = opt.backbone.n_flat
    arrays = {"loss": torch.tensor([loss]), "grad": opt.grad[:P], "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
    arrays.update({f"param.{k}": v for k, v in net.named_parameters()})
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.detach().to("cpu", torch.float32).numpy())


class _EpochLoader:
    """what FusedAdamW.train_epoch reads from project.DeviceFrameLoader: resident streams + the epoch's frame order"""

    def __init__(self, xs, ys, T, batch, n_frames):
        self.x, self.y, self.frame_length, self.stride, self.batch_size, self.n = xs, ys, T, 1, batch, n_frames
        self._order = torch.randperm(n_frames, generator=torch.Generator().manual_seed(11)).to(xs.device)

    def epoch_order(self):
        return self._order


def strong_scaling_epoch(H, T, global_batch, dev, dist, world, steps=200):
    """`steps` train_pa steps of DGRU(H) at a FIXED global batch sharded over the ranks, through the native epoch loop; max over ranks"""
    from opendpd_amd import CoreModel
    from opendpd_amd.train_funcs import FusedAdamW
    torch.manual_seed(5)
    net = CoreModel(2, H, 1, "dgru").to(dev)
    opt = FusedAdamW(net, lr=5e-4)
    n_frames = global_batch * steps
    xs, ys = synth_frames(n_frames, T, seed=77, device=dev, materialize=False)     # the same stream on every rank
    loader = _EpochLoader(xs, ys, T, global_batch, n_frames)
    if not opt.can_run_epoch(loader):
        return {"skipped": "no native epoch loop for this shard size / collective"}
    best = None
    for it in range(3):          # first pass = warm-up; best of the other two
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = opt.train_epoch(loader, "l2", 200.0)
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        el = torch.tensor([time.perf_counter() - t0], device=dev, dtype=torch.float64)
        if dist is not None:
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
        if it and (best is None or float(el.item()) < best):
            best = float(el.item())
    return {"global_batch": global_batch, "frames_per_gpu": global_batch / world, "steps": steps, "ms_per_step": 1e3 * best / steps,
            "value": global_batch * T * steps / best, "unit": "IQ samples/s", "loss_last": float(losses[-1].item())}


def cpu_baseline(H, T, budget_1t_s=4.0, budget_nt_s=2.0, big_batch=8192):
    """Reference-step port (oracle) on the host cores; bounded sample of the same workload (~25-30 s in total).  OpenMP over the
    sequences of a batch.  Two batches: the reference's 256 x T (arguments.py:32) — where a 256-sequence batch does not scale to every
    core of a large host, so the thread count is swept — and a CPU-saturating `big_batch` x T at the thread counts that did best.
    `value` / `cores` report the best rate over both; `by_batch` keeps each batch's own best, so that GPU / CPU ratios are formed at
    MATCHED batch (main() adds them)."""
    from oracle.oracle import Oracle, make_model
    o = Oracle("f32")
    m = make_model("dgru", H)
    rng = np.random.RandomState(0)
    P = o.param_count(m)
    cores = o.max_threads()
    try:
        cores = min(cores, len(os.sched_getaffinity(0)))
    except AttributeError:
        pass

    def make(B):
        x = (0.05 + 0.8 * rng.rand(B, T, 2)).astype(np.float32)
        t = rng.rand(B, T, 2).astype(np.float32)
        return dict(B=B, x=x, t=t, p=(rng.randn(P) * 0.2).astype(np.float32), mom=np.zeros(P, np.float32), var=np.zeros(P, np.float32),
                    scratch=(np.empty_like(x), np.empty_like(x), np.empty(P, np.float32)))

    def timed(w, budget, max_steps):
        o.train_step(m, w["p"], w["x"], w["t"], w["mom"], w["var"], 1, 5e-4, 200.0, scratch=w["scratch"])  # warm-up
        n, t0 = 0, time.perf_counter()
        while True:
            o.train_step(m, w["p"], w["x"], w["t"], w["mom"], w["var"], n + 2, 5e-4, 200.0, scratch=w["scratch"])
            n += 1
            el = time.perf_counter() - t0
            if el > budget or n >= max_steps:
                return n, el

    small = make(256)
    o.set_threads(1)
    n1, el1 = timed(small, budget_1t_s, 200)
    sweep = {1: 256 * T * n1 / el1}
    steps = {1: (n1, el1)}
    for nt in sorted({c for c in (4, 8, 16, 32, 64, cores) if 1 < c <= cores}):
        o.set_threads(nt)
        n, el = timed(small, budget_nt_s, 2000)
        sweep[nt] = 256 * T * n / el
        steps[nt] = (n, el)
    best = max(sweep, key=sweep.get)
    total = sum(v[1] for v in steps.values())
    by_batch = {"256": {"value": sweep[best], "cores": best, "steps": steps[best][0], "seconds": steps[best][1]}}
    # the CPU-saturating batch: every core has >= 64 sequences; thread counts = all cores and the two best of the small sweep
    big = make(big_batch)
    big_sweep = {}
    for nt in sorted({cores, *sorted(sweep, key=sweep.get)[-2:]} - {1}) or [1]:
        o.set_threads(nt)
        n, el = timed(big, budget_nt_s, 50)
        big_sweep[nt] = (big_batch * T * n / el, n, el)
        total += el
    bbest = max(big_sweep, key=lambda k: big_sweep[k][0])
    by_batch[str(big_batch)] = {"value": big_sweep[bbest][0], "cores": bbest, "steps": big_sweep[bbest][1], "seconds": big_sweep[bbest][2],
                                "threads_swept": {str(k): round(v[0]) for k, v in big_sweep.items()}}
    top = max(by_batch, key=lambda k: by_batch[k]["value"])
    return {"value": by_batch[top]["value"], "unit": "IQ samples/s", "cores": by_batch[top]["cores"], "kind": "port",
            "value_1thread": sweep[1], "host_cores_visible": cores, "batch": int(top),
            "threads_swept": {str(k): round(v) for k, v in sweep.items()}, "by_batch": by_batch,
            "sample": f"{by_batch[top]['steps']} train steps of DGRU H{H} on a {top}x{T} synthetic batch ({by_batch[top]['seconds']:.1f} s at "
                      f"{by_batch[top]['cores']} OpenMP threads over sequences; thread sweep at 256x{T} and {big_batch}x{T}: {total:.0f} s of CPU in total)"}


HEADLINE_SOURCES = ("gru_s16.hip", "odpd_s16.h", "odpd_device.h", "odpd_seq.h")


def kernel_source_sha1(files=HEADLINE_SOURCES):
    """identifies the build of a kernel group: sha1 over its sources (default: the headline kernel's)"""
    import hashlib
    h = hashlib.sha1()
    for f in files:
        h.update(open(os.path.join(ROOT, "opendpd_amd", "csrc", f), "rb").read())
    return h.hexdigest()


def measured_traffic(key):
    """HBM bytes per step of a workload from the PMC passes recorded in profiles/pmc_traffic.json (rocprofv3 cannot run inside this
    process): valid for the kernel SOURCES it was measured on — an entry carries the list of source files and their sha1, changed
    sources report None."""
    pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        ent = json.load(open(pmc)).get(key, {})
        if ent and ent.get("source_sha1") == kernel_source_sha1(tuple(ent.get("source_files", HEADLINE_SOURCES))):
            return ent.get("hbm_bytes_per_launch")
    except Exception:
        pass
    return None


def host_cpu_info():
    """what the CPU baseline had to run on: logical CPUs, the affinity mask of this process and the cgroup CPU quota (cpu.max: "max" or
    quota / period in microseconds) — a quota below the visible core count is why a thread sweep peaks early and collapses beyond it"""
    info = {"nproc": os.cpu_count()}
    try:
        info["affinity"] = len(os.sched_getaffinity(0))
    except AttributeError:
        info["affinity"] = None
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            raw = open(path).read().split()
            if path.endswith("cpu.max"):
                quota = None if raw[0] == "max" else float(raw[0]) / float(raw[1])
            else:
                q = float(raw[0])
                quota = None if q <= 0 else q / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            info["cgroup_source"] = path
            break
        except Exception:
            continue
    info["cgroup_cpu_quota_cores"] = quota
    try:
        info["loadavg_1min"] = os.getloadavg()[0]
    except OSError:
        pass
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                info["model"] = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return info


def bare_collective_us(comm, n_floats, dev, reps=1000):
    """microseconds per all-reduce of `n_floats` floats through a library-owned communicator, `reps` back to back on the stream"""
    buf = torch.zeros(n_floats, dtype=torch.float32, device=dev)
    for _ in range(20):
        comm.allreduce_sum_(buf)
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        comm.allreduce_sum_(buf)
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=65536, help="frames per GPU per step (saturating batch)")
    ap.add_argument("--ref-batch", type=int, default=256, help="reference batch (arguments.py:32) timed as a side figure")
    ap.add_argument("--hidden", type=int, default=13)
    ap.add_argument("--frame-length", type=int, default=200)
    ap.add_argument("--materialized", action="store_true",
                    help="feed (B,T,2) frame tensors (what IQFrameDataset materialises) instead of frames addressed in place "
                         "inside the resident I/Q stream (SURVEY §8 f3; same kernels, same arithmetic)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-cascade", action="store_true", help="skip the train_dpd (cascade) side figure")
    ap.add_argument("--no-strong", action="store_true", help="skip the strong-scaling figures at the reference's global batch sizes")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what their last step left the caller (loss, parameters, gradient, AdamW moments) "
                         "as DIR/<name>.npy (float32; rank 0)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # functional test of the N > 1 path on a single-GPU box (tools/dist_smoke.sh): every rank on device 0, gloo backend
    backend = os.environ.get("ODPD_BENCH_BACKEND", "nccl")
    if os.environ.get("ODPD_BENCH_SINGLE_DEVICE"):
        local = 0
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback in the product path)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1 or "RANK" in os.environ:
        # one process per GPU, RCCL process group over xGMI ("nccl" is RCCL on ROCm).  Under torchrun a world of ONE rank goes through
        # the same rendezvous / process group / barriers as a real job (tests/test_dp_gpu.py runs that on the one-GPU box)
        import torch.distributed as dist_mod
        from opendpd_amd import dist as odist
        odist.init(backend, device=dev, single=True)
        dist = dist_mod if dist_mod.is_initialized() else None
    assert world == args.gpus or world == 1, f"WORLD_SIZE={world} but --gpus {args.gpus}"

    from opendpd_amd import CoreModel
    from opendpd_amd.train_funcs import FusedAdamW
    H, T, B = args.hidden, args.frame_length, args.batch
    torch.manual_seed(0)                      # identical replicas on every rank
    net = CoreModel(2, H, 1, "dgru").to(dev)
    opt = FusedAdamW(net, lr=5e-4)
    # each rank owns its shard of the global batch: B stride-1 frames of its own stream
    if args.materialized:
        x, t = synth_frames(B, T, seed=1000 + rank, device=dev)
    else:
        from opendpd_amd.train_funcs import FrameBatch
        xs_, ys_ = synth_frames(B, T, seed=1000 + rank, device=dev, materialize=False)
        x, t = FrameBatch(xs_, ys_, torch.arange(B, device=dev, dtype=torch.int64), T, 1), None
    count = world * B * T * 2
    el, kern_ms, loss = run_steps(opt, x, t, args.steps, args.warmup, count, dist, events=True)
    if args.dump_outputs and rank == 0:      # before any side figure trains this model further
        dump_outputs(args.dump_outputs, net, opt, loss)
    el_t = torch.tensor([el], device=dev, dtype=torch.float64)
    if dist is not None:
        dist.all_reduce(el_t, op=dist.ReduceOp.MAX)
    el = float(el_t.item())
    value = world * B * T * args.steps / el

    # side figure: the same step back to back for >= 2 s (the headline's timed region is 20 steps = ~32 ms: this one is at steady clocks)
    sustained = None
    if not os.environ.get("ODPD_BENCH_NO_SUSTAINED"):
        n_s = max(args.steps, int(2.0 / (el / args.steps)) + 1)
        el_s, _, _ = run_steps(opt, x, t, n_s, 0, count, dist)
        el_s_t = torch.tensor([el_s], device=dev, dtype=torch.float64)
        if dist is not None:
            dist.all_reduce(el_s_t, op=dist.ReduceOp.MAX)
        sustained = {"steps": n_s, "seconds": float(el_s_t.item()), "ms_per_step": 1e3 * float(el_s_t.item()) / n_s,
                     "value": world * B * T * n_s / float(el_s_t.item()), "unit": "IQ samples/s"}

    # side figure: BASELINE configs[1]'s "bf16" — the same step with the resident streams STORED as bf16 pairs (4 bytes per I/Q sample,
    # odpd_frames_t.sample_format; widened exactly, fp32 arithmetic): halves the algorithmic bytes of a step that is compute bound
    bf16_frames = None
    if not args.materialized:
        netb = CoreModel(2, H, 1, "dgru").to(dev)
        optb = FusedAdamW(netb, lr=5e-4)
        xb = FrameBatch(xs_.to(torch.bfloat16), ys_.to(torch.bfloat16), torch.arange(B, device=dev, dtype=torch.int64), T, 1)
        elb, kernb, lossb = run_steps(optb, xb, None, max(3, min(args.steps, 10)), 2, count, dist, events=True)
        elb_t = torch.tensor([elb], device=dev, dtype=torch.float64)
        if dist is not None:
            dist.all_reduce(elb_t, op=dist.ReduceOp.MAX)
        nb = max(3, min(args.steps, 10))
        bf16_frames = {"workload": "the headline step on bf16-stored streams (fp32 arithmetic on the stored values)", "value": world * B * T * nb / float(elb_t.item()),
                       "unit": "IQ samples/s", "ms_per_step": 1e3 * float(elb_t.item()) / nb, "kernel_ms": kernb, "loss": lossb,
                       "algorithmic_bytes_per_sample": 8.0}
        del netb, optb, xb

    # side figure: BASELINE configs[3] — train_pa VDLSTM H13, the same batch per GPU, sharded the same way (tensor inputs: its
    # large-batch kernel takes (B,T,2) frames)
    cfg4 = None
    if not args.no_cascade:
        torch.manual_seed(4)
        net4 = CoreModel(2, 13, 1, "vdlstm").to(dev)
        opt4_ = FusedAdamW(net4, lr=5e-4)
        B4 = min(B, 32768)
        x4, t4 = synth_frames(B4, T, seed=2000 + rank, device=dev)
        n4 = max(3, min(args.steps, 10))
        el4_, _, loss4_ = run_steps(opt4_, x4, t4, n4, 2, world * B4 * T * 2, dist)
        el4_t = torch.tensor([el4_], device=dev, dtype=torch.float64)
        if dist is not None:
            dist.all_reduce(el4_t, op=dist.ReduceOp.MAX)
        tf4 = flops_train_pa_vdlstm(13) * world * B4 * T * n4 / float(el4_t.item()) / 1e12 / world
        cfg4 = {"workload": f"train_pa VDLSTM H13 ({net4.backbone.n_flat} params), T={T}, {B4} frames per GPU", "batch_per_gpu": B4,
                "value": world * B4 * T * n4 / float(el4_t.item()), "unit": "IQ samples/s", "ms_per_step": 1e3 * float(el4_t.item()) / n4,
                "loss": loss4_,
                "roofline": {"bound": "mfma", "achieved": tf4, "peak": VALU_FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf4 / VALU_FP32_PEAK_TFLOPS,
                             "algorithmic_flops_per_sample": flops_train_pa_vdlstm(13), "kernel": "lstm16_train_kernel<VDLSTM, 1 unit tile>",
                             "traffic": measured_traffic(f"vdlstm_h13_b{B4}_t{T}"),
                             "hbm": {"achieved": ALGO_BYTES_PER_SAMPLE * B4 * T * n4 / float(el4_t.item()) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                     "frac": ALGO_BYTES_PER_SAMPLE * B4 * T * n4 / float(el4_t.item()) / 1e9 / HBM_PEAK_GBS}}}
        del net4, opt4_, x4, t4

    # side figure (r06): train_pa of the PA every train_dpd run trains first — DGRU H23 (2 751 parameters; bash_scripts/OpenDPDv2.sh:39-52) —
    # at 32 768 frames per GPU: the fused train step on the bf16 matrix pipe with three-way operand splits (csrc/gru_s16x.hip,
    # gru16x_train_kernel), and the same step on the exact-fp32 kernel it replaced (knob "s16x_train" = 0) beside it
    h23 = None
    if not args.no_cascade and not args.materialized:
        from opendpd_amd import _lib as _l
        B23 = min(B, 32768)
        n23 = max(3, min(args.steps, 10))
        x23 = FrameBatch(xs_, ys_, torch.arange(B23, device=dev, dtype=torch.int64), T, 1)
        res23 = {}
        for knob in (1, 0):
            _l.load().odpd_set_tuning(b"s16x_train", knob)
            torch.manual_seed(23)
            o23 = FusedAdamW(CoreModel(2, 23, 1, "dgru").to(dev), lr=5e-4)
            el23, k23, loss23 = min((run_steps(o23, x23, None, n23, 2, world * B23 * T * 2, dist, events=True) for _ in range(2)), key=lambda r: r[0])
            e_t = torch.tensor([el23], device=dev, dtype=torch.float64)
            if dist is not None:
                dist.all_reduce(e_t, op=dist.ReduceOp.MAX)
            res23[knob] = (float(e_t.item()), k23, loss23, o23.backbone.n_flat)
            del o23
        _l.load().odpd_set_tuning(b"s16x_train", 1)
        el23, k23, loss23, np23 = res23[1]
        tf23 = flops_train_pa_dgru(23) * B23 * T / (k23 * 1e-3) / 1e12
        h23 = {"workload": f"train_pa DGRU H23 ({np23} params), T={T}, {B23} frames per GPU, fused fwd+MSE+BPTT+clip200+AdamW step", "batch_per_gpu": B23,
               "value": world * B23 * T * n23 / el23, "unit": "IQ samples/s", "ms_per_step": 1e3 * el23 / n23, "loss": loss23,
               "arithmetic": "v_mfma_f32_16x16x32_bf16 on three-way bf16 operand splits, six term products per product (>= 2^-16), fp32 accumulation, weight "
                             "gradient with both operands split: fp32-equivalent (parameter gradients <= 1.5e-6 of the fp64 oracle, tests/test_gru_s16x_train_gpu.py)",
               "exact_fp32_kernel": {"kernel": "gru16n_kernel<DGRU6, fused train> (v_mfma_f32_16x16x4_f32)", "ms_per_step": 1e3 * res23[0][0] / n23,
                                     "kernel_ms": res23[0][1], "loss": res23[0][2]},
               "roofline": {"bound": "mfma", "achieved": tf23, "peak": VALU_FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf23 / VALU_FP32_PEAK_TFLOPS,
                            "algorithmic_flops_per_sample": flops_train_pa_dgru(23), "kernel": "gru16x_train_kernel<DGRU6> (bf16x3 matrix pipe)", "kernel_ms": k23,
                            "traffic": measured_traffic(f"dgru_h23_b{B23}_t{T}"),
                            "note": "priced against the fp32 roof (157.3 TFLOP/s) because the arithmetic is fp32-equivalent; the instructions run on the bf16 pipe",
                            "hbm": {"achieved": ALGO_BYTES_PER_SAMPLE * B23 * T / (k23 * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": ALGO_BYTES_PER_SAMPLE * B23 * T / (k23 * 1e-3) / 1e9 / HBM_PEAK_GBS}}}
        del x23

    # side figure: the reference batch size (launch/latency-bound regime)
    ref = None
    if args.ref_batch and args.ref_batch != B:
        net2 = CoreModel(2, H, 1, "dgru").to(dev)
        opt2 = FusedAdamW(net2, lr=5e-4)
        if args.materialized:
            xr, tr = x[:args.ref_batch].contiguous(), t[:args.ref_batch].contiguous()
        else:
            xr, tr = FrameBatch(xs_, ys_, torch.arange(args.ref_batch, device=dev, dtype=torch.int64), T, 1), None
        elr, _, _ = run_steps(opt2, xr, tr, max(args.steps, 50), args.warmup, world * args.ref_batch * T * 2, dist)
        elr_t = torch.tensor([elr], device=dev, dtype=torch.float64)
        if dist is not None:
            dist.all_reduce(elr_t, op=dist.ReduceOp.MAX)
        ref = {"batch_per_gpu": args.ref_batch, "value": world * args.ref_batch * T * max(args.steps, 50) / float(elr_t.item()),
               "ms_per_step": 1e3 * float(elr_t.item()) / max(args.steps, 50)}

    # side figure: the same step at 8 192 frames (the batch at which the CPU baseline saturates the host's cores: matched-batch ratio)
    matched_8192 = None
    if world == 1 and not args.no_cpu_baseline and not args.materialized:
        net8 = CoreModel(2, H, 1, "dgru").to(dev)
        opt8 = FusedAdamW(net8, lr=5e-4)
        x8 = FrameBatch(xs_, ys_, torch.arange(8192, device=dev, dtype=torch.int64), T, 1)
        el8 = min(run_steps(opt8, x8, None, 30, 3, 8192 * T * 2, None)[0] for _ in range(2))
        matched_8192 = 8192 * T * 30 / el8
        del net8, opt8, x8

    # side figures of the reference's own shapes (latency regime, one sequence per wave): one evaluation pass over the APA_200MHz test
    # segment (net_eval, train_funcs.py:57-90: (1, 19 662, 2)) and the train step of the other recurrent families at the reference batch
    ref_shapes = None
    if world == 1 and ref is not None and not args.materialized:
        import time as _time
        ref_shapes = {}
        with torch.no_grad():
            xe = xs_[:19662].reshape(1, 19662, 2).contiguous() if xs_.shape[0] >= 19662 else None
            if xe is not None:
                net2.eval()
                for _ in range(3):
                    net2(xe)
                torch.cuda.synchronize()
                t0_ = _time.perf_counter()
                for _ in range(10):
                    net2(xe)
                torch.cuda.synchronize()
                ms = (_time.perf_counter() - t0_) / 10 * 1e3
                ref_shapes["eval_pass"] = {"workload": f"net_eval forward of DGRU H{H} on one (1, 19662, 2) segment", "ms": ms, "value": 19662 / ms * 1e3,
                                           "unit": "IQ samples/s"}
        xm = xs_.unfold(0, T, 1)[:args.ref_batch].permute(0, 2, 1).contiguous()
        tm = ys_.unfold(0, T, 1)[:args.ref_batch].permute(0, 2, 1).contiguous()
        steps_ = {}
        for bb_, h_ in (("gru", 11), ("lstm", 14), ("vdlstm", 13), ("pgjanet", 11), ("deltajanet", 15), ("bojanet", 12), ("apnrru", 8), ("dvrjanet", 12), ("mcldnn", 8)):
            torch.manual_seed(2)
            opt_ = FusedAdamW(CoreModel(2, h_, 1, bb_, **({"num_dvr_units": 3} if bb_ == "dvrjanet" else {})).to(dev), lr=5e-4)
            el_ = min(run_steps(opt_, xm, tm, 50, args.warmup, args.ref_batch * T * 2, None)[0] for _ in range(3))   # best of three: a one-off stall is 50 steps' worth here
            steps_[f"{bb_} H{h_}"] = {"ms_per_step": 1e3 * el_ / 50, "value": args.ref_batch * T * 50 / el_}
        ref_shapes["train_step"] = {"batch_per_gpu": args.ref_batch, "frame_length": T, "unit": "IQ samples/s", "backbones": steps_}

    # side figure: the train_dpd step (models.py:163-176) — the same 1k-parameter DGRU as the DPD in front of a frozen
    # DGRU PA model: DPD forward, PA forward, loss, PA backward (dL/du only), DPD backward, reduce, clip + AdamW
    dpd = None
    if world == 1 and not args.no_cascade:
        from opendpd_amd import CascadedModel
        torch.manual_seed(1)
        casc = CascadedModel(dpd_model=CoreModel(2, H, 1, "dgru"), pa_model=CoreModel(2, H, 1, "dgru"))
        casc.freeze_pa_model()
        casc = casc.to(dev)
        opt3 = FusedAdamW(casc, lr=5e-4)
        n3 = max(3, min(args.steps, 10))
        xc = x if args.materialized else xs_.unfold(0, T, 1)[:B].permute(0, 2, 1).contiguous()   # the cascade takes tensors
        tc = xc.clone()
        el3, _, loss3 = min((run_steps(opt3, xc, tc, n3, 2, world * B * T * 2, dist) for _ in range(2)), key=lambda r: r[0])   # (side figures: best of two short runs — a one-off allocator stall is worth several steps here)

        def priced(flops_per_sample, el_, n_, spans, kernels):
            """the cascade step against the fp32 MFMA / vector roof: algorithmic flops (DPD fwd + hidden-side dgrad + wgrad, frozen PA fwd +
            dgrad) over the whole step's time; `kernels` = the launch groups with their HIP-event times"""
            tf = flops_per_sample * B * T / (el_ / n_) / 1e12
            return {"bound": "mfma", "achieved": tf, "peak": VALU_FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / VALU_FP32_PEAK_TFLOPS,
                    "algorithmic_flops_per_sample": flops_per_sample, "kernels": kernels, "kernel_ms": spans,
                    "hbm": {"achieved": ALGO_BYTES_PER_SAMPLE * B * T / (el_ / n_) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": ALGO_BYTES_PER_SAMPLE * B * T / (el_ / n_) / 1e9 / HBM_PEAK_GBS}}

        dpd = {"workload": f"train_dpd: DGRU H{H} DPD -> frozen DGRU H{H} PA (cascade step: DPD fwd, frozen-PA fwd + loss + dL/du in one launch, DPD bwd), target = x",
               "value": B * T * n3 / el3, "unit": "IQ samples/s", "ms_per_step": 1e3 * el3 / n3, "loss": loss3,
               "roofline": priced(flops_train_pa_dgru(H) + flops_frozen_dgru(H), el3, n3, cascade_spans(opt3, xc, tc, world * B * T * 2),
                                  {"dpd_fwd": "gru16_fwd_kernel<DGRU6>", "pa_fwd_loss_dx": "gru16_train_kernel<DGRU6, frozen: loss + dL/du>",
                                   "dpd_bwd": "gru16_bwd_kernel<DGRU6>", "reduce_clip_optimiser": "reduce_partials_kernel + clip_adamw_kernel"})}
        del casc, opt3
        # north_star's target sentence: "IQ samples/sec in the train_dpd step for a ~1k-param DGRU" — the 1 041-parameter DGRU H13 as the
        # DPD in front of the frozen PA model the reference's OpenDPDv2 flow trains first (bash_scripts/OpenDPDv2.sh: dgru, hidden 23)
        torch.manual_seed(1)
        casc = CascadedModel(dpd_model=CoreModel(2, H, 1, "dgru"), pa_model=CoreModel(2, 23, 1, "dgru"))
        casc.freeze_pa_model()
        casc = casc.to(dev)
        optn = FusedAdamW(casc, lr=5e-4)
        eln, _, lossn = min((run_steps(optn, xc, tc, n3, 2, world * B * T * 2, dist) for _ in range(2)), key=lambda r: r[0])
        dpd["north_star"] = {"workload": f"train_dpd: DGRU H{H} ({net.backbone.n_flat} params) DPD -> frozen DGRU H23 PA (OpenDPDv2's PA), target = x",
                             "value": B * T * n3 / eln, "unit": "IQ samples/s", "ms_per_step": 1e3 * eln / n3, "loss": lossn,
                             "roofline": priced(flops_train_pa_dgru(H) + flops_frozen_dgru(23), eln, n3, cascade_spans(optn, xc, tc, world * B * T * 2),
                                                {"dpd_fwd": "gru16_fwd_kernel<DGRU6>", "pa_fwd_loss_dx": "gru16x_lossdx_kernel<DGRU6> (bf16x3 matrix pipe; frozen: loss + dL/du)",
                                                 "dpd_bwd": "gru16_bwd_kernel<DGRU6>", "reduce_clip_optimiser": "reduce_partials_kernel + clip_adamw_kernel"})}
        del casc, optn
        # BASELINE configs[2]: TRes-DeltaGRU H15 (thx .01, thh .05) DPD in front of a frozen DGRU H23 PA, same batch
        torch.manual_seed(2)
        casc = CascadedModel(dpd_model=CoreModel(2, 15, 1, "deltagru_tcnskip", thx=0.01, thh=0.05), pa_model=CoreModel(2, 23, 1, "dgru"))
        casc.freeze_pa_model()
        casc = casc.to(dev)
        opt4 = FusedAdamW(casc, lr=5e-4)
        el4, _, loss4 = min((run_steps(opt4, xc, tc, n3, 2, world * B * T * 2, dist) for _ in range(2)), key=lambda r: r[0])
        dpd["config3"] = {"workload": "train_dpd: TRes-DeltaGRU H15 (thx 0.01, thh 0.05) DPD -> frozen DGRU H23 PA, target = x",
                          "value": B * T * n3 / el4, "unit": "IQ samples/s", "ms_per_step": 1e3 * el4 / n3, "loss": loss4,
                          "roofline": priced(FLOPS_TRAIN_TRES15 + flops_frozen_dgru(23), el4, n3, cascade_spans(opt4, xc, tc, world * B * T * 2),
                                             {"dpd_fwd": "delta16_fwd_kernel<TRES>", "pa_fwd_loss_dx": "gru16x_lossdx_kernel<DGRU6> (bf16x3 matrix pipe; frozen: loss + dL/du)",
                                              "dpd_bwd": "delta16_bwd_kernel<TRES>", "reduce_clip_optimiser": "reduce_partials_kernel + clip_adamw_kernel"})}
        del casc, opt4
        # BASELINE configs[4]: quantisation-aware QGRU H10 (W8A8) DPD in front of the frozen DGRU H23 PA (integer-grid cell, csrc/qat_s16.hip)
        from types import SimpleNamespace
        from opendpd_amd.quant import get_quant_model
        torch.manual_seed(3)
        qdpd = get_quant_model(SimpleNamespace(quant=True, n_bits_w=8, n_bits_a=8, pretrained_model=""), CoreModel(2, 10, 1, "qgru"))
        casc = CascadedModel(dpd_model=qdpd, pa_model=CoreModel(2, 23, 1, "dgru"))
        casc.freeze_pa_model()
        casc = casc.to(dev)
        casc.train()
        opt5 = FusedAdamW(casc, lr=5e-4)
        el5, _, loss5 = min((run_steps(opt5, xc, tc, n3, 2, world * B * T * 2, dist) for _ in range(2)), key=lambda r: r[0])
        dpd["config5"] = {"workload": "train_dpd: quantisation-aware QGRU H10 (W8A8, 515 params) DPD -> frozen DGRU H23 PA, target = x",
                          "value": B * T * n3 / el5, "unit": "IQ samples/s", "ms_per_step": 1e3 * el5 / n3, "loss": loss5,
                          "roofline": priced(FLOPS_TRAIN_QGRU10 + flops_frozen_dgru(23), el5, n3, cascade_spans(opt5, xc, tc, world * B * T * 2),
                                             {"dpd_fwd": "qat16u_fwd_kernel<Q4, LUT, 3 unit slots per lane>", "pa_fwd_loss_dx": "gru16x_lossdx_kernel<DGRU6> (bf16x3 matrix pipe; frozen: loss + dL/du)",
                                              "dpd_bwd": "qat16u_bwd_kernel<Q4, LUT, 3 unit slots per lane>", "reduce_clip_optimiser": "reduce_partials_kernel + clip_adamw_kernel"})}
        del xc, tc, casc, opt5
        # the same step at the reference's own batch size (latency regime): GRU-family pairs run the one-launch cascade step
        # (csrc/gru_cascade.hip: DPD wave + frozen-PA wave per frame), the others the chained one-sequence-per-wave launches
        if args.ref_batch and args.ref_batch != B:
            rb = args.ref_batch
            xr_ = xs_.unfold(0, T, 1)[:rb].permute(0, 2, 1).contiguous()
            tr_ = xr_.clone()
            small = {}
            for name_, dkw, pkw in (("GRU15 -> frozen GRU23 (the registry's default sizes)", dict(hidden_size=15, backbone_type="gru"), dict(hidden_size=23, backbone_type="gru")),
                                    (f"DGRU{H} -> frozen DGRU{H}", dict(hidden_size=H, backbone_type="dgru"), dict(hidden_size=H, backbone_type="dgru")),
                                    ("config3: TRes-DeltaGRU15 -> frozen DGRU23", dict(hidden_size=15, backbone_type="deltagru_tcnskip", thx=0.01, thh=0.05),
                                     dict(hidden_size=23, backbone_type="dgru")),
                                    ("config5: quantisation-aware QGRU10 W8A8 -> frozen DGRU23", dict(hidden_size=10, backbone_type="qgru", bits=8),
                                     dict(hidden_size=23, backbone_type="dgru")),
                                    ("OpenDPDv2 QAT stage: quantisation-aware TRes-DeltaGRU15 W16A16 -> frozen DGRU23",
                                     dict(hidden_size=15, backbone_type="deltagru_tcnskip", thx=0.01, thh=0.05, bits=16), dict(hidden_size=23, backbone_type="dgru"))):
                torch.manual_seed(4)
                dm = CoreModel(2, num_layers=1, **{k_: v_ for k_, v_ in dkw.items() if k_ != "bits"})
                if "bits" in dkw:      # quantisation-aware DPD: the reference's surgery on the float model (quant/__init__.py:20-37)
                    dm = get_quant_model(SimpleNamespace(quant=True, n_bits_w=dkw["bits"], n_bits_a=dkw["bits"], pretrained_model=""), dm)
                casc = CascadedModel(dpd_model=dm, pa_model=CoreModel(2, num_layers=1, **pkw))
                casc.freeze_pa_model()
                casc = casc.to(dev)
                casc.train()
                o_ = FusedAdamW(casc, lr=5e-4)
                el_ = min(run_steps(o_, xr_, tr_, 50, 3, rb * T * 2, None)[0] for _ in range(3))
                small[name_] = {"ms_per_step": 1e3 * el_ / 50, "value": rb * T * 50 / el_,
                                "launches": "one (DPD wave + PA wave per frame)" if o_.cascade_one_launch(rb, T, dev) is not None else "chained"}
                del casc, o_
            dpd["reference_batch"] = {"batch_per_gpu": rb, "frame_length": T, "unit": "IQ samples/s", "cascades": small}
            del xr_, tr_

    # vector-issue speed of this box (ns per wave instruction per SIMD of a pure v_fmac loop: 1.74 on the r06 boxes = four cycles at 2.3 GHz): the issue-bound
    # kernels' times scale with it, so a slower line from another box can be told from a slower build (`config.issue_probe_ns`)
    issue_probe_ns = None
    if rank == 0:
        import ctypes as _C
        from opendpd_amd import _lib as _pl
        _ns = _C.c_double(0.0)
        if _pl.load().odpd_probe_issue_ns(_pl.stream_ptr(), 20000, _C.byref(_ns)) == 0:
            issue_probe_ns = round(_ns.value, 4)

    # RCCL sees all N ranks in every N > 1 run, whichever transport carries the gradient: one sum of ones over the process group
    # ("nccl" = RCCL on ROCm) on the GPU; the count comes back in the line (`config.rccl_ranks_seen`)
    rccl_ranks_seen = None
    if dist is not None:
        ones = torch.ones(1, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(ones)
        rccl_ranks_seen = int(ones.item()) if dist.get_backend() == "nccl" else None
    # which collective carried the gradient (identical on every rank: the communicator is built collectively)
    nc = opt.native_comm()
    from opendpd_amd import dist as odist_
    collective = {"kind": nc.kind if nc is not None else ("torch" if world > 1 else "none"),
                  "description": nc.describe() if nc is not None else ("torch.distributed all_reduce of P+4 floats per step" if world > 1 else "none (one GPU)"),
                  "process_group": dist.get_backend() if dist is not None else None, "message_floats": net.backbone.n_flat + 4,
                  "timeouts": nc.errors() if nc is not None else 0,
                  # every communicator the run tried, in order, with the verdict all ranks agreed on and the stage that failed
                  "candidates": list(odist_.candidate_log)}
    alt = None
    if world > 1 and nc is not None and nc.kind in ("xchg", "rccl") and not os.environ.get("ODPD_BENCH_NO_COMM_AB"):
        other = "rccl" if nc.kind == "xchg" else "xchg"
        alt = odist_.NativeComm(dev, other)
        collective["candidates"] = list(odist_.candidate_log)
        # the bare collective: microseconds per sum of P + 4 floats, 1 000 back to back, on each transport that passed its self-test
        bare = {nc.kind: bare_collective_us(nc, net.backbone.n_flat + 4, dev)}
        bare[other] = bare_collective_us(alt, net.backbone.n_flat + 4, dev) if alt.ok else None
        collective["bare_us_per_allreduce"] = bare
    # STRONG scaling at the reference's own global batch sizes (arguments.py:32 default 256; the scripts' 64): the global batch is
    # fixed and sharded over the N ranks (256 / N frames per GPU), whole epochs of steps issued by the native loop (odpd_train_epoch /
    # odpd_train_epoch_dp: no Python between steps) — the regime in which the reference trains and in which the ~4 KB collective is a
    # visible share of the step.  `value` = global IQ samples/s.
    strong = None
    if not args.no_strong:
        strong = {}
        for gb in (256, 64):
            strong[f"global_batch_{gb}"] = strong_scaling_epoch(H, T, gb, dev, dist, world)
        # N > 1: the same epochs over the OTHER library-owned collective (one-shot exchange vs RCCL), so that one run of the driver's
        # command prices both at the batch size where the collective is a visible share of the step.  Built collectively like the first.
        if alt is not None:
            from opendpd_amd import dist as odist
            other = alt.kind
            if alt.ok:
                keep, odist._native = odist._native, alt
                try:
                    strong[f"collective_{other}"] = {f"global_batch_{gb}": strong_scaling_epoch(H, T, gb, dev, dist, world) for gb in (256, 64)}
                finally:
                    odist._native = keep
            else:
                strong[f"collective_{other}"] = {"unavailable": alt.why}
            strong["collective_of_the_figures_above"] = nc.kind
    if alt is not None and alt.ok:
        alt.close()

    if rank == 0:
        achieved = ALGO_BYTES_PER_SAMPLE * B * T / (kern_ms * 1e-3) / 1e9
        tflops = FLOP_PER_SAMPLE.get(H, 0) * B * T / (kern_ms * 1e-3) / 1e12
        s16 = opt.train_workspace(B, T, dev) is not None     # which fused kernel served this batch (csrc/gru_family.hip)
        kernel_name = "gru16_train_kernel<DGRU6,true> (16 seq/wave, MFMA)" if s16 else "gru_train_kernel<1,DGRU6,true> (4 seq/wave, DPP)"
        # HBM bytes per launch from the PMC passes of tools/profile_pmc.sh (rocprofv3 cannot run inside this process): valid for the
        # kernel SOURCE it was measured on — the entry carries the sha1 of csrc/gru_s16.hip + odpd_s16.h, a changed kernel reports null
        traffic = measured_traffic(f"dgru_h{H}_b{B}_t{T}" + ("_materialized" if args.materialized else ""))

        def brief(d, key):
            """one BASELINE config as the judge's parsed line keeps it: rate, step time, its roofline against the fp32 MFMA / vector roof"""
            if not d:
                return None
            r = d["roofline"]
            return {"workload": d["workload"], "value": d["value"], "unit": "IQ samples/s", "ms_per_step": d["ms_per_step"], "bound": "mfma",
                    "achieved": r["achieved"], "peak": r["peak"], "unit_roof": "TFLOP/s", "frac": r["frac"],
                    "algorithmic_flops_per_sample": r["algorithmic_flops_per_sample"], "hbm_frac": r["hbm"]["frac"],
                    "traffic": r.get("traffic", measured_traffic(key)), "kernel_ms": r.get("kernel_ms")}
        per_config = {"north_star_train_dpd": brief(dpd["north_star"], f"train_dpd_dgru13_dgru23_b{B}_t{T}") if dpd else None,
                      "config3": brief(dpd["config3"], f"train_dpd_tres15_dgru23_b{B}_t{T}") if dpd else None,
                      "config4": brief(cfg4, "") if cfg4 else None,
                      "train_pa_h23": brief(h23, "") if h23 else None,
                      "config5": brief(dpd["config5"], f"train_dpd_qgru10_dgru23_b{B}_t{T}") if dpd else None}
        out = {
            "metric": "iq_samples_per_sec_train", "value": value, "unit": "IQ samples/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * el / args.steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"train_pa DGRU H{H} ({net.backbone.n_flat} params) on APA_200MHz-shaped frames, "
                                   f"T={T}, fused fwd+MSE+BPTT+clip200+AdamW step",
                       "inputs": "(B,T,2) frame tensors" if args.materialized else "stride-1 frames addressed in place in the resident I/Q stream",
                       "batch_per_gpu": B, "global_batch": world * B, "frame_length": T,
                       "parallelism": f"dp{world}", "loss": float(loss),
                       # the train_dpd step of north_star's target sentence, same batch (details under "train_dpd")
                       "train_dpd_workload": dpd["north_star"]["workload"] if dpd else None,
                       "train_dpd_value": dpd["north_star"]["value"] if dpd else None,
                       "train_dpd_ms_per_step": dpd["north_star"]["ms_per_step"] if dpd else None,
                       "config3_value": dpd["config3"]["value"] if dpd else None, "config4_value": cfg4["value"] if cfg4 else None,
                       "config5_value": dpd["config5"]["value"] if dpd else None,
                       "train_pa_h23_value": h23["value"] if h23 else None,
                       "train_pa_h23_value_exact_fp32_kernel": (world * h23["batch_per_gpu"] * T / (h23["exact_fp32_kernel"]["ms_per_step"] * 1e-3)) if h23 else None,
                       # scalars the driver's parsed line keeps (the nested forms stay below and under "collective")
                       "collective_kind": collective.get("kind"), "collective_timeouts": collective.get("timeouts"),
                       "collective_bare_us_xchg": (collective.get("bare_us_per_allreduce") or {}).get("xchg"),
                       "collective_bare_us_rccl": (collective.get("bare_us_per_allreduce") or {}).get("rccl"),
                       "collective_candidates": "; ".join(f"{c.get('kind')}: {'ok' if c.get('ok') else 'failed (' + str(c.get('why'))[:100] + ')'}"
                                                          for c in collective.get("candidates") or [] if isinstance(c, dict)) or None,
                       "rccl_ranks_seen": rccl_ranks_seen, "process_group": collective.get("process_group"),
                       "hsa_enable_ipc_mode_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), "issue_probe_ns": issue_probe_ns,
                       "collective": {k: collective.get(k) for k in ("kind", "candidates", "bare_us_per_allreduce", "timeouts")}},
            "roofline": {"bound": "mfma", "achieved": tflops, "peak": VALU_FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": tflops / VALU_FP32_PEAK_TFLOPS, "traffic": traffic,
                         "kernel": kernel_name, "kernel_ms": kern_ms,
                         "algorithmic_flops_per_launch": FLOP_PER_SAMPLE.get(H, 0) * B * T,
                         "algorithmic_flops_per_sample": FLOP_PER_SAMPLE.get(H, 0),
                         "kernel_source_sha1": kernel_source_sha1(),
                         "train_dpd_frac": dpd["north_star"]["roofline"]["frac"] if dpd else None,
                         "train_dpd_hbm_frac": dpd["north_star"]["roofline"]["hbm"]["frac"] if dpd else None,
                         # per-config scalars (the driver's parsed line keeps scalars only; the nested forms are under "configs")
                         **{f"{k}_{f}": (per_config[c] or {}).get(f) for k, c in (("train_dpd", "north_star_train_dpd"), ("config3", "config3"),
                                                                                   ("config4", "config4"), ("config5", "config5"), ("train_pa_h23", "train_pa_h23"))
                            for f in ("frac", "traffic", "ms_per_step") if not (k == "train_dpd" and f == "frac")},
                         # arithmetic of each priced step: dtype "f32" rests on these statements
                         "arithmetic": "fp32 (exact-f32 MFMA, fp32 VALU, v_exp_f32 / v_rcp_f32 activations)",
                         "train_dpd_arithmetic": "DPD kernels fp32; frozen DGRU H23 PA on v_mfma_f32_16x16x32_bf16 with three-way bf16 operand splits "
                                                 "(six term products >= 2^-16, fp32 accumulation: fp32-equivalent, not bit-fp32; asserted <= 1.5e-6 of the fp64 "
                                                 "oracle and <= 3 x the exact-fp32 kernel's own error in tests/test_gru_s16x_gpu.py)",
                         "configs": per_config,
                         "hbm": {"achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                                 "algorithmic_bytes_per_launch": ALGO_BYTES_PER_SAMPLE * B * T}},
            "sustained": sustained,
            "bf16_frame_storage": bf16_frames,
            "reference_batch": ref,
            "config4": cfg4,
            "train_pa_h23": h23,
            "reference_shapes": ref_shapes,
            "train_dpd": dpd,
            "collective": collective,
            "strong_scaling": strong,
        }
        if world == 1 and not args.no_cpu_baseline:
            cb = cpu_baseline(H, T)
            # GPU / CPU at MATCHED batch (the headline's 65 536-frame batch is a different regime from a 256-frame CPU step)
            gpu_at = {"256": ref["value"] if ref is not None and args.ref_batch == 256 else None, "8192": matched_8192}
            cb["gpu_over_cpu_at_matched_batch"] = {k: (gpu_at.get(k) / v["value"] if gpu_at.get(k) else None) for k, v in cb["by_batch"].items()}
            cb["gpu_value_at_matched_batch"] = gpu_at
            cb["host"] = host_cpu_info()
            q = cb["host"].get("cgroup_cpu_quota_cores")
            cb["why_the_sweep_peaks_where_it_does"] = (
                f"the process may use {q:.0f} CPUs' worth of time per period (cgroup cpu.max) while {cb['host']['nproc']} logical CPUs are visible: "
                "OpenMP teams beyond the quota are throttled and time-sliced, so the rate peaks near the quota and collapses above it"
                if q and q < (cb["host"].get("affinity") or cb["host"]["nproc"]) else
                "no cgroup CPU quota below the visible core count: the sweep is limited by the oracle's per-sequence OpenMP loop "
                "(256 sequences per batch: more threads than ~16 leave each with too few sequences per step; the 8 192-frame batch scales further)")
            out["cpu_baseline"] = cb
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
