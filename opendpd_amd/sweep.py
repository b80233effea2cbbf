"""Lockstep sweeps: K independent `train_pa` runs — the seeds x hidden-size loops of the reference's bash_scripts/train_all_pa.sh:26-57, which
start one process per run — trained TOGETHER on one GPU.  At the reference's batch sizes one run occupies 256 (batch 64: 64) of the chip's
>= 8 192 wave slots and its step is a chain of three launches of ~0.1 ms; here every step of the epoch is ONE fused train launch that carries
all K runs of a model shape (run k owns workgroups [k G, (k + 1) G) and sees exactly the launch it would have had alone), one row reduction
and one clip + AdamW launch (csrc: odpd_train_epoch_sweep), and the evaluation passes of the K models are one launch per batch of segments
(odpd_backbone_fwd_sweep).  Each run is BIT-IDENTICAL to its solo run — same seeded initialisation, same epoch orders (each run keeps its
own copy of the global RNG state, swapped in around everything that draws from it), same kernels, same reduction order — and writes the same
`save/` and `log/` files (tests/test_sweep_gpu.py compares them with solo runs).  Runs whose shape the sweep kernels do not serve (other
families, batches beyond the one-sequence-per-wave regime) advance through the ordinary per-run epoch, in the same lockstep loop.

`train_dpd_sweep` does the same for `train_dpd` (bash_scripts/train_all_dpd.sh: seeds x DPD backbones, each DPD in front of the frozen PA of
its own seed).  Its step is the one-launch cascade step, which gives every frame a workgroup with a CU's LDS to itself: at batch 64 a solo
run occupies 64 CUs, and the launch that carries K runs (csrc: odpd_train_epoch_cascade_sweep) fills the rest of the chip while every run
stays its solo run bit for bit — for train_dpd the chip-filling mode and the exact mode are the same mode.  The delta thresholds of a
deltagru / deltagru_tcnskip DPD are one more axis of such a sweep (`thresholds=`: the THX / THH knobs of bash_scripts/OpenDPDv2.sh): runs that
differ in their pair share the launch too, each workgroup reading its run's pair from a device table (csrc: odpd_train_epoch_cascade_sweep_th)."""
import ctypes as C
import random
import time

import numpy as np
import torch

from . import _lib
from .models import CascadedModel, CoreModel
from .project import Project, count_net_params
from .train_funcs import FusedAdamW, _epoch_shape, _loss_kind, _sample_format, cascade_rows, rows_buffer


def _call_desc(bb):
    """the descriptor of a call on this backbone, asked for where it is used (NativeBackbone.call_desc: the module's mode as it stands
    then); None for a backbone that runs through ATen"""
    return bb.call_desc() if getattr(bb, "native", False) else None


class _Rng:
    """one run's private copy of the process-global RNG states (torch CPU, numpy, random): `with run.rng:` swaps it in and back out"""

    def __init__(self):
        self.state = None
        self._outer = None

    @staticmethod
    def _get():
        return torch.get_rng_state(), np.random.get_state(), random.getstate()

    @staticmethod
    def _set(st):
        torch.set_rng_state(st[0]); np.random.set_state(st[1]); random.setstate(st[2])

    def __enter__(self):
        self._outer = self._get()
        if self.state is not None:
            self._set(self.state)
        return self

    def __exit__(self, *exc):
        self.state = self._get()
        self._set(self._outer)
        return False


class _Run:
    def __init__(self, proj):
        self.proj, self.rng = proj, _Rng()
        self.net = self.opt = self.sched = self.loaders = self.criterion = None
        self.partials = self.losses = self.order = self.workspace = None


def _setup(run):
    """steps/train_pa.py:10-59 up to the training loop (project.run_train_pa), under the run's own RNG"""
    p = run.proj
    p.set_device()
    run.loaders, input_size = p.build_dataloaders()
    run.net = CoreModel(input_size, p.PA_hidden_size, p.PA_num_layers, p.PA_backbone, window_size=p.window_size,
                        num_dvr_units=p.num_dvr_units).to(p.device)
    p.build_logger(p.gen_pa_model_id(count_net_params(run.net)))
    run.opt, run.sched = p.build_optimizer(run.net)
    run.criterion = p.build_criterion()


def _group_key(run):
    p = run.proj
    return (p.PA_backbone, p.PA_hidden_size, p.PA_num_layers, p.batch_size, p.frame_length, p.frame_stride, p.loss_type, p.opt_type,
            p.dataset_label, p.frame_storage, p.grad_clip_val)


def _epoch_tables(runs, n, T, n_steps, dev, workspace):
    """What both lockstep epoch entry points take for the runs of a group: the odpd_sweep_run_t table — every run's epoch order (its own
    shuffle, drawn from its own RNG stream), fresh per-step losses and `workspace(run)` (a tensor or None) in the `workspace` slot — the
    odpd_frames_t over the shared train streams (the orders are per run) and the tail of AdamW arguments: first step, betas, eps, weight
    decay of run 0 (the group key makes them the group's), clip norm."""
    table = (_lib.SweepRun * len(runs))()
    for k, r in enumerate(runs):
        r.net.train()
        with r.rng:
            r.order = r.loaders[0].epoch_order()
        r.losses = torch.empty(n_steps, dtype=torch.float32, device=dev)
        ws = workspace(r)
        table[k] = _lib.SweepRun(r.opt.backbone.flat_params(full_check=True).data_ptr(), r.opt.grad.data_ptr(), r.opt.exp_avg.data_ptr(),
                                 r.opt.exp_avg_sq.data_ptr(), r.partials.data_ptr(), r.losses.data_ptr(), None,
                                 ws.data_ptr() if ws is not None else None, r.order.data_ptr(), float(r.opt.param_groups[0]["lr"]))
    opt0, train0 = runs[0].opt, runs[0].loaders[0]
    assert all(r.opt.step_count == opt0.step_count for r in runs)
    fr = _lib.Frames(train0.x.data_ptr(), train0.y.data_ptr(), None, n, T, train0.stride, _sample_format(train0.x, train0.y), 0)
    g0 = opt0.param_groups[0]
    return table, fr, (opt0.step_count + 1, float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]), float(g0["weight_decay"]),
                       float(runs[0].proj.grad_clip_val or 0.0))


def _epoch_done(runs, n_steps):
    """after a lockstep epoch was issued: the K epoch means — each the reduction its solo run makes (train_funcs.net_train), queued back to
    back and read with ONE synchronisation — into the runs' logs, and the optimisers' bookkeeping of train_funcs' own epoch loops"""
    means = torch.stack([r.losses.double().mean() for r in runs]).cpu() if n_steps else None
    for k, r in enumerate(runs):
        r.opt.step_count += n_steps
        r.opt.last_epoch_losses = r.losses
        r.opt._keepalive = r.order     # the launches read `order` asynchronously
        r.proj.log_train["loss"] = float(means[k].item()) if means is not None else float("nan")


class _Group:
    """runs of one model shape on one dataset: what one sweep launch can carry"""

    def __init__(self, runs, exact=True):
        self.runs, self.exact = runs, exact
        r0 = runs[0]
        lib = _lib.load()
        train = r0.loaders[0]
        self.T, self.n = train.frame_length, train.n
        self.B, self.n_steps, self.last = _epoch_shape(train)
        fused = all(isinstance(r.opt, FusedAdamW) and r.opt.kind == "adamw" and r.opt.pa is None and r.opt.world_size() == 1
                    and getattr(r.net.backbone, "frozen_mask", None) is None for r in runs)
        kind = _loss_kind(r0.criterion)
        self.kind = kind
        ok = bool(fused and kind is not None and self.desc is not None and len(runs) > 1 and train.x.is_cuda)
        # throughput mode: the 16-sequences-per-wave kernel for every run (K x B / 16 waves fill the chip); exact mode: the kernel a solo run
        # takes at this batch size (its frame state fills a CU's LDS: no more than one run's worth of frames is ever resident)
        self.flags = _lib.SWEEP_S16 if (ok and not exact and train.x.dtype == torch.float32 and lib.odpd_sweep_s16_supported(C.byref(self.desc))) else 0
        self.train_sweep = bool(ok and (self.flags or (lib.odpd_sweep_train_supported(C.byref(self.desc), self.B, self.T)
                                                       and lib.odpd_sweep_train_supported(C.byref(self.desc), self.last, self.T))))
        self.dev = train.x.device if hasattr(train, "x") else None
        self.scratch = None
        self._tuning_gen = None
        self._size_buffers()

    @property
    def desc(self):
        """run 0's descriptor (the group key makes it the group's), asked for at each use"""
        return _call_desc(self.runs[0].net.backbone)

    def _size_buffers(self):
        """partial rows / workspace / scratch of every run, sized for the CURRENT kernel-selection knobs (odpd_set_tuning: gp_max_batch,
        s16_occupancy, s16_min_batch .. change the grids the kernels write); re-done by train_epoch when odpd_tuning_generation has moved
        (a stale buffer under a larger grid would be a device out-of-bounds write)"""
        lib = _lib.load()
        runs, bb = self.runs, self.runs[0].net.backbone
        self._tuning_gen = int(lib.odpd_tuning_generation())
        if self.train_sweep:
            rows = max(int(lib.odpd_sweep_partial_rows(C.byref(self.desc), b, self.T, self.flags)) for b in {self.B, self.last})
            ws = max(int(lib.odpd_sweep_workspace_floats(C.byref(self.desc), b, self.T, self.flags)) for b in {self.B, self.last})
            P = bb.n_flat
            for r in runs:
                r.opt._ensure(self.dev)
                r.partials = rows_buffer(rows, P, self.dev)
                r.workspace = torch.empty(ws, dtype=torch.float32, device=self.dev) if ws > 0 else None
            self.scratch = torch.empty(int(lib.odpd_sweep_scratch_bytes(len(runs), self.n_steps)), dtype=torch.uint8, device=self.dev)

    # ---- one training epoch of every run of the group ----
    def train_epoch(self):
        from .train_funcs import _check_exchange_health, net_train
        if not self.train_sweep:
            for r in self.runs:
                with r.rng:
                    r.net = net_train(r.proj.log_train, r.net, r.loaders[0], r.opt, r.criterion, r.proj.grad_clip_val, r.proj.device)
            return
        lib = _lib.load()
        if int(lib.odpd_tuning_generation()) != self._tuning_gen:
            self._size_buffers()
        table, fr, adamw = _epoch_tables(self.runs, self.n, self.T, self.n_steps, self.dev, lambda r: r.workspace)
        rc = lib.odpd_train_epoch_sweep(_lib.stream_ptr(), C.byref(self.desc), len(self.runs), table, _lib.LOSS_IDS[self.kind], C.byref(fr), self.B,
                                        *adamw, self.flags, C.c_void_p(self.scratch.data_ptr()))
        _lib.check(rc, "odpd_train_epoch_sweep")
        _epoch_done(self.runs, self.n_steps)

    # ---- validation + test of every run of the group (train_funcs.net_eval_pair, the K forwards as one launch per batch pair) ----
    def eval_epoch(self):
        from .metrics import calculate_metrics
        from .train_funcs import net_eval, net_eval_pair
        lib = _lib.load()
        p0 = self.runs[0].proj
        batches, lists = None, None
        if p0.eval_val and p0.eval_test and self.desc is not None and len(self.runs) > 1:
            lists = _loader_passes(self.runs)
            ba, bb_ = lists[0]
            if _pairable(ba, bb_):
                xs = [torch.cat((fa, fb), dim=0).to(self.dev).float().contiguous() for (fa, _), (fb, _) in zip(ba, bb_)]
                if all(lib.odpd_sweep_fwd_supported(C.byref(self.desc), x.shape[0], x.shape[1]) for x in xs):
                    batches = (ba, bb_, xs)
        if batches is None:
            if lists is not None:      # the passes over the loaders were made above
                _eval_pairs_per_run(self.runs, lists)
                return
            for r in self.runs:
                with r.rng:
                    self._eval_solo(r, calculate_metrics, net_eval, net_eval_pair)
            return
        ba, bb_, xs = batches
        self._eval_sweep(ba, bb_, xs, calculate_metrics)

    @staticmethod
    def _eval_solo(r, calculate_metrics, net_eval, net_eval_pair):
                p = r.proj
                if p.eval_val and p.eval_test:
                    _, (pv, tv), (pt, tt) = net_eval_pair(p.log_val, p.log_test, r.net, r.loaders[1], r.loaders[2], r.criterion, p.device)
                    p.log_val = calculate_metrics(p.args, p.log_val, pv, tv)
                    p.log_test = calculate_metrics(p.args, p.log_test, pt, tt)
                elif p.eval_val:
                    _, pred, truth = net_eval(p.log_val, r.net, r.loaders[1], r.criterion, p.device)
                    p.log_val = calculate_metrics(p.args, p.log_val, pred, truth)
                elif p.eval_test:
                    _, pred, truth = net_eval(p.log_test, r.net, r.loaders[2], r.criterion, p.device)
                    p.log_test = calculate_metrics(p.args, p.log_test, pred, truth)

    def _eval_sweep(self, ba, bb_, xs, calculate_metrics):
        lib = _lib.load()
        K = len(self.runs)
        scratch = torch.empty(int(lib.odpd_sweep_scratch_bytes(K, 0)), dtype=torch.uint8, device=self.dev)
        outs = [([], [], []) for _ in range(K)], [([], [], []) for _ in range(K)]
        with torch.no_grad():
            for (fa, ta), (fb, tb), x in zip(ba, bb_, xs):
                ta, tb = ta.to(self.dev), tb.to(self.dev)
                ys = [torch.empty(x.shape[0], x.shape[1], 2, dtype=torch.float32, device=self.dev) for _ in range(K)]
                table = (_lib.SweepRun * K)()
                for k, r in enumerate(self.runs):
                    r.net.eval()
                    table[k] = _lib.SweepRun(r.net.backbone.flat_params().data_ptr(), None, None, None, None, None, ys[k].data_ptr(), None, None, 0.0)
                _lib.check(lib.odpd_backbone_fwd_sweep(_lib.stream_ptr(), C.byref(self.desc), K, table, x.shape[0], x.shape[1], _lib.ptr(x),
                                                       C.c_void_p(scratch.data_ptr())), "odpd_backbone_fwd_sweep")
                for k, r in enumerate(self.runs):
                    for (losses, pred, truth), o, t in ((outs[0][k], ys[k][:fa.shape[0]], ta), (outs[1][k], ys[k][fa.shape[0]:], tb)):
                        losses.append(r.criterion(o, t)); pred.append(o); truth.append(t)
        _metrics_many(self.runs, outs)


def _metrics_many(runs, outs):
    """host side of the K x 2 evaluations at sweep level: one device-to-host copy per split for all runs' predictions, one for every loss,
    the split's ground truth once (the runs of a group share their dataset), metrics over the (K, segments, nperseg) stack with one
    FFT / Welch call per split (metrics.calculate_metrics_many: each run's numbers are those of its own calculate_metrics call).
    outs[split][k] = (losses, predictions, ground truth) of run k, one entry per batch"""
    from .metrics import calculate_metrics_many
    K = len(runs)
    for split, name in ((0, "log_val"), (1, "log_test")):
        per_run = outs[split]
        if not per_run[0][0]:
            for r in runs:
                getattr(r.proj, name)["loss"] = float("nan")
            continue
        loss_m = torch.stack([torch.stack([l.float() for l in per_run[k][0]]) for k in range(K)]).cpu().numpy()      # (K, batches)
        preds = torch.stack([torch.cat(per_run[k][1], dim=0) for k in range(K)]).cpu().numpy()                       # (K, segments, nperseg, 2)
        truth = torch.cat(per_run[0][2], dim=0).cpu().numpy()
        stats = []
        for k, r in enumerate(runs):
            getattr(r.proj, name)["loss"] = float(np.mean(loss_m[k]))
            stats.append(getattr(r.proj, name))
        done = calculate_metrics_many(runs[0].proj.args, stats, [preds[k] for k in range(K)], [truth] * K)
        for r, st in zip(runs, done):
            setattr(r.proj, name, st)


def _flush_loggers(runs, failed):
    """the deferred checkpoints of every run, at the end of the sweep loop.  `failed`: the exception that ended the loop (None: it finished) —
    a flush that fails then must not mask it and is reported as a warning; after a finished loop a failing flush is the sweep's error (every
    other run is still flushed first)"""
    import warnings
    first = None
    for r in runs:
        try:
            r.proj.logger.flush()
        except Exception as e:
            if failed is not None:
                warnings.warn(f"checkpoint of {r.proj.path_save_file_best} not written ({type(e).__name__}: {e}) while the sweep ended with "
                              f"{type(failed).__name__}", RuntimeWarning, stacklevel=2)
            elif first is None:
                first = e
    if first is not None:
        raise first


def _loader_passes(runs):
    """[(validation batches, test batches)] per run.  One pass over a torch DataLoader draws its base seed from the global RNG even without
    shuffling: every run makes the two passes its solo epoch makes, under its own RNG copy — the NEXT epoch's shuffle depends on it"""
    lists = []
    for r in runs:
        with r.rng:
            lists.append((list(r.loaders[1]), list(r.loaders[2])))
    return lists


def _pairable(ba, bb_):
    return len(ba) == len(bb_) and all(fa.shape[1:] == fb.shape[1:] for (fa, _), (fb, _) in zip(ba, bb_))


def _eval_pairs_per_run(runs, lists):
    """train_funcs.net_eval_pair per run on batches already drawn (their RNG draws were made with the passes)"""
    from .metrics import calculate_metrics
    from .train_funcs import net_eval_pair
    for r, pre in zip(runs, lists):
        p = r.proj
        _, (pv, tv), (pt, tt) = net_eval_pair(p.log_val, p.log_test, r.net, pre[0], pre[1], r.criterion, p.device)
        p.log_val = calculate_metrics(p.args, p.log_val, pv, tv)
        p.log_test = calculate_metrics(p.args, p.log_test, pt, tt)


def _sweep_loop(runs, groups, n_epochs, metric):
    """the lockstep loop of both sweeps; sweep-level bookkeeping: history rows are appended (project.CsvLogger), an
    improved model is remembered on the device and its checkpoint written once, when the sweep ends or is interrupted (`flush`), instead of
    one torch.save per run and improving epoch"""
    for r in runs:
        r.proj.logger.defer_checkpoints = True
    start = time.time()
    failed = None
    try:
        for epoch in range(n_epochs):
            for g in groups:
                g.train_epoch()
            for g in groups:
                g.eval_epoch()
            for r in runs:      # (log row, best-model bookkeeping, plateau scheduler: nothing here draws from an RNG — no state swap)
                r.proj.finish_epoch(r.net, r.opt, r.sched, epoch, start, metric)
    except BaseException as e:
        failed = e
        raise
    finally:
        _flush_loggers(runs, failed)


def train_pa_sweep(dataset_name=None, seeds=(0,), hidden_sizes=None, PA_backbone="gru", PA_hidden_size=23, n_epochs=100, batch_size=256,
                   lr=5e-4, accelerator="cuda", frame_length=200, exact=True, **kwargs):
    """`opendpd.api.train_pa` (opendpd/api.py:27-104) for every (hidden size, seed) pair, the runs of one model shape advancing in lockstep
    on one GPU.  Returns one result dictionary per run ({'status', 'model_path', 'log_path', 'seed', 'PA_hidden_size', 'lockstep',
    'mode'}), in hidden-size-major order.
    exact=True: every run on the kernels its solo `train_pa` takes — the files are those the solo calls would have written, bit for bit;
    at the reference's batch sizes those kernels keep a frame's whole BPTT state in LDS (one frame per CU), so the GPU part of K runs costs K
    solo epochs and the gain is the launch count.  exact=False (throughput mode, GRU family with hidden <= 16): the training steps run on
    the 16-sequences-per-wave MFMA kernel, K x batch / 16 waves at once — each run then equals its solo run with that kernel forced
    (odpd_set_tuning("s16_min_batch", 0)) bit for bit, and the default solo run to float tolerance (a different summation order)."""
    if not dataset_name:
        raise ValueError("train_pa_sweep requires dataset_name. Create a dataset first with create_dataset().")
    from . import data as D
    runs = []
    from . import project as PJ
    D._share = {}      # one parse of the dataset's CSV files for all runs ...
    PJ._stream_share = {}      # ... and one upload of its train streams (read-only on the device)
    try:
        for H in (list(hidden_sizes) if hidden_sizes else [PA_hidden_size]):
            for seed in seeds:
                run = _Run(None)
                with run.rng:      # Project.__init__ seeds the global RNGs (project.py:108-112): from here on this run owns its own copy of them
                    run.proj = Project(step="train_pa", dataset_name=dataset_name, PA_backbone=PA_backbone, PA_hidden_size=int(H), n_epochs=n_epochs,
                                       batch_size=batch_size, lr=lr, accelerator=accelerator, frame_length=frame_length, seed=int(seed), **kwargs)
                    _setup(run)
                runs.append(run)
    finally:
        D._share = None
        PJ._stream_share = None
    groups = {}
    for r in runs:
        groups.setdefault(_group_key(r), []).append(r)
    groups = [_Group(v, exact=exact) for v in groups.values()]
    _sweep_loop(runs, groups, n_epochs, "NMSE")
    return [{"status": "completed", "model_path": r.proj.path_save_file_best, "log_path": r.proj.path_log_file_best, "seed": r.proj.seed,
             "PA_hidden_size": r.proj.PA_hidden_size, "lockstep": bool(g_.train_sweep),
             "mode": ("s16" if g_.flags else "exact") if g_.train_sweep else "per-run"}
            for g_ in groups for r in g_.runs]


# ---------------------------------------------------------------------------------------------------------------------------------------
# train_dpd
# ---------------------------------------------------------------------------------------------------------------------------------------
def _setup_dpd(run):
    """steps/train_dpd.py:14-90 up to the training loop (project.run_train_dpd), under the run's own RNG: the frozen PA is the one `train_pa`
    saved for this run's seed"""
    import os

    from .quant import get_quant_model
    p = run.proj
    p.set_device()
    run.loaders, input_size = p.build_dataloaders()
    pa = CoreModel(input_size, p.PA_hidden_size, p.PA_num_layers, p.PA_backbone, window_size=p.window_size, num_dvr_units=p.num_dvr_units)
    pa_id = p.gen_pa_model_id(count_net_params(pa))
    pa.load_state_dict(torch.load(os.path.join("save", p.dataset_label, "train_pa", pa_id + ".pt"), map_location="cpu"))
    dpd = CoreModel(input_size, p.DPD_hidden_size, p.DPD_num_layers, p.DPD_backbone, window_size=p.window_size, num_dvr_units=p.num_dvr_units,
                    thx=p.thx, thh=p.thh)
    dpd = get_quant_model(p, dpd)
    p.build_logger(p.gen_dpd_model_id(count_net_params(dpd)))
    net = CascadedModel(dpd_model=dpd, pa_model=pa)
    net.freeze_pa_model()
    run.net = net.to(p.device)
    run.opt, run.sched = p.build_optimizer(run.net)
    run.criterion = p.build_criterion()


def _dpd_group_key(run):
    p = run.proj
    # the thresholds of a float deltagru / deltagru_tcnskip DPD are a per-run value of the launch (_DpdGroup._size_buffers), not part of its shape
    th = (None, None) if p.DPD_backbone in ("deltagru", "deltagru_tcnskip") and not p.quant else (p.thx, p.thh)
    return (p.DPD_backbone, p.DPD_hidden_size, p.DPD_num_layers, p.PA_backbone, p.PA_hidden_size, p.PA_num_layers, p.batch_size, p.frame_length,
            p.frame_stride, p.loss_type, p.opt_type, p.dataset_label, p.frame_storage, p.grad_clip_val, *th, p.quant, p.n_bits_w,
            p.n_bits_a, p.pretrained_model, p.quant_dir_label, p.q_pretrain)


class _DpdGroup:
    """train_dpd runs of one (DPD, PA) shape pair on one dataset: what one cascade sweep launch can carry"""

    def __init__(self, runs):
        self.runs = runs
        r0 = runs[0]
        train = r0.loaders[0]
        self.T, self.n = train.frame_length, train.n
        self.B, self.n_steps, self.last = _epoch_shape(train)
        self.dev = train.x.device if hasattr(train, "x") else None
        self.kind = _loss_kind(r0.criterion)
        fused = all(isinstance(r.opt, FusedAdamW) and r.opt.kind == "adamw" and r.opt.pa is not None and r.opt.world_size() == 1
                    and r.opt.native_comm() is None and r.opt.pa.native and r.opt.backbone.native
                    and getattr(r.opt.backbone, "frozen_mask", None) is None for r in runs)
        self.eligible = bool(fused and self.kind is not None and len(runs) > 1 and hasattr(train, "epoch_order") and train.x.is_cuda
                             and train.x.dtype == torch.float32)
        self.train_sweep = False
        self.thresholds = None
        self.scratch = None
        self._tuning_gen = None
        self._size_buffers()

    # run 0's descriptors (the group key makes them the group's — but for the thresholds of a delta DPD, which `thresholds` carries per run where
    # they differ), asked for at each use
    @property
    def dpd_desc(self):
        return _call_desc(getattr(self.runs[0].net.dpd_model, "backbone", None))

    @property
    def pa_desc(self):
        """the frozen PA's, as run 0's optimiser launches with it (asked for in `eligible` groups only: those have a fused optimiser)"""
        return self.runs[0].opt._pa_desc()

    def _size_buffers(self):
        """whether a cascade sweep launch serves the group — runs of one threshold pair: odpd_train_epoch_cascade_sweep with run 0's descriptor;
        of differing pairs: odpd_train_epoch_cascade_sweep_th with the K pairs in `thresholds` — and the partial rows / scratch of every run, under
        the CURRENT kernel-selection knobs (odpd_set_tuning: cascade_one_launch, gp_max_batch ..); re-done by train_epoch when
        odpd_tuning_generation has moved"""
        lib = _lib.load()
        self._tuning_gen = int(lib.odpd_tuning_generation())
        pairs = [(float(r.proj.thx), float(r.proj.thh)) for r in self.runs]
        self.thresholds = None if all(p == pairs[0] for p in pairs) else (C.c_float * (2 * len(pairs)))(*(v for p in pairs for v in p))
        supported = lib.odpd_sweep_cascade_supported if self.thresholds is None else lib.odpd_sweep_cascade_th_supported
        self.train_sweep = bool(self.eligible and all(
            supported(C.byref(self.dpd_desc), C.byref(self.pa_desc), b, self.T) == 1 for b in {self.B, self.last}))
        if self.train_sweep:
            rows = max(cascade_rows(self.dpd_desc, self.pa_desc, b, self.T) for b in {self.B, self.last})
            for r in self.runs:
                r.opt._ensure(self.dev)
                r.partials = rows_buffer(rows, r.opt.backbone.n_flat, self.dev)
            scratch_bytes = lib.odpd_sweep_cascade_scratch_bytes if self.thresholds is None else lib.odpd_sweep_cascade_th_scratch_bytes
            self.scratch = torch.empty(int(scratch_bytes(len(self.runs), self.n_steps)), dtype=torch.uint8, device=self.dev)

    # ---- one training epoch of every run of the group ----
    def train_epoch(self):
        from .train_funcs import net_train
        lib = _lib.load()
        if int(lib.odpd_tuning_generation()) != self._tuning_gen:
            self._size_buffers()
        if not self.train_sweep:
            for r in self.runs:
                with r.rng:
                    r.net = net_train(r.proj.log_train, r.net, r.loaders[0], r.opt, r.criterion, r.proj.grad_clip_val, r.proj.device)
            return
        # workspace slot: a delta DPD's four sparsity counters (None while switched off)
        table, fr, adamw = _epoch_tables(self.runs, self.n, self.T, self.n_steps, self.dev, lambda r: r.opt.backbone._stats_buffer(self.dev))
        pa_flat = [r.opt.pa.flat_params(full_check=True) for r in self.runs]
        pa_tab = (C.c_void_p * len(self.runs))(*(f.data_ptr() for f in pa_flat))
        if self.thresholds is None:
            rc = lib.odpd_train_epoch_cascade_sweep(_lib.stream_ptr(), C.byref(self.dpd_desc), C.byref(self.pa_desc), len(self.runs), table, pa_tab,
                                                    _lib.LOSS_IDS[self.kind], C.byref(fr), self.B, *adamw, C.c_void_p(self.scratch.data_ptr()))
            _lib.check(rc, "odpd_train_epoch_cascade_sweep")
        else:
            rc = lib.odpd_train_epoch_cascade_sweep_th(_lib.stream_ptr(), C.byref(self.dpd_desc), C.byref(self.pa_desc), len(self.runs), table, pa_tab,
                                                       self.thresholds, _lib.LOSS_IDS[self.kind], C.byref(fr), self.B, *adamw,
                                                       C.c_void_p(self.scratch.data_ptr()))
            _lib.check(rc, "odpd_train_epoch_cascade_sweep_th")
        _epoch_done(self.runs, self.n_steps)

    # ---- validation + test of every run of the group: what train_funcs.net_eval_pair computes for each run ----
    def eval_epoch(self):
        from .metrics import calculate_metrics
        from .train_funcs import net_eval, net_eval_pair
        lib = _lib.load()
        p0, K = self.runs[0].proj, len(self.runs)
        if not (p0.eval_val and p0.eval_test) or K == 1:
            for r in self.runs:
                with r.rng:
                    _Group._eval_solo(r, calculate_metrics, net_eval, net_eval_pair)
            return
        lists = _loader_passes(self.runs)
        ba, bb_ = lists[0]
        if not _pairable(ba, bb_):      # the splits do not pair up: net_eval_pair's own fallback, per run
            _eval_pairs_per_run(self.runs, lists)
            return
        dpd_float = self.dpd_desc is not None and int(self.dpd_desc.bits_w) == 0 and all(
            getattr(r.net.dpd_model.backbone, "native", False) for r in self.runs)
        scratch = torch.empty(int(lib.odpd_sweep_scratch_bytes(K, 0)), dtype=torch.uint8, device=self.dev)
        outs = [([], [], []) for _ in range(K)], [([], [], []) for _ in range(K)]
        with torch.no_grad():
            for r in self.runs:
                r.net.eval()
            for (fa, ta), (fb, tb) in zip(ba, bb_):
                fa, ta, fb, tb = fa.to(self.dev), ta.to(self.dev), fb.to(self.dev), tb.to(self.dev)
                x = torch.cat((fa, fb), dim=0)
                # the DPD stage of the K runs: one launch where the evaluation sweep serves the shape (the kernel a solo forward takes) ...
                if (dpd_float and x.dtype == torch.float32
                        and lib.odpd_sweep_fwd_supported(C.byref(self.dpd_desc), x.shape[0], x.shape[1]) == 1):
                    x = x.contiguous()
                    us = [torch.empty(x.shape[0], x.shape[1], 2, dtype=torch.float32, device=self.dev) for _ in range(K)]
                    table = (_lib.SweepRun * K)()
                    for k, r in enumerate(self.runs):
                        table[k] = _lib.SweepRun(r.net.dpd_model.backbone.flat_params().data_ptr(), None, None, None, None, None, us[k].data_ptr(),
                                                 None, None, 0.0)
                    _lib.check(lib.odpd_backbone_fwd_sweep(_lib.stream_ptr(), C.byref(self.dpd_desc), K, table, x.shape[0], x.shape[1], _lib.ptr(x),
                                                           C.c_void_p(scratch.data_ptr())), "odpd_backbone_fwd_sweep")
                else:      # ... else per run (delta DPDs count their sparsity statistics in this forward; quantised DPDs)
                    us = [r.net.dpd_model(x) for r in self.runs]
                # the PA stage per run, with the call the solo run makes: the PAs differ, and stacking would change the batch size (and so the kernel)
                for k, r in enumerate(self.runs):
                    y = r.net.pa_model(us[k])
                    for (losses, pred, truth), o, t in ((outs[0][k], y[:fa.shape[0]], ta), (outs[1][k], y[fa.shape[0]:], tb)):
                        losses.append(r.criterion(o, t)); pred.append(o); truth.append(t)
        _metrics_many(self.runs, outs)


def _threshold_pairs(thresholds, thx, thh, DPD_backbone):
    """the (thx, thh) pairs of train_dpd_sweep(thresholds=...) as floats, or ValueError for what cannot be a sweep: the runs' files are named
    after f"{v:.3f}" of their pair, and only for a delta backbone (project.gen_dpd_model_id)"""
    import math
    if thx or thh:
        raise ValueError("train_dpd_sweep: give either thresholds=[(thx, thh), ..] or thx= / thh=, not both")
    try:
        pairs = [(float(a), float(b)) for a, b in thresholds]
    except (TypeError, ValueError):
        raise ValueError("train_dpd_sweep: thresholds must be a sequence of (thx, thh) pairs") from None
    if not pairs:
        raise ValueError("train_dpd_sweep: thresholds holds no pair")
    for pair in pairs:
        if not all(math.isfinite(v) and v >= 0.0 for v in pair):
            raise ValueError(f"train_dpd_sweep: the thresholds {pair} are not finite numbers >= 0")
    names = [(f"{a:.3f}", f"{b:.3f}") for a, b in pairs]
    if len(set(names)) != len(names):
        raise ValueError(f"train_dpd_sweep: two threshold pairs would write the same files (model IDs carry them as THX_%.3f_THH_%.3f): {names}")
    if len(pairs) > 1 and "delta" not in DPD_backbone:
        raise ValueError(f"train_dpd_sweep: the model ID of a {DPD_backbone!r} DPD holds no thresholds, {len(pairs)} pairs would overwrite each other")
    return pairs


def train_dpd_sweep(dataset_name=None, seeds=(0,), hidden_sizes=None, DPD_backbone="deltagru_tcnskip", DPD_hidden_size=15, PA_backbone="gru",
                    PA_hidden_size=23, n_epochs=100, batch_size=256, lr=5e-4, accelerator="cuda", frame_length=200, thx=0.0, thh=0.0,
                    thresholds=None, **kwargs):
    """`opendpd.api.train_dpd` for every (DPD hidden size, seed) pair, the runs of one (DPD, PA) shape pair advancing in lockstep on one GPU:
    every training step of a group is ONE cascade launch for all its runs (+ one row reduction, one clip + AdamW launch).  Each run trains in
    front of the frozen PA `train_pa` saved for its own seed and is its solo `train_dpd` bit for bit (same files under `save/` and `log/`).
    Returns one result dictionary per run ({'status', 'model_path', 'log_path', 'seed', 'DPD_hidden_size', 'lockstep'}), in
    hidden-size-major order.  Groups the sweep launch does not serve (quantised DPDs, other families or optimisers, a single run) advance
    through the ordinary per-run epoch inside the same loop ('lockstep': False).
    thresholds: a sequence of (thx, thh) pairs instead of the one pair thx= / thh= — the runs are then every (hidden size, pair, seed), in that
    nesting order, and each result also carries 'thx' and 'thh'.  Float deltagru / deltagru_tcnskip runs that differ only in their pair form one
    group and share its launches, each at its own thresholds (evaluation stays per run: every module counts its own sparsity); for any other
    DPD each pair is a group of its own.  ValueError: thresholds together with a non-zero thx / thh, a negative or non-finite value, two pairs
    that print alike at three decimals (they would write the same files), several pairs for a backbone that is not a delta one."""
    if not dataset_name:
        raise ValueError("train_dpd_sweep requires dataset_name. Create a dataset first with create_dataset().")
    pairs = [(thx, thh)] if thresholds is None else _threshold_pairs(thresholds, thx, thh, DPD_backbone)
    from . import data as D
    from . import project as PJ
    runs = []
    D._share = {}      # one parse of the dataset's CSV files for all runs ...
    PJ._stream_share = {}      # ... and one upload of its train streams (read-only on the device)
    try:
        for H in (list(hidden_sizes) if hidden_sizes else [DPD_hidden_size]):
            for pair in pairs:
                for seed in seeds:
                    run = _Run(None)
                    with run.rng:      # Project.__init__ seeds the global RNGs (project.py:108-112): from here on this run owns its own copy of them
                        run.proj = Project(step="train_dpd", dataset_name=dataset_name, DPD_backbone=DPD_backbone, DPD_hidden_size=int(H),
                                           PA_backbone=PA_backbone, PA_hidden_size=PA_hidden_size, n_epochs=n_epochs, batch_size=batch_size, lr=lr,
                                           accelerator=accelerator, frame_length=frame_length, seed=int(seed), thx=pair[0], thh=pair[1], **kwargs)
                        _setup_dpd(run)
                    runs.append(run)
    finally:
        D._share = None
        PJ._stream_share = None
    groups = {}
    for r in runs:
        groups.setdefault(_dpd_group_key(r), []).append(r)
    groups = [_DpdGroup(v) for v in groups.values()]
    _sweep_loop(runs, groups, n_epochs, "ACLR_AVG")
    return [{"status": "completed", "model_path": r.proj.path_save_file_best, "log_path": r.proj.path_log_file_best, "seed": r.proj.seed,
             "DPD_hidden_size": r.proj.DPD_hidden_size, "lockstep": bool(g_.train_sweep),
             **({} if thresholds is None else {"thx": r.proj.thx, "thh": r.proj.thh})} for g_ in groups for r in g_.runs]
