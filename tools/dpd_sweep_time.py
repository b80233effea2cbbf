"""Times one train_dpd epoch of K runs (about 2 000 frames, batch 64, frames of 50 and of 200 samples) two ways, in one process:
  (a) K sequential odpd_train_epoch_cascade calls — one run after the other, what K solo train_dpd processes' GPU work adds up to;
  (b) one odpd_train_epoch_cascade_sweep call — every step ONE cascade launch of K x 64 workgroups, one reduction, one clip + AdamW launch;
for K in {1, 2, 4, 8, 16} and the pairs dgru 8 -> dgru 8 and TRes-DeltaGRU 15 -> dgru 23.  Device events around each window, (a) and (b)
alternating for nine rounds after a warm-up of both; median with min and max, per epoch.  A timed window holds as many epochs as make it last
--window-ms (at least --epochs; the same number for (a) and (b)).  The verdict column says whether (b) is slower than (a) beyond the span
of (a)'s own rounds: "ok" while median(b) <= max(a).  Writes <out-dir>/dpd_sweep_time.txt and .json.

--mode threshold: the THRESHOLD sweep instead — TRes-DeltaGRU 15 -> dgru 23 at T = 50, K in {2, 4, 8} runs that differ in their (thx, thh)
pair as well; (a) K sequential odpd_train_epoch_cascade calls, each with a descriptor carrying its run's pair (what runs of differing thresholds
cost without the per-run table), (b) one odpd_train_epoch_cascade_sweep_th call.  Writes <out-dir>/dpd_threshold_sweep_time.txt and .json.
--dpd / --frame-lengths / --ks narrow the cases (re-measuring single rows); --tag names the output files apart.

    python tools/dpd_sweep_time.py [--out-dir profiles] [--rounds 9] [--epochs 4] [--window-ms 250] [--frames 2000]
                                   [--mode seed|threshold] [--dpd NAME] [--frame-lengths 50,200] [--ks 1,2,4,8,16] [--tag TAG]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = [("dgru", 8, "dgru", 8, 0.0, 0.0), ("deltagru_tcnskip", 15, "dgru", 23, 0.01, 0.05)]
KS = (1, 2, 4, 8, 16)
# --mode threshold: run k of K at TH_PAIRS[k] — from dense (0, 0) over the flagship script's pair (0.01, 0.05) to most deltas masked
TH_PAIR, TH_TS, TH_KS = PAIRS[1], (50,), (2, 4, 8)
TH_PAIRS = [(0.0, 0.0), (0.01, 0.05), (0.02, 0.1), (0.05, 0.02), (0.1, 0.2), (0.2, 0.1), (0.4, 0.3), (0.005, 0.01)]
BATCH = 64
BETAS, EPS, WD, MAX_NORM, LR = (0.9, 0.999), 1e-8, 0.01, 200.0, 1e-4


def _model(bb, H, seed, thx=0.0, thh=0.0):
    from opendpd_amd import CoreModel
    torch.manual_seed(seed)
    m = CoreModel(2, H, 1, bb, thx=thx, thh=thh).cuda()
    return m.backbone.desc, m.backbone.flat_params().detach().clone().contiguous()


class Case:
    def __init__(self, pair, T, K, n_frames, thresholds=None):
        from opendpd_amd import _lib
        self.L, self.lib = _lib, _lib.load()
        dbb, dh, pbb, ph, thx, thh = pair
        self.K, self.T, self.n = K, T, n_frames
        self.th = thresholds      # K (thx, thh) pairs: the threshold sweep (None: the seed sweep at the pair of `pair`)
        self.n_steps = (n_frames + BATCH - 1) // BATCH
        rng = np.random.RandomState(T + K)
        ns = n_frames + T - 1
        amp, phase = 0.05 + 0.85 * rng.rand(ns), 2 * np.pi * rng.rand(ns)
        x = np.stack([amp * np.cos(phase), amp * np.sin(phase)], -1).astype(np.float32)
        y = (0.7 * x + 0.05 * rng.randn(ns, 2)).astype(np.float32)
        self.x, self.y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        dm = [_model(dbb, dh, 100 + k, thx, thh) for k in range(K)]
        pm = [_model(pbb, ph, 200 + k) for k in range(K)]
        self.dpd, self.pa = dm[0][0], pm[0][0]
        self.descs = [_lib.ModelDesc(self.dpd.backbone, self.dpd.hidden, *(thresholds[k] if thresholds else (thx, thh)), 0, 0, self.dpd.flags)
                      for k in range(K)]
        self.pa_p = [m[1] for m in pm]
        P = self.P = dm[0][1].numel()
        tail = n_frames - (self.n_steps - 1) * BATCH
        supported = self.lib.odpd_sweep_cascade_th_supported if thresholds else self.lib.odpd_sweep_cascade_supported
        assert all(supported(C.byref(self.dpd), C.byref(self.pa), b, T) == 1 for b in (BATCH, tail)), (pair, T)
        rows = max(int(self.lib.odpd_cascade_rows(C.byref(self.dpd), C.byref(self.pa), b, T)) for b in (BATCH, tail))
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
        g = torch.Generator().manual_seed(K)
        delta = "delta" in dbb
        # two sets of run buffers, so that (a) and (b) train the same K runs from the same start
        self.sets = [[dict(p=dm[k][1].clone(), g=z(P + _lib.LOSS_COLS), m=z(P), v=z(P), losses=z(self.n_steps),
                           part=torch.empty(rows, P + _lib.LOSS_COLS, dtype=torch.float32, device="cuda"),
                           stats=z(4, torch.float64) if delta else None) for k in range(K)] for _ in range(2)]
        self.orders = [torch.randperm(n_frames, generator=g).cuda() for _ in range(K)]
        scratch_bytes = self.lib.odpd_sweep_cascade_th_scratch_bytes if thresholds else self.lib.odpd_sweep_cascade_scratch_bytes
        self.scratch = torch.empty(int(scratch_bytes(K, self.n_steps)), dtype=torch.uint8, device="cuda")
        self.step = [1, 1]

    def _frames(self, order):
        return self.L.Frames(self.x.data_ptr(), self.y.data_ptr(), order.data_ptr() if order is not None else None, self.n, self.T, 1,
                             self.L.SAMPLES_F32, 0)

    def sequential(self):
        L, lib = self.L, self.lib
        for k, b in enumerate(self.sets[0]):
            fr = self._frames(self.orders[k])
            L.check(lib.odpd_train_epoch_cascade(L.stream_ptr(), None, C.byref(self.descs[k]), C.byref(self.pa), 0, C.byref(fr), BATCH, -1, L.ptr(b["p"]),
                                                 L.ptr(self.pa_p[k]), L.ptr(b["g"]), L.ptr(b["m"]), L.ptr(b["v"]), self.step[0], LR, BETAS[0], BETAS[1],
                                                 EPS, WD, MAX_NORM, None, L.ptr(b["part"]), L.ptr(b["stats"]), L.ptr(b["losses"])),
                    "odpd_train_epoch_cascade")
        self.step[0] += self.n_steps

    def sweep(self):
        L, lib, K = self.L, self.lib, self.K
        table, pa_tab = (L.SweepRun * K)(), (C.c_void_p * K)()
        for k, b in enumerate(self.sets[1]):
            table[k] = L.SweepRun(b["p"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), b["part"].data_ptr(),
                                  b["losses"].data_ptr(), None, b["stats"].data_ptr() if b["stats"] is not None else None,
                                  self.orders[k].data_ptr(), LR)
            pa_tab[k] = self.pa_p[k].data_ptr()
        fr = self._frames(None)
        if self.th:
            th = (C.c_float * (2 * K))(*(v for p in self.th for v in p))
            L.check(lib.odpd_train_epoch_cascade_sweep_th(L.stream_ptr(), C.byref(self.dpd), C.byref(self.pa), K, table, pa_tab, th, 0, C.byref(fr), BATCH,
                                                          self.step[1], BETAS[0], BETAS[1], EPS, WD, MAX_NORM, C.c_void_p(self.scratch.data_ptr())),
                    "odpd_train_epoch_cascade_sweep_th")
            self.step[1] += self.n_steps
            return
        L.check(lib.odpd_train_epoch_cascade_sweep(L.stream_ptr(), C.byref(self.dpd), C.byref(self.pa), K, table, pa_tab, 0, C.byref(fr), BATCH,
                                                   self.step[1], BETAS[0], BETAS[1], EPS, WD, MAX_NORM, C.c_void_p(self.scratch.data_ptr())),
                "odpd_train_epoch_cascade_sweep")
        self.step[1] += self.n_steps

    def same(self):
        return all(torch.equal(a["p"], b["p"]) and torch.equal(a["losses"], b["losses"]) and (a["stats"] is None or torch.equal(a["stats"], b["stats"]))
                   for a, b in zip(*self.sets))

    def sparsity(self):
        """zeroed share of the input and of the hidden deltas of every run of (b), over all its epochs so far (delta DPDs)"""
        return [(float(b["stats"][0] / b["stats"][1]), float(b["stats"][2] / b["stats"][3])) for b in self.sets[1]]


def _window(fn, epochs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(epochs):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / epochs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out-dir", default="profiles")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--epochs", type=int, default=4, help="epochs per timed window")
    ap.add_argument("--window-ms", type=float, default=250.0, help="least duration of a timed window")
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--mode", choices=("seed", "threshold"), default="seed")
    ap.add_argument("--dpd", default="", help="only the pairs whose DPD backbone has this name")
    ap.add_argument("--frame-lengths", default="", help="comma-separated; default 50,200 (threshold mode: 50)")
    ap.add_argument("--ks", default="", help="comma-separated; default 1,2,4,8,16 (threshold mode: 2,4,8)")
    ap.add_argument("--tag", default="", help="suffix of the output files' names")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpd_sweep_time.py needs a GPU: there is nothing to time without one")
    th_mode = args.mode == "threshold"
    ints = lambda text, default: tuple(int(v) for v in text.split(",")) if text else default
    pairs = [p for p in ([TH_PAIR] if th_mode else PAIRS) if not args.dpd or p[0] == args.dpd]
    rows = []
    for pair in pairs:
        for T in ints(args.frame_lengths, TH_TS if th_mode else (50, 200)):
            for K in ints(args.ks, TH_KS if th_mode else KS):
                c = Case(pair, T, K, args.frames, TH_PAIRS[:K] if th_mode else None)
                for _ in range(2):      # warm-up of both paths (code objects, allocator), the same number of epochs each
                    c.sequential(); c.sweep()
                torch.cuda.synchronize()
                one = min(_window(c.sequential, 1), _window(c.sweep, 1))      # (one epoch each: the two stay in step)
                epochs = max(args.epochs, min(400, int(args.window_ms / max(one, 1e-3)) + 1))
                ta, tb = [], []
                for _ in range(args.rounds):
                    ta.append(_window(c.sequential, epochs))
                    tb.append(_window(c.sweep, epochs))
                rows.append(dict(dpd=f"{pair[0]} {pair[1]}", pa=f"{pair[2]} {pair[3]}", batch=BATCH, T=T, K=K, frames=args.frames,
                                 steps=c.n_steps, epochs_per_window=epochs, sweep_within_sequential_span=bool(statistics.median(tb) <= max(ta)),
                                 sequential_ms=dict(median=statistics.median(ta), min=min(ta), max=max(ta)),
                                 sweep_ms=dict(median=statistics.median(tb), min=min(tb), max=max(tb)),
                                 ratio=statistics.median(ta) / statistics.median(tb), bit_identical=bool(c.same()),
                                 **(dict(thresholds=TH_PAIRS[:K], zeroed_dx_dh=c.sparsity()) if th_mode else {})))
                print(rows[-1], flush=True)
    lines = [f"one train_dpd epoch of K runs: {args.frames} frames, batch {BATCH} ({rows[0]['steps']} steps); ms per epoch, device events, "
             f"median [min .. max] of {args.rounds} alternating rounds (windows of >= {args.window_ms:.0f} ms: 'ep' epochs each); {torch.cuda.get_device_name(0)}",
             "(a) K sequential odpd_train_epoch_cascade calls, run k at its own (thx, thh)   (b) one odpd_train_epoch_cascade_sweep_th call   "
             "same: (b)'s runs == (a)'s, bit for bit (parameters, losses, counters)" if th_mode else
             "(a) K sequential odpd_train_epoch_cascade calls   (b) one odpd_train_epoch_cascade_sweep call   same: (b)'s runs == (a)'s, bit for bit",
             "verdict: ok = median(b) <= max(a), i.e. (b) not slower than (a) beyond the span of (a)'s own rounds",
             "", f"{'DPD -> PA':34s} {'T':>4s} {'K':>3s} {'ep':>4s}  {'(a) sequential':>28s}  {'(b) sweep':>28s}  {'a/b':>6s}  same  verdict"]
    fmt = lambda d: f"{d['median']:8.2f} [{d['min']:7.2f} .. {d['max']:7.2f}]"
    for r in rows:
        lines.append(f"{r['dpd'] + ' -> ' + r['pa']:34s} {r['T']:4d} {r['K']:3d} {r['epochs_per_window']:4d}  {fmt(r['sequential_ms']):>28s}  "
                     f"{fmt(r['sweep_ms']):>28s}  {r['ratio']:6.2f}  {'yes ' if r['bit_identical'] else 'NO  '}  "
                     f"{'ok' if r['sweep_within_sequential_span'] else 'SLOWER'}")
    if th_mode:
        lines += ["", "run k of a row runs at pair k of " + ", ".join(f"({a:g}, {b:g})" for a, b in TH_PAIRS),
                  "zeroed share of the input / hidden deltas per run, over all epochs of (b):"]
        lines += [f"  K = {r['K']}: " + "  ".join(f"{dx:.2f} / {dh:.2f}" for dx, dh in r["zeroed_dx_dh"]) for r in rows]
    os.makedirs(args.out_dir, exist_ok=True)
    name = ("dpd_threshold_sweep_time" if th_mode else "dpd_sweep_time") + args.tag
    with open(os.path.join(args.out_dir, name + ".txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(args.out_dir, name + ".json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, window_ms=args.window_ms, rows=rows), f, indent=1)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
