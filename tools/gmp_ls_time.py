#!/usr/bin/env python3
"""Time of odpd_gmp_gram (csrc/gmp_ls.hip: the 496 x 496 fp64 normal equations of the gmp fit, basis formed in the kernel) at 1 x 23 040 (the
DPA_200MHz training stream's length) and 1 x 1 000 000 synthetic samples, beside the numpy fp64 route on the same machine's CPUs at 23 040
(basis materialised, A^T A through BLAS) and the host solve (opendpd_amd.fit.solve_ridge).  Device-event timings after warm-up, median and
span; the achieved rate counts the useful flops 2 N 496^2 of a sample count N (the kernel issues about as many again: it forms the upper
triangle of 16 x 16 tiles, two matrix rows per sample).
usage (GPU box): PYTHONPATH=. python tools/gmp_ls_time.py [--out FILE] [--rounds N]
                 PYTHONPATH=. python tools/gmp_ls_time.py --direct [--out FILE] [--iterations N] [--epochs N]      (see direct())"""
import argparse
import json
import os
import time

import numpy as np
import torch

from opendpd_amd import gmp_gram, solve_ridge

COLS = 496


def numpy_gram(x, t):
    """the fp64 route a numpy user takes: [A | b] of one sequence (gmp.py:25-46, zero history) materialised, then one GEMM"""
    x, t = x.astype(np.float64), t.astype(np.float64)
    T, M = len(x), 11
    u = np.concatenate([np.zeros(M - 1, dtype=np.complex128), x[:, 0] + 1j * x[:, 1]])
    a = np.concatenate([np.zeros(2 * (M - 1)), np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])])
    pw, n = [a, a * a, a * a * a, (a * a) * (a * a)], np.arange(T)
    cols = [u[n + m] for m in range(M)] + [u[n + m] * pw[d][n + i + m] for d in range(4) for i in range(M) for m in range(M)]
    phi = np.stack(cols + [t[:, 0] + 1j * t[:, 1]], axis=1)
    A = np.concatenate([phi.real, phi.imag], 0)
    return A.T @ A


def signal(T, seed):
    rng = np.random.RandomState(seed)
    amp, ph = 0.05 + 0.85 * rng.rand(T, 1), 2 * np.pi * rng.rand(T, 1)
    x = np.concatenate([amp * np.cos(ph), amp * np.sin(ph)], -1).astype(np.float32)
    return x, (0.5 * rng.randn(T, 2)).astype(np.float32)


def span(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def direct(a):
    """--direct: fit_dpd_direct on DPA_200MHz (tests/golden/dpa200_dataset.npz, written out as a dataset in a scratch directory) through two
    PA models — fit_pa's gmp and a dgru trained by train_pa — from the indirect start, beside train_dpd --DPD_backbone gmp epochs on the same
    PA in the same process.  Per row of each run's own history: loss, step, the cascade's validation / test NMSE and ACLR; per run the
    wall time of a row (iteration or epoch with its evaluation, from the log's TIME column) and of refine_gmp_dpd alone (second call)."""
    import tempfile
    import pandas as pd
    import opendpd_amd as od
    from opendpd_amd import data as D
    from opendpd_amd.fit import fit_gmp, refine_gmp_dpd
    from opendpd_amd.project import _direct_project, run_fit_dpd_direct
    golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "dpa200_dataset.npz")
    d = dict(np.load(golden))
    os.chdir(tempfile.mkdtemp(prefix="gmp_dla_"))
    ds = os.path.join("datasets", "DPA_200MHz")
    os.makedirs(ds)
    open(os.path.join(ds, "spec.json"), "w").write(str(d.pop("spec")))
    for k, v in d.items():
        pd.DataFrame(v, columns=["I", "Q"]).to_csv(os.path.join(ds, f"{k}.csv"), index=False)
    F, cols = a.frame_length, ["TRAIN_LOSS", "VAL_NMSE", "VAL_ACLR_AVG", "TEST_NMSE", "TEST_ACLR_AVG"]
    result = []
    for backbone, hidden in (("gmp", 11), ("dgru", a.pa_hidden)):
        kw = dict(dataset_name="DPA_200MHz", PA_backbone=backbone, PA_hidden_size=hidden, frame_length=F, accelerator="cuda")
        if backbone == "gmp":
            pa_log = od.fit_pa(dataset_name="DPA_200MHz", frame_length=F)["log_path"]
        else:
            pa_log = od.train_pa(n_epochs=a.pa_epochs, batch_size=64, lr=5e-3, **kw)["log_path"]
        pa_nmse = float(pd.read_csv(pa_log)["TEST_NMSE"].iloc[0])
        proj = _direct_project(a.iterations, 1e-6, "ila", dict(kw))
        net = run_fit_dpd_direct(proj, iterations=a.iterations)
        run, hist = net.dpd_model.gmp_refine, pd.read_csv(proj.path_log_file_hist)
        # the loop alone, second call in the process (no evaluation, no files): same frames, same start
        Xtr, ytr = D.load_dataset("DPA_200MHz")[:2]
        n = len(Xtr) // F
        fr = lambda s: torch.as_tensor(np.asarray(s[:n * F]), dtype=torch.float32).cuda().reshape(n, F, 2)
        alone = []
        for _ in range(3):
            dpd = fit_gmp(fr(ytr / proj.target_gain), fr(Xtr))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps = len(refine_gmp_dpd(dpd, net.pa_model, fr(Xtr), proj.target_gain, iterations=a.iterations).gmp_refine["steps"])
            alone.append((time.perf_counter() - t0) * 1e3 / max(steps, 1))
        per_row = lambda h: float(h["TIME:"].iloc[-1] - h["TIME:"].iloc[0]) * 60e3 / max(len(h) - 1, 1)
        sgd = pd.read_csv(od.train_dpd(DPD_backbone="gmp", DPD_hidden_size=11, n_epochs=a.epochs, batch_size=64, lr=5e-3, **kw)["log_path"]
                          .replace(os.sep + "best" + os.sep, os.sep + "history" + os.sep))
        print(f"\nPA {backbone} H {hidden} (TEST_NMSE {pa_nmse:.2f} dB), {n} frames of {F}: fit_dpd_direct stopped by '{run['stopped']}'; "
              f"{per_row(hist):.1f} ms per logged iteration, refine_gmp_dpd alone {span(alone)['median']:.1f} ms per iteration "
              f"({span(alone)['min']:.1f} .. {span(alone)['max']:.1f}); train_dpd gmp {per_row(sgd):.1f} ms per epoch")
        print("| run | row | step | " + " | ".join(cols) + " |\n|---|---|---|" + "---|" * len(cols))
        for name, h, steps in (("fit_dpd_direct", hist, ["start"] + run["steps"]), ("train_dpd gmp", sgd, ["-"] * len(sgd))):
            for i in range(len(h)):
                print(f"| {name} | {i} | {steps[i]} | " + " | ".join(f"{h[c].iloc[i]:.8f}" if c == "TRAIN_LOSS" else f"{h[c].iloc[i]:.2f}" for c in cols) + " |",
                      flush=True)
        result.append(dict(pa=backbone, pa_hidden=hidden, pa_test_nmse=pa_nmse, frames=n, frame_length=F, refine=dict(run, w=None),
                           direct_ms_per_row=per_row(hist), refine_alone_ms_per_iteration=span(alone), train_dpd_ms_per_epoch=per_row(sgd),
                           direct=hist[cols].to_dict("list"), train_dpd=sgd[cols].to_dict("list")))
    if a.out:
        json.dump(result, open(a.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--direct", action="store_true", help="the fit_dpd_direct table of docs/design/gmp_ls.md instead of the Gram timings")
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--frame_length", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=8, help="--direct: train_dpd epochs to set beside the iterations")
    ap.add_argument("--pa_hidden", type=int, default=8, help="--direct: hidden size of the recurrent (dgru) PA")
    ap.add_argument("--pa_epochs", type=int, default=10, help="--direct: train_pa epochs of the recurrent PA")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmp_ls_time.py measures on a HIP device; none found")
    if a.direct:
        a.out = a.out and os.path.abspath(a.out)
        return direct(a)
    rows = []
    print("| samples | odpd_gmp_gram ms, median (min .. max) | useful Tflop/s | numpy fp64 ms | solve_ridge ms |\n|---|---|---|---|---|")
    for T in (23040, 1000000):
        x, t = signal(T, T)
        xd, td = torch.from_numpy(x[None]).cuda(), torch.from_numpy(t[None]).cuda()
        for _ in range(3):
            G = gmp_gram(xd, td)
        torch.cuda.synchronize()
        reps = 20 if T < 100000 else 3
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                gmp_gram(xd, td)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        row = dict(B=1, T=T, gram_ms=span(ms), useful_flops=2.0 * T * COLS * COLS)
        row["useful_tflops"] = row["useful_flops"] / (row["gram_ms"]["median"] * 1e-3) / 1e12
        t0 = time.perf_counter()
        sol = solve_ridge(G, 1e-6)
        row["solve_ridge_ms"] = (time.perf_counter() - t0) * 1e3
        row["e_min"], row["e_max"] = sol.e_min, sol.e_max
        cpu = "-"
        if T < 100000:
            numpy_gram(x, t)
            cms = []
            for _ in range(3):
                t0 = time.perf_counter()
                Gn = numpy_gram(x, t)
                cms.append((time.perf_counter() - t0) * 1e3)
            row["numpy_ms"] = span(cms)
            d = np.sqrt(np.diag(Gn))
            row["max_err_over_bound"] = float(np.max(np.abs(G.cpu().numpy() - Gn) / ((2 * T + 64) * 2.0 ** -53 * np.outer(d, d))))
            cpu = f"{row['numpy_ms']['median']:.0f}"
        g = row["gram_ms"]
        print(f"| 1 x {T} | {g['median']:.3f} ({g['min']:.3f} .. {g['max']:.3f}) | {row['useful_tflops']:.2f} | {cpu} | {row['solve_ridge_ms']:.0f} |",
              flush=True)
        rows.append(row)
    if a.out:
        json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
