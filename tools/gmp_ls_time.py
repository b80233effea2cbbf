#!/usr/bin/env python3
"""Time of odpd_gmp_gram (csrc/gmp_ls.hip: the 496 x 496 fp64 normal equations of the gmp fit, basis formed in the kernel) at 1 x 23 040 (the
DPA_200MHz training stream's length) and 1 x 1 000 000 synthetic samples, beside the numpy fp64 route on the same machine's CPUs at 23 040
(basis materialised, A^T A through BLAS) and the host solve (opendpd_amd.fit.solve_ridge).  Device-event timings after warm-up, median and
span; the achieved rate counts the useful flops 2 N 496^2 of a sample count N (the kernel issues about as many again: it forms the upper
triangle of 16 x 16 tiles, two matrix rows per sample).
usage (GPU box): PYTHONPATH=. python tools/gmp_ls_time.py [--out FILE] [--rounds N]"""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmp_ls_time.py measures on a HIP device; none found")
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
