#!/usr/bin/env python3
"""Which kernel every split-path and fused call of the five recurrent families launches, and every bit it writes, for comparing two builds of
the library: a refactor of the host code that chooses those kernels (gru_plan, lstm_plan, delta_plan, janet_plan, qat_plan, split_step and
fused_step of csrc/capi.hip) may move no launch to another kernel, no buffer to another size and no bit.

    python tools/split_kernels.py dump OUT.npz            one library ($OPENDPD_HIP_LIB, else the in-tree one): every C ABI call below, every output
    python tools/split_kernels.py compare A.npz B.npz     the two dumps as uint32 patterns and their kernel lists; exit status 1 if anything differs
    python tools/split_kernels.py run LIB_A LIB_B DIR     a fresh child process per library (dump, with ODPD_AUDIT_LDS=1), then compare

Calls, per (family member, hidden, knob base, B, T): odpd_backbone_fwd without and with ckpt; odpd_backbone_bwd with partials, with dx, with
both; odpd_frozen_loss_dx (float GRU family); odpd_train_fwd_bwd.  Every buffer is sized by the library's own queries (odpd_ckpt_floats,
odpd_partial_rows, odpd_train_workspace_floats, odpd_frozen_loss_rows); a call whose query refuses is not made and the code is kept in its
place.  The knob bases of tests/test_knob_layout_cpu.py force the 16-sequences-per-wave and the row-rotated sides, the built-in crossovers
pick the one-sequence-per-wave kernels at these shapes.  `dump` keeps the `[odpd-lds]` lines of its own stderr (kernel name, dynamic LDS
bytes: one per distinct pair) next to the arrays; an output of more than 2^12 words is kept as its SHA-256 (eight words); return codes are
kept too.  The sparsity counters of the delta backbones are atomic sums in launch order and stay out."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys
import zlib

import numpy as np

BS, TS, HIDDEN = (3, 37, 600), (20, 260), (8, 20, 30)
GRU = ("gru", "dgru", "qgru", "qgru_amp1")
DELTA = ("deltagru", "deltagru_tcnskip", "deltajanet")
KNOBS = ("s16_min_batch", "s16_occupancy", "gp_max_batch", "cascade_one_launch", "xchg_fused", "s16x", "s16x_train", "lstm_pack", "qat_u3")
BASES = {"s16": {"s16_min_batch": 0, "s16_occupancy": 1, "gp_max_batch": 0}, "rot": {"s16_min_batch": 1 << 30, "s16_occupancy": 1, "gp_max_batch": 1 << 30},
         "default": {"s16_min_batch": -1, "s16_occupancy": 0, "gp_max_batch": -1}}      # (every other knob: 1)


def cases():
    """(name, backbone, H, thx, thh, bits, flags by name): what the five families' own kernels take (pgjanet 17 .. 32 is a lane-per-unit route)"""
    out = [(f"{bb}_H{H}", bb, H, 0.0, 0.0, 0, ()) for bb in GRU + ("lstm", "vdlstm") for H in HIDDEN]
    out += [(f"{bb}_H{H}{'_dx' if fl else ''}", bb, H, 0.01, 0.05, 0, fl) for bb in DELTA for H in HIDDEN for fl in ((), ("NEED_DX",))]
    out += [("pgjanet_H8", "pgjanet", 8, 0.0, 0.0, 0, ()), ("pgjanet_H16", "pgjanet", 16, 0.0, 0.0, 0, ())]
    out += [(f"{bb}_q8_H{H}", bb, H, 0.01 if bb in DELTA else 0.0, 0.05 if bb in DELTA else 0.0, 8, ()) for bb in GRU + ("deltagru_tcnskip",) for H in HIDDEN]
    return out


def words(t):
    """a tensor's bit pattern as uint32 words; large ones as their SHA-256"""
    a = t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint32)
    if a.size > 1 << 12:
        return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint32).copy()
    return a.copy()


def dump(path):
    import torch
    from opendpd_amd import _lib
    lib = _lib.load()
    dev, out, nan = "cuda", {}, float("nan")      # outputs start as one fixed pattern, so that what a kernel leaves unwritten compares as well
    st, p = _lib.stream_ptr(), _lib.ptr

    def fresh(*shape):
        return torch.full(shape, nan, device=dev, dtype=torch.float32)

    def code(v):
        return np.asarray([v], dtype=np.int64).view(np.uint32)
    for base, values in BASES.items():
        for k in KNOBS:
            assert lib.odpd_set_tuning(k.encode(), C.c_int64(values.get(k, 1))) == 0, k
        for name, bb, H, thx, thh, bits, flags in cases():
            d = _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, thx, thh, bits, bits, sum(getattr(_lib, "FLAG_" + f) for f in flags))
            m = C.byref(d)
            P = lib.odpd_param_count(m)
            if P <= 0:      # (a quantised model the 16-sequences-per-wave kernels do not take at this hidden size)
                out[f"{base}/{name}/param_count"] = code(P)
                continue
            rng = np.random.RandomState(zlib.crc32(name.encode()))
            pv = (rng.rand(P) * 0.1 + 0.01) if bits else (rng.rand(P) - 0.5) * (2.0 / np.sqrt(H + 1.0))      # (quantised: every scale parameter positive)
            params = torch.from_numpy(pv.astype(np.float32)).to(dev)
            for B in BS:
                for T in TS:
                    key = f"{base}/{name}/B{B}_T{T}"
                    x = (rng.rand(B, T, 2) - 0.5) * 1.6
                    x = torch.from_numpy((x + 0.05 * np.sign(x)).astype(np.float32)).to(dev)
                    dy = torch.from_numpy(((rng.rand(B, T, 2) - 0.5) * 0.3).astype(np.float32)).to(dev)
                    target = torch.from_numpy(((rng.rand(B, T, 2) - 0.5) * 1.2).astype(np.float32)).to(dev)
                    nck, rows, frows = lib.odpd_ckpt_floats(m, B, T), lib.odpd_partial_rows(m, B, T, 0), lib.odpd_partial_rows(m, B, T, 1)
                    ws, lrows = lib.odpd_train_workspace_floats(m, B, T), lib.odpd_frozen_loss_rows(m, B, T)
                    out[key + "/sizes"] = np.asarray([nck, rows, frows, ws, lrows], dtype=np.int64).view(np.uint32)
                    rcs = []
                    stats = torch.zeros(4, device=dev, dtype=torch.float64) if bb in DELTA else None
                    y0 = fresh(B, T, 2)
                    rcs.append(lib.odpd_backbone_fwd(st, m, B, T, p(params), p(x), p(y0), None, p(stats)))
                    out[key + "/fwd/y"] = words(y0)
                    if nck >= 0 and rows > 0:
                        y1, ck = fresh(B, T, 2), fresh(max(nck, 1))
                        rcs.append(lib.odpd_backbone_fwd(st, m, B, T, p(params), p(x), p(y1), p(ck), p(stats)))
                        out[key + "/fwd_ckpt/y"], out[key + "/fwd_ckpt/ckpt"] = words(y1), words(ck)
                        if rcs[-1] == 0:
                            for tag, wp, wx in (("nw", 1, 0), ("dx", 0, 1), ("nw_dx", 1, 1)):
                                part, dx = fresh(rows, P + _lib.LOSS_COLS) if wp else None, fresh(B, T, 2) if wx else None
                                rcs.append(lib.odpd_backbone_bwd(st, m, B, T, p(params), p(x), p(dy), p(ck), p(part), p(dx)))
                                for nm, t in (("partials", part), ("dx", dx)):
                                    if t is not None:
                                        out[f"{key}/bwd_{tag}/{nm}"] = words(t)
                    if lrows > 0 and nck >= 0:      # the frozen-PA loss step: workspace = the checkpoint floats of the shape
                        du, loss, work = fresh(B, T, 2), fresh(lrows, _lib.LOSS_COLS), fresh(max(nck, 1))
                        rcs.append(lib.odpd_frozen_loss_dx(st, m, 0, B, T, B * T * 2, p(params), p(x), p(target), p(du), p(loss), p(work)))
                        out[key + "/lossdx/du"], out[key + "/lossdx/loss_rows"] = words(du), words(loss)
                    if frows > 0 and ws >= 0:       # the fused train step (workspace: checkpoints, or the delta backbones' four counters — zeroed)
                        part, work = fresh(frows, P + _lib.LOSS_COLS), torch.zeros(max(ws, 8), device=dev, dtype=torch.float32)
                        rcs.append(lib.odpd_train_fwd_bwd(st, m, 0, B, T, B * T * 2, p(params), p(x), p(target), p(part), p(work)))
                        out[key + "/train/partials"] = words(part)
                    torch.cuda.synchronize()
                    out[key + "/rc"] = np.asarray(rcs, dtype=np.int32).view(np.uint32)
    np.savez_compressed(path, **out)
    print(f"{_lib.lib_path()}: {len(out)} arrays of {len(cases())} cases x {len(BASES)} knob bases x {len(BS) * len(TS)} shapes -> {path}")


def kernels(text):
    """the sorted (kernel, dynamic LDS bytes) pairs of the `[odpd-lds]` lines"""
    return sorted(set(re.findall(r"^\[odpd-lds\] (\S+) lds=(\d+)", text, flags=re.M)))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    ka, kb = set(a.files), set(b.files)
    bad = sorted(ka ^ kb)
    for k in sorted(ka & kb):
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
            bad.append(k)
    failed = sorted(k for k in ka & kb if k.endswith("/rc") and a[k].any())
    print(f"{len(ka & kb)} arrays compared, {len(bad)} differ; shapes with a call that returned an error (same on both sides unless listed): {len(failed)}")
    for k in bad[:40]:
        print("  differs:", k)
    la, lb = (kernels(open(f + ".lds").read()) if os.path.exists(f + ".lds") else None for f in (pa, pb))
    if la is None or lb is None:
        print("no kernel lists next to the dumps (ODPD_AUDIT_LDS was not set): not compared")
        return 1 if bad else 0
    print(f"kernel lists: {len(la)} and {len(lb)} (kernel, LDS bytes) pairs, {'equal' if la == lb else 'DIFFERENT'}")
    for k in sorted(set(la) ^ set(lb))[:40]:
        print("  only in", "A:" if k in la else "B:", *k)
    return 1 if bad or la != lb or not la else 0


def run(lib_a, lib_b, outdir):
    os.makedirs(outdir, exist_ok=True)
    outs = []
    for tag, lib in (("a", lib_a), ("b", lib_b)):
        outs.append(os.path.join(outdir, f"split_kernels_{tag}.npz"))
        env = dict(os.environ, OPENDPD_HIP_LIB=os.path.abspath(lib), ODPD_AUDIT_LDS="1")
        try:      # (the whole dump takes seconds: a child that is still there after three minutes hangs, and nothing more is started)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "dump", outs[-1]], env=env, stderr=subprocess.PIPE, text=True, timeout=180)
        except subprocess.TimeoutExpired:
            print(f"the dump of {lib} did not end within 180 s: stopped")
            return 124
        with open(outs[-1] + ".lds", "w") as f:
            f.write("".join(ln + "\n" for ln in r.stderr.splitlines() if ln.startswith("[odpd-lds]")))
        sys.stderr.write("".join(ln + "\n" for ln in r.stderr.splitlines() if not ln.startswith("[odpd-lds]")))
        if r.returncode != 0:
            return r.returncode
    return compare(*outs)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    mode, args = (sys.argv[1] if len(sys.argv) > 1 else ""), sys.argv[2:]
    if mode == "dump" and len(args) == 1:
        dump(args[0])
    elif mode == "compare" and len(args) == 2:
        sys.exit(compare(*args))
    elif mode == "run" and len(args) == 3:
        sys.exit(run(*args))
    else:
        sys.exit(__doc__)
