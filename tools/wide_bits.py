#!/usr/bin/env python3
"""Bit patterns of everything the lane-per-unit kernels write (csrc/gru_wide.hip, lstm_wide.hip, vdlstm_wide.hip, delta_wide.hip,
deltajanet_wide.hip, janet_wide.hip, gru_layers2.hip, lstm_layers2.hip), for comparing two builds of the library: a refactor of these
files may move instructions, it must not move a bit.

    python tools/wide_bits.py dump OUT.npz            one library ($OPENDPD_HIP_LIB, else the in-tree one): every C ABI call below, every output
    python tools/wide_bits.py compare A.npz B.npz     the two dumps as uint32 patterns; exit status 1 if any array differs
    python tools/wide_bits.py run LIB_A LIB_B DIR     a fresh child process per library (dump), then compare

Calls: odpd_backbone_fwd with and without ckpt; odpd_backbone_bwd with partials and dx, partials alone, dx alone; on the state route the
_state pair, the backward also with dh0 alone.  Cases: every backbone these files serve at the block edges of its hidden size, at shapes
with one step, odd lengths, exactly one chunk, a ragged second chunk, several chunks, more sequences than one per CU and a batch beyond
the grid cap; the delta backbones with thresholds (0, 0) and (0.01, 0.05) including the sparsity counters; quantised heads on lstm and
deltajanet.  An output of more than 2^12 words is kept as its SHA-256 (eight words); return codes are kept too."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import zlib

import numpy as np

SHAPES = ((1, 1), (3, 5), (4, 64), (5, 70), (2, 200), (70, 33), (1100, 6))
WIDE = ("gru", "dgru", "qgru", "qgru_amp1", "lstm", "vdlstm", "deltagru", "deltagru_tcnskip", "deltajanet")
STATE = TWO = ("gru", "dgru", "qgru", "qgru_amp1", "lstm")
DELTA = ("deltagru", "deltagru_tcnskip", "deltajanet")


def cases():
    """(name, backbone, H, thx, thh, bits, flags by name)"""
    out = []
    for bb in WIDE:
        for H in (33, 48, 64):
            for thx, thh in (((0.0, 0.0), (0.01, 0.05)) if bb in DELTA else ((0.0, 0.0),)):
                out.append((f"{bb}_H{H}" + (f"_th{thx}_{thh}" if bb in DELTA else ""), bb, H, thx, thh, 0, ()))
    out += [(f"pgjanet_H{H}", "pgjanet", H, 0.0, 0.0, 0, ()) for H in (17, 32)]
    out += [(f"{bb}_x2_H{H}", bb, H, 0.0, 0.0, 0, ("TWO_LAYERS",)) for bb in TWO for H in (8, 23, 32)]
    out += [(f"{bb}_state_H{H}", bb, H, 0.0, 0.0, 0, ("INIT_STATE",)) for bb in STATE for H in (1, 16, 17, 40, 64)]
    out += [("lstm_q8_H48", "lstm", 48, 0.0, 0.0, 8, ()), ("deltajanet_q8_H40", "deltajanet", 40, 0.0, 0.0, 8, ())]
    return out


def words(t):
    """a tensor's bit pattern as uint32 words (doubles: two words each); large ones as their SHA-256"""
    a = t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint32)
    if a.size > 1 << 12:
        return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint32).copy()
    return a.copy()


def dump(path):
    import torch
    from opendpd_amd import _lib
    lib = _lib.load()
    dev, out, wild = "cuda", {}, []      # wild: outputs that hold a non-finite value (a comparison of NaN payloads would say nothing)
    nan = float("nan")      # outputs start as one fixed pattern, so that what a kernel leaves unwritten compares as well

    def fresh(*shape, dtype=torch.float32):
        return torch.full(shape, nan, device=dev, dtype=dtype)
    for name, bb, H, thx, thh, bits, flags in cases():
        fl = sum(getattr(_lib, "FLAG_" + f) for f in flags)
        d = _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, thx, thh, bits, bits, fl)
        state = "INIT_STATE" in flags
        P = lib.odpd_param_count(C.byref(d))
        assert P > 0, (name, P)
        rng = np.random.RandomState(zlib.crc32(name.encode()))
        pv = ((rng.rand(P) - 0.5) * (2.0 / np.sqrt(H + 1.0))).astype(np.float32)
        if bits:
            pv[-3:] = np.float32([0.01, 0.02, 0.0005])      # the three scale parameters of the quantised head
        params = torch.from_numpy(pv).to(dev)
        for B, T in SHAPES:
            key = f"{name}/B{B}_T{T}"
            x = (rng.rand(B, T, 2) - 0.5) * 1.6
            x = torch.from_numpy((x + 0.05 * np.sign(x)).astype(np.float32)).to(dev)
            dy = torch.from_numpy(((rng.rand(B, T, 2) - 0.5) * 0.3).astype(np.float32)).to(dev)
            h0 = torch.from_numpy(((rng.rand(B, H) - 0.5) * 0.8).astype(np.float32)).to(dev) if state else None
            nck, rows = lib.odpd_ckpt_floats(C.byref(d), B, T), lib.odpd_partial_rows(C.byref(d), B, T, 0)
            assert nck > 0 and rows > 0, (key, nck, rows)
            st, p = _lib.stream_ptr(), _lib.ptr

            def fwd(y, ck, stats):
                if state:
                    return lib.odpd_backbone_fwd_state(st, C.byref(d), B, T, p(params), p(x), p(h0), p(y), p(ck))
                return lib.odpd_backbone_fwd(st, C.byref(d), B, T, p(params), p(x), p(y), p(ck), p(stats))

            def bwd(ck, part, dx, dh0):
                if state:
                    return lib.odpd_backbone_bwd_state(st, C.byref(d), B, T, p(params), p(x), p(h0), p(dy), p(ck), p(part), p(dx), p(dh0))
                return lib.odpd_backbone_bwd(st, C.byref(d), B, T, p(params), p(x), p(dy), p(ck), p(part), p(dx))
            rcs = []
            # forward without and with the per-step records
            y0, s0 = fresh(B, T, 2), torch.zeros(4, device=dev, dtype=torch.float64)
            rcs.append(fwd(y0, None, s0 if bb in DELTA else None))
            y1, ck, s1 = fresh(B, T, 2), fresh(nck), torch.zeros(4, device=dev, dtype=torch.float64)
            rcs.append(fwd(y1, ck, s1 if bb in DELTA else None))
            if bb == "dgru" and "TWO_LAYERS" not in flags and rcs[-1] == 0:
                # gru_wide.hip copies the fc_hid pre-activations to record slot 5 from LDS rows of which it has written columns < H only:
                # lanes >= H of that slot hold whatever an earlier kernel left in LDS (the backward never uses them)
                ck.view(B, T, 6, 64)[:, :, 5, H:] = 0.0
            out[key + "/fwd/y"], out[key + "/fwd_ckpt/y"], out[key + "/fwd_ckpt/ckpt"] = words(y0), words(y1), words(ck)
            if rcs[-1] == 0 and not all(bool(torch.isfinite(t).all()) for t in (y0, y1)):      # (not ckpt: a record may have slots no kernel writes)
                wild.append(key + "/fwd")
            if bb in DELTA:
                out[key + "/fwd/stats"], out[key + "/fwd_ckpt/stats"] = words(s0), words(s1)
            # backward: partials and dx, partials alone, dx alone; the state route: each with dh0, and dh0 alone
            if rcs[-1] == 0:
                for tag, wp, wx, wh in (("nw_dx", 1, 1, 1), ("nw", 1, 0, 1), ("dx", 0, 1, 1)) + ((("dh0", 0, 0, 1),) if state else ()):
                    part = fresh(rows, P + _lib.LOSS_COLS) if wp else None
                    dx = fresh(B, T, 2) if wx else None
                    dh0 = fresh(B, H) if (wh and state) else None
                    rcs.append(bwd(ck, part, dx, dh0))
                    for nm, t in (("partials", part), ("dx", dx), ("dh0", dh0)):
                        if t is not None:
                            out[f"{key}/bwd_{tag}/{nm}"] = words(t)
                            if not bool(torch.isfinite(t).all()):
                                wild.append(f"{key}/bwd_{tag}/{nm}")
            torch.cuda.synchronize()
            out[key + "/rc"] = np.asarray(rcs, dtype=np.int32).view(np.uint32)
    np.savez_compressed(path, **out)
    if wild:
        raise SystemExit(f"{len(wild)} outputs hold non-finite values, e.g. {wild[:5]}: the inputs are wrong")
    print(f"{_lib.lib_path()}: {len(out)} arrays of {len(cases())} cases x {len(SHAPES)} shapes -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    ka, kb = set(a.files), set(b.files)
    bad = sorted(ka ^ kb)
    for k in sorted(ka & kb):
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
            bad.append(k)
    failed = sorted(k for k in ka & kb if k.endswith("/rc") and a[k].any())
    print(f"{len(ka & kb)} arrays compared, {len(bad)} differ; calls that returned an error (same on both sides unless listed): {len(failed)}")
    for k in bad[:40]:
        print("  differs:", k)
    for k in failed[:20]:
        print("  error codes:", k, a[k].view(np.int32).tolist())
    return 1 if bad else 0


def run(lib_a, lib_b, outdir):
    os.makedirs(outdir, exist_ok=True)
    outs = []
    for tag, lib in (("a", lib_a), ("b", lib_b)):
        outs.append(os.path.join(outdir, f"wide_bits_{tag}.npz"))
        subprocess.run([sys.executable, os.path.abspath(__file__), "dump", outs[-1]], env=dict(os.environ, OPENDPD_HIP_LIB=os.path.abspath(lib)), check=True)
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
