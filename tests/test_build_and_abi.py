"""CPU checks: the HIP library builds for gfx950, loads, and exports every symbol that
include/opendpd_hip.h declares; the registry mirrors the reference's names / state-dict keys."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_and_exports_header_symbols():
    import __graft_entry__ as g
    g.build()
    from opendpd_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "opendpd_hip.h")).read()
    declared = set(re.findall(r"\b(odpd_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} declared in the header but not exported"
    assert declared == set(_lib.exported_symbols())
    assert lib.odpd_abi_version() == _lib.ABI_VERSION == 13


def test_no_kernel_spills_beyond_the_recorded_allowance():
    """Every instantiation's register / scratch usage is recorded at build time (-Rpass-analysis=kernel-resource-usage ->
    lib/kernel_resources.json).  A kernel that starts to spill, or spills more than when it was validated
    (csrc/known_scratch.json), is where a compiler bump changes schedules silently: fail here, re-validate, then re-record."""
    import __graft_entry__ as g
    g.build()
    from opendpd_amd import build as hb
    assert os.path.exists(hb.RESOURCES)
    assert hb.unexpected_scratch() == []


def test_param_counts_match_reference():
    import ctypes as C
    from opendpd_amd import _lib
    lib = _lib.load()
    # N_PARAM values measured on the reference
    for bb, H, P in [("gru", 11, 519), ("gru", 23, 1911), ("dgru", 13, 1041), ("dgru", 23, 2751), ("lstm", 14, 1038),
                     ("vdlstm", 13, 1118), ("deltagru", 15, 1067), ("deltagru_tcnskip", 15, 999), ("tcnn", 35, 1015),
                     ("pgjanet", 11, 959), ("qgru", 10, 502), ("qgru_amp1", 16, 1090), ("gmp", 11, 495), ("rvtdcnn", 25, 1007),
                     ("rvtdcnn", 6, 266), ("neuraltx", 36, 986), ("deltajanet", 15, 722), ("deltajanet", 22, 1366)]:
        d = _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, 0, 0, 0, 0, 0)
        assert lib.odpd_param_count(C.byref(d)) == P, bb
    # quantised models (bits_w > 0): + the quantiser scales of the surgery's result [measured on the reference: tests/golden/quant_*.npz]
    for bb, H, P in [("qgru", 10, 515), ("gru", 11, 532), ("gru", 23, 1924), ("dgru", 13, 1057), ("dgru", 23, 2767), ("qgru", 20, 1615),
                     ("qgru", 30, 3315), ("deltagru_tcnskip", 15, 1012), ("deltagru_tcnskip", 30, 3337)]:
        d = _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, 0, 0, 8, 8, 0)
        assert lib.odpd_param_count(C.byref(d)) == P, bb
    # ... the heads-only surgeries (float core + INT_Linear heads: three scales per head) [tests/golden/quant_{lstm,vdlstm,deltajanet,neuraltx,rvtdcnn}_*.npz]
    for bb, H, P in [("lstm", 14, 1041), ("lstm", 40, 7125), ("vdlstm", 13, 1127), ("deltajanet", 12, 509), ("neuraltx", 12, 341), ("rvtdcnn", 12, 508),
                     ("rvtdcnn", 32, 1288), ("pgjanet", 11, 977), ("pgjanet", 24, 4292)]:
        d = _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, 0, 0, 8, 8, 0)
        assert lib.odpd_param_count(C.byref(d)) == P, bb
    # bits_w > 0 on a backbone without a quantised model is refused (never answered with the float kernels); dvrjanet's bits_w is its DVR count
    for bb in ("apnrru", "bojanet", "mcldnn", "deltagru", "gmp", "tcnn"):
        d = _lib.ModelDesc(_lib.BACKBONE_IDS[bb], 11, 0, 0, 8, 8, 0)
        assert lib.odpd_param_count(C.byref(d)) == -1, bb      # ODPD_EINVAL
        assert lib.odpd_partial_rows(C.byref(d), 4, 10, 0) == -1, bb
    assert lib.odpd_param_count(C.byref(_lib.ModelDesc(_lib.BACKBONE_IDS["dvrjanet"], 8, 0, 0, 4, 0, 0))) > 0


@pytest.mark.parametrize("name,bb", [("gru_h11", "gru"), ("dgru_h13", "dgru"), ("dgru_h23", "dgru"),
                                     ("qgru_h10", "qgru"), ("qgru_amp1_h10", "qgru_amp1"),
                                     ("lstm_h14", "lstm"), ("vdlstm_h13", "vdlstm"),
                                     ("deltagru_h15_th", "deltagru"), ("tres_h15_th", "deltagru_tcnskip"),
                                     ("pgjanet_h11", "pgjanet"), ("tcnn_c35", "tcnn"), ("gmp_m11", "gmp"),
                                     ("rvtdcnn_h25", "rvtdcnn"), ("neuraltx_c36", "neuraltx"), ("deltajanet_h15", "deltajanet")])
def test_registry_init_is_bit_identical_to_reference(name, bb):
    """Same seed -> same RNG consumption -> identical initial state dict (keys, order, values)."""
    from opendpd_amd import CoreModel
    from tests.golden_util import Fixture
    fx = Fixture(name)
    # orthogonal_ goes through LAPACK's QR, whose last bit depends on the thread count of the PROCESS (seen on the 256-core GPU host when this
    # file ran after a test that had set another OpenMP team size).  The fixtures were generated at the build container's default; the
    # construction below runs single-threaded first and, if an orthogonally initialised tensor then differs, once more at the ambient count —
    # one of the two reproduces the fixture BIT FOR BIT.  Every tensor that is not orthogonally initialised must be bit-identical outright.
    def construct():
        torch.manual_seed(0)
        return CoreModel(2, fx.meta["hidden"], 1, bb, thx=fx.meta.get("thx", 0), thh=fx.meta.get("thh", 0))

    # the tensors nn.init.orthogonal_ touches: every "weight" of the recurrent core `backbone.rnn.*` (backbones/native.py:49-51, deltagru.py:51-53);
    # heads, TCN, pgjanet's Linear gates are xavier / kaiming / default — elementwise RNG draws, exact at any thread count
    ortho = [k for k in construct().state_dict() if k.startswith("backbone.rnn.") and "weight" in k]
    keep = torch.get_num_threads()
    tried = {}
    try:
        for nt in dict.fromkeys((keep, 1, 8)):
            torch.set_num_threads(nt)
            net = construct()
            sd = net.state_dict()
            tried[nt] = [k for k in sd if not np.array_equal(sd[k].numpy(), fx["sd/" + k])]
            if not tried[nt]:
                break
    finally:
        torch.set_num_threads(keep)
    assert list(sd.keys()) == fx.keys("sd")
    for nt, bad in tried.items():
        assert all(k in ortho for k in bad), (nt, bad)      # only QR-initialised tensors may depend on the thread count
    best = min(tried.values(), key=len)
    for k in best:       # no thread count of this host reproduced LAPACK's last bit: the tensor must still be the same matrix to one ulp
        assert np.abs(sd[k].numpy() - fx["sd/" + k]).max() < 5e-7, k
    assert sum(p.numel() for p in net.parameters()) == fx.meta["n_param"]


def test_no_cpu_fallback():
    from opendpd_amd import CoreModel
    net = CoreModel(2, 8, 1, "gru")
    with pytest.raises(RuntimeError):
        net(torch.rand(2, 5, 2))


def test_registry_errors():
    from opendpd_amd import CoreModel
    with pytest.raises(ValueError):
        CoreModel(2, 8, 1, "not_a_backbone")


def test_flat_buffer_survives_load_and_move():
    from opendpd_amd import CoreModel
    net = CoreModel(2, 9, 1, "dgru")
    f = net.backbone.flat_params()
    sd = {k: v.clone() + 1 for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    assert net.backbone.flat_params().data_ptr() == f.data_ptr()
    cat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    assert torch.equal(cat, net.backbone.flat_params())
    net = net.double().float()   # _apply re-points every parameter
    cat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    assert torch.equal(cat, net.backbone.flat_params())


def _asm_statements(text):
    """the parenthesised bodies of the asm statements of a source text (balanced parentheses; macro continuations joined)"""
    import re
    text = text.replace("\\\n", " ")
    out = []
    for m in re.finditer(r"\basm\b\s*(?:volatile\s*)?\(", text):
        depth, j = 1, m.end()
        while depth and j < len(text):
            depth += {"(": 1, ")": -1}.get(text[j], 0)
            j += 1
        out.append(text[m.end():j - 1])
    return out


def test_multi_instruction_asm_groups_take_early_clobber_accumulators():
    """The rotated-dot-product groups of csrc/odpd_device.h are several v_fmac_f32_dpp in ONE asm statement: an accumulator declared "+v" may
    be given the register of an input that holds the same value at entry (a weight proved to be the constant 0 next to an accumulator that
    starts at 0 — found in r03: rotation 8 of an 8-unit LSTM multiplied by the running sum).  Every asm statement with more
    than one instruction must declare its read-write operands early-clobber ("+&v")."""
    import glob
    import re
    csrc = os.path.join(ROOT, "opendpd_amd", "csrc")

    def offenders(text):
        bad = []
        for body in _asm_statements(text):
            n_instr = body.count("v_fmac_f32_dpp") + len(re.findall(r"ODPD_DPPF\(", body)) + 3 * len(re.findall(r"ODPD_F3\(", body))
            if n_instr > 1 and '"+v"' in body:
                bad.append(body[:80])
        return bad

    dev = open(os.path.join(csrc, "odpd_device.h")).read()
    assert offenders(dev.replace('"+&v"', '"+v"')), "the check must see the groups"        # (self-test on the pre-fix form)
    for path in sorted(glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip"))):
        assert not offenders(open(path).read()), os.path.basename(path)


def test_instruction_bearing_asm_never_has_a_pure_vgpr_output():
    """Root cause of the r02 wrong-result build (r04, tools/asm_mfma_hazards.py): `relu_` was `asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(v))`.
    A write-only asm output is the FIRST writer of whatever register the allocator picks — possibly the C operand of a v_mfma issued a
    few slots earlier, which the XDL pipeline is still reading; the compiler's hazard recognizer does not look inside asm, so no wait
    state is inserted (a read-write "+v" operand always has a compiler-visible definition in between, which pays the wait).  Rule: an
    asm statement that contains an instruction may not declare "=v" / "=&v" outputs."""
    import glob
    import re
    csrc = os.path.join(ROOT, "opendpd_amd", "csrc")

    def offenders(text):
        bad = []
        for body in _asm_statements(text):
            template = body.split(":")[0]
            has_instr = bool(re.search(r"\b[vs]_[a-z0-9_]+", template)) or "ODPD_" in template
            if has_instr and re.search(r'"=&?v"', body):
                bad.append(body[:90])
        return bad

    assert offenders('asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(v));'), "the check must see the r03 form of relu_"
    assert not offenders('asm volatile("" : "+v"(p));') and not offenders('asm("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2" : "+&v"(a) : "v"(b), "v"(c));')
    for path in sorted(glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip"))):
        text = open(path).read()
        # (the reproduction switch ODPD_RELU_ASM keeps the old form behind an #ifdef that no build defines)
        text = re.sub(r"#ifdef ODPD_RELU_ASM.*?#else", "", text, flags=re.S)
        assert not offenders(text), os.path.basename(path)


def test_isa_scan_finds_the_r02_hazard_in_its_reproduction_build():
    """tools/asm_mfma_hazards.py on csrc/gru_s16n.hip compiled as the avoided r02 flavour (-DODPD_RELU_ASM): exactly
    one kernel — gru16n_kernel<DGRU, fused frozen-PA step, four K-chunks>, the one that computed wrong results — has an inline-asm
    instruction overwriting the C operand of an in-flight v_mfma; the source as built today has none."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("haz", os.path.join(ROOT, "tools", "asm_mfma_hazards.py"))
    haz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(haz)
    src = os.path.join(ROOT, "opendpd_amd", "csrc", "gru_s16n.hip")
    findings, n_asm = haz.scan(haz.isa_of(src, ("ODPD_RELU_ASM",)), 18, 3)
    war = {f[0] for f in findings if f[1] == "WAR-SrcC"}
    assert n_asm > 100 and war == {"_ZN4odpd13gru16n_kernelILi1ELb1ELi2ELi0ELb0ELb1ELi4EEEvNS_7SeqArgsE"}, war
    findings, n_asm = haz.scan(haz.isa_of(src), 18, 3)
    assert n_asm == 0 and not findings


def test_every_tuning_knob_is_documented_settable_without_a_gpu_and_every_layout_knob_moves_the_generation():
    """odpd_set_tuning's keys (csrc/capi.hip) = the keys include/opendpd_hip.h describes; each is accepted, an unknown key answers ODPD_EINVAL, and a
    key that changes a buffer size or a checkpoint layout bumps odpd_tuning_generation (callers re-size on it: train_funcs.FusedAdamW, sweep._Group;
    the autograd backward refuses to run across a change: backbones/native.py)"""
    import re
    from opendpd_amd import _lib
    src = open(os.path.join(ROOT, "opendpd_amd", "csrc", "capi.hip")).read()
    keys = re.findall(r'!strcmp\(key, "(\w+)"\)', src)
    assert len(keys) >= 8 and len(set(keys)) == len(keys)
    header = open(os.path.join(ROOT, "include", "opendpd_hip.h")).read()
    for k in keys:
        assert f'"{k}"' in header, f"tuning knob {k} is not described in include/opendpd_hip.h"
    lib = _lib.load()
    restore = {"s16_min_batch": -1, "s16_occupancy": 0, "gp_max_batch": -1}      # (knobs whose default is not 1)
    for k in keys:
        g0 = lib.odpd_tuning_generation()
        assert lib.odpd_set_tuning(k.encode(), restore.get(k, 1)) == 0, k
        sized = k not in ("xchg_fused", "lstm_pack")
        assert (lib.odpd_tuning_generation() > g0) == sized, k
    assert lib.odpd_set_tuning(b"no_such_knob", 1) == -1


def test_bench_and_package_set_the_ipc_mode_before_any_gpu_call():
    """the driver's own `torch.distributed.run ... bench.py` line must be self-sufficient — HSA_ENABLE_IPC_MODE_LEGACY=0 (dmabuf IPC:
    RCCL and the hipIpc gradient exchange need it on this image) is set by bench.py BEFORE it imports torch, and by the package at import"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    i_env, i_torch = src.index('os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")'), src.index("\nimport torch")
    assert i_env < i_torch
    assert "export HSA_ENABLE_IPC_MODE_LEGACY" not in open(os.path.join(ROOT, "tools", "scale.sh")).read()
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "HSA_ENABLE_IPC_MODE_LEGACY"}
    out = subprocess.run([sys.executable, "-c", "import os, opendpd_amd; print(os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY'))"], env=env, cwd=ROOT,
                         capture_output=True, text=True)
    assert out.stdout.strip().splitlines()[-1] == "0", out.stderr[-500:]


def test_sources_may_carry_their_own_build_flags():
    """`// odpd-build-flags:` (build.py): gru_s16x.hip asks for VGPR-form MFMAs; the flags are part of the object's cache record"""
    import json
    from opendpd_amd import build as hb
    src = os.path.join(hb.CSRC, "gru_s16x.hip")
    head = "".join(open(src).readlines()[:60])
    assert "// odpd-build-flags: -mllvm -amdgpu-mfma-vgpr-form" in head
    rec = os.path.join(ROOT, "build", "obj", "default", "gru_s16x.o.res.json")
    if os.path.exists(rec):      # (an in-tree build exists: its record carries the file's own flags)
        assert "-amdgpu-mfma-vgpr-form" in json.load(open(rec))["flags"]
