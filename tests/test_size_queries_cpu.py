"""What the size queries answer, pinned to a table recorded from the library of commit 88450c9 (the parent of the change that moved the
launchers onto the shared host helpers), without a GPU.

A size query (odpd_ckpt_floats, odpd_partial_rows, ...) must pick the kernel, the launch shape and the LDS-resident-state limit that the
launch itself picks: the caller sizes its buffers by the one and the kernel writes them by the other.  Both read the same host functions
(`*_uses_*` predicates, `*_shape`, `gp_rows`, `gp_eval_batch_fits`, `s16_min_batch_or`), so a host-side change that moves a crossover, a row
cap or a refusal shows here as another number.  tests/size_queries.json holds, for every (model, knob base, B, T) of the grid below, the
answers of QUERIES in order; `python tests/test_size_queries_cpu.py` writes it from the library `$OPENDPD_HIP_LIB` names (else the in-tree one).

Every query of the header that takes a model and a batch shape answers without a device and is on the list; none had to stay out.  (The
scratch-size queries odpd_sweep_scratch_bytes / odpd_sweep_cascade_scratch_bytes take no model and choose no kernel.)

The built-in crossovers scale with the CU count: without a device the library assumes 256, which is what the MI355X reports.  On a device
with another count the recorded answers do not apply and the module skips."""
import ctypes as C
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:      # (run as a script to write the record)
    sys.path.insert(0, os.path.dirname(HERE))
from tests.test_knob_layout_cpu import BASE, BASES, DEFAULTS, PROBES  # noqa: E402

RECORD = os.path.join(HERE, "size_queries.json")

# (name, backbone, hidden, thx, thh, bits_w, bits_a, flags): the probes of test_knob_layout_cpu.py, the 16-sequences-per-wave f4 backbones, a
# deltajanet, the widest row-rotated gru / lstm and a two-layer gru
MODELS = [(n, bb, H, thx, thh, bits, bits, "NEED_DX" if fl == "NEED_DX" else "") for n, bb, H, thx, thh, bits, fl in PROBES] + [
    ("bojanet8", "bojanet", 8, 0.0, 0.0, 0, 0, ""), ("apnrru9", "apnrru", 9, 0.0, 0.0, 0, 0, ""),
    ("dvrjanet8_k4", "dvrjanet", 8, 0.0, 0.0, 4, 0, ""),      # (bits_w carries num_dvr_units)
    ("mcldnn8", "mcldnn", 8, 0.0, 0.0, 0, 0, ""), ("deltajanet12", "deltajanet", 12, 0.01, 0.05, 0, 0, ""),
    ("gru30", "gru", 30, 0.0, 0.0, 0, 0, ""), ("lstm20", "lstm", 20, 0.0, 0.0, 0, 0, ""), ("gru11_x2", "gru", 11, 0.0, 0.0, 0, 0, "TWO_LAYERS")]
PA = ("dgru", 23)      # the frozen model behind every probe in the cascade queries
# both sides of 2 x, 4 x, 32 x and 64 x 256 CUs; the last frame length is too long for LDS-resident state (ODPD_EUNSUPPORTED on record)
BS, TS = (1, 3, 37, 513, 1027, 8200, 16400), (1, 65, 200, 4000)
# the two explicit bases of test_knob_layout_cpu.py, and the built-in defaults (crossovers from the CU count)
KNOBS = dict(BASES, default={k: DEFAULTS.get(k, 1) for k in BASE})
QUERIES = ("ckpt_floats", "partial_rows(fused=0)", "partial_rows(fused=1)", "train_workspace_floats", "frozen_loss_rows", "cascade_rows",
           "sweep_partial_rows(0)", "sweep_partial_rows(SWEEP_S16)", "sweep_workspace_floats(0)", "sweep_workspace_floats(SWEEP_S16)",
           "framed_train_supported_shape", "sweep_train_supported", "sweep_fwd_supported", "sweep_s16_supported", "sweep_cascade_supported")


def _desc(bb, H, thx=0.0, thh=0.0, bits_w=0, bits_a=0, flags=""):
    from opendpd_amd import _lib
    fl = {"": 0, "NEED_DX": _lib.FLAG_NEED_DX, "TWO_LAYERS": _lib.FLAG_TWO_LAYERS}[flags]
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, thx, thh, bits_w, bits_a, fl)


def _answers(lib, d, pa, B, T):
    from opendpd_amd import _lib
    m, p = C.byref(d), C.byref(pa)
    return [int(v) for v in (
        lib.odpd_ckpt_floats(m, B, T), lib.odpd_partial_rows(m, B, T, 0), lib.odpd_partial_rows(m, B, T, 1),
        lib.odpd_train_workspace_floats(m, B, T), lib.odpd_frozen_loss_rows(m, B, T), lib.odpd_cascade_rows(m, p, B, T),
        lib.odpd_sweep_partial_rows(m, B, T, 0), lib.odpd_sweep_partial_rows(m, B, T, _lib.SWEEP_S16),
        lib.odpd_sweep_workspace_floats(m, B, T, 0), lib.odpd_sweep_workspace_floats(m, B, T, _lib.SWEEP_S16),
        lib.odpd_framed_train_supported_shape(m, B, T), lib.odpd_sweep_train_supported(m, B, T), lib.odpd_sweep_fwd_supported(m, B, T),
        lib.odpd_sweep_s16_supported(m), lib.odpd_sweep_cascade_supported(m, p, B, T))]


def _set(lib, knobs):
    for k, v in knobs.items():
        assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k


def measure(lib):
    """{model: {base: [answers of QUERIES at (B, T) for B in BS for T in TS]}} under the live library"""
    pa, out = _desc(*PA), {}
    try:
        for base, knobs in KNOBS.items():
            _set(lib, knobs)
            for name, *model in MODELS:
                d = _desc(*model)
                out.setdefault(name, {})[base] = [_answers(lib, d, pa, B, T) for B in BS for T in TS]
    finally:
        _set(lib, KNOBS["default"])
    return out


def pack(table):
    """the table with every distinct answer row stored once (most shapes of a model share theirs)"""
    rows = sorted({tuple(r) for bases in table.values() for cells in bases.values() for r in cells})
    index = {r: i for i, r in enumerate(rows)}
    return {"queries": list(QUERIES), "batches": list(BS), "frame_lengths": list(TS), "rows": [list(r) for r in rows],
            "cells": {n: {b: [index[tuple(r)] for r in cells] for b, cells in bases.items()} for n, bases in table.items()}}


def unpack(rec):
    return {n: {b: [rec["rows"][i] for i in cells] for b, cells in bases.items()} for n, bases in rec["cells"].items()}


@pytest.fixture(scope="module")
def lib():
    import torch
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if cus != 256:
            pytest.skip(f"the record holds the answers for 256 CUs, this device has {cus}")
    from opendpd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def record():
    rec = json.load(open(RECORD))
    assert (tuple(rec["queries"]), tuple(rec["batches"]), tuple(rec["frame_lengths"])) == (QUERIES, BS, TS)
    return unpack(rec)


@pytest.fixture(scope="module")
def live(lib):
    return measure(lib)


def test_the_record_covers_the_grid(record):
    assert set(record) == {m[0] for m in MODELS}
    for name, bases in record.items():
        assert set(bases) == set(KNOBS), name
        assert all(len(cells) == len(BS) * len(TS) and all(len(r) == len(QUERIES) for r in cells) for cells in bases.values()), name
    assert os.path.getsize(RECORD) < 64 * 1024


def test_every_model_is_served_somewhere_under_every_base(record):
    """not vacuous: a non-negative checkpoint size and positive backward rows at one (B, T) at least, for every model under every base;
    and the refusals of the long frame are on record"""
    for name, bases in record.items():
        for base, cells in bases.items():
            assert any(r[0] >= 0 and r[1] > 0 for r in cells), (name, base)
    assert any(r[2] < 0 for bases in record.values() for cells in bases.values() for r in cells[len(TS) - 1::len(TS)])


@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_the_size_queries_answer_what_the_record_holds(live, record, name):
    for base in KNOBS:
        for i, (got, want) in enumerate(zip(live[name][base], record[name][base])):
            diff = {q: (g, w) for q, g, w in zip(QUERIES, got, want) if g != w}
            assert not diff, (name, base, "B", BS[i // len(TS)], "T", TS[i % len(TS)], "query: (answer, recorded)", diff)


if __name__ == "__main__":
    from opendpd_amd import _lib
    with open(RECORD, "w") as f:
        json.dump(pack(measure(_lib.load())), f, separators=(",", ":"))
        f.write("\n")
    print(f"{RECORD}: {os.path.getsize(RECORD)} bytes from {_lib.lib_path()}")
