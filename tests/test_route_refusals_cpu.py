"""What the launch entry points refuse, and with which code, before they touch the device — pinned to a table recorded from the library of
commit 42db9ef (the parent of the change that resolves each descriptor's kernel route once for the whole C ABI).

odpd_backbone_fwd / _bwd, odpd_backbone_fwd_state / _bwd_state, odpd_train_fwd_bwd, odpd_train_fwd_bwd_framed and odpd_frozen_loss_dx choose
their kernel from the descriptor and the batch shape; a shape none serves is answered ODPD_EINVAL (-1) or ODPD_EUNSUPPORTED (-2) in front of
the first HIP call.  The grid: every descriptor of tests/test_size_queries_cpu.py and tests/test_route_queries_cpu.py, the two explicit knob
bases of tests/test_knob_layout_cpu.py (a -1 knob asks the device for its CU count), B in (3, 1027), T in (20, 4000), nine calls each.
tests/route_refusals.json holds, per (descriptor, call), one character per (base, B, T): "1" / "2" where the parent's library answered
-1 / -2, "." where it went on to launch.  Only the refusals are tested: `left_out` of the record counts the other cells — that a served
shape stays served is held by the size records and the GPU suites.  `python tests/test_route_refusals_cpu.py` writes the record from the
library `$OPENDPD_HIP_LIB` names (else the in-tree one).

The pointers are dummies nobody may read, so a refusal turned into a launch must meet "no device", not memory: the module skips where a
HIP device is present.  Without one a wrongly served cell answers a HIP error and fails the comparison."""
import ctypes as C
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:      # (run as a script to write the record)
    sys.path.insert(0, os.path.dirname(HERE))
from tests import test_route_queries_cpu as rq  # noqa: E402
from tests import test_size_queries_cpu as sq  # noqa: E402
from tests.test_knob_layout_cpu import BASE, BASES, DEFAULTS  # noqa: E402

RECORD = os.path.join(HERE, "route_refusals.json")
PTR = 0x1000      # a non-null pointer nobody reads
BS, TS = (3, 1027), (20, 4000)
CALLS = ("fwd", "bwd(partials)", "bwd(dx)", "fwd_state", "bwd_state", "train", "framed(workspace=NULL)", "framed(workspace)", "frozen_loss_dx")
FUSED = CALLS[5:]
CODES = {-1: "1", -2: "2"}
# one descriptor of the two records per forward / backward-only kernel set
ROUTES = {"gru_wide": "gru40", "lstm_wide": "lstm40", "vdlstm_wide": "vdlstm40", "delta_wide": "deltagru40", "deltajanet_wide": "deltajanet40",
          "pgjanet_wide": "pgjanet20", "pgjanet_q": "pgjanet11_w8a8", "bojanet_q": "bojanet8_qc", "dvrjanet_q": "dvrjanet8_k4_qc",
          "gru2": "gru11_x2", "lstm2": "lstm11_x2", "gru_state": "gru11_h0", "lstm_state": "lstm9_h0"}


def models():
    """{name: descriptor} of both records"""
    out = {name: sq._desc(*model) for name, *model in sq.MODELS}
    out.update({name: rq.desc(*model) for name, *model, _ in rq.MODELS})
    return out


def call(lib, what, d, B, T):
    from opendpd_amd import _lib
    m, count = C.byref(d), B * T * 2
    if what == "fwd":
        return lib.odpd_backbone_fwd(None, m, B, T, PTR, PTR, PTR, PTR, None)
    if what.startswith("bwd("):
        return lib.odpd_backbone_bwd(None, m, B, T, PTR, PTR, PTR, PTR, *((PTR, None) if what == "bwd(partials)" else (None, PTR)))
    if what == "fwd_state":
        return lib.odpd_backbone_fwd_state(None, m, B, T, PTR, PTR, PTR, PTR, PTR)
    if what == "bwd_state":
        return lib.odpd_backbone_bwd_state(None, m, B, T, PTR, PTR, PTR, PTR, PTR, PTR, None, None)
    if what == "train":
        return lib.odpd_train_fwd_bwd(None, m, 0, B, T, count, PTR, PTR, PTR, PTR, PTR)
    if what.startswith("framed("):
        fr = _lib.Frames(PTR, PTR, PTR, B, T, 1, _lib.SAMPLES_F32, 0)
        return lib.odpd_train_fwd_bwd_framed(None, m, 0, C.byref(fr), 0, B, count, PTR, PTR, None if "NULL" in what else PTR)
    assert what == "frozen_loss_dx"
    return lib.odpd_frozen_loss_dx(None, m, 0, B, T, count, PTR, PTR, PTR, PTR, PTR, PTR)


def _knobs(lib, values):
    for k, v in values.items():
        assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k


def cells():
    return [(base, B, T) for base in BASES for B in BS for T in TS]


def measure(lib, only=None):
    """{model: {call: one character per cell}}; only: the record — its "." cells are not called"""
    out = {name: {c: "" for c in CALLS} for name in models()}
    try:
        for i, (base, B, T) in enumerate(cells()):
            if i % (len(BS) * len(TS)) == 0:
                _knobs(lib, BASES[base])
            for name, d in models().items():
                for c in CALLS:
                    skip = only is not None and only[name][c][i] == "."
                    out[name][c] += "." if skip else CODES.get(call(lib, c, d, B, T), ".")
    finally:
        _knobs(lib, {k: DEFAULTS.get(k, 1) for k in BASE})
    return out


@pytest.fixture(scope="module")
def record():
    rec = json.load(open(RECORD))
    assert (tuple(rec["calls"]), tuple(rec["bases"]), tuple(rec["batches"]), tuple(rec["frame_lengths"])) == (CALLS, tuple(BASES), BS, TS)
    return rec


def test_the_record_covers_the_grid_and_says_what_it_leaves_out(record):
    table = record["cells"]
    assert set(table) == set(models())
    assert all(set(row) == set(CALLS) and all(len(s) == len(cells()) and set(s) <= set("12.") for s in row.values()) for row in table.values())
    assert record["left_out"] == sum(s.count(".") for row in table.values() for s in row.values()) > 0
    assert os.path.getsize(RECORD) < 64 * 1024


def test_every_call_every_refused_descriptor_and_every_route_is_on_record(record):
    table = record["cells"]
    for c in CALLS:
        assert any(set(row[c]) & set("12") for row in table.values()), c
    for name, *_, label in rq.MODELS:
        if label == "refused":
            assert all(set(s) <= set("12") for s in table[name].values()), name      # refused by every call at every shape
    for route, name in ROUTES.items():      # forward / backward only: no fused entry point serves them
        for c in FUSED:
            assert set(table[name][c]) <= set("12"), (route, c)


def test_refusals_come_with_the_recorded_code_before_any_device_call(record):
    import torch
    if torch.cuda.is_available():
        pytest.skip("dummy pointers: a refusal turned into a launch must meet 'no device', not memory")
    from opendpd_amd import _lib
    got, want = measure(_lib.load(), only=record["cells"]), record["cells"]
    diff = {(name, c): (got[name][c], want[name][c]) for name in want for c in CALLS if got[name][c] != want[name][c]}
    assert not diff, ("(model, call): (answers, recorded) per (base, B, T) of", cells(), diff)


if __name__ == "__main__":
    from opendpd_amd import _lib
    table = measure(_lib.load())
    rec = {"calls": list(CALLS), "bases": list(BASES), "batches": list(BS), "frame_lengths": list(TS),
           "left_out": sum(s.count(".") for row in table.values() for s in row.values()), "cells": table}
    with open(RECORD, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    n = sum(len(s) for row in table.values() for s in row.values())
    print(f"{RECORD}: {os.path.getsize(RECORD)} bytes, {n - rec['left_out']} refusals of {n} cells, from {_lib.lib_path()}")
