"""Where the five recurrent families change kernels on the batch axis, pinned to a table recorded from the library of commit aec595a (the
parent of the change that resolves each family's split-path kernel once), without a GPU.

tests/test_size_queries_cpu.py samples seven batch sizes; the crossovers of the split path (`*_uses_*` predicates of gru_family.hip,
lstm_family.hip, delta_family.hip, janet_family.hip and the quantised kernels) sit between them.  Here the batch sizes are found, not
guessed: `python tests/test_split_plan_cpu.py` scans B = 1 .. 20 000 at every frame length of TS with the library `$OPENDPD_HIP_LIB` names
(else the in-tree one) and keeps, per model, every B at which one of QUERIES leaves its staircase, and B - 1.  An answer such as
ceil(B / 4) x 64 grows by the same step at the same distance for as long as one kernel and one launch shape serve the batch; a step of
another size, a step at another distance, a step that fails to come (a grid cap) or a refusal is a change point.  tests/split_plan.json
holds the answers of QUERIES at those batch sizes for every (model, hidden size, knob base, T).

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
from tests.test_knob_layout_cpu import BASE, BASES, DEFAULTS  # noqa: E402

RECORD = os.path.join(HERE, "split_plan.json")

# (name, backbone, thx, thh, bits, flags): every backbone of the five families, float and W8A8 where a quantised model exists (deltagru has
# none), the delta backbones with and without ODPD_FLAG_NEED_DX
_PLAIN = [(bb, bb, 0.0, 0.0) for bb in ("gru", "dgru", "qgru", "qgru_amp1", "lstm", "vdlstm", "pgjanet")]
_DELTA = [(bb, bb, 0.01, 0.05) for bb in ("deltagru", "deltagru_tcnskip", "deltajanet")]
MODELS = ([(n, bb, thx, thh, bits, "") for n, bb, thx, thh in _PLAIN for bits in (0, 8)] +
          [(n, bb, thx, thh, bits, fl) for n, bb, thx, thh in _DELTA for bits in ((0,) if bb == "deltagru" else (0, 8)) for fl in ("", "NEED_DX")])
MODELS = [(f"{n}{'_w8a8' if bits else ''}{'_dx' if fl else ''}", bb, thx, thh, bits, fl) for n, bb, thx, thh, bits, fl in MODELS]
HIDDEN = (1, 8, 16, 17, 24, 25, 32)
SCAN_B, TS = 20000, (20, 200, 1000)
KNOBS = dict(BASES, default={k: DEFAULTS.get(k, 1) for k in BASE})
QUERIES = ("ckpt_floats", "partial_rows(fused=0)", "partial_rows(fused=1)", "train_workspace_floats", "frozen_loss_rows")
CUS = 256
BUILT_IN = (2 * CUS, 32 * CUS, 48 * CUS, 64 * CUS)      # the multiples of the CU count that the predicates build in


def _desc(bb, H, thx, thh, bits, flags):
    from opendpd_amd import _lib
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, thx, thh, bits, bits, _lib.FLAG_NEED_DX if flags == "NEED_DX" else 0)


def _answers(lib, m, B, T):
    return (int(lib.odpd_ckpt_floats(m, B, T)), int(lib.odpd_partial_rows(m, B, T, 0)), int(lib.odpd_partial_rows(m, B, T, 1)),
            int(lib.odpd_train_workspace_floats(m, B, T)), int(lib.odpd_frozen_loss_rows(m, B, T)))


def _set(lib, knobs):
    for k, v in knobs.items():
        assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k


def change_points(rows):
    """rows[i] = the answers at B = i + 1: the batch sizes at which an answer leaves its staircase (see the module's docstring)"""
    marks = {1}
    for q in range(len(rows[0])):
        last, size, gap, fresh = 1, None, None, True      # the last step: its batch size, height, distance from the one before; it was a change
        for B in range(2, len(rows) + 1):
            d = rows[B - 1][q] - rows[B - 2][q]
            if d:
                change = not fresh and (d, B - last) != (size, gap)      # (the step that follows a change sets the new staircase's measure)
                if change:
                    marks.add(B)
                last, size, gap, fresh = B, d, B - last, change
            elif gap is not None and B == last + gap:      # the step that was due did not come
                marks.add(B)
                gap = None
    return marks


def scan(model):
    """the change points of one model over every hidden size, knob base and frame length (run in a process of its own: the knobs are global)"""
    from opendpd_amd import _lib
    lib, out = _lib.load(), {}
    name, *rest = model
    for H in HIDDEN:
        m, marks = C.byref(_desc(rest[0], H, *rest[1:])), set()
        for knobs in KNOBS.values():
            _set(lib, knobs)
            for T in TS:
                marks |= change_points([_answers(lib, m, B, T) for B in range(1, SCAN_B + 1)])
        out[H] = sorted(marks | {b - 1 for b in marks if b > 1})
    _set(lib, KNOBS["default"])
    return name, out


def measure(lib, batches):
    """{model: {hidden: {base: [answers of QUERIES at (B, T) for B in batches[model][hidden] for T in TS]}}} under the live library"""
    out = {}
    try:
        for base, knobs in KNOBS.items():
            _set(lib, knobs)
            for name, *rest in MODELS:
                for H in HIDDEN:
                    m = C.byref(_desc(rest[0], H, *rest[1:]))
                    out.setdefault(name, {}).setdefault(H, {})[base] = [list(_answers(lib, m, B, T)) for B in batches[name][H] for T in TS]
    finally:
        _set(lib, KNOBS["default"])
    return out


def pack(batches, table):
    """everything distinct stored once and referred to by index: the answers ("values"), the answer rows, the lists of batch sizes, the lists
    of cells (one per knob base), and the columns [batch list, cells under each base] that the models' hidden sizes point at — the hidden
    sizes of one kernel set, and the backbones of one family, mostly share theirs"""
    rows = sorted({tuple(r) for hs in table.values() for bases in hs.values() for cells in bases.values() for r in cells})
    values = sorted({v for r in rows for v in r})
    vi, index = {v: i for i, v in enumerate(values)}, {r: i for i, r in enumerate(rows)}
    blists, clists, cols, models = {}, {}, {}, {}
    for name, hs in table.items():
        for H, bases in hs.items():
            col = (blists.setdefault(tuple(batches[name][H]), len(blists)),
                   *(clists.setdefault(tuple(index[tuple(r)] for r in bases[b]), len(clists)) for b in KNOBS))
            models.setdefault(name, []).append(cols.setdefault(col, len(cols)))
    return {"queries": list(QUERIES), "hidden": list(HIDDEN), "frame_lengths": list(TS), "bases": list(KNOBS), "values": values,
            "rows": [[vi[v] for v in r] for r in rows], "batches": [list(b) for b in blists], "cells": [list(c) for c in clists],
            "columns": [list(c) for c in cols], "models": models}


def unpack(rec):
    batches, table = {}, {}
    rows = [[rec["values"][i] for i in r] for r in rec["rows"]]
    for name, ids in rec["models"].items():
        for H, i in zip(rec["hidden"], ids):
            col = rec["columns"][i]
            batches.setdefault(name, {})[H] = rec["batches"][col[0]]
            table.setdefault(name, {})[H] = {b: [rows[j] for j in rec["cells"][c]] for b, c in zip(rec["bases"], col[1:])}
    return batches, table


@pytest.fixture(scope="module")
def lib():
    import torch
    if torch.cuda.is_available():
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if cus != CUS:
            pytest.skip(f"the record holds the answers for {CUS} CUs, this device has {cus}")
    from opendpd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def record():
    rec = json.load(open(RECORD))
    assert (tuple(rec["queries"]), tuple(rec["hidden"]), tuple(rec["frame_lengths"]), tuple(rec["bases"])) == (QUERIES, HIDDEN, TS, tuple(KNOBS))
    return unpack(rec)


@pytest.fixture(scope="module")
def live(lib, record):
    return measure(lib, record[0])


def test_the_record_covers_the_grid(record):
    batches, table = record
    assert set(table) == {m[0] for m in MODELS}
    for name, hs in table.items():
        assert set(hs) == set(HIDDEN), name
        for H, bases in hs.items():
            assert set(bases) == set(KNOBS), (name, H)
            assert all(len(cells) == len(batches[name][H]) * len(TS) and all(len(r) == len(QUERIES) for r in cells) for cells in bases.values())
    assert os.path.getsize(RECORD) < 64 * 1024


def test_every_model_is_served_somewhere_under_every_base(record):
    """not vacuous: a non-negative checkpoint size and positive backward rows at one (hidden, B, T) at least, for every model under every base"""
    for name, hs in record[1].items():
        for base in KNOBS:
            assert any(r[0] >= 0 and r[1] > 0 for bases in hs.values() for r in bases[base]), (name, base)


@pytest.mark.parametrize("multiple", BUILT_IN)
def test_a_change_point_lies_next_to_every_built_in_crossover(record, multiple):
    """B <= 2 x CUs (one sequence per wave), B >= 32 x / 48 x / 64 x CUs (the 16-sequences-per-wave kernels of hidden 17 .. 32, of the quantised
    models, of hidden <= 16): the scan found each of them, at the multiple itself or one past it"""
    found = {b for hs in record[0].values() for bs in hs.values() for b in bs}
    assert {multiple, multiple + 1} <= found, sorted(b for b in found if abs(b - multiple) < 20)


@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_the_queries_answer_what_the_record_holds(live, record, name):
    batches, table = record
    for H in HIDDEN:
        for base in KNOBS:
            for i, (got, want) in enumerate(zip(live[name][H][base], table[name][H][base])):
                diff = {q: (g, w) for q, g, w in zip(QUERIES, got, want) if g != w}
                assert not diff, (name, H, base, "B", batches[name][H][i // len(TS)], "T", TS[i % len(TS)], "query: (answer, recorded)", diff)


if __name__ == "__main__":
    from multiprocessing import Pool

    from opendpd_amd import _lib
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        found = dict(pool.map(scan, MODELS, chunksize=1))
    with open(RECORD, "w") as f:
        json.dump(pack(found, measure(_lib.load(), found)), f, separators=(",", ":"))
        f.write("\n")
    print(f"{RECORD}: {os.path.getsize(RECORD)} bytes from {_lib.lib_path()}")
