"""What the size queries answer for the descriptors tests/size_queries.json leaves out, pinned to a table recorded from the library of
commit 42db9ef (the parent of the change that resolves each descriptor's kernel route once for the whole C ABI), without a GPU.

tests/test_size_queries_cpu.py holds the row-rotated and 16-sequences-per-wave kernels to their answers; none of its descriptors takes a
forward / backward-only route.  This record holds exactly those: the lane-per-unit kernels of 33 .. 64 hidden units (pgjanet: 17 .. 32), the
in-cell quantised pgjanet / bojanet / dvrjanet, the two-layer models, the state route (ODPD_FLAG_INIT_STATE) — each with descriptors that ask
for such a route and are refused —, the non-recurrent backbones, a model with quantised heads and a hidden size no kernel takes.  On top of
the fifteen queries of that module it asks odpd_param_count and odpd_framed_train_supported.  tests/route_queries.json holds the answers over
the same (knob base, B, T) grid; `python tests/test_route_queries_cpu.py` writes it from the library `$OPENDPD_HIP_LIB` names (else the
in-tree one).

Without a device the library assumes 256 CUs; on a device with another count the module skips (as tests/test_size_queries_cpu.py)."""
import ctypes as C
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:      # (run as a script to write the record)
    sys.path.insert(0, os.path.dirname(HERE))
from tests.test_size_queries_cpu import BS, KNOBS, PA, TS, _answers, _set, pack, unpack  # noqa: E402
from tests.test_size_queries_cpu import QUERIES as SIZE_QUERIES  # noqa: E402

RECORD = os.path.join(HERE, "route_queries.json")
QUERIES = SIZE_QUERIES + ("param_count", "framed_train_supported")
W8A8 = (8, 8)
# (name, backbone, hidden, thx, thh, (bits_w, bits_a), flags, label).  label: "served" — some kernel takes the model at some batch shape under
# every knob base; "refused" — the descriptor asks for a forward / backward-only route that does not serve it: every query that can answer a
# code answers a negative one, everywhere; "no kernel" — asks for no such route, and no kernel takes the hidden size
MODELS = [
    # lane per unit, float
    ("gru40", "gru", 40, 0.0, 0.0, (0, 0), (), "served"), ("dgru64", "dgru", 64, 0.0, 0.0, (0, 0), (), "served"),
    ("qgru_amp1_33", "qgru_amp1", 33, 0.0, 0.0, (0, 0), (), "served"), ("lstm40", "lstm", 40, 0.0, 0.0, (0, 0), (), "served"),
    ("vdlstm40", "vdlstm", 40, 0.0, 0.0, (0, 0), (), "served"), ("deltagru40", "deltagru", 40, 0.01, 0.05, (0, 0), (), "served"),
    ("deltagru_tcnskip40", "deltagru_tcnskip", 40, 0.01, 0.05, (0, 0), (), "served"),
    ("deltajanet40", "deltajanet", 40, 0.01, 0.05, (0, 0), (), "served"),
    # pgjanet: lane per unit, in-cell quantised, and quantised at a hidden size only the float kernels take
    ("pgjanet20", "pgjanet", 20, 0.0, 0.0, (0, 0), (), "served"), ("pgjanet11_w8a8", "pgjanet", 11, 0.0, 0.0, W8A8, (), "served"),
    ("pgjanet40_w8a8", "pgjanet", 40, 0.0, 0.0, W8A8, (), "refused"),
    # ODPD_FLAG_QUANT_CELL (dvrjanet: num_dvr_units in thx)
    ("bojanet8_qc", "bojanet", 8, 0.0, 0.0, W8A8, ("QUANT_CELL",), "served"), ("dvrjanet8_k4_qc", "dvrjanet", 8, 4.0, 0.0, W8A8, ("QUANT_CELL",), "served"),
    ("gru11_qc", "gru", 11, 0.0, 0.0, (0, 0), ("QUANT_CELL",), "refused"), ("bojanet20_qc", "bojanet", 20, 0.0, 0.0, W8A8, ("QUANT_CELL",), "refused"),
    # ODPD_FLAG_TWO_LAYERS
    ("lstm11_x2", "lstm", 11, 0.0, 0.0, (0, 0), ("TWO_LAYERS",), "served"), ("gru40_x2", "gru", 40, 0.0, 0.0, (0, 0), ("TWO_LAYERS",), "refused"),
    # ODPD_FLAG_INIT_STATE
    ("gru11_h0", "gru", 11, 0.0, 0.0, (0, 0), ("INIT_STATE",), "served"), ("gru40_h0", "gru", 40, 0.0, 0.0, (0, 0), ("INIT_STATE",), "served"),
    ("lstm9_h0", "lstm", 9, 0.0, 0.0, (0, 0), ("INIT_STATE",), "served"), ("pgjanet11_h0", "pgjanet", 11, 0.0, 0.0, (0, 0), ("INIT_STATE",), "refused"),
    ("gru11_x2_h0", "gru", 11, 0.0, 0.0, (0, 0), ("INIT_STATE", "TWO_LAYERS"), "refused"),
    # not recurrent
    ("tcnn16", "tcnn", 16, 0.0, 0.0, (0, 0), (), "served"), ("neuraltx12", "neuraltx", 12, 0.0, 0.0, (0, 0), (), "served"),
    ("gmp11", "gmp", 11, 0.0, 0.0, (0, 0), (), "served"), ("rvtdcnn25", "rvtdcnn", 25, 0.0, 0.0, (0, 0), (), "served"),
    ("rvtdcnn25_w8a8", "rvtdcnn", 25, 0.0, 0.0, W8A8, (), "served"),
    # quantised heads on a float core; a hidden size past every kernel
    ("lstm9_w8a8", "lstm", 9, 0.0, 0.0, W8A8, (), "served"), ("gru70", "gru", 70, 0.0, 0.0, (0, 0), (), "no kernel")]
# the queries that answer a size or a code (the others answer 0 / 1), and of those the ones of the routes' own entry points: a refused
# descriptor gets a negative answer from each (the sweep and cascade queries test the family first and may answer 0 floats)
CODED = ("ckpt_floats", "partial_rows(fused=0)", "partial_rows(fused=1)", "train_workspace_floats", "frozen_loss_rows", "param_count")
YES_NO = ("framed_train_supported_shape", "framed_train_supported")


def desc(bb, H, thx=0.0, thh=0.0, bits=(0, 0), flags=()):
    from opendpd_amd import _lib
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, thx, thh, bits[0], bits[1], sum(getattr(_lib, "FLAG_" + f) for f in flags))


def answers(lib, d, pa, B, T):
    m = C.byref(d)
    return _answers(lib, d, pa, B, T) + [int(lib.odpd_param_count(m)), int(lib.odpd_framed_train_supported(m))]


def measure(lib):
    """{model: {base: [answers of QUERIES at (B, T) for B in BS for T in TS]}} under the live library"""
    pa, out = desc(*PA), {}
    try:
        for base, knobs in KNOBS.items():
            _set(lib, knobs)
            for name, *model, _ in MODELS:
                d = desc(*model)
                out.setdefault(name, {})[base] = [answers(lib, d, pa, B, T) for B in BS for T in TS]
    finally:
        _set(lib, KNOBS["default"])
    return out


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


def test_served_models_are_served_and_refused_ones_refused_under_every_base(record):
    """not vacuous: a non-negative checkpoint size and positive backward rows at one (B, T) at least, for every served model under every
    base; and every refused descriptor answers a code wherever a code can be answered, 0 where the answer is yes or no"""
    col = {q: i for i, q in enumerate(QUERIES)}
    for name, *_, label in MODELS:
        for base, cells in record[name].items():
            if label == "served":
                assert any(r[0] >= 0 and r[1] > 0 for r in cells), (name, base)
            elif label == "refused":
                assert all(r[col[q]] < 0 for r in cells for q in CODED) and all(r[col[q]] == 0 for r in cells for q in YES_NO), (name, base)
            else:
                assert all(r[0] < 0 and r[1] < 0 for r in cells) and all(r[col["param_count"]] > 0 for r in cells), (name, base)


@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_the_queries_answer_what_the_record_holds(live, record, name):
    for base in KNOBS:
        for i, (got, want) in enumerate(zip(live[name][base], record[name][base])):
            diff = {q: (g, w) for q, g, w in zip(QUERIES, got, want) if g != w}
            assert not diff, (name, base, "B", BS[i // len(TS)], "T", TS[i % len(TS)], "query: (answer, recorded)", diff)


if __name__ == "__main__":
    from opendpd_amd import _lib
    with open(RECORD, "w") as f:
        json.dump(dict(pack(measure(_lib.load())), queries=list(QUERIES)), f, separators=(",", ":"))
        f.write("\n")
    print(f"{RECORD}: {os.path.getsize(RECORD)} bytes from {_lib.lib_path()}")
