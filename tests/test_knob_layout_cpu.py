"""What each kernel-selection knob (odpd_set_tuning) does to the buffers an autograd forward sizes and its backward reads, without a GPU.

The size queries (odpd_ckpt_floats, odpd_partial_rows, odpd_train_workspace_floats) pick their kernel from the live knobs, exactly as the
launches do.  A checkpoint written under one knob value and read under another is read in the wrong layout — past its end where the sizes
differ, as wrong gradients where they agree (the `qat_u3` slot count, the `s16x_train` two-step records).  The autograd bridge
(backbones/native.py: _BackboneFn) refuses a backward whose forward ran under another odpd_tuning_generation; these tests hold the library to
its half of that contract: every knob that changes a size moves the generation, and the two knobs outside it change none.

Every knob is flipped between two explicit values (no -1 "built-in crossover": that one asks the device for its CU count)."""
import ctypes as C
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# two explicit values per knob, and the values every other knob holds while one is flipped: once with the 16-sequences-per-wave kernels
# serving every batch, once with them serving none (the one-sequence-per-wave fused kernels are only chosen then)
FLIPS = {"s16_min_batch": (0, 1 << 30), "s16_occupancy": (1, 2), "gp_max_batch": (0, 1 << 30), "cascade_one_launch": (1, 0),
         "xchg_fused": (1, 0), "s16x": (1, 0), "s16x_train": (1, 0), "lstm_pack": (1, 0), "qat_u3": (1, 0)}
BASE = {"s16_min_batch": 0, "s16_occupancy": 1, "gp_max_batch": 0, "cascade_one_launch": 1, "xchg_fused": 1, "s16x": 1, "s16x_train": 1,
        "lstm_pack": 1, "qat_u3": 1}
BASES = {"s16": BASE, "rot": dict(BASE, s16_min_batch=1 << 30, gp_max_batch=1 << 30)}
DEFAULTS = {"s16_min_batch": -1, "s16_occupancy": 0, "gp_max_batch": -1}     # (knobs whose built-in value is not 1)
UNSIZED = ("xchg_fused", "lstm_pack")      # change no buffer size and no checkpoint layout: outside the generation

# (name, backbone, hidden, thx, thh, bits, flags)
PROBES = [("gru11", "gru", 11, 0.0, 0.0, 0, 0), ("dgru13", "dgru", 13, 0.0, 0.0, 0, 0), ("dgru23", "dgru", 23, 0.0, 0.0, 0, 0),
          ("lstm9", "lstm", 9, 0.0, 0.0, 0, 0), ("vdlstm13", "vdlstm", 13, 0.0, 0.0, 0, 0),
          ("deltagru15", "deltagru", 15, 0.01, 0.05, 0, 0), ("deltagru15_dx", "deltagru", 15, 0.01, 0.05, 0, "NEED_DX"),
          ("pgjanet11", "pgjanet", 11, 0.0, 0.0, 0, 0), ("qgru10_w8a8", "qgru", 10, 0.0, 0.0, 8, 0), ("dgru8_w8a8", "dgru", 8, 0.0, 0.0, 8, 0)]
BS, TS = (3, 37, 1027), (1, 65, 200)


def _desc(bb, H, thx, thh, bits, flags):
    from opendpd_amd import _lib
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, thx, thh, bits, bits, _lib.FLAG_NEED_DX if flags == "NEED_DX" else 0)


def _sizes(lib, d, B, T):
    """the four buffer sizes of one (model, B, T) under the live knobs (a negative answer = not served, recorded as such)"""
    return (int(lib.odpd_ckpt_floats(C.byref(d), B, T)), int(lib.odpd_partial_rows(C.byref(d), B, T, 0)),
            int(lib.odpd_partial_rows(C.byref(d), B, T, 1)), int(lib.odpd_train_workspace_floats(C.byref(d), B, T)))


def _set(lib, key, value):
    assert lib.odpd_set_tuning(key.encode(), C.c_int64(value)) == 0, key


@pytest.fixture(scope="module")
def lib():
    from opendpd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def table(lib):
    """{(probe, knob, B, T, base): (sizes at the first value, sizes at the second, generation moved by each of the two sets)}"""
    out = {}
    try:
        for (base, values), (knob, (v0, v1)) in itertools.product(BASES.items(), FLIPS.items()):
            for k, v in values.items():
                _set(lib, k, v)
            for name, bb, H, thx, thh, bits, flags in PROBES:
                d = _desc(bb, H, thx, thh, bits, flags)
                for B in BS:
                    for T in TS:
                        _set(lib, knob, v0)
                        g0 = lib.odpd_tuning_generation()
                        s0 = _sizes(lib, d, B, T)
                        _set(lib, knob, v1)
                        g1 = lib.odpd_tuning_generation()
                        s1 = _sizes(lib, d, B, T)
                        _set(lib, knob, v0)
                        out[(name, knob, B, T, base)] = (s0, s1, (g1 > g0, lib.odpd_tuning_generation() > g1))
    finally:
        for k in BASE:
            _set(lib, k, DEFAULTS.get(k, 1))
    return out


def test_the_flip_table_covers_every_knob_of_the_library():
    src = open(os.path.join(ROOT, "opendpd_amd", "csrc", "capi.hip")).read()
    assert set(re.findall(r'!strcmp\(key, "(\w+)"\)', src)) == set(FLIPS) == set(BASE)


def test_every_probe_is_served(table):
    """the probe grid is real: the split-path checkpoint and backward rows exist for every model and shape (a probe the library refuses
    would make every comparison below vacuous)"""
    for key, (s0, s1, _) in table.items():
        for s in (s0, s1):
            assert s[0] >= 0 and s[1] > 0, (key, s)


@pytest.mark.parametrize("knob", sorted(FLIPS))
def test_a_knob_that_changes_a_buffer_size_moves_the_generation(table, knob):
    rows = {k: v for k, v in table.items() if k[1] == knob}
    changed = [k for k, (s0, s1, _) in rows.items() if s0 != s1]
    bumps = {g for (_, _, g) in rows.values()}
    if changed:
        assert bumps == {(True, True)}, (knob, changed[:4])
    if knob in UNSIZED:
        assert not changed, (knob, changed[:4])
        assert bumps == {(False, False)}, knob
    else:
        assert bumps == {(True, True)}, knob       # (the layout knobs move it too: same sizes, other records)


def test_the_size_changing_knobs_do_change_sizes_on_the_probe_grid(table):
    """every generation-bumping knob but the two same-size layout knobs (and cascade_one_launch, which only answers odpd_cascade_rows) changes
    at least one size somewhere on the grid: the CPU-side record that a forward/backward flip of it reads a buffer of another size"""
    for knob in ("s16_min_batch", "s16_occupancy", "gp_max_batch", "s16x"):
        assert any(s0 != s1 for key, (s0, s1, _) in table.items() if key[1] == knob), knob


def test_s16_min_batch_at_gru11_batch3_quadruples_the_checkpoint(table):
    """row-rotated kernel: ceil(B/4) four-sequence groups x 64 lanes per checkpoint; S16 kernels: ceil(B/16) sixteen-sequence tasks x 256 —
    an S16 backward behind a row-rotated forward would read 4x the floats the forward allocated"""
    for T in TS:
        s_s16, s_rot, _ = table[("gru11", "s16_min_batch", 3, T, "s16")]
        assert s_rot[0] > 0 and s_s16[0] == 4 * s_rot[0], (T, s_s16, s_rot)


def test_qat_u3_at_qgru10_keeps_the_checkpoint_size(table):
    """three or four unit slots per lane: the same checkpoint floats (the slot count moves units inside each record), so a flip between
    forward and backward would read a buffer of the right size in the wrong layout — nothing but the generation can tell"""
    for B in BS:
        for T in TS:
            s3, s4, moved = table[("qgru10_w8a8", "qat_u3", B, T, "s16")]
            assert s3[0] == s4[0] > 0 and moved == (True, True), (B, T, s3, s4)


def test_s16x_train_keeps_every_size_of_a_17_to_24_unit_model(table):
    """s16x_train: the workspace answers the larger of the two layouts, so the flip changes no size at DGRU 23 — a same-size layout knob"""
    for B in BS:
        for T in TS:
            s0, s1, moved = table[("dgru23", "s16x_train", B, T, "s16")]
            assert s0 == s1 and moved == (True, True), (B, T, s0, s1)
