"""What the native epoch entry points refuse, and with which code, before they touch the device.

odpd_train_epoch, _opt, _dp, _cascade, _split, _sweep, _cascade_sweep and odpd_backbone_fwd_sweep validate their arguments (ODPD_EINVAL = -1)
and the shapes they serve (ODPD_EUNSUPPORTED = -2) in front of their first HIP call, the argument errors first.  Every call of the table
below is one of those: the pointers are dummies that are never dereferenced, and the selection knobs hold explicit values (a -1 knob asks
the device for its CU count).  The expected codes are what the library answered when the table was written; the loops have since been
moved onto one shared driver, and this table is what holds the driver to the same answers."""
import ctypes as C

import pytest

EINVAL, EUNSUPPORTED = -1, -2
KNOBS = {"s16_min_batch": 1 << 30, "s16_occupancy": 1, "gp_max_batch": 1 << 30, "cascade_one_launch": 1}
DEFAULTS = {"s16_min_batch": -1, "s16_occupancy": 0, "gp_max_batch": -1, "cascade_one_launch": 1}
PTR = 0x1000      # a non-null pointer nobody reads
T, BATCH, N_FRAMES, K = 20, 4, 7, 2


def _desc(bb="dgru", H=13, flags=0):
    from opendpd_amd import _lib
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, 0.0, 0.0, 0, 0, flags)


def _frames(order=PTR, fmt=None):
    from opendpd_amd import _lib
    return _lib.Frames(PTR, PTR, order, N_FRAMES, T, 1, _lib.SAMPLES_F32 if fmt is None else fmt, 0)


def _runs(**over):
    """K complete run records; `over` replaces one field of the LAST one (every run is looked at)"""
    from opendpd_amd import _lib
    table = (_lib.SweepRun * K)()
    for k in range(K):
        table[k] = _lib.SweepRun(PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 5e-4)
    for key, val in over.items():
        setattr(table[K - 1], key, val)
    return table


ADAMW = (5e-4, 0.9, 0.999, 1e-8, 0.01, 0.0)      # lr, betas, eps, weight decay, clip norm


def _call(lib, entry, m=None, pa=None, fr=None, batch=BATCH, first_step=1, opt_kind=None, params=PTR, comm=PTR, runs=None, last_pa=PTR, flags=0,
          n_runs=K):
    """one call of `entry` with complete arguments, except for what the case overrides"""
    m, pa = m or _desc(), pa or _desc("gru", 11)
    fr = fr or _frames(None if "sweep" in entry else PTR)
    runs = runs if runs is not None else _runs()
    pa_tab = (C.c_void_p * K)(*([PTR] * (K - 1) + [last_pa]))
    bufs3, kind = (PTR, PTR, PTR), (-1 if opt_kind is None else opt_kind)
    if entry == "epoch":
        return lib.odpd_train_epoch(None, C.byref(m), 0, C.byref(fr), batch, params, *bufs3, first_step, *ADAMW, *bufs3)
    if entry == "opt":
        return lib.odpd_train_epoch_opt(None, C.byref(m), 0, C.byref(fr), batch, 2 if opt_kind is None else opt_kind, params, *bufs3, first_step,
                                        5e-4, 0.0, *bufs3)
    if entry == "dp":
        return lib.odpd_train_epoch_dp(None, comm, C.byref(m), 0, C.byref(fr), batch, kind, params, *bufs3, first_step, *ADAMW, *bufs3)
    if entry == "cascade":      # (comm = NULL: one process)
        return lib.odpd_train_epoch_cascade(None, None, C.byref(m), C.byref(pa), 0, C.byref(fr), batch, kind, params, *bufs3, PTR, first_step, *ADAMW,
                                            None, PTR, None, PTR)
    if entry == "split":
        return lib.odpd_train_epoch_split(None, C.byref(m), 0, C.byref(fr), batch, kind, params, *bufs3, first_step, *ADAMW, None,
                                          *bufs3, *bufs3, PTR, None, PTR)
    if entry == "sweep":
        return lib.odpd_train_epoch_sweep(None, C.byref(m), n_runs, runs, 0, C.byref(fr), batch, first_step, *ADAMW[1:], flags, PTR)
    if entry == "cascade_sweep":
        return lib.odpd_train_epoch_cascade_sweep(None, C.byref(m), C.byref(pa), n_runs, runs, pa_tab, 0, C.byref(fr), batch, first_step, *ADAMW[1:], PTR)
    assert entry == "fwd_sweep"
    return lib.odpd_backbone_fwd_sweep(None, C.byref(m), n_runs, runs, batch, T, params, PTR)


LOOPS = ("epoch", "opt", "dp", "cascade", "split")
SWEEPS = ("sweep", "cascade_sweep")


def _cases():
    from opendpd_amd import _lib
    bf16 = lambda order=PTR: _frames(order, _lib.SAMPLES_BF16)
    c = []
    for e in LOOPS:
        c += [(e, "null params", dict(params=None), EINVAL), (e, "first_step 0", dict(first_step=0), EINVAL),
              (e, "batch 0", dict(batch=0), EINVAL), (e, "null order", dict(fr=_frames(None)), EINVAL)]
    for e in SWEEPS:
        c += [(e, "a run without params", dict(runs=_runs(params=None)), EINVAL), (e, "a run without order", dict(runs=_runs(order=None)), EINVAL),
              (e, "first_step 0", dict(first_step=0), EINVAL), (e, "batch 0", dict(batch=0), EINVAL), (e, "no runs", dict(n_runs=0), EINVAL)]
    c += [("dp", "null comm", dict(comm=None), EINVAL),
          ("dp", "null comm comes first", dict(comm=None, m=_desc("gru", 48), params=None), EINVAL),
          ("opt", "opt_kind 9", dict(opt_kind=9), EINVAL), ("opt", "opt_kind -1", dict(opt_kind=-1), EINVAL),
          ("dp", "opt_kind 9", dict(opt_kind=9), EINVAL), ("cascade", "opt_kind 9", dict(opt_kind=9), EINVAL),
          ("split", "opt_kind 9", dict(opt_kind=9), EINVAL),
          ("sweep", "S16 without a workspace", dict(flags=_lib.SWEEP_S16, runs=_runs(workspace=None)), EINVAL),
          ("cascade_sweep", "a run without its PA", dict(last_pa=None), EINVAL),
          ("cascade_sweep", "counters not 8-byte aligned", dict(runs=_runs(workspace=PTR + 4)), EINVAL),
          ("fwd_sweep", "a run without y", dict(runs=_runs(y=None)), EINVAL), ("fwd_sweep", "null x", dict(params=None), EINVAL),
          ("fwd_sweep", "no runs", dict(n_runs=0), EINVAL),
          # bf16 frames on a backbone or a loop that wants fp32 streams
          ("epoch", "bf16 frames, lstm", dict(fr=bf16(), m=_desc("lstm", 9)), EUNSUPPORTED),
          ("opt", "bf16 frames, gmp", dict(fr=bf16(), m=_desc("gmp", 13)), EUNSUPPORTED),
          ("dp", "bf16 frames, lstm", dict(fr=bf16(), m=_desc("lstm", 9)), EUNSUPPORTED),
          ("cascade", "bf16 frames", dict(fr=bf16()), EUNSUPPORTED), ("split", "bf16 frames", dict(fr=bf16(), m=_desc("gru", 48)), EUNSUPPORTED),
          ("sweep", "bf16 frames, lstm", dict(fr=bf16(None), m=_desc("lstm", 9)), EUNSUPPORTED),
          ("cascade_sweep", "bf16 frames", dict(fr=bf16(None)), EUNSUPPORTED),
          # shapes no frame-reading / sweep kernel serves
          ("epoch", "gru H48 (lane per unit)", dict(m=_desc("gru", 48)), EUNSUPPORTED),
          ("opt", "gru H48 (lane per unit)", dict(m=_desc("gru", 48)), EUNSUPPORTED),
          ("sweep", "gru H48 (lane per unit)", dict(m=_desc("gru", 48)), EUNSUPPORTED),
          ("sweep", "lstm", dict(m=_desc("lstm", 9)), EUNSUPPORTED),
          ("fwd_sweep", "gru H48 (lane per unit)", dict(m=_desc("gru", 48)), EUNSUPPORTED),
          ("cascade", "lstm PA behind a dgru DPD", dict(pa=_desc("lstm", 9)), EUNSUPPORTED),
          ("cascade_sweep", "lstm PA behind a dgru DPD", dict(pa=_desc("lstm", 9)), EUNSUPPORTED),
          ("split", "ODPD_FLAG_INIT_STATE", dict(m=_desc("gru", 48, _lib.FLAG_INIT_STATE)), EUNSUPPORTED),
          # an argument error is reported in front of an unsupported shape
          ("epoch", "gru H48 and null params", dict(m=_desc("gru", 48), params=None), EINVAL),
          ("cascade", "lstm PA and first_step 0", dict(pa=_desc("lstm", 9), first_step=0), EINVAL),
          ("split", "init state and opt_kind 9", dict(m=_desc("gru", 48, _lib.FLAG_INIT_STATE), opt_kind=9), EINVAL),
          ("cascade_sweep", "bf16 frames and a run without its PA", dict(fr=bf16(None), last_pa=None), EINVAL)]
    return c


@pytest.fixture(scope="module")
def lib():
    from opendpd_amd import _lib
    lib = _lib.load()
    for k, v in KNOBS.items():
        assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k
    yield lib
    for k, v in DEFAULTS.items():
        assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k


def test_the_table_covers_the_eight_entry_points():
    assert {c[0] for c in _cases()} == set(LOOPS) | set(SWEEPS) | {"fwd_sweep"}


@pytest.mark.parametrize("entry", LOOPS + SWEEPS + ("fwd_sweep",))
def test_refusals_come_with_their_code_before_any_device_call(lib, entry):
    got = {what: _call(lib, entry, **over) for e, what, over, _ in _cases() if e == entry}
    assert got == {what: code for e, what, _, code in _cases() if e == entry}
