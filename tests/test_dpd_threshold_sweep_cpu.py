"""What the threshold sweep of the delta DPDs (opendpd_amd/sweep.py::train_dpd_sweep(thresholds=...), csrc odpd_train_epoch_cascade_sweep_th)
answers before any device call: the argument checks of the new entry point (called the way tests/test_epoch_args_cpu.py calls its neighbours:
dummy pointers nobody reads, explicit selection knobs), odpd_sweep_cascade_th_supported against the live odpd_sweep_cascade_supported over the
grid of tests/test_size_queries_cpu.py, the scratch size rule, and the ValueErrors of the Python entry point."""
import ctypes as C
import os
import re

import pytest

from tests.test_epoch_args_cpu import ADAMW, BATCH, DEFAULTS, EINVAL, EUNSUPPORTED, K, KNOBS, PTR, _frames, _runs
from tests.test_size_queries_cpu import BS, TS
from tests.test_size_queries_cpu import KNOBS as BASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"odpd_sweep_cascade_th_supported": 4, "odpd_sweep_cascade_th_scratch_bytes": 2, "odpd_train_epoch_cascade_sweep_th": 17}
NO_TABLE = object()      # a NULL where _call would otherwise build the table


def _desc(bb, H, thx=0.0, thh=0.0, bits=0):
    from opendpd_amd import _lib
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, thx, thh, bits, bits, 0)


def _call(lib, m=None, pa=None, fr=None, batch=BATCH, first_step=1, runs=None, last_pa=PTR, n_runs=K, thresholds=(0.0, 0.0, 0.01, 0.05), pa_tab=True,
          scratch=PTR):
    from opendpd_amd import _lib
    m, pa = m or _desc("deltagru_tcnskip", 15, 0.1, 0.1), pa or _desc("dgru", 23)
    fr = fr or _frames(None)
    runs = None if runs is NO_TABLE else runs if runs is not None else _runs()
    tab = (C.c_void_p * K)(*([PTR] * (K - 1) + [last_pa])) if pa_tab else None
    th = None if thresholds is NO_TABLE else (C.c_float * (2 * K))(*thresholds)
    return lib.odpd_train_epoch_cascade_sweep_th(None, C.byref(m), C.byref(pa), n_runs, runs, tab, th, 0, C.byref(fr), batch, first_step, *ADAMW[1:], scratch)


@pytest.fixture(scope="module")
def lib():
    from opendpd_amd import _lib
    lib = _lib.load()
    for k, v in KNOBS.items():
        assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k
    yield lib
    for k, v in DEFAULTS.items():
        assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k


def test_entry_points_are_declared_and_bound_with_the_same_argument_counts():
    from opendpd_amd import _lib
    header = open(os.path.join(ROOT, "include", "opendpd_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n in ARGS.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/opendpd_hip.h"
        assert len(m.group(1).split(",")) == n, (name, m.group(1))
        assert name in _lib.exported_symbols()
        assert len(_lib._EXPORTS[name][1]) == n, name
    assert _lib.load().odpd_abi_version() == 13      # new entry points only: no struct moved


def test_argument_errors_come_before_any_device_call(lib):
    from opendpd_amd import _lib
    nan, inf = float("nan"), float("inf")
    bf16 = _frames(None, _lib.SAMPLES_BF16)
    cases = {"no threshold table": dict(thresholds=NO_TABLE), "a NaN entry": dict(thresholds=(0.0, 0.0, nan, 0.05)),
             "an infinite entry": dict(thresholds=(0.0, inf, 0.01, 0.05)), "a negative entry": dict(thresholds=(0.0, 0.0, 0.01, -1e-3)),
             "no runs": dict(n_runs=0), "no run table": dict(runs=NO_TABLE), "no PA table": dict(pa_tab=False), "no scratch": dict(scratch=None),
             "first_step 0": dict(first_step=0), "batch 0": dict(batch=0), "a run without params": dict(runs=_runs(params=None)),
             "a run without order": dict(runs=_runs(order=None)), "a run without its PA": dict(last_pa=None),
             "counters not 8-byte aligned": dict(runs=_runs(workspace=PTR + 4)),
             # an argument error is reported in front of what is not served
             "bf16 frames and a NaN entry": dict(fr=bf16, thresholds=(nan, 0.0, 0.0, 0.0)),
             "a dgru DPD and no threshold table": dict(m=_desc("dgru", 13), thresholds=NO_TABLE)}
    assert {what: _call(lib, **over) for what, over in cases.items()} == {what: EINVAL for what in cases}


def test_what_is_not_served_is_refused_before_any_device_call(lib):
    from opendpd_amd import _lib
    cases = {"bf16 frames": dict(fr=_frames(None, _lib.SAMPLES_BF16)), "a dgru DPD": dict(m=_desc("dgru", 13)), "an lstm DPD": dict(m=_desc("lstm", 9)),
             "a deltajanet DPD": dict(m=_desc("deltajanet", 12, 0.01, 0.05)), "a quantised deltagru_tcnskip": dict(m=_desc("deltagru_tcnskip", 15, bits=16)),
             "an lstm PA": dict(pa=_desc("lstm", 9))}
    assert {what: _call(lib, **over) for what, over in cases.items()} == {what: EUNSUPPORTED for what in cases}


@pytest.mark.parametrize("base", sorted(BASES))
def test_th_supported_is_the_cascade_sweep_query_for_the_two_delta_kinds_and_zero_elsewhere(base):
    from opendpd_amd import _lib
    lib = _lib.load()
    pa = _desc("dgru", 23)
    served = {}
    try:
        for k, v in BASES[base].items():
            assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k
        for bb, H in (("deltagru", 7), ("deltagru_tcnskip", 15), ("dgru", 13), ("lstm", 9), ("deltajanet", 12)):
            d = _desc(bb, H, 0.01, 0.05)
            for B in BS:
                for T in TS:
                    old = lib.odpd_sweep_cascade_supported(C.byref(d), C.byref(pa), B, T)
                    new = lib.odpd_sweep_cascade_th_supported(C.byref(d), C.byref(pa), B, T)
                    assert new == (old if bb in ("deltagru", "deltagru_tcnskip") else 0), (bb, H, B, T, old, new)
                    served[bb] = served.get(bb, 0) + new
        q = _desc("deltagru_tcnskip", 15, 0.01, 0.05, bits=16)
        assert all(lib.odpd_sweep_cascade_th_supported(C.byref(q), C.byref(pa), B, T) == 0 for B in BS for T in TS)
    finally:
        for k, v in BASES["default"].items():
            assert lib.odpd_set_tuning(k.encode(), C.c_int64(v)) == 0, k
    if BASES[base].get("cascade_one_launch", 1) and BASES[base].get("gp_max_batch", -1) != 0:      # (not vacuous where the step is switched on)
        assert served["deltagru"] > 0 and served["deltagru_tcnskip"] > 0, served
    assert served["dgru"] == served["lstm"] == served["deltajanet"] == 0


def test_scratch_holds_the_pairs_on_top_of_the_seed_sweeps_and_refuses_no_runs():
    from opendpd_amd import _lib
    lib = _lib.load()
    f, seed = lib.odpd_sweep_cascade_th_scratch_bytes, lib.odpd_sweep_cascade_scratch_bytes
    for K_ in (1, 3, 4, 9, 64, 1000):
        for steps in (0, 10, 1000):
            assert f(K_, steps) >= seed(K_, steps) + 8 * K_      # a (thx, thh) pair of floats per run
    assert f(8, 10) > f(4, 10) and f(3, 1000) > f(3, 10)
    assert f(0, 10) < 0 and f(-1, 10) < 0 and f(2, -1) < 0


def test_value_errors_come_before_the_dataset_is_opened():
    from opendpd_amd import data as D
    from opendpd_amd.sweep import train_dpd_sweep
    kw = dict(dataset_name="no_such_dataset_anywhere", seeds=(0,), accelerator="cpu", n_epochs=1)
    with pytest.raises(ValueError, match="not both"):
        train_dpd_sweep(thresholds=[(0.0, 0.0), (0.01, 0.05)], thx=0.01, **kw)
    with pytest.raises(ValueError, match="not both"):
        train_dpd_sweep(thresholds=[(0.0, 0.0)], thh=0.05, **kw)
    for bad in ((-0.01, 0.0), (0.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(ValueError, match="finite"):
            train_dpd_sweep(thresholds=[(0.0, 0.0), bad], **kw)
    with pytest.raises(ValueError, match="same files"):
        train_dpd_sweep(thresholds=[(0.01, 0.05), (0.0101, 0.0499)], **kw)
    with pytest.raises(ValueError, match="holds no thresholds"):
        train_dpd_sweep(thresholds=[(0.0, 0.0), (0.01, 0.05)], DPD_backbone="dgru", **kw)
    with pytest.raises(ValueError, match="pairs"):
        train_dpd_sweep(thresholds=[0.01, 0.05], **kw)
    with pytest.raises(ValueError, match="no pair"):
        train_dpd_sweep(thresholds=[], **kw)
    # what is no such error reaches the dataset: distinct pairs, and ONE pair for a backbone whose model ID holds none
    with pytest.raises(FileNotFoundError, match="no_such_dataset_anywhere"):
        train_dpd_sweep(thresholds=[(0.0, 0.0), (0.01, 0.05)], **kw)
    with pytest.raises(FileNotFoundError, match="no_such_dataset_anywhere"):
        train_dpd_sweep(thresholds=[(0.0, 0.0)], DPD_backbone="dgru", **kw)
    assert D._share is None


def test_float_delta_runs_of_differing_pairs_share_a_group_and_no_others():
    from types import SimpleNamespace

    from opendpd_amd.sweep import _dpd_group_key

    def key(bb, thx, thh, quant=False):
        p = SimpleNamespace(DPD_backbone=bb, DPD_hidden_size=15, DPD_num_layers=1, PA_backbone="dgru", PA_hidden_size=8, PA_num_layers=1, batch_size=64,
                            frame_length=50, frame_stride=1, loss_type="l2", opt_type="adamw", dataset_label="d", frame_storage="f32",
                            grad_clip_val=200.0, thx=thx, thh=thh, quant=quant, n_bits_w=8, n_bits_a=8, pretrained_model="", quant_dir_label="",
                            q_pretrain=False)
        return _dpd_group_key(SimpleNamespace(proj=p))

    for bb in ("deltagru", "deltagru_tcnskip"):
        assert key(bb, 0.0, 0.0) == key(bb, 0.01, 0.05)
        assert key(bb, 0.0, 0.0, quant=True) != key(bb, 0.01, 0.05, quant=True)      # quantised delta DPDs keep the per-run epoch, one group per pair
        assert key(bb, 0.0, 0.0) != key(bb, 0.0, 0.0, quant=True)
    assert key("deltajanet", 0.0, 0.0) != key("deltajanet", 0.01, 0.05)
    assert key("deltagru", 0.0, 0.0) != key("deltagru_tcnskip", 0.0, 0.0)
