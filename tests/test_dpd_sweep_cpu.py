"""What the lockstep train_dpd sweep (opendpd_amd/sweep.py::train_dpd_sweep, csrc odpd_train_epoch_cascade_sweep) answers before any device
query: its three C entry points as the header declares them and `_lib` binds them, the scratch size rule, the argument contract."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"odpd_sweep_cascade_supported": 4, "odpd_sweep_cascade_scratch_bytes": 2, "odpd_train_epoch_cascade_sweep": 16}


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
    lib = _lib.load()
    assert lib.odpd_abi_version() == 13      # new entry points only: no struct moved


def test_scratch_grows_with_runs_and_steps_and_refuses_no_runs():
    from opendpd_amd import _lib
    lib = _lib.load()
    f = lib.odpd_sweep_cascade_scratch_bytes
    assert 0 < f(1, 0) <= f(2, 0) < f(64, 0)
    assert f(4, 10) >= f(4, 0) + 4 * 10 * 4                     # K x n_steps step sizes (floats)
    for K in (1, 4, 9, 64):
        assert f(K, 10) >= K * (80 + 8 + 10 * 4)                # per run: a table entry (80 bytes), a PA pointer, its step sizes
    assert f(8, 10) > f(4, 10)
    assert f(3, 1000) > f(3, 10)
    assert f(0, 10) < 0 and f(-1, 10) < 0 and f(2, -1) < 0


def test_argument_contract():
    import opendpd_amd
    from opendpd_amd import data as D
    from opendpd_amd.sweep import train_dpd_sweep
    assert opendpd_amd.train_dpd_sweep is train_dpd_sweep and "train_dpd_sweep" in opendpd_amd.__all__
    with pytest.raises(ValueError, match="dataset_name"):
        train_dpd_sweep()
    with pytest.raises(ValueError, match="dataset_name"):
        train_dpd_sweep(dataset_name=None, seeds=(0, 1))
    # a failing setup must not leave the CSV cache of the sweep behind for later solo runs
    with pytest.raises(FileNotFoundError, match="no_such_dataset_anywhere"):
        train_dpd_sweep(dataset_name="no_such_dataset_anywhere", seeds=(0, 1), accelerator="cpu", n_epochs=1)
    assert D._share is None


def test_a_failing_flush_neither_masks_the_loops_exception_nor_goes_unnoticed():
    from types import SimpleNamespace

    from opendpd_amd.sweep import _flush_loggers, _sweep_loop

    class Logger:
        def __init__(self, fail):
            self.fail, self.flushed, self.defer_checkpoints = fail, False, False

        def flush(self):
            self.flushed = True
            if self.fail:
                raise OSError("disk full")

    def runs():
        return [SimpleNamespace(proj=SimpleNamespace(logger=Logger(f), path_save_file_best="best.pt")) for f in (True, False)]

    class Group:
        def train_epoch(self):
            raise KeyError("from the loop")

    # the loop's own error surfaces, the lost checkpoint is reported as a warning, and every logger was still flushed
    rs = runs()
    with pytest.warns(RuntimeWarning, match="best.pt not written"), pytest.raises(KeyError):
        _sweep_loop(rs, [Group()], 1, "NMSE")
    assert all(r.proj.logger.flushed and r.proj.logger.defer_checkpoints for r in rs)
    # a loop that finished: a failing flush is the error — also when the caller happens to be handling another exception
    rs = runs()
    try:
        raise ValueError("the caller's own business")
    except ValueError:
        with pytest.raises(OSError, match="disk full"):
            _sweep_loop(rs, [], 0, "NMSE")
    assert all(r.proj.logger.flushed for r in rs)
    with pytest.raises(OSError):
        _flush_loggers(runs(), None)
