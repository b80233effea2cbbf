"""Threshold sweeps of the delta DPDs (opendpd_amd/sweep.py::train_dpd_sweep(thresholds=...), csrc odpd_train_epoch_cascade_sweep_th): K train_dpd
runs that differ in their (thx, thh) pair — the THX / THH knobs of the reference's bash_scripts/OpenDPDv2.sh — carried by ONE cascade launch per
step, each workgroup at its run's pair.  Every run must stay its solo run bit for bit: at the C ABI against K calls of odpd_train_epoch_cascade,
each with a descriptor carrying its run's pair, and at the API against K solo train_dpd(thx=.., thh=..) calls.  The shapes and the harness are
those of tests/test_dpd_sweep_gpu.py.

The cases are `_check_*` functions, listed by `_cases` and run by ONE test, which reports every case that failed, under its name: together
they take about as long as one case of a neighbouring file, and the GPU suite already holds some five thousand items."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import tests.test_dpd_sweep_gpu as seed_sweep
from tests.golden_util import GOLDEN
from tests.test_dpd_sweep_gpu import BETAS, EINVAL, EPS, EUNSUPPORTED, PA_KW, WD, _abs, _same_files, _train_pas

pytestmark = pytest.mark.gpu

PAIRS = [(0.0, 0.0), (0.05, 0.02), (0.4, 0.3)]
# ... of the runs that differ in nothing else: thx of the middle pair moved from 0.05 to 0.2, because on these streams (samples of 0.1 .. 0.8 per
# component) no input delta of a frame's FIRST step lies below 0.05 — at T = 1 the run at (0.05, 0.02) would be the run at (0, 0), counters and
# all.  By the CPU oracle the first batch then zeroes 0 < 2 < 8 (deltagru_tcnskip 15) and 0 < 4 < 7 (deltagru 7) input deltas at T = 1, and three
# distinct counts of both kinds at T = 33 and 50 (_check_runs_that_differ_only_in_their_thresholds asserts it before it launches anything)
PAIRS_ALONE = [(0.0, 0.0), (0.2, 0.02), (0.4, 0.3)]
MODELS = [("deltagru_tcnskip", 15, "dgru", 23), ("deltagru", 7, "gru", 11)]
SHAPES = [(1, "l2"), (33, "l1"), (50, "l2"), (50, "l1")]      # T = 1 (one step), 33 (chunk + 1), 50 (the scripts' length)


class _ThRuns(seed_sweep._Runs):
    """K = len(pairs) runs of one delta (DPD, PA) pair at 12 frames, stride 3, batches of 5 (tail 2), 400 samples — run k at pairs[k].
    same_start: all runs from ONE initial DPD, PA buffer, epoch order and learning rate, so that only the thresholds tell them apart"""

    def __init__(self, dpd_bb, dpd_h, pa_bb, pa_h, T, pairs=PAIRS, same_start=False):
        super().__init__(dpd_bb, dpd_h, pa_bb, pa_h, K=len(pairs), T=T, n_frames=12, stride=3, batch=5, n_samples=400, shared_pa=same_start)
        self.pairs = [tuple(map(float, p)) for p in pairs]
        if same_start:
            self.p0, self.orders, self.lrs = [self.p0[0]] * self.K, [self.orders[0]] * self.K, [self.lrs[0]] * self.K
        self.descs = [self.desc_with(*p) for p in self.pairs]

    def desc_with(self, thx, thh, bits=0):
        return self._lib.ModelDesc(self.dpd.backbone, self.dpd.hidden, thx, thh, bits, bits, self.dpd.flags)

    def first_step_norms(self, loss):
        """pre-clip gradient norm of every solo run's first step, each at its own thresholds"""
        out, keep = [], self.dpd
        try:
            for k in range(self.K):
                self.dpd = self.descs[k]
                out.append(super().first_step_norms(loss)[k])
        finally:
            self.dpd = keep
        return out

    def solo(self, loss, max_norm):
        """K calls of odpd_train_epoch_cascade, run k with the descriptor that carries its pair"""
        L, lib, res = self._lib, self.lib, []
        for k in range(self.K):
            b = self._fresh(k)
            fr = self._frames(self.orders[k])
            rc = lib.odpd_train_epoch_cascade(L.stream_ptr(), None, C.byref(self.descs[k]), C.byref(self.pa), L.LOSS_IDS[loss], C.byref(fr), self.batch,
                                              -1, L.ptr(b["p"]), L.ptr(self.pa_p[k]), L.ptr(b["g"]), L.ptr(b["m"]), L.ptr(b["v"]), 1, self.lrs[k],
                                              BETAS[0], BETAS[1], EPS, WD, max_norm, None, L.ptr(b["part"]), L.ptr(b["stats"]), L.ptr(b["losses"]))
            L.check(rc, "odpd_train_epoch_cascade")
            res.append(b)
        torch.cuda.synchronize()
        return res

    NO_TABLE = object()

    def call_th(self, bufs, loss, max_norm, thresholds=None, K=None, scratch=True, first_step=1, sample_format=None, dpd=None, pa_desc=None,
                batch=None):
        """odpd_train_epoch_cascade_sweep_th; thresholds: a flat list (default: the runs' pairs), NO_TABLE = NULL"""
        L, lib = self._lib, self.lib
        table = (L.SweepRun * self.K)()
        pa_tab = (C.c_void_p * self.K)()
        for k, b in enumerate(bufs):
            table[k] = L.SweepRun(b["p"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), b["part"].data_ptr(),
                                  b["losses"].data_ptr(), None, b["stats"].data_ptr(), self.orders[k].data_ptr(), self.lrs[k])
            pa_tab[k] = self.pa_p[k].data_ptr()
        flat = [v for p in self.pairs for v in p] if thresholds is None else thresholds
        th = None if flat is self.NO_TABLE else (C.c_float * (2 * self.K))(*flat)
        fr = self._frames(None)
        if sample_format is not None:
            fr.sample_format = sample_format
        self._scratch = torch.empty(int(lib.odpd_sweep_cascade_th_scratch_bytes(self.K, self.n_steps)), dtype=torch.uint8, device="cuda")
        return lib.odpd_train_epoch_cascade_sweep_th(L.stream_ptr(), C.byref(dpd if dpd is not None else self.dpd),
                                                     C.byref(pa_desc if pa_desc is not None else self.pa), self.K if K is None else K, table, pa_tab,
                                                     th, L.LOSS_IDS[loss], C.byref(fr), self.batch if batch is None else batch, first_step, BETAS[0],
                                                     BETAS[1], EPS, WD, max_norm, C.c_void_p(self._scratch.data_ptr()) if scratch else None)

    def swept_th(self, loss, max_norm, **kw):
        bufs = [self._fresh(k) for k in range(self.K)]
        self._lib.check(self.call_th(bufs, loss, max_norm, **kw), "odpd_train_epoch_cascade_sweep_th")
        torch.cuda.synchronize()
        return bufs

    def clipping_norm(self, loss):
        """a max_norm that clips at least one run's first step, from the first-step norms as tests/test_dpd_sweep_gpu.py takes it"""
        norms = self.first_step_norms(loss)
        assert all(np.isfinite(n) and n > 0 for n in norms)
        max_norm = 0.7 * max(norms)
        assert sum(n > max_norm for n in norms) >= 1
        return max_norm


def _assert_same(solo, swept):
    for k, (a, b) in enumerate(zip(solo, swept)):
        for key in ("p", "m", "v", "losses", "stats"):
            assert torch.equal(a[key], b[key]), (k, key, a[key].flatten()[:4].tolist(), b[key].flatten()[:4].tolist())
        assert torch.isfinite(a["losses"]).all() and torch.isfinite(a["p"]).all()
        st = a["stats"].tolist()
        assert st[1] > 0 and st[3] > 0 and 0 <= st[0] <= st[1] and 0 <= st[2] <= st[3]      # (the counters were written)


def _check_each_run_equals_its_solo_epoch_at_its_own_thresholds(dpd_bb, dpd_h, pa_bb, pa_h, T, loss):
    """runs with their own parameters, PAs, orders, learning rates AND threshold pairs; the launch's descriptor carries the harness's 0.1 / 0.1"""
    r = _ThRuns(dpd_bb, dpd_h, pa_bb, pa_h, T)
    max_norm = r.clipping_norm(loss)
    _assert_same(r.solo(loss, max_norm), r.swept_th(loss, max_norm))


def _oracle_counts(r, dpd_bb, dpd_h, k):
    """[dx_zeros, dx_numel, dh_zeros, dh_numel] of run k's first batch at its initial parameters, by the CPU oracle's restatement of the delta cell"""
    from oracle.oracle import Oracle, make_model
    x = r.x.cpu().numpy()
    frames = np.stack([x[f * r.stride:f * r.stride + r.T] for f in r.orders[k].cpu().tolist()[:r.batch]])
    _, st = Oracle("f32").forward(make_model(dpd_bb, dpd_h, *r.pairs[k]), r.p0[k].cpu().numpy(), np.ascontiguousarray(frames))
    return st.tolist()


def _check_runs_that_differ_only_in_their_thresholds(dpd_bb, dpd_h, pa_bb, pa_h, T, loss):
    """one initial DPD, PA buffer, order and learning rate for all runs: a kernel that read one pair for the whole launch would train K equal runs"""
    r = _ThRuns(dpd_bb, dpd_h, pa_bb, pa_h, T, pairs=PAIRS_ALONE, same_start=True)
    # the condition on the inputs: these streams and pairs give three distinct counts in both counters (at T = 1 every hidden delta is 0 and
    # |0| < thh holds for any positive thh: there only the input deltas tell the runs apart)
    want = [_oracle_counts(r, dpd_bb, dpd_h, k) for k in range(r.K)]
    assert want[0][0] < want[1][0] < want[2][0], want
    if T >= 33:
        assert want[0][2] < want[1][2] < want[2][2], want
    max_norm = r.clipping_norm(loss)
    swept = r.swept_th(loss, max_norm)
    _assert_same(r.solo(loss, max_norm), swept)
    if T >= 33:
        for a in range(r.K):
            for b in range(a + 1, r.K):
                assert not torch.equal(swept[a]["p"], swept[b]["p"]), (a, b)
        for i in (0, 2):      # dx_zeros, dh_zeros: strictly increasing with the threshold
            z = [s["stats"][i].item() for s in swept]
            assert z[0] < z[1] < z[2], (i, z)
    else:
        assert not torch.equal(swept[0]["p"], swept[1]["p"]) and not torch.equal(swept[0]["p"], swept[2]["p"])


def _check_the_descriptors_own_pair_is_ignored(dpd_bb, dpd_h, pa_bb, pa_h):
    r = _ThRuns(dpd_bb, dpd_h, pa_bb, pa_h, 50)
    max_norm = r.clipping_norm("l2")
    _assert_same(r.solo("l2", max_norm), r.swept_th("l2", max_norm, dpd=r.desc_with(9.0, 9.0)))


def _check_equal_pairs_give_the_seed_sweep_of_that_pair(dpd_bb, dpd_h, pa_bb, pa_h, pair):
    r = _ThRuns(dpd_bb, dpd_h, pa_bb, pa_h, 33, pairs=[pair] * 3)
    max_norm = r.clipping_norm("l1")
    r.dpd = r.descs[0]      # odpd_train_epoch_cascade_sweep: the pair in the descriptor
    seed = r.swept("l1", max_norm)
    _assert_same(seed, r.swept_th("l1", max_norm, dpd=r.desc_with(9.0, 9.0)))


def _check_entry_points_refuse_what_they_do_not_serve():
    from opendpd_amd import _lib
    lib, ids = _lib.load(), _lib.BACKBONE_IDS
    r = _ThRuns("deltagru_tcnskip", 15, "dgru", 23, 20)
    bufs = [r._fresh(k) for k in range(r.K)]
    assert lib.odpd_sweep_cascade_th_supported(C.byref(r.dpd), C.byref(r.pa), 5, 20) == 1
    assert r.call_th(bufs, "l2", 200.0) == 0
    # unsupported pairs, batches and samples
    dgru = _lib.ModelDesc(ids["dgru"], 13, 0.0, 0.0, 0, 0, 0)
    lstm = _lib.ModelDesc(ids["lstm"], 9, 0.0, 0.0, 0, 0, 0)
    lstm_pa = _lib.ModelDesc(ids["lstm"], 8, 0.0, 0.0, 0, 0, 0)
    for dpd, pa in ((dgru, r.pa), (lstm, r.pa), (r.desc_with(0.1, 0.1, bits=16), r.pa), (r.dpd, lstm_pa)):
        assert lib.odpd_sweep_cascade_th_supported(C.byref(dpd), C.byref(pa), 5, 20) == 0
        assert r.call_th(bufs, "l2", 200.0, dpd=dpd, pa_desc=pa) == EUNSUPPORTED
    big = 1
    while lib.odpd_cascade_rows(C.byref(r.dpd), C.byref(r.pa), big, 20) > 0:
        big *= 2
        assert big < (1 << 20)
    assert lib.odpd_sweep_cascade_th_supported(C.byref(r.dpd), C.byref(r.pa), big, 20) == 0
    big_runs = _ThRuns("deltagru_tcnskip", 15, "dgru", 23, 20)
    big_runs.n = big       # (refused before anything is launched: the streams are never read)
    assert big_runs.call_th(bufs, "l2", 200.0, batch=big) == EUNSUPPORTED
    assert r.call_th(bufs, "l2", 200.0, sample_format=_lib.SAMPLES_BF16) == EUNSUPPORTED
    # invalid arguments
    ok = [v for p in r.pairs for v in p]
    assert r.call_th(bufs, "l2", 200.0, thresholds=r.NO_TABLE) == EINVAL
    assert r.call_th(bufs, "l2", 200.0, thresholds=ok[:3] + [float("nan")] + ok[4:]) == EINVAL
    assert r.call_th(bufs, "l2", 200.0, thresholds=ok[:4] + [-0.01] + ok[5:]) == EINVAL
    assert r.call_th(bufs, "l2", 200.0, K=0) == EINVAL
    assert r.call_th(bufs, "l2", 200.0, scratch=False) == EINVAL
    assert r.call_th(bufs, "l2", 200.0, first_step=0) == EINVAL
    assert lib.odpd_sweep_cascade_th_scratch_bytes(0, 10) < 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _workdir(path):
    """what the `workdir` fixture of tests/test_dpd_sweep_gpu.py sets up, for one case: the golden dataset under `path`, which becomes the
    working directory"""
    import pandas as pd
    d = dict(np.load(os.path.join(GOLDEN, "dpa200_dataset.npz")))
    ds = path / "datasets" / "DPA_200MHz"
    ds.mkdir(parents=True)
    (ds / "spec.json").write_text(str(d.pop("spec")))
    for k, v in d.items():
        pd.DataFrame(v, columns=["I", "Q"]).to_csv(ds / f"{k}.csv", index=False)
    old, old_env = os.getcwd(), os.environ.get("OPENDPD_DATASETS")
    os.chdir(path)
    os.environ["OPENDPD_DATASETS"] = str(path / "datasets")
    try:
        yield path
    finally:
        os.chdir(old)
        if old_env is None:
            os.environ.pop("OPENDPD_DATASETS", None)
        else:
            os.environ["OPENDPD_DATASETS"] = old_env


def _check_swept_pairs_write_the_files_of_their_solo_runs():
    import opendpd_amd as od
    pairs = [(0.0, 0.0), (0.01, 0.05), (0.1, 0.2)]
    _train_pas((0,))
    kw = dict(n_epochs=2, lr=1e-3, DPD_backbone="deltagru_tcnskip", DPD_hidden_size=15, **PA_KW)
    os.chdir("solo")
    solo = [_abs(od.train_dpd(seed=0, thx=a, thh=b, **kw)) for a, b in pairs]
    os.chdir(os.path.join("..", "swept"))
    swept = [_abs(r) for r in od.train_dpd_sweep(seeds=(0,), thresholds=pairs, **kw)]
    assert len(swept) == len(pairs) and all(r["lockstep"] for r in swept)      # one group, on the launch that carries a pair per run
    assert [(r["thx"], r["thh"]) for r in swept] == pairs
    hists = [_same_files(a, b) for a, b in zip(solo, swept)]
    dv = [tuple(h["SP_T_DV"].tolist()) for h in hists]
    assert len(set(dv)) == len(pairs), dv


def _check_the_runs_are_hidden_size_then_pair_then_seed():
    import opendpd_amd as od
    pairs = [(0.0, 0.0), (0.01, 0.05)]
    _train_pas((0, 1))
    kw = dict(n_epochs=1, lr=1e-3, DPD_backbone="deltagru_tcnskip", **PA_KW)
    os.chdir("swept")
    swept = [_abs(r) for r in od.train_dpd_sweep(seeds=(0, 1), hidden_sizes=(8, 15), thresholds=pairs, **kw)]
    assert [(r["DPD_hidden_size"], (r["thx"], r["thh"]), r["seed"]) for r in swept] == [(H, p, s) for H in (8, 15) for p in pairs for s in (0, 1)]
    assert all(r["lockstep"] for r in swept)
    os.chdir(os.path.join("..", "solo"))
    solo = _abs(od.train_dpd(seed=1, DPD_hidden_size=15, thx=0.01, thh=0.05, **kw))
    _same_files(solo, swept[7])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the test
# ---------------------------------------------------------------------------------------------------------------------------------------
def _cases(tmp_path):
    """(name, callable) of every case, in the order they run"""
    part = functools.partial
    for m in MODELS:
        for T, loss in SHAPES:
            yield f"each run == its solo epoch at its own thresholds [{m[0]} {m[1]} -> {m[2]} {m[3]}, T {T}, {loss}]", part(
                _check_each_run_equals_its_solo_epoch_at_its_own_thresholds, *m, T, loss)
    for m in MODELS:
        for T, loss in SHAPES:
            yield f"runs that differ only in their thresholds [{m[0]} {m[1]} -> {m[2]} {m[3]}, T {T}, {loss}]", part(
                _check_runs_that_differ_only_in_their_thresholds, *m, T, loss)
    for m in MODELS:
        yield f"the descriptor's own pair is ignored [{m[0]} {m[1]} -> {m[2]} {m[3]}]", part(_check_the_descriptors_own_pair_is_ignored, *m)
    for m in MODELS:
        for pair in ((0.05, 0.02), (0.0, 0.0)):
            yield f"equal pairs give the seed sweep of that pair [{m[0]} {m[1]} -> {m[2]} {m[3]}, {pair}]", part(
                _check_equal_pairs_give_the_seed_sweep_of_that_pair, *m, pair)
    yield "the entry points refuse what they do not serve", _check_entry_points_refuse_what_they_do_not_serve

    def in_workdir(name, check):
        with _workdir(tmp_path / name):
            check()
    yield "API: swept pairs write the files of their solo runs", part(in_workdir, "files", _check_swept_pairs_write_the_files_of_their_solo_runs)
    yield "API: the runs are hidden size, then pair, then seed", part(in_workdir, "order", _check_the_runs_are_hidden_size_then_pair_then_seed)


def test_threshold_sweeps_stay_their_solo_runs(tmp_path):
    """every case above; a case whose assertion fails is recorded under its name and the others still run (any other exception — a HIP error
    among them — ends the test at once)"""
    failed, n = [], 0
    for name, check in _cases(tmp_path):
        n += 1
        try:
            check()
        except AssertionError as e:
            failed.append(f"{name}: {str(e)[:800]}")
    assert n == 2 * len(MODELS) * len(SHAPES) + len(MODELS) + 2 * len(MODELS) + 3
    assert not failed, f"{len(failed)} of {n} cases failed:\n" + "\n".join(failed)
