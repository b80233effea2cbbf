"""Lockstep train_dpd sweeps (opendpd_amd/sweep.py::train_dpd_sweep, csrc odpd_train_epoch_cascade_sweep): K train_dpd runs of the reference's
seed sweep (bash_scripts/train_all_dpd.sh) carried by ONE cascade launch per step must each stay the solo run bit for bit — at the C ABI
(parameters, both optimiser states, per-step losses, a delta DPD's sparsity counters against K calls of odpd_train_epoch_cascade) and at the
API (the files under save/ and log/ against K solo train_dpd calls)."""
import ctypes as C
import os
import shutil

import numpy as np
import pandas as pd
import pytest
import torch

from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu

EUNSUPPORTED, EINVAL = -2, -1
BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.01


# ---------------------------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------------------------
def _model(bb, H, seed, thx=0.0, thh=0.0):
    from opendpd_amd import CoreModel
    torch.manual_seed(seed)
    m = CoreModel(2, H, 1, bb, thx=thx, thh=thh).cuda()
    return m.backbone.desc, m.backbone.flat_params().detach().clone().contiguous()


def _streams(n_samples, seed):
    rng = np.random.RandomState(seed)
    x = (rng.uniform(0.1, 0.8, (n_samples, 2)) * rng.choice([-1.0, 1.0], (n_samples, 2))).astype(np.float32)
    y = (0.5 * rng.randn(n_samples, 2)).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


class _Runs:
    """K runs of one (DPD, PA) pair: their initial buffers, and the two ways to train them for one epoch"""

    def __init__(self, dpd_bb, dpd_h, pa_bb, pa_h, K, T, n_frames, stride, batch, n_samples, shared_pa=False, delta_th=0.1):
        from opendpd_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        delta = "delta" in dpd_bb
        th = delta_th if delta else 0.0
        self.delta, self.K, self.T, self.n, self.stride, self.batch = delta, K, T, n_frames, stride, batch
        self.n_steps = (n_frames + batch - 1) // batch
        assert (n_frames - 1) * stride + T <= n_samples
        self.x, self.y = _streams(n_samples, 7 * T + dpd_h)
        dm = [_model(dpd_bb, dpd_h, 100 + k, th, th) for k in range(K)]
        self.dpd, self.p0 = dm[0][0], [m[1] for m in dm]
        pm = [_model(pa_bb, pa_h, 200 + (0 if shared_pa else k)) for k in range(K)]
        self.pa = pm[0][0]
        self.pa_p = [pm[0][1]] * K if shared_pa else [m[1] for m in pm]
        self.P = int(self.lib.odpd_param_count(C.byref(self.dpd)))
        assert self.P == self.p0[0].numel()
        g = torch.Generator().manual_seed(T + K)
        self.orders = [torch.randperm(n_frames, generator=g).cuda() for _ in range(K)]
        self.lrs = [1e-3 * (k + 1) for k in range(K)]
        full, tail = min(batch, n_frames), n_frames - (self.n_steps - 1) * batch
        self.rows = max(int(self.lib.odpd_cascade_rows(C.byref(self.dpd), C.byref(self.pa), b, T)) for b in {full, tail})
        assert self.rows > 0

    def _fresh(self, k):
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
        return dict(p=self.p0[k].clone(), g=z(self.P + self._lib.LOSS_COLS), m=z(self.P), v=z(self.P), losses=z(self.n_steps),
                    part=torch.empty(self.rows, self.P + self._lib.LOSS_COLS, dtype=torch.float32, device="cuda"),
                    stats=z(4, torch.float64) if self.delta else None)

    def _frames(self, order):
        L = self._lib
        return L.Frames(self.x.data_ptr(), self.y.data_ptr(), order.data_ptr() if order is not None else None, self.n, self.T, self.stride,
                        L.SAMPLES_F32, 0)

    def first_step_norms(self, loss):
        """pre-clip gradient norm of every solo run's first step: the launches odpd_train_epoch_cascade starts with"""
        L, lib, out = self._lib, self.lib, []
        B = min(self.batch, self.n)
        for k in range(self.K):
            b = self._fresh(k)
            L.check(lib.odpd_cascade_fwd_bwd(L.stream_ptr(), C.byref(self.dpd), C.byref(self.pa), L.LOSS_IDS[loss], B, self.T, B * self.T * 2, L.ptr(b["p"]),
                                             L.ptr(self.pa_p[k]), L.ptr(self.x), L.ptr(self.y), L.ptr(self.orders[k]), self.stride, L.ptr(b["part"]),
                                             None), "odpd_cascade_fwd_bwd")
            L.check(lib.odpd_reduce_partials(L.stream_ptr(), int(lib.odpd_cascade_rows(C.byref(self.dpd), C.byref(self.pa), B, self.T)), self.P,
                                             L.ptr(b["part"]), L.ptr(b["g"]), 0), "odpd_reduce_partials")
            out.append(float(b["g"][:self.P].double().norm().item()))
        return out

    def solo(self, loss, max_norm):
        L, lib, res = self._lib, self.lib, []
        for k in range(self.K):
            b = self._fresh(k)
            fr = self._frames(self.orders[k])
            rc = lib.odpd_train_epoch_cascade(L.stream_ptr(), None, C.byref(self.dpd), C.byref(self.pa), L.LOSS_IDS[loss], C.byref(fr), self.batch, -1,
                                              L.ptr(b["p"]), L.ptr(self.pa_p[k]), L.ptr(b["g"]), L.ptr(b["m"]), L.ptr(b["v"]), 1, self.lrs[k], BETAS[0],
                                              BETAS[1], EPS, WD, max_norm, None, L.ptr(b["part"]), L.ptr(b["stats"]), L.ptr(b["losses"]))
            L.check(rc, "odpd_train_epoch_cascade")
            res.append(b)
        torch.cuda.synchronize()
        return res

    def call_sweep(self, bufs, loss, max_norm, K=None, runs=True, pa=True, scratch=True, first_step=1, sample_format=None, dpd=None, pa_desc=None,
                   batch=None):
        L, lib = self._lib, self.lib
        K_ = self.K if K is None else K
        table = (L.SweepRun * self.K)()
        pa_tab = (C.c_void_p * self.K)()
        for k, b in enumerate(bufs):
            table[k] = L.SweepRun(b["p"].data_ptr(), b["g"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), b["part"].data_ptr(),
                                  b["losses"].data_ptr(), None, b["stats"].data_ptr() if b["stats"] is not None else None,
                                  self.orders[k].data_ptr(), self.lrs[k])
            pa_tab[k] = self.pa_p[k].data_ptr()
        fr = self._frames(None)
        if sample_format is not None:
            fr.sample_format = sample_format
        self._scratch = torch.empty(int(lib.odpd_sweep_cascade_scratch_bytes(self.K, self.n_steps)), dtype=torch.uint8, device="cuda")
        return lib.odpd_train_epoch_cascade_sweep(L.stream_ptr(), C.byref(dpd if dpd is not None else self.dpd),
                                                  C.byref(pa_desc if pa_desc is not None else self.pa), K_, table if runs else None,
                                                  pa_tab if pa else None, L.LOSS_IDS[loss], C.byref(fr), self.batch if batch is None else batch,
                                                  first_step, BETAS[0], BETAS[1], EPS, WD, max_norm,
                                                  C.c_void_p(self._scratch.data_ptr()) if scratch else None)

    def swept(self, loss, max_norm):
        bufs = [self._fresh(k) for k in range(self.K)]
        self._lib.check(self.call_sweep(bufs, loss, max_norm), "odpd_train_epoch_cascade_sweep")
        torch.cuda.synchronize()
        return bufs


def _assert_same(solo, swept, delta):
    for k, (a, b) in enumerate(zip(solo, swept)):
        for key in ("p", "m", "v", "losses"):
            assert torch.equal(a[key], b[key]), (k, key)
        assert torch.isfinite(a["losses"]).all() and torch.isfinite(a["p"]).all()
        if delta:
            assert torch.equal(a["stats"], b["stats"]), (k, a["stats"].tolist(), b["stats"].tolist())
            st = a["stats"].tolist()
            # the thresholds zero some deltas (at T = 1 every hidden delta: h starts at zero, |0 - 0| < thh)
            assert st[0] > 0 and st[2] > 0 and st[1] > st[0] and st[3] >= st[2]


# (DPD -> PA): every kernel (GRU family, delta, lstm), both DPD block counts and the three PA variants
PAIRS = [("gru", 5, "gru", 3), ("dgru", 13, "dgru", 23), ("qgru", 20, "dgru", 8), ("qgru_amp1", 10, "gru", 27),
         ("deltagru_tcnskip", 15, "dgru", 23), ("deltagru", 7, "gru", 11), ("lstm", 9, "dgru", 8)]


@pytest.mark.parametrize("T,loss", [(1, "l2"), (33, "l1"), (50, "l2"), (50, "l1")])
@pytest.mark.parametrize("dpd_bb,dpd_h,pa_bb,pa_h", PAIRS)
def test_swept_epoch_equals_the_solo_epochs_bit_for_bit(dpd_bb, dpd_h, pa_bb, pa_h, T, loss):
    """K = 3 runs with their own parameters, PAs, epoch orders and learning rates; 12 frames at stride 3 in batches of 5 (tail: 2 frames);
    T = 1 (one step), 33 (chunk + 1), 50 (the scripts' length); a max_norm that clips at least one run's first step"""
    r = _Runs(dpd_bb, dpd_h, pa_bb, pa_h, K=3, T=T, n_frames=12, stride=3, batch=5, n_samples=400)
    norms = r.first_step_norms(loss)
    assert all(np.isfinite(n) and n > 0 for n in norms)
    max_norm = 0.7 * max(norms)
    assert sum(n > max_norm for n in norms) >= 1      # clipping is active
    _assert_same(r.solo(loss, max_norm), r.swept(loss, max_norm), r.delta)


@pytest.mark.parametrize("frames", [7, 3], ids=["tail", "one_short_batch"])
def test_swept_epoch_on_a_tail_and_on_one_short_batch(frames):
    """where the sweep's batch arithmetic can go wrong, at the smallest shape (K = 2, dgru H13 -> gru H11, T = 20, batches of 4): 7 frames =
    a full batch and a tail of 3, 3 frames = an epoch of one short batch"""
    r = _Runs("dgru", 13, "gru", 11, K=2, T=20, n_frames=frames, stride=1, batch=4, n_samples=frames + 20 - 1)
    max_norm = 0.7 * max(r.first_step_norms("l2"))      # (clips at least one run's first step)
    _assert_same(r.solo("l2", max_norm), r.swept("l2", max_norm), r.delta)


def test_more_workgroups_than_the_chip_holds_at_once():
    """K = 9 runs of batch 64: 576 workgroups, each with a CU's LDS to itself — they queue, and nothing may depend on their being resident"""
    r = _Runs("gru", 8, "dgru", 8, K=9, T=20, n_frames=64, stride=1, batch=64, n_samples=128)
    assert r.n_steps == 1 and r.rows == 64
    _assert_same(r.solo("l2", 200.0), r.swept("l2", 200.0), False)


def test_runs_may_share_one_pa_buffer():
    r = _Runs("dgru", 13, "dgru", 23, K=3, T=50, n_frames=12, stride=3, batch=5, n_samples=400, shared_pa=True)
    assert all(p.data_ptr() == r.pa_p[0].data_ptr() for p in r.pa_p)
    before = r.pa_p[0].clone()
    swept = r.swept("l2", 200.0)
    assert torch.equal(r.pa_p[0], before)
    _assert_same(r.solo("l2", 200.0), swept, False)
    assert torch.equal(r.pa_p[0], before)


def test_entry_points_refuse_what_they_do_not_serve():
    from opendpd_amd import _lib
    lib = _lib.load()
    r = _Runs("dgru", 8, "dgru", 8, K=2, T=20, n_frames=12, stride=3, batch=5, n_samples=400)
    bufs = [r._fresh(k) for k in range(r.K)]
    ids = _lib.BACKBONE_IDS
    assert lib.odpd_sweep_cascade_supported(C.byref(r.dpd), C.byref(r.pa), 5, 20) == 1
    assert r.call_sweep(bufs, "l2", 200.0) == 0
    # unsupported pairs and batches
    quant = _lib.ModelDesc(ids["dgru"], 8, 0.0, 0.0, 8, 8, 0)
    two = _lib.ModelDesc(ids["gru"], 8, 0.0, 0.0, 0, 0, _lib.FLAG_TWO_LAYERS)
    lstm_pa = _lib.ModelDesc(ids["lstm"], 8, 0.0, 0.0, 0, 0, 0)
    for dpd, pa in ((quant, r.pa), (two, r.pa), (r.dpd, lstm_pa)):
        assert lib.odpd_sweep_cascade_supported(C.byref(dpd), C.byref(pa), 5, 20) == 0
        assert r.call_sweep(bufs, "l2", 200.0, dpd=dpd, pa_desc=pa) == EUNSUPPORTED
    big = 1
    while lib.odpd_cascade_rows(C.byref(r.dpd), C.byref(r.pa), big, 20) > 0:
        big *= 2
        assert big < (1 << 20)
    assert lib.odpd_sweep_cascade_supported(C.byref(r.dpd), C.byref(r.pa), big, 20) == 0
    big_runs = _Runs("dgru", 8, "dgru", 8, K=2, T=20, n_frames=12, stride=3, batch=5, n_samples=400)
    big_runs.n = big       # (refused before anything is launched: the streams are never read)
    assert big_runs.call_sweep(bufs, "l2", 200.0, batch=big) == EUNSUPPORTED
    # invalid arguments
    assert r.call_sweep(bufs, "l2", 200.0, K=0) == EINVAL
    assert r.call_sweep(bufs, "l2", 200.0, runs=False) == EINVAL
    assert r.call_sweep(bufs, "l2", 200.0, pa=False) == EINVAL
    assert r.call_sweep(bufs, "l2", 200.0, scratch=False) == EINVAL
    assert r.call_sweep(bufs, "l2", 200.0, first_step=0) == EINVAL
    assert r.call_sweep(bufs, "l2", 200.0, sample_format=_lib.SAMPLES_BF16) == EUNSUPPORTED
    assert lib.odpd_sweep_cascade_scratch_bytes(0, 10) < 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def workdir(tmp_path):
    d = dict(np.load(os.path.join(GOLDEN, "dpa200_dataset.npz")))
    ds = tmp_path / "datasets" / "DPA_200MHz"
    ds.mkdir(parents=True)
    (ds / "spec.json").write_text(str(d.pop("spec")))
    for k, v in d.items():
        pd.DataFrame(v, columns=["I", "Q"]).to_csv(ds / f"{k}.csv", index=False)
    old = os.getcwd()
    os.chdir(tmp_path)
    os.environ["OPENDPD_DATASETS"] = str(tmp_path / "datasets")
    yield tmp_path
    os.chdir(old)


PA_KW = dict(dataset_name="DPA_200MHz", PA_backbone="dgru", PA_hidden_size=8, batch_size=64, frame_length=50, accelerator="cuda")


def _train_pas(seeds):
    """one train_pa epoch per seed in ./solo, the checkpoints copied to ./swept"""
    import opendpd_amd as od
    os.makedirs("solo", exist_ok=True)
    os.chdir("solo")
    for s in seeds:
        od.train_pa(seed=s, n_epochs=1, lr=1e-3, **PA_KW)
    os.chdir("..")
    shutil.copytree(os.path.join("solo", "save"), os.path.join("swept", "save"))


def _abs(r):
    return {k: (os.path.abspath(v) if k.endswith("_path") else v) for k, v in r.items()}


def _same_files(solo, swept):
    hs, hw = pd.read_csv(solo["log_path"].replace("best", "history")), pd.read_csv(swept["log_path"].replace("best", "history"))
    assert list(hs.columns) == list(hw.columns) and len(hs) == len(hw)
    for col in hs.columns:
        if col != "TIME:":
            assert hs[col].equals(hw[col]), (col, hs[col].tolist(), hw[col].tolist())
    sa, sb = torch.load(solo["model_path"], map_location="cpu"), torch.load(swept["model_path"], map_location="cpu")
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    return hs


@pytest.mark.parametrize("dpd_kw", [dict(DPD_backbone="dgru", DPD_hidden_size=8),
                                    dict(DPD_backbone="deltagru_tcnskip", DPD_hidden_size=15, thx=0.01, thh=0.05)], ids=["dgru8", "tres15"])
def test_swept_runs_write_the_files_of_their_solo_runs(workdir, dpd_kw):
    import opendpd_amd as od
    seeds = (0, 1, 2)
    _train_pas(seeds)
    kw = dict(n_epochs=2, lr=1e-3, **dpd_kw, **PA_KW)
    os.chdir("solo")
    solo = [_abs(od.train_dpd(seed=s, **kw)) for s in seeds]
    os.chdir(os.path.join("..", "swept"))
    swept = [_abs(r) for r in od.train_dpd_sweep(seeds=seeds, **kw)]
    assert len(swept) == len(seeds) and all(r["lockstep"] for r in swept)      # the one-launch-per-step path carried them
    assert [r["seed"] for r in swept] == list(seeds)
    for a, b in zip(solo, swept):
        hist = _same_files(a, b)
        if "delta" in dpd_kw["DPD_backbone"]:
            assert all(c in hist.columns for c in ("SP_T_DX", "SP_T_DH", "SP_T_DV", "HW_PARAM"))      # (compared with every other column)
            assert (hist["SP_T_DV"] > 0).all()


def test_hidden_sizes_form_one_group_per_shape(workdir):
    import opendpd_amd as od
    _train_pas((0, 1))
    kw = dict(n_epochs=2, lr=1e-3, DPD_backbone="dgru", **PA_KW)
    os.chdir("swept")
    swept = [_abs(r) for r in od.train_dpd_sweep(seeds=(0, 1), hidden_sizes=(8, 11), **kw)]
    assert [(r["DPD_hidden_size"], r["seed"]) for r in swept] == [(8, 0), (8, 1), (11, 0), (11, 1)]
    assert all(r["lockstep"] for r in swept)
    os.chdir(os.path.join("..", "solo"))
    solo = _abs(od.train_dpd(seed=1, DPD_hidden_size=11, **kw))
    _same_files(solo, swept[3])


def test_a_quantised_dpd_keeps_the_per_run_epoch_inside_the_loop(workdir):
    import opendpd_amd as od
    _train_pas((0, 1))
    kw = dict(n_epochs=2, lr=1e-3, DPD_backbone="qgru", DPD_hidden_size=10, quant=True, n_bits_w=8, n_bits_a=8, quant_dir_label="w8a8", **PA_KW)
    os.chdir("swept")
    swept = [_abs(r) for r in od.train_dpd_sweep(seeds=(0, 1), **kw)]
    assert len(swept) == 2 and not any(r["lockstep"] for r in swept)
    os.chdir(os.path.join("..", "solo"))
    solo = _abs(od.train_dpd(seed=1, **kw))
    _same_files(solo, swept[1])
