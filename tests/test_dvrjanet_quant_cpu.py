"""`--quant` on dvrjanet through the C ABI, without a GPU: the descriptor {ODPD_DVRJANET, bits_w > 0, bits_a > 0, thx = num_dvr_units,
ODPD_FLAG_QUANT_CELL} selects the kernels of csrc/dvrjanet_q.hip (nine INT_Linear inside the cell); here its sizes, the refusals around it, and
the routing of `get_quant_model` for a model that is not on a HIP device.  The kernels themselves: tests/test_dvrjanet_quant_gpu.py."""
import ctypes as C
import warnings

import pytest
import torch

from tests.golden_util import Fixture

EINVAL, EUNSUPPORTED = -1, -2
FIXTURES = [("quant_dvrjanet_h12_w8a8", 8), ("quant_dvrjanet_h10_w16a16", 16)]


def _desc(bb, H, K=3.0, bits_w=8, bits_a=8, flags=None, thh=0.0):
    from opendpd_amd import _lib
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, float(K), float(thh), bits_w, bits_a, _lib.FLAG_QUANT_CELL if flags is None else flags)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from opendpd_amd import _lib
    return _lib.load()


def test_param_count_is_the_quantised_modules(lib):
    """named_parameters() of the module after the surgery: K + 7H^2 + 7H + 2 float parameters + 9 x 3 scales (the fixtures' n_param)"""
    for name, _ in FIXTURES:
        fx = Fixture(name)
        H, K = fx.meta["hidden"], fx.meta["num_dvr_units"]
        assert lib.odpd_param_count(C.byref(_desc("dvrjanet", H, K))) == fx.meta["n_param"] == {12: 1124, 10: 802}[H]
    for H in range(1, 17):
        for K in range(1, 9):
            for bits in (8, 16):
                assert lib.odpd_param_count(C.byref(_desc("dvrjanet", H, K, bits, bits))) == 7 * H * H + 7 * H + 29 + K, (H, K)


def test_sizes_of_the_split_chain_are_positive_and_there_is_no_fused_step(lib):
    from opendpd_amd import _lib
    for H, K, B, T in ((12, 3, 256, 200), (16, 8, 3, 1), (1, 1, 4096, 200), (7, 4, 1, 19662)):
        for flags in (_lib.FLAG_QUANT_CELL, _lib.FLAG_QUANT_CELL | _lib.FLAG_EVAL):      # (the module's eval mode sets ODPD_FLAG_EVAL on the descriptor)
            d = _desc("dvrjanet", H, K, flags=flags)
            assert lib.odpd_ckpt_floats(C.byref(d), B, T) > 0
            rows = lib.odpd_partial_rows(C.byref(d), B, T, 0)
            assert 0 < rows <= B
            assert lib.odpd_partial_rows(C.byref(d), B, T, 1) == EUNSUPPORTED
            assert lib.odpd_train_workspace_floats(C.byref(d), B, T) == EUNSUPPORTED
            assert lib.odpd_frozen_loss_rows(C.byref(d), B, T) == EUNSUPPORTED
            assert lib.odpd_framed_train_supported(C.byref(d)) == 0 and lib.odpd_framed_train_supported_shape(C.byref(d), B, T) == 0
            assert lib.odpd_sweep_train_supported(C.byref(d), B, T) == 0 and lib.odpd_sweep_fwd_supported(C.byref(d), B, T) == 0
            assert lib.odpd_sweep_partial_rows(C.byref(d), B, T, 0) == EUNSUPPORTED
            assert lib.odpd_sweep_workspace_floats(C.byref(d), B, T, 0) == EUNSUPPORTED
            pa = _lib.ModelDesc(_lib.BACKBONE_IDS["dgru"], 13, 0.0, 0.0, 0, 0, 0)
            assert lib.odpd_cascade_rows(C.byref(d), C.byref(pa), B, T) == EUNSUPPORTED


def test_refusals_around_the_descriptor(lib):
    from opendpd_amd import _lib
    Q = _lib.FLAG_QUANT_CELL
    bad = [_desc("dvrjanet", 17), _desc("dvrjanet", 12, 0), _desc("dvrjanet", 12, 9), _desc("dvrjanet", 12, 2.5), _desc("dvrjanet", 12, -1),
           _desc("dvrjanet", 12, 3, thh=1.0), _desc("dvrjanet", 12, 3, thh=0.5),
           _desc("dvrjanet", 12, 3, 0, 8), _desc("dvrjanet", 12, 3, 8, 0), _desc("dvrjanet", 12, 3, 0, 0), _desc("dvrjanet", 12, 3, 17, 8),
           _desc("dvrjanet", 12, 3, 8, 17), _desc("dvrjanet", 8, 0.0, 4, 0),
           _desc("dvrjanet", 12, flags=Q | _lib.FLAG_INIT_STATE), _desc("dvrjanet", 12, flags=Q | _lib.FLAG_TWO_LAYERS),
           _desc("apnrru", 8, 3), _desc("apnrru", 8, 0), _desc("mcldnn", 8, 3), _desc("mcldnn", 8, 0), _desc("bojanet", 17, 0)]
    for d in bad:
        what = (d.backbone, d.hidden, d.thx, d.thh, d.bits_w, d.bits_a, d.flags)
        assert lib.odpd_param_count(C.byref(d)) == EUNSUPPORTED, what
        assert lib.odpd_ckpt_floats(C.byref(d), 4, 20) == EUNSUPPORTED, what
        assert lib.odpd_partial_rows(C.byref(d), 4, 20, 0) == EUNSUPPORTED, what
        assert lib.odpd_partial_rows(C.byref(d), 4, 20, 1) == EUNSUPPORTED, what
        assert lib.odpd_train_workspace_floats(C.byref(d), 4, 20) == EUNSUPPORTED, what
        assert lib.odpd_frozen_loss_rows(C.byref(d), 4, 20) == EUNSUPPORTED, what
        assert lib.odpd_sweep_workspace_floats(C.byref(d), 4, 20, 0) == EUNSUPPORTED, what
        assert lib.odpd_framed_train_supported(C.byref(d)) == 0, what


def test_the_float_descriptor_and_bojanets_answer_what_they_answered(lib):
    from opendpd_amd import _lib
    for H, K in ((12, 3), (8, 4), (16, 8)):
        f = _desc("dvrjanet", H, 0.0, K, 0, flags=0)                 # the float model: bits_w carries num_dvr_units
        assert lib.odpd_param_count(C.byref(f)) == K + 7 * H * H + 7 * H + 2
        assert lib.odpd_ckpt_floats(C.byref(f), 4, 20) > 0 and lib.odpd_partial_rows(C.byref(f), 4, 20, 0) > 0
    assert lib.odpd_param_count(C.byref(_desc("dvrjanet", 17, 0.0, 4, 0, flags=0))) == EUNSUPPORTED
    for H in (1, 12, 16):                                            # bojanet's quantised descriptor: thx plays no part in it
        assert lib.odpd_param_count(C.byref(_desc("bojanet", H, 0.0))) == 2 * H * H + 28 * H + 218
    assert lib.odpd_param_count(C.byref(_desc("bojanet", 12, 0.0, flags=0))) == EINVAL
    assert lib.odpd_abi_version() == _lib.ABI_VERSION == 13


def test_a_model_on_the_cpu_keeps_the_announced_aten_route():
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import QuantBOJANET, QuantDVRJANET, get_quant_model

    class P:
        quant = True
        n_bits_w = n_bits_a = 8
        pretrained_model = ""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        q = get_quant_model(P, CoreModel(2, 12, 1, "dvrjanet", num_dvr_units=3))
    assert any("ATen restatement of the quantised model" in str(x.message) for x in w)
    assert not q.backbone.native and not isinstance(q.backbone, QuantDVRJANET)
    # what the kernel route would serve: a HIP device, hidden <= 16, 1 .. 8 DVR units, bit widths the kernels take
    net, gpu = CoreModel(2, 12, 1, "dvrjanet", num_dvr_units=3), torch.device("cuda", 0)
    assert QuantDVRJANET.serves(net, 8, 8, gpu) and QuantDVRJANET.serves(net, 16, 16, gpu) and QuantDVRJANET.serves(net, 2, 2, gpu)
    assert not QuantDVRJANET.serves(net, 8, 8, torch.device("cpu")) and not QuantDVRJANET.serves(net, 32, 8, gpu)
    assert not QuantDVRJANET.serves(net, 8, 1, gpu) and not QuantBOJANET.serves(net, 8, 8, gpu)
    assert not QuantDVRJANET.serves(CoreModel(2, 12, 1, "bojanet"), 8, 8, gpu)


@pytest.mark.parametrize("name,bits", FIXTURES)
def test_the_kernel_backed_module_has_the_aten_routes_state_dict_and_rng(name, bits):
    """QuantDVRJANET is built on the CPU before it moves to the device: its construction draws what `_quantise_aten` draws and holds the same
    state dict (the reference's, through tests/test_quant_partial_cpu.py), the descriptor carries the flag through train / eval switches"""
    import numpy as np
    from opendpd_amd import CoreModel, _lib
    from opendpd_amd.quant import QuantDVRJANET, _quantise_dvrjanet
    fx = Fixture(name)
    net = CoreModel(2, fx.meta["hidden"], 1, "dvrjanet", num_dvr_units=fx.meta["num_dvr_units"])
    net.load_state_dict({k: torch.from_numpy(fx["fsd/" + k]) for k in fx.keys("fsd")})
    torch.manual_seed(123)
    q = _quantise_dvrjanet(net, bits, bits, "", torch.device("cpu"))
    rng_after = torch.rand(4).numpy()
    assert isinstance(q.backbone, QuantDVRJANET) and q.backbone.native
    sd = q.state_dict()
    assert list(sd.keys()) == fx.keys("sd")
    for k in fx.keys("sd"):
        assert np.array_equal(sd[k].numpy(), fx["sd/" + k]), k
    assert np.array_equal(rng_after, fx["rng_after"])
    assert sum(p.numel() for p in q.parameters()) == fx.meta["n_param"] == q.backbone.n_flat
    assert int(q.backbone.frozen_mask.sum()) == 9
    d = q.backbone.desc
    assert (d.bits_w, d.bits_a, d.thx, d.thh, d.hidden) == (bits, bits, float(fx.meta["num_dvr_units"]), 0.0, fx.meta["hidden"])
    for mode in (q.eval, q.train, q.eval):
        mode()
        q.backbone.sync_mode()
        assert q.backbone.desc.flags & _lib.FLAG_QUANT_CELL and bool(q.backbone.desc.flags & _lib.FLAG_EVAL) == (not q.training)
    with pytest.raises(RuntimeError):      # no CPU fallback
        q(torch.from_numpy(fx["x"]))


def test_pretrained_model_is_loaded_before_the_swap_and_a_bad_one_returns_the_float_model(tmp_path, capsys):
    """Base_GRUQuantEnv.load_model (quant_envs.py:173-182): strict load into the float holder, then the swap keeps the weights and draws fresh
    biases; any failure warns and hands back the float model — the same for the kernel-backed module as for the ATen route"""
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import QuantDVRJANET, _quantise_aten, _quantise_dvrjanet
    torch.manual_seed(1)
    donor, net = CoreModel(2, 9, 1, "dvrjanet", num_dvr_units=5), CoreModel(2, 9, 1, "dvrjanet", num_dvr_units=5)
    good, bad = str(tmp_path / "good.pt"), str(tmp_path / "bad.pt")
    torch.save(donor.state_dict(), good)
    torch.save({k: v for k, v in list(donor.state_dict().items())[:-1]}, bad)
    torch.manual_seed(7)
    q = _quantise_dvrjanet(net, 8, 8, good, torch.device("cpu"))
    torch.manual_seed(7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = _quantise_aten(net, 8, 8, good, torch.device("cpu"))
    assert isinstance(q.backbone, QuantDVRJANET)
    sq, sa = q.state_dict(), a.state_dict()
    assert list(sq) == list(sa) and all(torch.equal(sq[k], sa[k]) for k in sq)
    for k in ("backbone.W_ph.weight", "backbone.cs"):
        assert torch.equal(sq[k], donor.state_dict()[k]) and not torch.equal(sq[k], net.state_dict()[k])
    assert _quantise_dvrjanet(net, 8, 8, bad, torch.device("cpu")) is net
    assert _quantise_dvrjanet(net, 8, 8, str(tmp_path / "missing.pt"), torch.device("cpu")) is net
    assert capsys.readouterr().out.count("[WARN] Quantization setup failed") == 2
