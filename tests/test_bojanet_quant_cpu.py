"""`--quant` on bojanet through the C ABI, without a GPU: the descriptor {ODPD_BOJANET, bits_w > 0, bits_a > 0, ODPD_FLAG_QUANT_CELL} selects the
kernels of csrc/bojanet_q.hip (eight INT_Linear inside the cell); here its sizes, the refusals around it, and the routing of `get_quant_model`
for a model that is not on a HIP device.  The kernels themselves: tests/test_bojanet_quant_gpu.py."""
import ctypes as C
import warnings

import pytest
import torch

from tests.golden_util import Fixture

EINVAL, EUNSUPPORTED = -1, -2


def _desc(bb, H, bits_w=8, bits_a=8, flags=None):
    from opendpd_amd import _lib
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb], H, 0.0, 0.0, bits_w, bits_a, _lib.FLAG_QUANT_CELL if flags is None else flags)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from opendpd_amd import _lib
    return _lib.load()


def test_flag_constant_matches_the_header():
    import os
    import re
    from opendpd_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "opendpd_hip.h")).read()
    assert int(re.search(r"#define ODPD_FLAG_QUANT_CELL (\d+)", header).group(1)) == _lib.FLAG_QUANT_CELL == 16


def test_param_count_is_the_quantised_modules(lib):
    """named_parameters() of the module after the surgery: 2H^2 + 28H + 194 float parameters + 8 x 3 scales (the fixtures' n_param)"""
    for name, H in (("quant_bojanet_h12_w8a8", 12), ("quant_bojanet_h16_w16a16", 16)):
        assert lib.odpd_param_count(C.byref(_desc("bojanet", H))) == Fixture(name).meta["n_param"] == {12: 842, 16: 1178}[H]
    for H in range(1, 17):
        for bits in (8, 16):
            assert lib.odpd_param_count(C.byref(_desc("bojanet", H, bits, bits))) == 2 * H * H + 28 * H + 218, H


def test_sizes_of_the_split_chain_are_positive_and_there_is_no_fused_step(lib):
    from opendpd_amd import _lib
    for H, B, T in ((12, 256, 200), (16, 3, 15), (1, 4096, 200), (7, 1, 19662)):
        for flags in (_lib.FLAG_QUANT_CELL, _lib.FLAG_QUANT_CELL | _lib.FLAG_EVAL):      # (the module's eval mode sets ODPD_FLAG_EVAL on the descriptor)
            d = _desc("bojanet", H, flags=flags)
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


def test_the_flag_is_refused_everywhere_else(lib):
    from opendpd_amd import _lib
    bad = [_desc("bojanet", 17), _desc("bojanet", 18), _desc("gru", 11), _desc("gru", 11, 0, 0), _desc("pgjanet", 11), _desc("apnrru", 8),
           _desc("dvrjanet", 8, 4, 0), _desc("bojanet", 12, 0, 0), _desc("bojanet", 12, 8, 0), _desc("bojanet", 12, 17, 8), _desc("bojanet", 12, 8, 17),
           _desc("bojanet", 12, flags=_lib.FLAG_QUANT_CELL | _lib.FLAG_INIT_STATE), _desc("gru", 11, 0, 0, flags=_lib.FLAG_QUANT_CELL | _lib.FLAG_INIT_STATE),
           _desc("bojanet", 12, flags=_lib.FLAG_QUANT_CELL | _lib.FLAG_TWO_LAYERS), _desc("gru", 11, 0, 0, flags=_lib.FLAG_QUANT_CELL | _lib.FLAG_TWO_LAYERS)]
    for d in bad:
        what = (d.backbone, d.hidden, d.bits_w, d.bits_a, d.flags)
        assert lib.odpd_param_count(C.byref(d)) == EUNSUPPORTED, what
        assert lib.odpd_ckpt_floats(C.byref(d), 4, 20) == EUNSUPPORTED, what
        assert lib.odpd_partial_rows(C.byref(d), 4, 20, 0) == EUNSUPPORTED, what
        assert lib.odpd_partial_rows(C.byref(d), 4, 20, 1) == EUNSUPPORTED, what
        assert lib.odpd_train_workspace_floats(C.byref(d), 4, 20) == EUNSUPPORTED, what
        assert lib.odpd_frozen_loss_rows(C.byref(d), 4, 20) == EUNSUPPORTED, what
        assert lib.odpd_sweep_workspace_floats(C.byref(d), 4, 20, 0) == EUNSUPPORTED, what
        assert lib.odpd_framed_train_supported(C.byref(d)) == 0, what


def test_without_the_flag_the_answers_are_unchanged(lib):
    from opendpd_amd import _lib
    d = _desc("bojanet", 12, flags=0)                                # bits_w > 0 on bojanet without the flag: refused outright, never the float kernels
    assert lib.odpd_param_count(C.byref(d)) == EINVAL and lib.odpd_partial_rows(C.byref(d), 4, 20, 0) == EINVAL
    assert lib.odpd_ckpt_floats(C.byref(d), 4, 20) == EINVAL
    f = _desc("bojanet", 12, 0, 0, flags=0)                          # the float model
    assert lib.odpd_param_count(C.byref(f)) == 2 * 144 + 28 * 12 + 194
    assert lib.odpd_ckpt_floats(C.byref(f), 4, 20) > 0 and lib.odpd_partial_rows(C.byref(f), 4, 20, 0) > 0
    assert lib.odpd_param_count(C.byref(_desc("bojanet", 17, 0, 0, flags=0))) == EUNSUPPORTED
    assert lib.odpd_param_count(C.byref(_desc("pgjanet", 11, flags=0))) == 977      # the other model with quantised layers inside the cell
    assert lib.odpd_abi_version() == _lib.ABI_VERSION == 13


def test_a_model_on_the_cpu_keeps_the_announced_aten_route():
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import QuantBOJANET, get_quant_model

    class P:
        quant = True
        n_bits_w = n_bits_a = 8
        pretrained_model = ""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        q = get_quant_model(P, CoreModel(2, 12, 1, "bojanet"))
    assert any("ATen restatement of the quantised model" in str(x.message) for x in w)
    assert not q.backbone.native and not isinstance(q.backbone, QuantBOJANET)
    # what the kernel route would serve: a HIP device, hidden <= 16, bit widths the kernels take
    net = CoreModel(2, 12, 1, "bojanet")
    assert QuantBOJANET.serves(net, 8, 8, torch.device("cuda", 0)) and QuantBOJANET.serves(net, 16, 16, torch.device("cuda", 0))
    assert not QuantBOJANET.serves(net, 8, 8, torch.device("cpu")) and not QuantBOJANET.serves(net, 32, 8, torch.device("cuda", 0))
    assert not QuantBOJANET.serves(net, 8, 1, torch.device("cuda", 0))


def test_the_kernel_backed_module_has_the_aten_routes_state_dict_and_rng():
    """QuantBOJANET is built on the CPU before it moves to the device: its construction draws what `_quantise_aten` draws and holds the same
    state dict (the reference's, through tests/test_quant_partial_cpu.py), the descriptor carries the flag through train / eval switches"""
    import numpy as np
    from opendpd_amd import CoreModel, _lib
    from opendpd_amd.quant import QuantBOJANET, _quantise_bojanet
    for name, bits in (("quant_bojanet_h12_w8a8", 8), ("quant_bojanet_h16_w16a16", 16)):
        fx = Fixture(name)
        net = CoreModel(2, fx.meta["hidden"], 1, "bojanet")
        net.load_state_dict({k: torch.from_numpy(fx["fsd/" + k]) for k in fx.keys("fsd")})
        torch.manual_seed(123)
        q = _quantise_bojanet(net, bits, bits, "", torch.device("cpu"))
        rng_after = torch.rand(4).numpy()
        assert isinstance(q.backbone, QuantBOJANET) and q.backbone.native
        sd = q.state_dict()
        assert list(sd.keys()) == fx.keys("sd")
        for k in fx.keys("sd"):
            assert np.array_equal(sd[k].numpy(), fx["sd/" + k]), k
        assert np.array_equal(rng_after, fx["rng_after"])
        assert sum(p.numel() for p in q.parameters()) == fx.meta["n_param"] == q.backbone.n_flat
        assert int(q.backbone.frozen_mask.sum()) == 8
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
    from opendpd_amd.quant import QuantBOJANET, _quantise_aten, _quantise_bojanet
    torch.manual_seed(1)
    donor, net = CoreModel(2, 9, 1, "bojanet"), CoreModel(2, 9, 1, "bojanet")
    good, bad = str(tmp_path / "good.pt"), str(tmp_path / "bad.pt")
    torch.save(donor.state_dict(), good)
    torch.save({k: v for k, v in list(donor.state_dict().items())[:-1]}, bad)
    torch.manual_seed(7)
    q = _quantise_bojanet(net, 8, 8, good, torch.device("cpu"))
    torch.manual_seed(7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = _quantise_aten(net, 8, 8, good, torch.device("cpu"))
    assert isinstance(q.backbone, QuantBOJANET)
    sq, sa = q.state_dict(), a.state_dict()
    assert list(sq) == list(sa) and all(torch.equal(sq[k], sa[k]) for k in sq)
    assert torch.equal(sq["backbone.W_fh.weight"], donor.state_dict()["backbone.W_fh.weight"])
    assert not torch.equal(sq["backbone.W_fh.weight"], net.state_dict()["backbone.W_fh.weight"])
    assert _quantise_bojanet(net, 8, 8, bad, torch.device("cpu")) is net
    assert _quantise_bojanet(net, 8, 8, str(tmp_path / "missing.pt"), torch.device("cpu")) is net
    assert capsys.readouterr().out.count("[WARN] Quantization setup failed") == 2
