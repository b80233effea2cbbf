"""CoreModel.forward(x, h_0) with a given initial state, without a GPU: the ATen restatements (backbones/wide.py) reproduce the reference's
vectors with h_0 (tests/golden/h0_*.npz, tools/gen_golden_h0.py) in fp64 — they are the checker of tests/test_init_state_gpu.py —, the header
declares the state route, and a wrongly shaped h_0 is refused before any device call."""
import os
import re

import numpy as np
import pytest
import torch

from tests.golden_util import Fixture, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_FIXTURES = ["h0_gru_h8", "h0_dgru_h13", "h0_qgru_h10", "h0_qgru_amp1_h16", "h0_lstm_h9", "h0_gru_h40", "h0_lstm_h48"]


def restatement(fx):
    """the fp64 ATen restatement of the fixture's backbone, loaded with its state dict"""
    from opendpd_amd.backbones import wide as W
    m = fx.meta
    mod = W.build(m["backbone"], 2, m["hidden"], 1).double()
    mod.load_state_dict({k[len("backbone."):]: torch.from_numpy(fx["sd/" + k]).double() for k in fx.keys("sd")})
    return mod


@pytest.mark.parametrize("name", STATE_FIXTURES)
def test_restatement_reproduces_the_reference_with_h0(name):
    fx = Fixture(name)
    mod = restatement(fx)
    x = torch.from_numpy(fx["x"]).double().requires_grad_(True)
    h0 = torch.from_numpy(fx["h0"]).double().requires_grad_(True)
    y = mod(x, h0)
    loss = torch.nn.functional.mse_loss(y, torch.from_numpy(fx["tgt"]).double())
    loss.backward()
    assert rel_err(y.detach().numpy(), fx["y"]) < 2e-6
    assert abs(loss.item() - fx["loss"][0]) < 1e-6 * max(1.0, fx["loss"][0])
    assert rel_err(h0.grad.numpy(), fx["gh0"]) < 2e-5
    assert rel_err(x.grad.numpy(), fx["gx"]) < 2e-5
    for k, p in mod.named_parameters():
        assert rel_err(p.grad.numpy(), fx["g/backbone." + k]) < 2e-5, k
    # the state matters: from zero the output is another one
    with torch.no_grad():
        assert rel_err(mod(x, torch.zeros_like(h0)).numpy(), fx["y"]) > 1e-3


@pytest.mark.parametrize("name", ["h0_deltagru_tcnskip_h15", "h0_vdlstm_h8"])
def test_reference_ignores_h0_on_these_backbones(name):
    fx = Fixture(name)
    assert np.array_equal(fx["y"], fx["y_none"])


def test_header_declares_the_state_route():
    from opendpd_amd import _lib
    header = open(os.path.join(ROOT, "include", "opendpd_hip.h")).read()
    assert re.search(r"#define ODPD_FLAG_INIT_STATE 8\b", header) and _lib.FLAG_INIT_STATE == 8
    for sym in ("odpd_backbone_fwd_state", "odpd_backbone_bwd_state"):
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.exported_symbols()


@pytest.mark.parametrize("bb", ["gru", "dgru", "qgru", "qgru_amp1", "lstm"])
def test_wrong_h0_shape_raises_before_any_device_call(bb, monkeypatch):
    from opendpd_amd import CoreModel, _lib

    def no_device(*a, **k):
        raise AssertionError("the shape check must come before any device call")

    monkeypatch.setattr(_lib, "load", no_device)
    net = CoreModel(2, 8, 1, bb)
    x = torch.rand(2, 5, 2)
    for shape in ((1, 3, 8), (2, 2, 8), (1, 2, 7), (2, 8)):
        with pytest.raises(RuntimeError, match=re.escape(f"Expected hidden size (1, 2, 8), got {list(shape)}")):
            net(x, torch.ones(shape))
