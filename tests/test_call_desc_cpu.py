"""A backbone's descriptor is never written after construction (backbones/native.py): `desc` hands out a fresh odpd_model_t of the module as it
stands, `call_desc(need_dx, init_state)` the cached, read-only one of a single call, and every buffer FusedAdamW hands out is sized by the
descriptor of the call that will use it.  No device: the size queries run on the host, and the library — asked through a hand-built
odpd_model_t with the same fields — is the reference for every size here."""
import ctypes as C
import itertools

import pytest
import torch

SHAPES = ((3, 20), (19, 65), (300, 20))
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from opendpd_amd import _lib
    return _lib.load()


def _quantised(bb, H):
    from opendpd_amd import CoreModel
    from opendpd_amd.quant import _quantise_bojanet, get_quant_model

    class P:
        quant = True
        n_bits_w = n_bits_a = 8
        pretrained_model = ""
    if bb == "bojanet":      # (as tests/test_bojanet_quant_cpu.py builds the kernel-backed module without a device)
        return _quantise_bojanet(CoreModel(2, H, 1, bb), 8, 8, "", CPU)
    return get_quant_model(P, CoreModel(2, H, 1, bb))


def _models():
    """id -> (build, the structural fields of its odpd_model_t: hidden, thx, thh, bits_w, bits_a, flags; delta model; mode selects a kernel)"""
    from opendpd_amd import CoreModel, _lib
    f = lambda bb, H, L=1, thx=0.0, thh=0.0: (lambda: CoreModel(2, H, L, bb, thx=thx, thh=thh))
    return {
        "gru": (f("gru", 11), (11, 0.0, 0.0, 0, 0, 0), False, False),
        "gru-2-layers": (f("gru", 11, 2), (11, 0.0, 0.0, 0, 0, _lib.FLAG_TWO_LAYERS), False, False),
        "dgru": (f("dgru", 13), (13, 0.0, 0.0, 0, 0, 0), False, False),
        "lstm": (f("lstm", 9), (9, 0.0, 0.0, 0, 0, 0), False, False),
        "deltagru": (f("deltagru", 15, 1, 0.01, 0.05), (15, 0.01, 0.05, 0, 0, 0), True, False),
        "deltagru_tcnskip": (f("deltagru_tcnskip", 15, 1, 0.01, 0.05), (15, 0.01, 0.05, 0, 0, 0), True, False),
        "deltajanet": (f("deltajanet", 12, 1, 0.01, 0.05), (12, 0.0, 0.0, 0, 0, 0), True, False),      # (its layer runs with thresholds 0)
        "bojanet-w8a8": (lambda: _quantised("bojanet", 12), (12, 0.0, 0.0, 8, 8, _lib.FLAG_QUANT_CELL), False, True),
        "qgru-w8a8": (lambda: _quantised("qgru", 10), (10, 0.0, 0.0, 8, 8, 0), False, True),      # (a model whose eval() changes the answers)
    }


MODELS = ["gru", "gru-2-layers", "dgru", "lstm", "deltagru", "deltagru_tcnskip", "deltajanet", "bojanet-w8a8", "qgru-w8a8"]


def _hand_built(bb, fields, extra=0):
    from opendpd_amd import _lib
    H, thx, thh, bits_w, bits_a, flags = fields
    return _lib.ModelDesc(_lib.BACKBONE_IDS[bb.backbone_name], H, thx, thh, bits_w, bits_a, flags | extra)


def _fields(d):
    return (d.backbone, d.hidden, d.thx, d.thh, d.bits_w, d.bits_a, d.flags)


def _answers(lib, d, B, T):
    """the four size queries concerned, as the library answers them for this descriptor (sizes or error codes)"""
    return (int(lib.odpd_ckpt_floats(C.byref(d), B, T)), int(lib.odpd_partial_rows(C.byref(d), B, T, 0)),
            int(lib.odpd_partial_rows(C.byref(d), B, T, 1)), int(lib.odpd_train_workspace_floats(C.byref(d), B, T)))


def _modes(net, selects):
    """the modes a model is held in: train, and eval too where the mode selects a kernel — (switch, ODPD_FLAG_EVAL expected)"""
    from opendpd_amd import _lib
    return ((net.train, 0), (net.eval, _lib.FLAG_EVAL), (net.train, 0)) if selects else ((net.train, 0), (net.eval, 0))


@pytest.mark.parametrize("name", MODELS)
def test_desc_is_fresh_and_call_desc_states_the_selection(lib, name):
    from opendpd_amd import _lib
    build, fields, delta, selects = _models()[name]
    net = build()
    bb = net.backbone
    assert bb.native and bb.dx_needs_flag == delta
    for switch, eval_flag in _modes(net, selects):
        switch()
        want = _fields(_hand_built(bb, fields, eval_flag))
        assert _fields(bb.desc) == want      # exactly the structural bits, plus ODPD_FLAG_EVAL as the mode says
        before = bytes(bb.desc)
        for need_dx, init_state in itertools.product((False, True), repeat=2):
            d = bb.call_desc(need_dx=need_dx, init_state=init_state)
            extra = (_lib.FLAG_NEED_DX if need_dx and delta else 0) | (_lib.FLAG_INIT_STATE if init_state else 0)
            assert _fields(d) == _fields(_hand_built(bb, fields, eval_flag | extra))
            assert bb.call_desc(need_dx=need_dx, init_state=init_state) is d      # cached: nothing is built per call
            for B, T in SHAPES:
                assert _answers(lib, d, B, T) == _answers(lib, _hand_built(bb, fields, eval_flag | extra), B, T)
        assert bb.call_desc() is bb.call_desc(need_dx=False, init_state=False)
        assert bytes(bb.desc) == before
        mine = bb.desc
        mine.flags |= _lib.FLAG_NEED_DX | _lib.FLAG_INIT_STATE
        mine.hidden += 1
        assert bytes(bb.desc) == before and _fields(bb.call_desc()) == want


def _check_sizes(lib, opt, bb, d, B, T, pa=None, pd=None):
    """what the optimiser hands out on the CPU for (B, T) against the library's answers for the hand-built descriptors `d` (trained model) and
    `pd` (frozen PA): a size where the library gives one, a RuntimeError where it answers with an error code"""
    from opendpd_amd import _lib
    ck, rows_bwd, rows_fused, ws = _answers(lib, d, B, T)
    cols = bb.n_flat + _lib.LOSS_COLS
    for method, rows in ((opt.partials, rows_fused), (opt.bwd_partials, rows_bwd)):
        if rows < 0:
            with pytest.raises(RuntimeError, match="odpd_partial_rows failed"):
                method(B, T, CPU)
        else:
            assert tuple(method(B, T, CPU).shape) == (rows, cols)
    assert opt.has_fused(B, T) == (rows_fused > 0)
    if ws < 0:
        with pytest.raises(RuntimeError, match="odpd_train_workspace_floats failed"):
            opt.train_workspace(B, T, CPU)
    else:
        got = opt.train_workspace(B, T, CPU)
        if ws > 0:
            assert got.dtype == torch.float32 and tuple(got.shape) == (ws,)
        elif bb.dx_needs_flag or getattr(bb, "fused_stats", False):      # no scratch: the four sparsity counters
            assert got.dtype == torch.float64 and tuple(got.shape) == (4,)
        else:
            assert got is None
    if ck < 0:
        with pytest.raises(RuntimeError, match="odpd_ckpt_floats failed"):
            opt.cascade_buffers(B, T, CPU)
        return
    buf = opt.cascade_buffers(B, T, CPU)
    assert tuple(buf["ck_d"].shape) == (max(ck, 1),) and tuple(buf["u"].shape) == (B, T, 2)
    if pa is not None:
        ck_p, rows_p = _answers(lib, pd, B, T)[:2]
        assert tuple(buf["ck_p"].shape) == (max(ck_p, 1),)
        if pa.dx_needs_flag:
            assert tuple(buf["pa_part"].shape) == (rows_p, pa.n_flat + _lib.LOSS_COLS)
        frozen_rows = int(lib.odpd_frozen_loss_rows(C.byref(pd), B, T))
        assert (buf["loss_rows"] is None) == (frozen_rows <= 0)
        if frozen_rows > 0:
            assert tuple(buf["loss_rows"].shape) == (frozen_rows, _lib.LOSS_COLS)
        one = opt.cascade_one_launch(B, T, CPU)
        casc = int(lib.odpd_cascade_rows(C.byref(d), C.byref(pd), B, T))
        assert (one is None) == (casc <= 0) and (one is None or tuple(one.shape) == (casc, cols))


@pytest.mark.parametrize("name", MODELS)
def test_optimiser_buffers_are_the_librarys_sizes(lib, name):
    """.. under the built-in knobs, after a knob moved the generation, and after train() -> eval() -> train() where the mode selects a kernel:
    no cached buffer outlives the selection it was sized for"""
    from opendpd_amd import _lib
    from opendpd_amd.train_funcs import FusedAdamW
    build, fields, delta, selects = _models()[name]
    net = build()
    bb = net.backbone
    opt = FusedAdamW(net)
    before = bytes(bb.desc)
    try:
        for knob in (-1, 0, 1 << 30):      # the built-in value, the 16-sequences-per-wave kernels for every batch, for none
            _lib.check(lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(knob)), "odpd_set_tuning")
            for switch, eval_flag in _modes(net, selects):
                switch()
                for B, T in SHAPES:
                    _check_sizes(lib, opt, bb, _hand_built(bb, fields, eval_flag), B, T)
    finally:
        lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1))
    net.train()
    assert bytes(bb.desc) == before


@pytest.mark.parametrize("pa_name", ["deltagru", "gru"])
def test_cascade_buffers_are_sized_by_both_models_call_descriptors(lib, pa_name):
    """a dgru DPD in front of a frozen PA: the PA's checkpoint and scratch rows are those of ITS call — with ODPD_FLAG_NEED_DX where it is a
    delta model, whatever an autograd-style request on the PA module asked for in between"""
    from opendpd_amd import CascadedModel, CoreModel, _lib
    from opendpd_amd.train_funcs import FusedAdamW
    build, pa_fields, delta, _ = _models()[pa_name]
    dpd, pa = CoreModel(2, 8, 1, "dgru"), build()
    net = CascadedModel(dpd_model=dpd, pa_model=pa)
    net.freeze_pa_model()
    opt = FusedAdamW(net)
    d = _hand_built(dpd.backbone, (8, 0.0, 0.0, 0, 0, 0))
    pd = _hand_built(pa.backbone, pa_fields, _lib.FLAG_NEED_DX if delta else 0)
    before = bytes(dpd.backbone.desc), bytes(pa.backbone.desc)
    try:
        for knob in (-1, 0):
            _lib.check(lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(knob)), "odpd_set_tuning")
            for B, T in SHAPES:
                pa.backbone.call_desc(need_dx=False), pa.backbone.call_desc(need_dx=True, init_state=True)      # other callers' selections
                _check_sizes(lib, opt, dpd.backbone, d, B, T, pa.backbone, pd)
    finally:
        lib.odpd_set_tuning(b"s16_min_batch", C.c_int64(-1))
    assert (bytes(dpd.backbone.desc), bytes(pa.backbone.desc)) == before
