"""The hyper-parameters of FusedSGD / FusedRMSprop / FusedAdam other than `lr` are constants of the fused kernels (the reference's own,
project.py:274-297).  They are marshalled for the library in one place, FusedAdamW._hyper, which refuses an edited one on every path that
passes them on — a single step, sharded or not, and the three native epoch loops — before any library call."""
import pytest


@pytest.fixture()
def sgd(monkeypatch):
    """FusedSGD over a native model with an edited momentum, and a library that must not be reached"""
    from opendpd_amd import CoreModel, _lib
    from opendpd_amd.train_funcs import FusedSGD
    opt = FusedSGD(CoreModel(2, 13, 1, "dgru"), lr=1e-3)
    opt.param_groups[0]["momentum"] = 0.5

    def no_library():
        raise AssertionError("the library was reached before the hyper-parameters were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    return opt


@pytest.mark.parametrize("path", ["train_epoch", "train_epoch_cascade", "train_epoch_split"])
def test_an_edited_momentum_is_refused_before_an_epoch_loop(sgd, path):
    with pytest.raises(NotImplementedError, match="only 'lr' can be changed"):
        getattr(sgd, path)(object(), "l2", 0.0)      # (the loader is not looked at either)
    assert sgd.step_count == 0


def test_an_edited_momentum_is_refused_before_a_step_sharded_or_not(sgd):
    for comm in (None, object()):
        with pytest.raises(NotImplementedError, match="only 'lr' can be changed"):
            sgd.apply(0.0, stream=0, comm=comm)
    assert sgd.step_count == 0


def test_lr_is_the_one_hyper_parameter_the_other_optimisers_take():
    from opendpd_amd import CoreModel, _lib
    from opendpd_amd.train_funcs import FusedAdamW, FusedRMSprop, FusedSGD
    net = CoreModel(2, 13, 1, "dgru")
    assert FusedSGD(net, lr=1e-3)._hyper() == (_lib.OPTIMIZER_IDS["sgd"], 1e-3, 0.0, 0.0, 0.0, 0.0)
    assert FusedAdamW(net, lr=2e-3, betas=(0.8, 0.9), eps=1e-7, weight_decay=0.1)._hyper() == (-1, 2e-3, 0.8, 0.9, 1e-7, 0.1)
    opt = FusedRMSprop(net)
    opt.param_groups[0]["lr"] = 0.25      # (what a scheduler does)
    assert opt._hyper()[:2] == (_lib.OPTIMIZER_IDS["rmsprop"], 0.25)
    opt.param_groups[0]["alpha"] = 0.9
    with pytest.raises(NotImplementedError, match="alpha"):
        opt._hyper()
