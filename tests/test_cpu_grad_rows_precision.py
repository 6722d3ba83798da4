"""grad_rows_precision (the numeric mode of the rows that carry the backward) without a GPU: option parsing and validation, which backbones
declare the split-bf16 backward."""
import argparse

import pytest


def _args(**kw):
    return argparse.Namespace(**kw)


def test_option_validation(monkeypatch):
    from semireward_amd.algorithms.srflexmatch import backbone_class, grad_rows_precision
    from semireward_amd.nets import bert, hubert, vit, wave2vec, wrn
    monkeypatch.delenv("SR_GRAD_ROWS_PRECISION", raising=False)
    nets = [vit.VisionTransformer, bert.ClassificationBert, wave2vec.ClassificationWave2Vec, hubert.ClassificationHubert, wrn.WideResNet]
    for cls in nets:
        assert grad_rows_precision(_args(), cls) == "bf16"
        assert grad_rows_precision(_args(grad_rows_precision="bf16"), cls) == "bf16"
        with pytest.raises(ValueError):
            grad_rows_precision(_args(grad_rows_precision="fp32"), cls)
    assert grad_rows_precision(_args(grad_rows_precision="bf16x3"), vit.VisionTransformer) == "bf16x3"
    for cls in nets[1:]:
        with pytest.raises(NotImplementedError, match=cls.__name__):
            grad_rows_precision(_args(grad_rows_precision="bf16x3"), cls)
    # the environment variable is the fallback of a missing args field (bench.py), the args field wins
    monkeypatch.setenv("SR_GRAD_ROWS_PRECISION", "bf16x3")
    assert grad_rows_precision(_args(), vit.VisionTransformer) == "bf16x3"
    assert grad_rows_precision(_args(grad_rows_precision="bf16"), vit.VisionTransformer) == "bf16"
    assert grad_rows_precision(_args(grad_rows_precision="bf16"), bert.ClassificationBert) == "bf16"
    with pytest.raises(NotImplementedError):
        grad_rows_precision(_args(), wrn.WideResNet)
    monkeypatch.setenv("SR_GRAD_ROWS_PRECISION", "half")
    with pytest.raises(ValueError):
        grad_rows_precision(_args(), vit.VisionTransformer)
    # the two options are independent: neither reads the other's field or variable
    monkeypatch.delenv("SR_GRAD_ROWS_PRECISION")
    monkeypatch.setenv("SR_READ_ROWS_PRECISION", "bf16x3")
    assert grad_rows_precision(_args(read_rows_precision="bf16x3"), vit.VisionTransformer) == "bf16"
    assert backbone_class(vit.vit_base_patch16_96) is vit.VisionTransformer


def test_backbones_declare_the_backward():
    from semireward_amd.nets import bert, hubert, surface, vit, wave2vec, wrn
    assert surface.ModuleSurface.precise_grad_rows is False
    assert vit.VisionTransformer.precise_grad_rows is True
    for cls in (bert.ClassificationBert, wave2vec.ClassificationWave2Vec, hubert.ClassificationHubert, wrn.WideResNet):
        assert cls.precise_grad_rows is False, cls.__name__


@pytest.mark.parametrize("bad", ["fp32", "bf16x2", ""])
def test_validation_comes_before_device_work(monkeypatch, bad):
    """The algorithm refuses a bad value or an unsupported backbone in its constructor before the backbone is built."""
    from semireward_amd.algorithms import get_algorithm
    from semireward_amd.nets import vit, wrn
    monkeypatch.delenv("SR_GRAD_ROWS_PRECISION", raising=False)
    built = []

    def vit_builder(*a, **k):
        built.append(1)
        raise AssertionError("the backbone must not be built")
    vit_builder.__module__ = vit.__name__

    def wrn_builder(*a, **k):
        built.append(1)
        raise AssertionError("the backbone must not be built")
    wrn_builder.__module__ = wrn.__name__
    args = _args(algorithm="srflexmatch", grad_rows_precision=bad, num_classes=10)
    with pytest.raises(ValueError):
        get_algorithm(args, vit_builder)
    args = _args(algorithm="srflexmatch", grad_rows_precision="bf16x3", num_classes=10)
    with pytest.raises(NotImplementedError, match="WideResNet"):
        get_algorithm(args, wrn_builder)
    assert not built
