"""Resume == the run that never stopped, for SRFlexMatch on the tiny WideResNet (classic_cv: SGD, EMA, every model() call moving the BatchNorm
running statistics and num_batches_tracked): the check of tests/test_gpu_resume.py, whose helpers it uses, on the configuration that file does
not have."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_resume as R                   # noqa: E402

NAME = "srflexmatch_wrn"
CASE = (dict(algorithm="srflexmatch", optim="SGD", lr=0.03, momentum=0.9, weight_decay=1e-3, layer_decay=1.0, ema_m=0.999, p_cutoff=0.12), "wrn")


def test_resume_equals_the_uninterrupted_run_srflexmatch_wrn(tmp_path, monkeypatch):
    monkeypatch.setitem(R.CASES, NAME, CASE)
    a = R.build(NAME)
    for i in range(6):                        # it = 0 .. 5: stage-1 updates, start_timing = 3 (K = sr_decay() passes from it = 4), the N_k boundary at it = 4
        R.step(a, NAME, i)
    torch.cuda.synchronize()
    nbt = int(a.model.buffers["bn1.num_batches_tracked"])
    assert nbt > 6                            # K + 1 model() calls per step moved it, not one
    a.it -= 1
    a.save_model("latest_model.pth", str(tmp_path))
    a.it += 1
    saved = R.state_of(a)
    b = R.build(NAME)
    b.load_model(str(tmp_path / "latest_model.pth"))
    loaded = R.state_of(b)
    assert set(saved) == set(loaded) and any(k.endswith("num_batches_tracked") for k in saved)
    for k in saved:
        assert torch.equal(saved[k], loaded[k]), k
    ma, mb = [], []
    for i in range(6, 9):
        R.step(a, NAME, i, ma)
        R.step(b, NAME, i, mb)
    torch.cuda.synchronize()
    for (m1, p1), (m2, p2) in zip(ma, mb):
        assert len(m1) == len(m2) >= 2
        assert all(torch.equal(x, y) for x, y in zip(m1, m2))
        assert p1 is None or torch.equal(p1, p2)
    sa, sb = R.state_of(a), R.state_of(b)
    assert int(sa["buffer.bn1.num_batches_tracked"]) == int(sb["buffer.bn1.num_batches_tracked"]) > nbt
    for k in sa:
        if sa[k].dtype in (torch.int64, torch.int32, torch.bool) or not bool(torch.isfinite(sa[k]).all()):
            assert torch.equal(sa[k], sb[k]), k
            continue
        if k.startswith("hook."):
            assert torch.allclose(sa[k], sb[k], rtol=1e-5, atol=1e-7), k
            continue
        num, den = float((sa[k].double() - sb[k].double()).norm()), float(sa[k].double().norm()) + 1e-30
        assert num / den <= 1e-6, (k, num / den)
