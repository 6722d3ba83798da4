"""Every kernel of csrc/enc_ops.hip and csrc/optim.hip on the MI355X, element by element against float64: the cases, references, bounds and verify
functions of tests/_enc_cases.py, which tests/test_cpu_enc_cases.py shows accepting the float32 restatement of every case and rejecting each
planted fault.  No tuning variable is set: the shapes reach each template by the dispatchers' own rules.
Each test prints 'headroom <id> <output> <max |got - want| / tol>' (profiles/enc_cases_headroom.txt keeps the largest per kernel and output)."""
import pytest
import torch

import _enc_cases as E
from semireward_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = lambda cs: [c["id"] for c in cs]          # noqa: E731


def run(cls, c):
    L = cls(c, DEV)
    L.run_hip()
    torch.cuda.synchronize()
    H = L.verify()
    for k, v in sorted(H.items()):
        print("headroom %s %s %.4f" % (c["id"], k, v))
    if not H:
        print("headroom %s same_bits 0.0000" % c["id"])             # (every output of the case is held to the same bits)
    assert all(v <= 1.0 for v in H.values()), H


@pytest.mark.parametrize("c", E.EMBED_CASES, ids=IDS(E.EMBED_CASES))
def test_embed_ln_case(c):
    run(E.EmbedLaunch, c)


@pytest.mark.parametrize("c", E.PLN_FWD_CASES, ids=IDS(E.PLN_FWD_CASES))
def test_postln_fwd_case(c):
    run(E.PlnFwdLaunch, c)


@pytest.mark.parametrize("c", E.PLN_BWD_CASES, ids=IDS(E.PLN_BWD_CASES))
def test_postln_bwd_case(c):
    run(E.PlnBwdLaunch, c)


@pytest.mark.parametrize("c", E.POOL_CASES, ids=IDS(E.POOL_CASES))
def test_meanpool_case(c):
    run(E.PoolLaunch, c)


@pytest.mark.parametrize("c", E.GELU_CASES, ids=IDS(E.GELU_CASES))
def test_gelu_case(c):
    run(E.GeluLaunch, c)


@pytest.mark.parametrize("c", E.CAST_CASES, ids=IDS(E.CAST_CASES))
def test_dropout_cast_case(c):
    run(E.CastLaunch, c)


@pytest.mark.parametrize("c", E.MASK_CASES, ids=IDS(E.MASK_CASES))
def test_mask_lengths_case(c):
    run(E.MaskLaunch, c)


@pytest.mark.parametrize("c", E.ADAM_CASES, ids=IDS(E.ADAM_CASES))
def test_adamw_flat_case(c):
    run(E.AdamLaunch, c)


@pytest.mark.parametrize("c", E.CLIP_CASES, ids=IDS(E.CLIP_CASES))
def test_clip_grad_coef_case(c):
    run(E.ClipLaunch, c)


def test_refused_arguments_raise_and_write_nothing():
    """SR_EINVAL reaches the caller as a RuntimeError naming the entry point; nothing is launched, so the outputs keep their contents."""
    O = E.Out(DEV)
    M, D = 8, 256
    f = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    x, xb, mean, rstd = O.new("x", (M, 768)), O.new("xb", (M, 768), torch.bfloat16), O.new("mean", (M,)), O.new("rstd", (M,))
    part = O.new("part", (2, 2, 768))
    ids = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    calls = {
        "embed_ln_fwd D=256": lambda: ops.embed_ln_fwd(ids, None, f(4, D), f(4, D), f(2, D), f(D), f(D), 1e-12, x, xb, mean, rstd, 2, 4, D),
        "embed_ln_bwd D=256": lambda: ops.embed_ln_bwd(f(M, D), ids, None, f(4, D), f(4, D), f(2, D), f(M), f(M), f(D), x, x, x, x, x, 2, 4, D, 0),
        "postln_fwd D=256": lambda: ops.postln_fwd(f(M, D), f(D), f(D), 1e-12, x, xb, mean, rstd, M, D),
        "postln_bwd D=256": lambda: ops.postln_bwd(f(M, D), f(M, D), f(M), f(M), f(D), x, xb, mean, rstd, M, D),
        "postln_bwd_part D=256": lambda: ops.postln_bwd_part(f(M, D), f(M, D), f(M), f(M), f(D), x, xb, part, 2, M, D),
        "postln_fwd without x and without statistics": lambda: ops.postln_fwd(f(M, 128), f(128), f(128), 1e-12, None, xb, None, None, M, 128),
        "postln_bwd_part n_rep=0": lambda: ops.postln_bwd_part(f(M, 128), f(M, 128), f(M), f(M), f(128), x, xb, part, 0, M, 128),
        "dropout_cast odd n": lambda: ops.dropout_cast(f(16), xb, 7),
    }
    for what, call in calls.items():
        with pytest.raises(RuntimeError, match="invalid argument"):
            call()
        print("refused: " + what)
    torch.cuda.synchronize()
    O.check("refused arguments")
    for name, (buf, _) in O.bufs.items():
        assert E.is_pattern(buf), name
