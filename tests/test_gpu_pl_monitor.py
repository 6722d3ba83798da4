"""srhip_pl_monitor (csrc/pl_monitor.hip) against the numpy restatement of tests/_pl_monitor_cases.py: every integer exactly, the fp64 sums
within 2^-39 relative, run-to-run bits, accumulation over launches, sentinels around both state blocks, the label-error flag and the
argument checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pl_monitor_cases as PC                 # noqa: E402
from semireward_amd import _lib, ops          # noqa: E402
from semireward_amd.core.pl_monitor import PlMonitor   # noqa: E402

DEV = "cuda:0"
# fp64 sums: at most 2^13 additions of non-negative terms, each rounding 2^-53 relative to the running sum, in the kernel and in the
# restatement alike: 2 * 2^13 * 2^-53
SUM_BOUND = 2.0 ** -39
SENTINEL = 0x5EEDFACE0BADBEEF
_REF = {}


def case_and_ref(P, nu, C, **kw):
    """A case and its restatement, computed once and shared (treated as read-only)."""
    key = (P, nu, C, tuple(sorted(kw.items())))
    if key not in _REF:
        case = PC.make_case(P, nu, C, **kw)
        _REF[key] = (case, PC.restate(case))
    return _REF[key]


def fresh_state(C):
    """[sentinel | istate | sentinel sentinel | fstate | sentinel] in one int64 buffer: (buffer, istate view, fstate view)."""
    W = ops.pl_monitor_words(C)
    buf = torch.zeros(W + ops.PL_SUMS + 4, dtype=torch.int64, device=DEV)
    buf[0] = buf[W + 1] = buf[W + 2] = buf[W + 7] = SENTINEL
    return buf, buf[1:W + 1], buf[W + 3:W + 7].view(torch.float64)


def read_state(buf, C):
    W = ops.pl_monitor_words(C)
    h = buf.cpu().numpy()
    assert [int(h[i]) for i in (0, W + 1, W + 2, W + 7)] == [SENTINEL] * 4, "a sentinel word beside the state was overwritten"
    assert not h[14:17].any()                                  # the reserved header words are never written
    words = np.concatenate([h[1:W + 1], h[W + 3:W + 7]])
    return PlMonitor.state_from_words(words, C), words.tobytes()


def dev(a, offset=False):
    """The array on the device; offset: a view one element past an aligned base (4 bytes off for fp32: the scalar-load path)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(DEV)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.to(DEV)
    v = buf[1:]
    assert v.data_ptr() % 16 == t.element_size() % 16
    return v


def launch(case, state, offset=False, launches=1):
    _, ist, fst = state
    P, nu, C = case["P"], case["nu"], case["C"]
    a = dict(pseudo=dev(case["pseudo"]), m0=dev(case["masks"][0], offset), mk=dev(case["masks"][P - 1], offset), m2=dev(case["mask2"], offset),
             r=dev(case["reward"], offset), idx=dev(case["idx_ulb"]), tg=dev(case["targets"]))
    for _ in range(launches):
        ops.pl_monitor(a["pseudo"], a["m0"], a["mk"], a["m2"], a["r"], a["idx"], a["tg"], P, nu, C, ist, fst)


def run(case, offset=False, launches=1):
    st = fresh_state(case["C"])
    launch(case, st, offset, launches)
    return read_state(st[0], case["C"])


def check(got, want, what, scale=1):
    diff = PC.state_equal_ints(got, {k: (v * scale if k != "flag" else v) for k, v in want.items()})
    assert not diff, (what, {k: (got[k], want[k]) for k in diff})
    sums = [("sum_w", got["sum_w"], want["sum_w"]), ("sum_w_correct", got["sum_w_correct"], want["sum_w_correct"]),
            ("sum_r[0]", got["sum_r"][0], want["sum_r"][0]), ("sum_r[1]", got["sum_r"][1], want["sum_r"][1])]
    for name, g, w in sums:
        w = w * scale
        print("pl_monitor %s: %s %.17g (restatement %.17g, rel %.2e)" % (what, name, g, w, abs(g - w) / max(abs(w), 1e-300)))
        assert abs(g - w) <= SUM_BOUND * abs(w), (what, name, g, w)


@pytest.mark.parametrize("P,nu,C", PC.SHAPES, ids=["%dx%dx%d" % s for s in PC.SHAPES])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_shapes_against_the_restatement(P, nu, C, soft):
    ops.check_label_errors()
    case, want = case_and_ref(P, nu, C, soft=soft)
    assert P * nu <= 2 ** 13 and not want["flag"]
    got, bits = run(case)
    check(got, want, "%dx%dx%d %s" % (P, nu, C, "soft" if soft else "hard"))
    ops.check_label_errors()                                    # no flag
    # the scalar-load path (reward / mask2 four bytes past an aligned base): the same bits
    got_u, bits_u = run(case, offset=True)
    assert bits_u == bits
    # the same launch again: the same bits; three launches into one state: three times the counts (fp64 sums within the bound)
    assert run(case)[1] == bits
    got3, _ = run(case, launches=3)
    check(got3, want, "3 launches", scale=3)
    ops.check_label_errors()


def test_contents_cover_the_edges():
    """What the cases are said to hold: unknown rows, mask2 zeros, the bin-edge rewards and a NaN, soft weights."""
    case, want = case_and_ref(9, 56, 100, soft=True)
    r = case["reward"]
    assert np.isnan(r).sum() == 1 and (r == 0).any() and (r == 1).any() and want["reward_bad"] <= 1
    for k in range(1, 32):
        e = np.float32(k / 32.0)
        assert (r == e).any() and (r == np.nextafter(e, np.float32(0))).any()
    assert (case["mask2"] == 0).any() and want["rows_unknown"] > 0 and want["m2"] < want["gen_rows"]
    assert any(0 < v < 1 for v in case["masks"][8]) and want["sum_w"] < want["sel"] and want["hist"].sum() > 300
    assert want["sel_correct"] > 0 and want["sel_correct"] < want["sel"] < want["rows"]


def test_every_row_unknown():
    case, want = case_and_ref(3, 40, 7, unknown=1.0)
    got, _ = run(case)
    assert want["rows_unknown"] == 40 and want["rows"] == 0
    check(got, want, "all unknown")
    assert got["steps"] == 1 and got["rows_unknown"] == 40 and not got["hist"].any() and got["sum_w"] == 0.0
    ops.check_label_errors()


@pytest.mark.parametrize("bad", ["idx=-1", "idx=n_ulb", "target=C", "idx=2^40", "target=2^40"])
@pytest.mark.parametrize("P,nu,C", [(1, 7, 10), (3, 5, 4), (2, 40, 3000)])
def test_out_of_range_rows_set_the_flag_and_touch_no_counter(bad, P, nu, C):
    ops.check_label_errors()
    good, _ = case_and_ref(P, nu, C)
    case = dict(good, idx_ulb=good["idx_ulb"].copy(), targets=good["targets"].copy())
    j = nu // 2
    if bad.startswith("idx"):
        case["idx_ulb"][j] = {"idx=-1": -1, "idx=n_ulb": case["n_ulb"], "idx=2^40": 1 << 40}[bad]
    else:
        case["targets"][case["idx_ulb"][j]] = C if bad == "target=C" else 1 << 40
    want = PC.restate(case)
    assert want["flag"]
    got, _ = run(case)
    with pytest.raises(IndexError, match="monitor"):
        ops.check_label_errors()
    ops.check_label_errors()                                    # reset by the failed check
    check(got, want, bad)
    # the other rows are counted as if the bad row were not in the batch
    keep = np.arange(nu) != j
    sub = dict(good, nu=nu - 1, idx_ulb=good["idx_ulb"][keep], pseudo=good["pseudo"].reshape(P, nu)[:, keep].reshape(-1),
               masks=[m[keep] for m in good["masks"]],
               mask2=None if P == 1 else good["mask2"].reshape(P - 1, nu)[:, keep].reshape(-1),
               reward=None if P == 1 else good["reward"].reshape(P - 1, nu)[:, keep].reshape(-1))
    alone = PC.restate(sub)
    assert not PC.state_equal_ints(got, alone)


def test_invalid_arguments_return_the_error_code_without_a_launch():
    f = _lib.lib().srhip_pl_monitor
    case, _ = case_and_ref(3, 5, 4)
    P, nu, C = 3, 5, 4
    buf, ist, fst = fresh_state(C)
    t = dict(pseudo=dev(case["pseudo"]), m0=dev(case["masks"][0]), mk=dev(case["masks"][2]), m2=dev(case["mask2"]), r=dev(case["reward"]),
             idx=dev(case["idx_ulb"]), tg=dev(case["targets"]))
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(pseudo=t["pseudo"].data_ptr(), m0=t["m0"].data_ptr(), mk=t["mk"].data_ptr(), m2=t["m2"].data_ptr(), r=t["r"].data_ptr(),
              idx=t["idx"].data_ptr(), tg=t["tg"].data_ptr(), n_ulb=case["n_ulb"], P=P, nu=nu, C=C, ist=ist.data_ptr(), fst=fst.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["pseudo"], a["m0"], a["mk"], a["m2"], a["r"], a["idx"], a["tg"], a["n_ulb"], a["P"], a["nu"], a["C"], a["ist"], a["fst"], s)
    for kw in (dict(pseudo=None), dict(m0=None), dict(mk=None), dict(idx=None), dict(tg=None), dict(ist=None), dict(fst=None), dict(P=0),
               dict(P=-1), dict(nu=0), dict(C=0), dict(n_ulb=0), dict(m2=None), dict(r=None), dict(m2=None, r=None),
               dict(ist=ist.data_ptr() + 4), dict(fst=fst.data_ptr() + 4), dict(P=1 << 20, nu=1 << 20)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    got, _ = read_state(buf, C)
    assert got["steps"] == 0 and not got["hist"].any() and got["rows"] == 0
    assert call(P=1, m2=None, r=None) == 0                       # K = 0 takes NULL mask2 / reward
    assert call() == 0
    got, _ = read_state(buf, C)
    assert got["steps"] == 2
    ops.check_label_errors()


def test_class_reads_one_copy_and_resets_the_window():
    case, want = case_and_ref(9, 56, 100, soft=True)
    mon = PlMonitor(case["targets"], 100, DEV, case["n_ulb"])
    masks = [dev(m) for m in case["masks"]]
    args = (8, masks, dev(case["pseudo"]), dev(case["reward"]), dev(case["mask2"]), dev(case["idx_ulb"]))
    mon.accumulate(*args)
    mon.accumulate(*args)
    peek = mon.read(reset=False)
    check(peek, want, "PlMonitor x2", scale=2)
    assert mon.read(reset=True)["rows"] == peek["rows"] and mon.read()["steps"] == 0 and not mon.block.any()
    vals = mon.log_values(5)
    mon.accumulate(*args)
    m = PlMonitor.metrics_from_state(want)
    for k, v in vals.items():
        assert float(v) == pytest.approx(m[k], rel=1e-12), k
    assert not mon.block.any()                                   # the log line's read started the next window
    with pytest.raises(ValueError, match="idx_ulb"):
        mon.accumulate(8, masks, args[2], args[3], args[4], None)
