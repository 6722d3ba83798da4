"""profiles/wrn_cases_headroom.txt from the 'headroom' / 'count' lines of `pytest tests/test_gpu_wrn_cases.py -q -s -m gpu`:
    python tools/wrn_cases_headroom.py <pytest output> > profiles/wrn_cases_headroom.txt
Largest |got - want| / bound per kernel (or convolution template) and output, with the case that set it."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _wrn_cases as WC          # noqa: E402

FAMILY = [("h-", "wrn_head_kernel"), ("bn-", "bn_reduce_kernel<false> / bn_fold_kernel / bn_apply_kernel / bn_act_kernel"),
          ("bwd-", "bn_reduce_kernel<true> / bn_bwd_apply_kernel"), ("im-", "im2col_kernel / im2col_bn_kernel / col2im_kernel"),
          ("fc-", "fc_fwd_kernel / fc_bwd_x_kernel / fc_bwd_w_kernel"), ("pool-", "avgpool_fwd_kernel"), ("sgd-", "sgd_flat_kernel"),
          ("w-", "conv_weight_prep[_grouped]_kernel / add_unpad[_grouped]_kernel"), ("flip-", "conv_weight_flip_grouped_kernel")]
FORM = {0: "given mean / invstd", 1: "running statistics", 2: "raw input", 3: "statistics folded from in_acc"}


def group_of(cid):
    for c in WC.CONV_CASES:
        if c["id"] == cid:
            return "%s, %s%s" % (c["kernel"], "input-gradient form" if c["flip"] else FORM[c["mode"]], ", %d passes" % c["shape"][7] if c["shape"][7] > 1 else "")
    return next(name for prefix, name in FAMILY if cid.startswith(prefix))


def main(path):
    best = collections.defaultdict(dict)
    ulp1 = collections.Counter()
    summary = ""
    for line in open(path):
        if " passed" in line or " failed" in line or " error" in line:
            summary = line.strip().strip("= ")                 # pytest's last line
        w = line.lstrip(".F").split()
        if len(w) == 4 and w[0] == "headroom":
            g, key, v = group_of(w[1]), w[2], float(w[3])
            if v >= best[g].get(key, (-1.0, ""))[0]:
                best[g][key] = (v, w[1])
        elif len(w) == 4 and w[0] == "count":
            ulp1[group_of(w[1])] += int(w[3])
    print("""tests/test_gpu_wrn_cases.py on one MI355X: largest |got - want| / bound per kernel (convolution: per template and input form) and output
(bound: the per-element bound of tests/_wrn_cases.py; 1.0 = at the bound), with the case that set it.  Written by tools/wrn_cases_headroom.py
from the 'headroom' lines of `pytest tests/test_gpu_wrn_cases.py -q -s -m gpu`, whose last line was: %s
%s
y of a convolution whose input goes through the BatchNorm sits just under 1 by construction: where the kernel rounded an activation near a
bf16 tie the other way, the difference IS the operand term of the bound; y_clean is the same figure over the outputs without an operand term
-- the headroom of the accumulation.  'mean' (the published mean against float64, bound: one rounding) is between 0.5 and 1 by construction.
var_far: the variance the next BatchNorm derives from acc_out on the far-from-zero channel (mean / std about 30), in units of its bound
C_SUM 2^-24 (E[y^2] + 2 |m| E|y|): what the fp32 per-lane partial sums cost there.  frac_w / frac_amb are shares of elements (with more than
one admissible bf16 value / that may take either derivative), not headrooms.  The filter layouts (conv_weight_prep[_grouped],
conv_weight_flip_grouped, add_unpad[_grouped]), im2col, avgpool_bwd, nchw_to_nhwc_bf16, dx_bf16 and the EMA of sgd_flat are held to the same
bits and have no figure.

constants: C_ACC = 8 x %.3f, C_R = 8 x %.3f, C_SUM = 8 x %.3f, C_BWD = 8 x %.3f, C_SGD = 8 x %.3f (measured on float32 restatements against
           float64: tests/test_cpu_wrn_cases.py measures them afresh)
published invstd / running statistics one ulp from the numpy statement of bn_finalize: %d of all cases (0: every one has the same bits)
""" % (summary or "(missing: the log is incomplete)",
       "Every case passed: no kernel is outside its bound." if summary and "failed" not in summary and "error" not in summary else
       "NOT every case passed: the figures below are those of the cases that reached their last assertion.",
       WC.C_ACC_MEASURED, WC.C_R_MEASURED, WC.C_SUM_MEASURED, WC.C_BWD_MEASURED, WC.C_SGD_MEASURED, sum(ulp1.values())))
    for g in sorted(best):
        print(g)
        for key, (v, cid) in sorted(best[g].items()):
            print("  %-12s %8.4f   (%s)" % (key, v, cid))
        print()


if __name__ == "__main__":
    main(sys.argv[1])
