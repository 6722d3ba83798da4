"""profiles/enc_cases_headroom.txt from the 'headroom' lines of `pytest tests/test_gpu_enc_cases.py -q -s -m gpu`:
    python tools/enc_cases_headroom.py <pytest output> > profiles/enc_cases_headroom.txt
Largest |got - want| / bound per kernel and output, with the case that set it."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _enc_cases as E          # noqa: E402


def group_of(cid):
    for _, c in E.all_cases():
        if c["id"] == cid:
            k = re.sub(r"(?<!,) ", " / ", c["kernel"])
            return k.replace("/ part", "(srhip_postln_bwd_part)").replace("/ dyn", "(srhip_adamw_flat_dyn)").replace("/ by-value", "(srhip_adamw_flat)")
    return cid


def main(path):
    best = collections.defaultdict(dict)
    summary = ""
    for line in open(path):
        if " passed" in line or " failed" in line or " error" in line:
            summary = line.strip().strip("= ")                 # pytest's last line
        w = line.lstrip(".F").split()
        if len(w) == 4 and w[0] == "headroom":
            g, key, v = group_of(w[1]), w[2], float(w[3])
            if v >= best[g].get(key, (-1.0, ""))[0]:
                best[g][key] = (v, w[1])
    print("""tests/test_gpu_enc_cases.py on one MI355X: largest |got - want| / bound per kernel (template and entry point) and output (bound: the per-element
bound of tests/_enc_cases.py; 1.0 = at the bound), with the case that set it.  Written by tools/enc_cases_headroom.py from the 'headroom' lines
of `pytest tests/test_gpu_enc_cases.py -q -s -m gpu`, whose last line was: %s
%s
A bf16 output (xb, dxb) sits just under 1 by construction: half a bf16 ulp is the bound's largest term, and some element always lands next to a
rounding tie.  same_bits: every output of the case is held to the same bits (dropout_cast, mask_lengths) and has no figure; so are, in every
case, the dropped elements, dword[pad_id], the filler rows of meanpool_bwd, pb, the EMA, coef_out[0], g after either zero_grad, the frozen
tensor, dyn against by-value, dx aliasing dy, the constant LayerNorm rows and everything a launch must not write.

constants (measured on float32 restatements against float64 in two summation orders, times 8; tests/test_cpu_enc_cases.py measures them afresh):
%s
intrinsics: no document of the ROCm installation states an accuracy for erff, expf or rsqrtf (searched: its share/ and include/hip), so the
           allowances are 8 times the worst error in ulps of torch's float32 erf, exp and rsqrt against float64 over the arguments the cases
           hand them (source: measurement):
%s
""" % (summary or "(missing: the log is incomplete)",
       "Every case passed: no kernel is outside its bound." if summary and "failed" not in summary and "error" not in summary else
       "NOT every case passed: the figures below are those of the cases that reached their last assertion.",
       "\n".join("           %s = 8 x %.3f" % (k, getattr(E, k + "_MEASURED")) for k in E.NAMES if k.startswith("C_")),
       "\n".join("           %s = 8 x %.3f" % (k, getattr(E, k + "_MEASURED")) for k in E.NAMES if not k.startswith("C_"))))
    for g in sorted(best):
        print(g)
        for key, (v, cid) in sorted(best[g].items()):
            print("  %-12s %8.4f   (%s)" % (key, v, cid))
        print()


if __name__ == "__main__":
    main(sys.argv[1])
