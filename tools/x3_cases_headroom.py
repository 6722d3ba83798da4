"""Folds the HEADROOM| lines that tests/test_gpu_x3_cases.py prints into profiles/x3_cases_headroom.txt:

    python -m pytest tests/test_gpu_x3_cases.py -q -s > x3_cases.log
    python tools/x3_cases_headroom.py x3_cases.log [commit] > profiles/x3_cases_headroom.txt

Per kernel, form and statement the largest |got - want| / bound over the cases, with the case that set it."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _x3_cases as X  # noqa: E402

HEAD = """tests/test_gpu_x3_cases.py on one MI355X: largest |got - want| / bound per kernel, form and statement (bound: the per-element bound of
tests/_x3_cases.py; 1.0 = at the bound), with the case that set it.  Written by tools/x3_cases_headroom.py from the HEADROOM| lines of
`pytest tests/test_gpu_x3_cases.py -q -s`%s.
':spec' is statement (1), the kernel against the float64 value of ah.bh + ah.bl + al.bh with the fp32 accumulation bound C_X3 2^-24 S3: the
real headroom of the kernels' arithmetic.  ':true' is statement (2), against the float64 product a.b with E = |al||bl| + |ra||b| + |a||rb|
added: E carries no constant and is attained wherever the residues of a short product share a sign, so these rows sit below 1 by the
cancellation inside E only (the float32 restatement reads the same).  The attention rows mix both kinds of term.

constants: C_X3 = 8 x %.3f = %.3f, C_ATT_F = 8 x %.3f = %.3f, C_ATT_B = 8 x %.3f = %.3f, C_FN = 8 x %.3f = %.3f, DGELU_ABS = 8 x %.3e
           (float32 restatements over 32-wide k-chunks in either order against float64); FN_ULP = %g ulp assumed for expf / logf / erff
"""


def main(log, commit=None):
    rows = {}
    for line in open(log):
        for m in re.finditer(r"HEADROOM\|([^|]+)\|([^|]+)\|([^|]+)\|([0-9.]+)\|(\S+)", line):
            k, form, name, r, cid = m.groups()
            if (k, form, name) not in rows or float(r) > rows[(k, form, name)][0]:
                rows[(k, form, name)] = (float(r), cid)
    out, last = [], None
    for (k, form, name), (r, cid) in sorted(rows.items()):
        if k != last:
            out.append("\n" + k)
            last = k
        out.append("  %-10s %-18s %.3f   (%s)" % (form, name, r, cid))
    spec = max(v[0] for (k, f, n), v in rows.items() if not n.endswith(":true"))
    print(HEAD % (" at commit " + commit if commit else "", X.C_X3_MEASURED, X.C_X3, X.C_ATT_F_MEASURED, X.C_ATT_F, X.C_ATT_B_MEASURED, X.C_ATT_B,
                  X.C_FN_MEASURED, X.C_FN, X.DGELU_ABS_MEASURED, X.FN_ULP)
          + "\n".join(out) + "\n\nlargest of all: %.3f; largest outside statement (2): %.3f" % (max(v[0] for v in rows.values()), spec))


if __name__ == "__main__":
    main(*sys.argv[1:3])
