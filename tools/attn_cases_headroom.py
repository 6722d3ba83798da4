"""Folds the HEADROOM| lines that tests/test_gpu_attn_cases.py prints into profiles/attn_cases_headroom.txt:

    python -m pytest tests/test_gpu_attn_cases.py -q -s > attn_cases.log
    python tools/attn_cases_headroom.py attn_cases.log [commit] > profiles/attn_cases_headroom.txt

Per kernel and output the largest |got - want| / bound over the cases, with the case that set it."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _attn_cases as A  # noqa: E402

HEAD = """tests/test_gpu_attn_cases.py on one MI355X: largest |got - want| / bound per kernel and output (bound: the per-element bound of
tests/_attn_cases.py; 1.0 = at the bound), with the case that set it.  Written by tools/attn_cases_headroom.py from the HEADROOM| lines of
`pytest tests/test_gpu_attn_cases.py -q -s`%s.
bf16 outputs and the probability read-outs (P(out), P(dv)) sit just under 1 by construction: the bound of a bf16 value is mostly half an ulp
of the rounded operands and of the result itself, and round-to-nearest over 1e5 .. 1e7 elements comes arbitrarily close to half an ulp.  The
fp32 outputs (lse, delta_ws) show the real headroom of the fp32 terms.  The fused block's float64 bound carries the first-order effect of
rounding every q, k and v element (all 64 terms of a score aligned), which no input reaches: a tenth of the bound; its out_scale row is
held against the unscaled launch instead (verify_out_scale), and out_scale_differs is the fraction of scaled elements that differ from
bf16(s * out) -- 0.147 or more expected of a result rounded once (asserted: at least %.2f), 0 for one rounded twice.

constants: C_F32 = 8 x %.3f = %.3f, C_BWD = 8 x %.3f = %.3f (measured: float32 restatements without the bf16 points, 16-key tiles in
           either order, vs float64, sampled heads of every case); EXP_ULP = 1 (v_exp_f32 / v_log_f32, instruction set reference)
kernels:   attn_fwd_kernel<NKT, VAR>, attn_fwd_pair_kernel<VAR>, attn_bwd_kernel<NKT, VAR, L2 form> with the blockIdx.y extent of the launch,
           attn_block_kernel<N> ("pair": srhip_gemm_nt + srhip_attn_fwd on the block's operands, in its own bound)
"""


def main(log, commit=None):
    rows = {}
    for line in open(log):
        for m in re.finditer(r"HEADROOM\|([^|]+)\|([^|]+)\|([^|]+)\|([0-9.]+)\|(\S+)", line):
            k, _, name, r, cid = m.groups()
            if (k, name) not in rows or float(r) > rows[(k, name)][0]:
                rows[(k, name)] = (float(r), cid)

    def order(k):
        m = re.search(r"<(\d+)", k)
        return (k.startswith("attn_block"), "bwd" in k, "pair" in k, int(m.group(1)) if m else 0, k)

    out, last = [], None
    for (k, name), (r, cid) in sorted(rows.items(), key=lambda kv: (order(kv[0][0]), kv[0][1])):
        if k != last:
            out.append("\n" + k)
            last = k
        out.append("  %-18s %.3f   (%s)" % (name, r, cid))
    top = max(v[0] for (k, n), v in rows.items() if n != "out_scale_differs")
    print(HEAD % (" at commit " + commit if commit else "", A.ONCE_ROUNDED_MIN, A.C_F32_MEASURED, A.C_F32, A.C_BWD_MEASURED, A.C_BWD)
          + "\n".join(out) + "\n\nlargest of all: %.3f" % top)


if __name__ == "__main__":
    main(*sys.argv[1:3])
