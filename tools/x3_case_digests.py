"""SHA-256 of every output arena's bits (padding included) of every launch of tests/_x3_cases.py, one line per case and output:

    python tools/x3_case_digests.py <tree root> > digests.txt

The cases, arenas and the library (semireward_amd/libsrhip.so) are the ones of <tree root>, so the listings of two built trees can be set
side by side: a change that keeps the x3 kernels' arithmetic gives identical listings (profiles/x3_one_engine.txt)."""
import hashlib
import os
import sys

ROOT = os.path.abspath(sys.argv[1])
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _x3_cases as X  # noqa: E402


def emit(cid, names, arenas):
    for n, a in zip(names, arenas):
        print("%s %s %s" % (cid, n, hashlib.sha256(a.bits().tobytes()).hexdigest()))


def main():
    assert os.path.dirname(os.path.abspath(X.__file__)) == os.path.join(ROOT, "tests") and X.ops.__file__.startswith(ROOT + os.sep)
    for c in X.GEMM_CASES:
        L = X.GemmLaunch(c, "cuda")
        L.run_hip()
        emit(c["id"], ("C", "aux_out"), L.outs)
    for ln in X.TN_LAUNCHES:
        L = X.TnLaunch(ln, "cuda")
        L.run_hip()
        emit(ln["id"], ["C%d" % i for i in range(len(L.P))] + ["dbias%d" % i for i, p in enumerate(L.P) if p["aD"] is not None], L.outs)
    for c in X.ATTN_CASES:
        L = X.AttnLaunch(c["id"], "cuda")
        L.run_fwd()
        emit(c["id"], ("out", "out_lse", "lse"), (L.out, L.out2, L.lse))
        L.run_bwd()
        emit(c["id"], ("dqkv", "delta_ws"), (L.dqkv, L.delta))


if __name__ == "__main__":
    main()
