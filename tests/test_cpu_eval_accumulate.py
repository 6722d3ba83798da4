"""csrc/eval.hip, host side (no GPU): the kernels of srhip_eval_accumulate as the compiler leaves them for gfx950."""
import os
import re
import shutil
import subprocess


def test_eval_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """The four instantiations (16-byte / scalar loads x register-resident / re-read rows) fit a 1024-thread workgroup: no scratch, no spills."""
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    assert hipcc is not None, "hipcc not found: the HIP extension cannot be built either (semireward_amd/build.py)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "semireward_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(root, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"), os.path.join(csrc, "eval.hip")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    assert len(out) == 4 and all("eval_accumulate_kernel" in n for n in out), sorted(out)
    for n, v in out.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (n, v)
        assert v["VGPRs"] <= 128, (n, v)                                    # 1024 threads = 4 waves per SIMD: at most 128 registers each
