"""Register budget of the kernel behind the last block's class-row launch (no GPU: hipcc's resource remarks for gfx950).
The row-pitch variant of the fused proj + MLP kernel is an instantiation of its own; the kernel every other launch takes must compile to what
it was, and the new one must fit the same budget."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semireward_amd", "csrc")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("remarks")
    cache = {}

    def get(src):
        if src in cache:
            return cache[src]
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c",
                            "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp / "o.o"), os.path.join(CSRC, src)],
                           capture_output=True, text=True, cwd=str(tmp))
        assert r.returncode == 0, r.stderr[-2000:]
        out, cur = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
            m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).strip()] = int(m.group(2))
        cache[src] = out
        return out
    return get


def test_every_fused_mlp_instantiation_keeps_two_waves_and_no_scratch(remarks):
    mlp = {k: v for k, v in remarks("mlp_fused.hip").items() if "mlp_fused_kernel" in k}
    # template arguments <384, 0, 4, PROJ, SPREAD, PITCH>: the kernel with a backward's rows, the two dense PROJ schedules, the row-pitch one
    assert sorted(k.split("mlp_fused_kernelILi384ELi0ELi4E")[1][:12] for k in mlp) == ["Lb0ELi0ELb0E", "Lb1ELi0ELb0E", "Lb1ELi1ELb0E", "Lb1ELi1ELb1E"]
    for k, v in mlp.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["Occupancy [waves/SIMD]"] >= 2, (k, v)
    # the dense kernel of every other launch is the code it was before the pitch existed: 255 registers (with the pitch as a run-time field
    # of the one instantiation it allocated 251, i.e. different code for the 22 full-size launches of a step)
    shipped = [v for k, v in mlp.items() if "Lb1ELi1ELb0E" in k]
    assert len(shipped) == 1 and shipped[0]["VGPRs"] == 255, shipped
