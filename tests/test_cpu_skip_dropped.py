"""The numpy reference of the DropPath plan (tests/_droppath_plan_cases.py) on the cases the device kernel is compared with it on
(tests/test_gpu_skip_dropped.py): its defining properties, checked without the reference's own sort."""
import numpy as np
import pytest

import _droppath_plan_cases as C


def test_a_plan_written_out_by_hand():
    K = C.KEPT
    dp = np.array([[[0, 0, 0, 0, 0], [K, 0, K, 0, K]],          # mixed: 0, 2, 4 keep the MLP branch (branch 0 does not matter)
                   [[K, K, K, K, K], [0, 0, 0, 0, 0]],          # everything dropped
                   [[0, 0, 0, 0, 0], [1, 1, K, 1, 1]]], dtype=np.float32)      # nothing dropped (1.0 = the factor of block 0)
    want = np.array([[3, 0, 2, 4, 1, 3], [0, 0, 1, 2, 3, 4], [5, 0, 1, 2, 3, 4]], dtype=np.int32)
    assert np.array_equal(C.plan_ref(dp), want)


@pytest.mark.parametrize("depth", C.DEPTHS)
@pytest.mark.parametrize("B", C.BATCHES)
def test_reference_plan_is_a_stable_partition(B, depth):
    t = C.table(depth, B)
    C.check_plan(C.plan_ref(t), t)
    # the cases hold what they are meant to hold: a block with nothing dropped, one with everything dropped, and (B > 1) mixed ones
    kept = (t[:, 1] != 0).sum(axis=1)
    assert kept[0] == B and kept[1] == 0
    if depth == 12 and B > 1:
        assert ((kept > 0) & (kept < B)).sum() >= 4
    # the column slice of the wider table is the same table, with the opposite decisions around it
    w = C.wide_table(depth, B)
    assert np.array_equal(w[:, :, C.MARGIN:C.MARGIN + B], t)
    assert ((w[:, :, C.MARGIN - 1] != 0) != (t[:, :, 0] != 0)).all() and ((w[:, :, C.MARGIN + B] != 0) != (t[:, :, -1] != 0)).all()
    assert np.array_equal(C.plan_ref(w[:, :, C.MARGIN:C.MARGIN + B]), C.plan_ref(t))


def test_a_negative_zero_factor_counts_as_dropped():
    dp = np.zeros((1, 2, 3), dtype=np.float32)
    dp[0, 1] = [-0.0, C.KEPT, 0.0]
    assert C.plan_ref(dp).tolist() == [[1, 1, 0, 2]]


def _resource_remarks(src, tmp_path):
    """hipcc's resource remarks for gfx950 of one source file: {mangled kernel name: {figure: value}}; no GPU."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "semireward_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(root, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"), os.path.join(csrc, src)],
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
    return out


def test_attention_kernel_with_the_early_exit_keeps_its_register_budget(tmp_path):
    """attn_block_kernel sits at 256 / 238 VGPRs; the exit for a dropped image in front of it must not push anything into scratch (a spilled
    value is reloaded behind s_waitcnt vmcnt(0), which drains the weight ring)."""
    ab = {k: v for k, v in _resource_remarks("attn_block.hip", tmp_path).items() if "attn_block_kernel" in k}
    assert len(ab) == 4                      # N = 257 and 197, each with the refills behind the barrier and spread over the stages
    for k, v in ab.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["Occupancy [waves/SIMD]"] >= 2, (k, v)


def test_planned_fused_mlp_kernel_fits_the_budget_of_the_dense_one(tmp_path):
    """mlp_planned_kernel (the row-mapped proj + MLP launch) shares its body with mlp_fused_kernel: no scratch, nothing spilled, at most 256
    VGPRs, two waves per SIMD -- and the dense kernel beside it is still the 255-register code of every other launch."""
    rm = _resource_remarks("mlp_fused.hip", tmp_path)
    planned = {k: v for k, v in rm.items() if "mlp_planned_kernel" in k}
    assert len(planned) == 1
    for k, v in planned.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 256 and v["Occupancy [waves/SIMD]"] >= 2, (k, v)
    dense = [v for k, v in rm.items() if "mlp_fused_kernelILi384ELi0ELi4ELb1ELi1ELb0E" in k]
    assert len(dense) == 1 and dense[0]["VGPRs"] == 255 and dense[0]["ScratchSize [bytes/lane]"] == 0, dense
