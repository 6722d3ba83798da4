"""CPU-only checks of the merged weight-gradient launch (srhip_gemm_tn_grouped_tail_f32): the binding's struct is the header's, bad tails are
refused before anything is launched, and the kernel that carries the tail keeps the register budget of the plain 128 x 128 kernel."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_struct_matches_the_header():
    from semireward_amd import _lib
    src = open(os.path.join(ROOT, "include", "srhip.h")).read()
    body = re.search(r"typedef struct srhip_dw_tail \{(.*?)\} srhip_dw_tail;", src, flags=re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[;,]", body)
    assert names == [n for n, _ in _lib.DwTail._fields_], names
    assert ctypes.sizeof(_lib.DwTail) == 12 * 8 + 8 * 4 == 128
    n_ptr = len(re.findall(r"\*", body))
    assert n_ptr == 12 and all(t is ctypes.c_void_p for _, t in _lib.DwTail._fields_[:12])


def test_bad_tails_are_refused_without_a_launch():
    from semireward_amd import _lib
    lib = _lib.lib()
    f = lib.srhip_gemm_tn_grouped_tail_f32
    one = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused on its arguments

    def rc(**kw):
        t = _lib.DwTail()
        t.D = 384
        for k, v in kw.items():
            setattr(t, k, v)
        return f(one, 1, 1, 1.0, 1.0, ctypes.addressof(t), None)
    assert f(one, 1, 1, 1.0, 1.0, None, None) == -1                               # no tail
    assert f(None, 1, 1, 1.0, 1.0, ctypes.addressof(_lib.DwTail()), None) == -1   # no table (and D = 0)
    assert rc(D=0) == -1
    assert rc(n_ln=2, n_rep=16) == -1                                            # LayerNorm copies without their table
    assert rc(C=10, B=2) == -1                                                   # head without operands
    assert rc(C=10, B=0, dlogits=4096, feat=4096, dWh=4096, dbh=4096) == -1
    pe = dict(dx=4096, img=4096, dpos=4096, dcls=4096, pe_ws=4096, B=2, in_chans=3, HW=32, ps=2)
    assert rc(**dict(pe, ps=0)) == -1 and rc(**dict(pe, HW=33)) == -1             # ps is tested before HW % ps
    assert rc(**dict(pe, ps=16)) == -1                                            # K = 768 taps: not the small-patch kernels' shape
    assert rc(**dict(pe, pe_ws=None)) == -1 and rc(**dict(pe, B=0)) == -1
    assert rc(**dict(pe, D=100)) == -1
    assert lib.srhip_patch_embed_bwd_fold(None, one, one, 2, 3, 32, 2, 384, None) == -1
    assert lib.srhip_patch_embed_bwd_fold(one, one, one, 2, 3, 32, 16, 384, None) == -1


def test_tail_kernel_keeps_the_tile_kernels_register_budget(tmp_path):
    """Three workgroups per CU is what the tile count of the ViT-S table is planned against (768 slots); the tail's bodies must not cost the
    tiles a register, and nothing may go to scratch."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "semireward_amd", "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "o.o"),
                        os.path.join(csrc, "gemm_tn.hip")], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    plain = [v for k, v in out.items() if "gemm_tn_grouped_f32_kernel" in k]
    tail = [v for k, v in out.items() if "gemm_tn_grouped_tail_f32_kernel" in k]
    assert len(plain) == 1 and len(tail) == 1
    for v in plain + tail:
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["Occupancy [waves/SIMD]"] >= 3, v
        assert v["LDS Size [bytes/block]"] == 49152, v
    assert tail[0]["VGPRs"] <= plain[0]["VGPRs"] + 8, (tail[0], plain[0])
