"""The 32x32 SGEMM tile with four K-groups runs two workgroups per CU on the forward product of the MNIST MLP, and its K loop -
like every loop of csrc/gemm_tile_body.inc - keeps K-tiles in flight in registers that inline-asm buffer loads write behind the
compiler's back: a spilled ring register would be saved before its load has landed.  So the instantiations the MLP step and
tiny-BERT launch (one product, and three products on one operand: XT = 1) must use no scratch, and the wave-private K loop must
not cost registers: before it existed the cooperative instantiations <32, 32, 16, 1, 1, true, true, true, true, 2, 4, 0> and
<..., 2, 4, 1> took 100 registers per lane (84 + 16 accumulators) and 0 bytes of scratch; that figure is the bound for them and
for their wave-private counterparts.  The loop of the wave-private form must contain no workgroup barrier: the one barrier of
the kernel is the K-group exchange behind it.  hipcc cross-compiles without a GPU: only these kernels are compiled here."""
import os
import re
import shutil
import subprocess
import pytest
from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")
PARENT_VGPRS = 100


def wave_private_prefetch():
    text = open(os.path.join(CSRC, "gemm.hip")).read()
    return int(re.search(r"#define LG_WAVE_PRIVATE_PD (\d+)", text).group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_k_group_tile_keeps_its_registers_and_has_no_barrier_in_the_loop(tmp_path):
    pd = wave_private_prefetch()
    coop = ["sgemm_mfma<32, 32, 16, 1, 1, true, true, true, true, 2, 4, %d>" % xt for xt in (0, 1)]
    private = ["sgemm_mfma<32, 32, 16, 1, 1, true, true, true, true, %d, 4, %d, true>" % (pd, xt) for xt in (0, 1)]
    text = open(os.path.join(CSRC, "gemm.hip")).read()
    cut = text.index("// Two independent products in ONE launch")
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    unit = tmp_path / "pkg" / "csrc" / "kgroups_only.hip"
    unit.write_text(text[:cut] + "".join("template __global__ void %s(GemmArgs);\n" % k for k in coop + private) + "}  // namespace lg\n")
    out = tmp_path / "kgroups.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), "kgroups_only.hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)
    assert len(kernels) == 4, [k for k, _ in kernels]
    for name, body in kernels:
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        print(name, "vgprs", vgprs, "scratch", scratch, "lds", lds)
        assert scratch == 0, "%s: %d bytes of scratch per lane" % (name, scratch)
        assert vgprs <= PARENT_VGPRS, "%s: %d registers, %d before the wave-private loop" % (name, vgprs, PARENT_VGPRS)
        assert lds <= 34816, "%s: %d bytes of LDS, 34816 before" % (name, lds)
    assert "scratch_load" not in asm and "scratch_store" not in asm and "scratch_" not in asm
    # the wave-private kernels (mangled names end in the WP flag: ...Lb1EEEv...): one barrier, and it lies behind the last MFMA
    for name, _ in kernels:
        code = asm[asm.index("\n%s:" % name):]
        code = code[:code.index("s_endpgm")]
        barriers = [m.start() for m in re.finditer(r"\bs_barrier\b", code)]
        last_mfma = max(m.start() for m in re.finditer(r"v_mfma_f32_32x32x2", code))
        if re.search(r"Li4ELi[01]ELb1EEEv", name):
            assert len(barriers) == 1 and barriers[0] > last_mfma, "%s: barriers at %s, last MFMA at %d" % (name, barriers, last_mfma)
        else:
            assert len(barriers) > 1, name        # (the cooperative loop: this check does tell the two forms apart)
