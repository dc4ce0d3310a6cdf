"""csrc/guide.hip holds ONE kernel, guide_rows_kernel: a grid of (slices, rows) workgroups, the catch-up of the
row's automaton in uniform scalars, the slice's words of the state's bitset staged in LDS, a store-only pass over the row's 16-byte
groups.  It keeps nothing per thread beyond a handful of scalars, so it must use 0 bytes of scratch and no AGPRs.  Only the
kernel's resource directives are read; the row is printed: it is the one of DESIGN.md 3m.  hipcc cross-compiles without a GPU."""
import os
import shutil
import pytest
from conftest import ROOT
from test_attention_causal_registers import resources, CSRC, HIPCC


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_the_guide_kernel_uses_no_scratch(tmp_path):
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    table = resources(tmp_path, "guide")
    assert len(table) == 1 and "guide_rows_kernel" in next(iter(table)), sorted(table)
    print("%-40s %8s %6s %6s" % ("kernel", "scratch", "vgprs", "sgprs"))          # (no MFMA: no AGPRs)
    for name, (scratch, vgprs, agprs, sgprs) in table.items():
        print("%-40s %8d %6d %6d" % (name, scratch, vgprs, sgprs))
        assert scratch == 0, "%s: %d bytes of scratch per lane" % (name, scratch)
        assert agprs == 0 and vgprs <= 64, "%s: %d VGPRs, %d AGPRs - 256 threads a row should need few" % (name, vgprs, agprs)
