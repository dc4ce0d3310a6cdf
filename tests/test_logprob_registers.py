"""csrc/logprob.hip holds ONE kernel, logprob_rows_kernel: a workgroup per row of logits, the row staged in LDS as
keys, the sum of exponentials as 64-bit integers, and per thread the 8 best (value, inverted index) keys of its elements - sixteen
registers that must stay registers: 0 bytes of scratch.  Only the kernel's resource directives are read; the row is printed: it
is the one of DESIGN.md 3l.  hipcc cross-compiles without a GPU."""
import os
import shutil
import pytest
from conftest import ROOT
from test_attention_causal_registers import resources, CSRC, HIPCC


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_the_logprob_kernel_uses_no_scratch(tmp_path):
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    table = resources(tmp_path, "logprob")
    assert len(table) == 1 and "logprob_rows_kernel" in next(iter(table)), sorted(table)
    print("%-40s %8s %6s %6s" % ("kernel", "scratch", "vgprs", "sgprs"))          # (no MFMA: no AGPRs)
    for name, (scratch, vgprs, agprs, sgprs) in table.items():
        print("%-40s %8d %6d %6d" % (name, scratch, vgprs, sgprs))
        assert scratch == 0, "%s: %d bytes of scratch per lane" % (name, scratch)
        # (the accumulation offset is rounded up to a multiple of 4: a negative difference means nothing lies behind it)
        assert agprs <= 0 and vgprs <= 64, "%s: %d VGPRs, %d AGPRs - the 8 best keys are 16 of them" % (name, vgprs, agprs)
