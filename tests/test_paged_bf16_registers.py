"""csrc/paged_bf16.hip holds the kernel body of extend.hip a third time (extend_body.h, attn_extend_body<D, false, true, KV16 = true>)
behind one kernel for D = 32 and 64 each, attn_paged_bf16<D>.  Next to what test_paged_registers.py says of the paged body, the
KV16 form holds both sides of a streamed key across the MFMA phase - 2 registers of bfloat16 words from the pool and 4 of floats
from the new tokens for every quad of the tile - and converts them on the way to LDS: more live values in front of every seam
store.  Every kernel must use 0 bytes of scratch.  Only the
kernels' resource directives are read.  The counts are printed: they are the rows of DESIGN.md 3h-9.  (That paged.hip still holds
its two kernels is test_paged_registers.py's, that extend.hip holds its four test_extend_packed_registers.py's.)  hipcc
cross-compiles without a GPU."""
import os
import re
import shutil
import pytest
from conftest import ROOT
from test_attention_causal_registers import resources, CSRC, HIPCC


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("paged_bf16")
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    return tmp_path


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_the_bf16_paged_attention_kernels_use_no_scratch(tree):
    table = resources(tree, "paged_bf16")
    kernels = {}
    for name in table:
        found = re.search(r"attn_paged_bf16ILi(\d+)E", name)
        assert found is not None, "a kernel of paged_bf16.hip that is no attn_paged_bf16<D>: %s" % name
        kernels[int(found.group(1))] = name
    assert sorted(kernels) == [32, 64] and len(table) == 2, sorted(table)
    print("%-52s %8s %6s %6s %6s" % ("kernel", "scratch", "vgprs", "agprs", "sgprs"))
    for d in sorted(kernels):
        print("%-52s %8d %6d %6d %6d" % ((kernels[d],) + table[kernels[d]]))
    for name in kernels.values():
        assert table[name][0] == 0, "%s: %d bytes of scratch per lane" % (name, table[name][0])
