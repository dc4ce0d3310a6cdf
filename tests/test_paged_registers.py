"""csrc/paged.hip holds the kernel body of extend.hip once more (extend_body.h, attn_extend_body<D, false, PAGED = true>) behind
one kernel for D = 32 and 64 each, attn_paged<D>; csrc/serve_paged.hip holds one kernel.  The softmax of the body holds a whole
row of the tile in registers between its passes, so that is where a spill would show, and the table lookup in front of every row
address adds live values to the load loops: every kernel must use 0 bytes of scratch.  Only the kernels' resource directives are
read.  The counts are printed: they are the rows of DESIGN.md 3h-8.  (That extend.hip still holds its four kernels with the
registers they had is test_extend_packed_registers.py's.)  hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import pytest
from conftest import ROOT
from test_attention_causal_registers import resources, CSRC, HIPCC


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("paged")
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    return tmp_path


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_the_paged_attention_kernels_use_no_scratch(tree):
    table = resources(tree, "paged")
    kernels = {}
    for name in table:
        found = re.search(r"attn_pagedILi(\d+)E", name)
        assert found is not None, "a kernel of paged.hip that is no attn_paged<D>: %s" % name
        kernels[int(found.group(1))] = name
    assert sorted(kernels) == [32, 64] and len(table) == 2, sorted(table)
    print("%-52s %8s %6s %6s %6s" % ("kernel", "scratch", "vgprs", "agprs", "sgprs"))
    for d in sorted(kernels):
        print("%-52s %8d %6d %6d %6d" % ((kernels[d],) + table[kernels[d]]))
    for name in kernels.values():
        assert table[name][0] == 0, "%s: %d bytes of scratch per lane" % (name, table[name][0])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_the_paged_commit_kernel_uses_no_scratch(tree):
    table = resources(tree, "serve_paged")
    assert len(table) == 1 and "serve_commit_paged" in list(table)[0], sorted(table)
    print("%-52s %8s %6s %6s %6s" % ("kernel", "scratch", "vgprs", "agprs", "sgprs"))
    for name, row in table.items():
        print("%-52s %8d %6d %6d %6d" % ((name,) + row))
        assert row[0] == 0, "%s: %d bytes of scratch per lane" % (name, row[0])
