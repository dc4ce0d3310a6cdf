"""csrc/sample_body.h holds the row body of the sampling launches, sample_row_body<LDS, GREEDY, OutT>: sample.hip instantiates it
behind sample_kernel (the global stream and its ticket protocol, GREEDY = false), sample_rows.hip behind sample_rows_kernel (a
table row per row, GREEDY = true).  Moving the body must have cost sample_kernel nothing: its LDS and memory variants keep the
VGPR counts of the build in front of the move (90 and 76 registers allocated, `.amdhsa_next_free_vgpr`) and 0 bytes of scratch, and
the four new kernels use 0 bytes of scratch as well - the body keeps 128-bit compares and 64-bit sums live across its passes, so
that is where a spill would show.  Only the kernels' resource directives are read.  The rows are printed: they are the table of
DESIGN.md 3j.  hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import pytest
from conftest import ROOT
from test_attention_causal_registers import resources, CSRC, HIPCC

PARENT_VGPRS = {1: 90, 0: 76}            # sample_kernel<LDS, .>: what sample.hip compiled to with the body in the file itself


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("sample_rows")
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    return tmp_path


def variants(table, stem):
    """{(lds, out letter): mangled name} of the four instantiations <LDS, OutT> of kernel `stem`"""
    found = {}
    for name in table:
        m = re.search(r"%sILb([01])E([il])E" % stem, name)
        assert m is not None, "a kernel that is no %s<LDS, OutT>: %s" % (stem, name)
        found[(int(m.group(1)), m.group(2))] = name
    assert sorted(found) == [(0, "i"), (0, "l"), (1, "i"), (1, "l")] and len(table) == 4, sorted(table)
    return found


def show(table, kernels):
    print("%-72s %8s %6s %6s" % ("kernel", "scratch", "vgprs", "sgprs"))          # (no MFMA anywhere: no AGPRs)
    for key in sorted(kernels):
        scratch, vgprs, _, sgprs = table[kernels[key]]
        print("%-72s %8d %6d %6d" % (kernels[key], scratch, vgprs, sgprs))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_the_per_request_kernels_use_no_scratch(tree):
    table = resources(tree, "sample_rows")
    kernels = variants(table, "sample_rows_kernel")
    show(table, kernels)
    for name in kernels.values():
        assert table[name][0] == 0, "%s: %d bytes of scratch per lane" % (name, table[name][0])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_sample_kernel_compiles_to_what_it_was(tree):
    table = resources(tree, "sample")
    kernels = variants(table, "sample_kernel")
    show(table, kernels)
    for (lds, _), name in kernels.items():
        scratch, vgprs = table[name][:2]
        assert scratch == 0, "%s: %d bytes of scratch per lane" % (name, scratch)
        assert vgprs == PARENT_VGPRS[lds], "%s: %d VGPRs, %d in front of the move of the body" % (name, vgprs, PARENT_VGPRS[lds])
