"""csrc/extend.hip holds ONE kernel body, attn_extend_body<D, PACKED>, behind two kernels for D = 32 and 64 each: attn_extend<D>
serves the three (b, m) entries, attn_packed<D> serves lg_attention_extend_packed_f32, where a slot's first token row (a word of
`cu`, uniform over the workgroup) takes the place of a batch pitch.  The softmax holds a whole row of the tile (16 float4) in
registers between its passes, so that is where a spill would show: every kernel of the file must use 0 bytes of scratch, as
DESIGN.md 3h-4 states for the two the parent commit had, and the packed form must hold no more vector registers than the (b, m)
form.  Only the kernels' resource directives are read.  The counts are printed: they are the rows of DESIGN.md 3h-7.  hipcc
cross-compiles without a GPU."""
import os
import re
import shutil
import pytest
from conftest import ROOT
from test_attention_causal_registers import resources, CSRC, HIPCC


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_every_extend_instantiation_uses_no_scratch(tmp_path):
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    table = resources(tmp_path, "extend")
    kernels = {}
    for name in table:
        found = re.search(r"(attn_extend|attn_packed)ILi(\d+)E", name)
        assert found is not None, "a kernel of extend.hip that is neither: %s" % name
        kernels[(found.group(1), int(found.group(2)))] = name
    assert sorted(kernels) == [("attn_extend", 32), ("attn_extend", 64), ("attn_packed", 32), ("attn_packed", 64)] and len(table) == 4, sorted(table)
    print("%-52s %8s %6s %6s %6s" % ("kernel", "scratch", "vgprs", "agprs", "sgprs"))
    for key in sorted(kernels):
        print("%-52s %8d %6d %6d %6d" % ((kernels[key],) + table[kernels[key]]))
    for name in kernels.values():
        assert table[name][0] == 0, "%s: %d bytes of scratch per lane" % (name, table[name][0])
    for d in (32, 64):
        assert table[kernels[("attn_packed", d)]][1] <= table[kernels[("attn_extend", d)]][1], (d, table)
