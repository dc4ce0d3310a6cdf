"""The CAUSAL instantiations of the fused attention forward (csrc/attention.hip attn_fwd<D, true, DROP, true>,
csrc/attention_long.hip attn_long_fwd<D, DROP, true>) add a row-dependent bound to the selection of the softmax and, in the long
form, a shorter chunk loop: neither may push a kernel into scratch.  The long softmax holds a whole row of the tile (16 float4) in
registers between its passes, so that is where a spill would show.  Each CAUSAL kernel must use no more scratch than its
non-causal counterpart of the same compile.  Only the kernels' resource directives are read.  The counts are printed: they are
the rows of DESIGN.md's table.  hipcc cross-compiles without a GPU."""
import os
import re
import shutil
import subprocess
import pytest
from conftest import ROOT

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")


def resources(tmp_path, source):
    """{mangled kernel name: (scratch bytes per lane, vgprs, agprs, sgprs)} of one source, compiled for the device only"""
    out = tmp_path / (source + ".s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), source + ".hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        sgprs = int(re.search(r"\.amdhsa_next_free_sgpr (\d+)", body).group(1))
        accum = re.search(r"\.amdhsa_accum_offset (\d+)", body)
        agprs = vgprs - int(accum.group(1)) if accum else 0       # unified file: what lies behind the offset are AGPRs
        found[name] = (scratch, vgprs, agprs, sgprs)
    return found


def bools(*flags):
    return "".join("Lb%dE" % f for f in flags)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(900)
def test_causal_instantiations_use_no_more_scratch_than_their_counterparts(tmp_path):
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    short, long = resources(tmp_path, "attention"), resources(tmp_path, "attention_long")

    def one(table, stem, tail):
        names = [n for n in table if re.search(r"%s\w*ILi%s" % (stem, tail), n)]
        assert len(names) == 1, (stem, tail, sorted(table))
        return names[0]

    pairs = []
    for d in (32, 64):
        for drop in (0, 1):
            # attn_fwd<D, TAIL, DROP, CAUSAL> / attn_long_fwd<D, DROP, CAUSAL>
            pairs.append((short, one(short, "attn_fwd", "%dE%s" % (d, bools(1, drop, 1))), one(short, "attn_fwd", "%dE%s" % (d, bools(1, drop, 0)))))
            pairs.append((long, one(long, "attn_long_fwd", "%dE%s" % (d, bools(drop, 1))), one(long, "attn_long_fwd", "%dE%s" % (d, bools(drop, 0)))))
    assert len({p[1] for p in pairs}) == 8
    print("%-52s %8s %6s %6s %6s" % ("kernel", "scratch", "vgprs", "agprs", "sgprs"))
    for table, causal, plain in pairs:
        for name in (plain, causal):
            print("%-52s %8d %6d %6d %6d" % ((name,) + table[name]))
        assert table[causal][0] <= table[plain][0], "%s: %d bytes of scratch per lane, %s has %d" % (causal, table[causal][0], plain, table[plain][0])
