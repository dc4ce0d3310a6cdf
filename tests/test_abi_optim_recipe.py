"""The two entry points of the optimizer recipe (norm launch, AdamW multi-tensor update) are declared in include/lghip.h,
prototyped in autograd/hip/lib.py and exported by the built library - with the same number of arguments everywhere."""
import os
import re
import pytest
from conftest import ROOT
from lightgrad_amd.autograd.hip import lib as hiplib

SYMBOLS = {"lg_grad_norm_clip_f32": 7, "lg_adamw_multi_dev_f32": 20}


def header_text():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_declared_prototyped_and_exported(name):
    decl = re.search(r"^\s*int\s+%s\s*\((.*?)\)\s*;" % name, header_text(), re.M | re.S)
    assert decl is not None, "%s is not declared in include/lghip.h" % name
    assert len(decl.group(1).split(",")) == SYMBOLS[name]
    assert name in hiplib.PROTOTYPES
    restype, argtypes = hiplib.PROTOTYPES[name]
    assert restype is hiplib.c_int and len(argtypes) == SYMBOLS[name]
    handle = hiplib.load_library()
    assert getattr(handle, name) is not None


def test_scratch_size_matches_the_header():
    assert re.search(r"#define LG_GRAD_NORM_PARTIALS\s+%d\b" % hiplib.GRAD_NORM_PARTIALS, header_text())
