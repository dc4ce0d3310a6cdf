"""The entry points of the LayerNorm launches with hidden dropout: declared in include/lghip.h, bound in python and exported by
the built library (no GPU needed: dlopen and symbol lookup only, the way tests/test_abi.py reads both)."""
from test_abi import declared
from lightgrad_amd.autograd.hip import lib as hiplib

NAMES = ("lg_dropout_layernorm_fwd_f32", "lg_dropout_layernorm_bwd_f32")


def test_the_entry_points_are_declared_bound_and_exported():
    names = declared("lghip.h")
    handle = hiplib.load_library()          # raises if the .so is missing or lacks a declared symbol
    for n in NAMES:
        assert n in names, "include/lghip.h does not declare %s" % n
        assert n in hiplib.PROTOTYPES, "no python prototype for %s" % n
        assert getattr(handle, n) is not None
    # thirteen and twelve arguments, as the header spells them
    assert len(hiplib.PROTOTYPES[NAMES[0]][1]) == 13 and len(hiplib.PROTOTYPES[NAMES[1]][1]) == 12
