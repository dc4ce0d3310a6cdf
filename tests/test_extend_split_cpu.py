"""The entry points of the split-key extend attention (csrc/extend_split.hip): declared in include/lghip.h, bound in python and
exported by the built library, and the answers of its predicate - pure host code, no GPU needed."""
from test_abi import declared
from lightgrad_amd.autograd.hip import lib as hiplib

NAMES = ("lg_attention_extend_split_f32", "lg_attention_extend_split_rows_f32", "lg_attention_extend_split_counts_f32",
         "lg_attention_extend_split_supported", "lg_attention_extend_split_slice")


def test_the_entry_points_are_declared_bound_and_exported():
    names = declared("lghip.h")
    handle = hiplib.load_library()          # raises if the .so is missing or lacks a declared symbol
    for n in NAMES:
        assert n in names, "include/lghip.h does not declare %s" % n
        assert n in hiplib.PROTOTYPES, "no python prototype for %s" % n
        assert getattr(handle, n) is not None
    # the operands of the 512-row entries, lse where p stood
    for n in NAMES[:3]:
        assert hiplib.PROTOTYPES[n] == hiplib.PROTOTYPES[n.replace("_split", "")]


def test_the_predicate_and_the_slice():
    handle = hiplib.load_library()
    supported = handle.lg_attention_extend_split_supported
    assert supported(128, 16384, 64) and supported(1, 1, 32) and supported(5, 513, 32)
    assert not supported(129, 16384, 64) and not supported(1, 16385, 64) and not supported(1, 8, 48) and not supported(9, 8, 64)
    assert handle.lg_attention_extend_split_slice() in (256, 512, 1024)
