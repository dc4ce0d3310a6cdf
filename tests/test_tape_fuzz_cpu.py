"""The program generator of tests/tape_fuzz.py, run on the CPU backend alone: every drawn program must run, and float32 must stay
close to a float64 run of the same program (a generator that draws exploding programs would make the GPU comparison meaningless)."""
import numpy as np
import pytest
from lightgrad_amd import CpuTensor
from common import float64_tape
from tape_fuzz import draw_program, run_program, compare


@pytest.mark.parametrize("block", range(4))
def test_programs_run_and_are_well_conditioned(block):
    for seed in range(block * 10, block * 10 + 10):
        prog = draw_program(seed)
        got = run_program(CpuTensor, prog)
        with float64_tape():
            ref = run_program(CpuTensor, prog, dtype=np.float64)
        assert len(got) >= 3
        compare(ref, got, rtol=5e-3, atol=5e-4, what="seed %d %r" % (seed, prog))


def test_the_shared_parameter_draw_leaves_every_earlier_program_as_it_was():
    """the shared-parameter keys come from a stream of their own: without them, seeds 0-620 (the ranges of the GPU tests) draw
    exactly the programs they drew before the ingredient existed (the digest of those programs) - and the plain draw, which
    those tests use, leaves the ingredient out"""
    import hashlib
    import json
    from tape_fuzz import SHARED_KEYS
    digest = hashlib.sha256()
    for seed in range(621):
        prog = draw_program(seed, shared=True)
        assert set(SHARED_KEYS) <= set(prog)
        plain = draw_program(seed)
        assert all(plain[k] is None for k in SHARED_KEYS) and {k: v for k, v in plain.items() if k not in SHARED_KEYS} == \
            {k: v for k, v in prog.items() if k not in SHARED_KEYS}
        digest.update(json.dumps({k: v for k, v in prog.items() if k not in SHARED_KEYS}, sort_keys=True).encode())
    assert digest.hexdigest() == "3ded6bdf25b1793ae75c5b03498ce36972711554d640da2bae95073d45870127"


@pytest.mark.parametrize("first", [700, 850, 900, 1100])
def test_shared_parameter_programs_are_well_conditioned(first):
    """the seed ranges of the shared-parameter GPU tests, every program that uses a parameter twice: float32 close to float64"""
    ran = 0
    for seed in range(first, first + 40):
        prog = draw_program(seed, shared=True)
        if prog["reuse"] is None and prog["penalty"] is None:
            continue
        got = run_program(CpuTensor, prog)
        with float64_tape():
            ref = run_program(CpuTensor, prog, dtype=np.float64)
        compare(ref, got, rtol=5e-3, atol=5e-4, what="seed %d %r" % (seed, prog))
        ran += 1
    assert ran >= 15
