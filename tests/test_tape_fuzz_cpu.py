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


# ---- the judge of the GPU tests (tape_fuzz.judge), tested on the CPU backend alone ------------------------------------------
@pytest.mark.parametrize("first", [0, 50, 100, 150])
def test_the_judge_notices_a_product_that_is_wrong_by_3e_5(first):
    """a fifth backend whose every matrix product, forward and backward, is `blas` times float32(1 + 3e-5): the judge refuses it
    in every kept program of seeds 0-199 whose outputs are not all exactly zero (a dead relu: no product reaches anything a
    user can see), where compare() against the float32 run, the rule it replaces, accepts it in more than half of them"""
    from tape_fuzz import cpu_runs, judge, product_order, scaled_product
    live, escaped, accepted_by_compare = 0, [], 0
    for seed in range(first, first + 50):
        prog = draw_program(seed)
        runs = cpu_runs(prog)
        if not runs.kept or runs.dead:
            continue
        with product_order(scaled_product(1 + 3e-5)):
            mutant = run_program(CpuTensor, prog)
        live += 1
        try:
            judge(runs.ref64, runs.variants, mutant, what="seed %d %r" % (seed, prog), known=runs.apart)
            escaped.append(seed)
        except AssertionError as e:
            assert ("seed %d " % seed) in str(e)
        try:
            compare(runs.variants["blas"], mutant)
            accepted_by_compare += 1
        except AssertionError:
            pass
    print("wrong product, seeds %d-%d: refused by the judge in %d of %d programs, accepted by compare() in %d" % (
        first, first + 49, live - len(escaped), live, accepted_by_compare))
    assert not escaped, "the judge accepted the wrong product in seeds %s" % escaped
    assert live >= 40 and 2 * accepted_by_compare > live, (live, accepted_by_compare)


def test_a_failure_of_the_judge_names_what_it_saw():
    from tape_fuzz import cpu_runs, judge
    prog = draw_program(0)
    runs = cpu_runs(prog)
    got = [(l, a * (1 + 1e-3) if l == "s0/out" else a) for l, a in runs.variants["blas"]]
    with pytest.raises(AssertionError) as failure:
        judge(runs.ref64, runs.variants, got, what="seed 0 %r" % (prog,))
    text = str(failure.value)
    assert "seed 0" in text and "s0/out" in text and "'dims'" in text and "max |got - blas|" in text
    assert all(name in text for name in runs.variants)
    with pytest.raises(AssertionError, match="different things"):
        judge(runs.ref64, runs.variants, got[:-1], what="seed 0")
    with pytest.raises(AssertionError):
        judge(runs.ref64, runs.variants, [(l, a + (np.inf if l == "s0/loss" else 0)) for l, a in got], what="seed 0")


def test_a_zero_reference_is_judged_by_norms():
    """where float64 says exactly 0: exactly 0 if every float32 run says so, otherwise no more than twice their largest norm"""
    from tape_fuzz import judge
    zero, tiny = np.zeros((2, 3)), np.full((2, 3), 1e-9)
    runs = lambda a: {n: [("s0/out", a)] for n in ("blas", "wide", "chunk7", "chunk16r")}      # noqa: E731
    assert judge([("s0/out", zero)], runs(zero), [("s0/out", zero)], what="") == {}
    with pytest.raises(AssertionError, match="exactly 0"):
        judge([("s0/out", zero)], runs(zero), [("s0/out", tiny * 1e-20)], what="")
    judge([("s0/out", zero)], runs(tiny), [("s0/out", 2 * tiny)], what="")
    with pytest.raises(AssertionError, match="exactly 0"):
        judge([("s0/out", zero)], runs(tiny), [("s0/out", 2.01 * tiny)], what="")


def _gpu_test_program_sets():
    from tape_fuzz import gpu_test_programs
    return sorted(gpu_test_programs().items())


@pytest.mark.parametrize("name,programs", _gpu_test_program_sets(), ids=[name for name, _ in _gpu_test_program_sets()])
def test_the_float32_variants_vouch_for_each_other_on_the_programs_of_the_gpu_tests(name, programs):
    """leave-one-out over the seed ranges of every GPU test: in a kept program each of the float32 runs passes the judge with
    the others as its yardstick, and the programs where one does not stay under the cap"""
    from tape_fuzz import cpu_runs, judge, within_the_cap, VARIANTS
    left_out, tally = [], {}
    for seed, prog in programs:
        runs = cpu_runs(prog)
        if not runs.kept:
            left_out.append(seed)
            continue
        for one in VARIANTS:
            others = {n: run for n, run in runs.variants.items() if n != one}
            judge(runs.ref64, others, runs.variants[one], what="seed %d, %s by the others, %r" % (seed, one, prog), known=runs.apart)
        judge(runs.ref64, runs.variants, runs.variants["blas"], what="seed %d" % seed, tally=tally, known=runs.apart)
    print("%s: %d programs, left out %s, %d observables, %d judged at the floor" % (
        name, len(programs), left_out, tally["observables"], tally["at_floor"]))
    assert within_the_cap(left_out, len(programs)), (name, left_out, len(programs))


def test_every_product_order_and_sum_order_is_the_same_sum():
    """the variants are evaluations of the same op: every product order within float32 rounding of the float64 product at sizes
    on both sides of their chunk and lane counts, every sum order of the float64 sum"""
    from tape_fuzz import PRODUCTS, _sum_over_lanes, _sum_left_to_right
    rng = np.random.RandomState(5)
    for m, k, n in [(1, 1, 1), (3, 7, 2), (8, 16, 5), (5, 17, 3), (33, 100, 10), (2, 257, 4), (4, 600, 3)]:
        a, b = rng.uniform(-1, 1, (m, k)).astype(np.float32), rng.uniform(-1, 1, (k, n)).astype(np.float32)
        exact = a.astype(np.float64) @ b.astype(np.float64)
        bound = k * 2.0 ** -24 * (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64))      # every order of k float32 adds
        for name, product in PRODUCTS.items():
            y = product(a, b)
            assert y.dtype == np.float32 and y.shape == (m, n), name
            assert (np.abs(y - exact) <= bound).all(), (name, m, k, n)
    for shape, axis in [((165,), None), ((33, 5), None), ((8, 24), 0), ((8, 24), -1), ((3, 130, 2), (0, 1)), ((2, 3, 70), 1)]:
        t = rng.uniform(-1, 1, shape).astype(np.float32)
        for keepdims in (False, True):
            exact = t.astype(np.float64).sum(axis=axis, keepdims=keepdims)
            bound = t.size * 2.0 ** -24 * np.abs(t).astype(np.float64).sum(axis=axis, keepdims=keepdims)
            for order in (_sum_over_lanes, _sum_left_to_right):
                y = order(t, axis, keepdims)
                assert y.dtype == np.float32 and y.shape == exact.shape, (order.__name__, shape, axis, keepdims)
                assert (np.abs(y - exact) <= bound).all(), (order.__name__, shape, axis)


def test_product_order_restores_the_op_and_the_bits():
    from lightgrad_amd.autograd.cpu import ops as cpu_ops
    from lightgrad_amd import nn as light_nn
    from tape_fuzz import product_order, variant
    inner = cpu_ops.dot.__mro__[1]
    before = inner.forward, inner.backward
    prog = draw_program(7)                               # a deep program: products of every shape, LayerNorm
    first = run_program(CpuTensor, prog)
    with product_order("wide"):
        assert inner.forward is not before[0]
        wide = run_program(CpuTensor, prog)
    assert (inner.forward, inner.backward) == before
    with pytest.raises(ZeroDivisionError):
        with product_order("chunk7"):
            1 / 0
    assert (inner.forward, inner.backward) == before
    with product_order("blas"):
        patched = run_program(CpuTensor, prog)
    again = run_program(CpuTensor, prog)
    assert any(not np.array_equal(a, b) for (_, a), (_, b) in zip(first, wide))          # the variant did change the rounding
    for (label, a), (_, b), (_, c) in zip(first, again, patched):
        np.testing.assert_array_equal(a, b, err_msg=label)
        np.testing.assert_array_equal(a, c, err_msg=label)
    saved = cpu_ops.sum.__mro__[1].forward, cpu_ops.tanh.__mro__[1].forward, light_nn.LayerNorm.forward
    with variant("together"):                            # every patch at once: products, activations, sums, LayerNorm
        assert cpu_ops.sum.__mro__[1].forward is not saved[0] and light_nn.LayerNorm.forward is not saved[2]
        together = run_program(CpuTensor, prog)
    assert (cpu_ops.sum.__mro__[1].forward, cpu_ops.tanh.__mro__[1].forward, light_nn.LayerNorm.forward) == saved
    assert (inner.forward, inner.backward) == before
    assert any(not np.array_equal(a, b) for (_, a), (_, b) in zip(first, together))
    for (label, a), (_, b) in zip(first, run_program(CpuTensor, prog)):
        np.testing.assert_array_equal(a, b, err_msg=label)
    a64 = np.random.RandomState(0).rand(5, 9)
    with product_order("chunk7"):                        # float64 and batched operands are not varied
        y = CpuTensor.from_numpy(a64) @ CpuTensor.from_numpy(a64.T.copy())
    np.testing.assert_array_equal(y.numpy(), a64 @ a64.T)
