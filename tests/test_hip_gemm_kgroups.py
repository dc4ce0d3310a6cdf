"""The 32x32 tile with four K-groups (csrc/gemm.hip, tile 5; the forward product of the MNIST MLP and tiny-BERT's small products)
through the raw C ABI, with its wave-private K loop and, for A/B, with the cooperative loop it replaced (LG_GEMM_KLOOP=coop).
K from 1 to 784 around the loop's step sizes (16 per wave, 64 per workgroup), M and N no multiples of 32, padded leading
dimensions, with and without bias, relu on the operand, accumulation and row sums.  Judged against float64 by the rule of
tests/common.py (assert_as_close_to_float64_as_the_cpu_backend); every case runs twice and must repeat bit for bit, and the two
loops must give the same bits.

The cases run in a child process (tests/kgroups_worker.py): the library reads LG_GEMM_TILE once, and the small K of this list
would not pick this tile on their own."""
import json
import numpy as np
import pytest
import kgroups_worker as W


def test_inputs_leave_a_float32_product_well_inside_the_rule():
    """no GPU: with these inputs a float32 product - numpy's own and a plain one-k-after-the-other sum, the least favourable
    order - stays below a quarter of the 1e-5 floor of the rule, so the GPU test measures the kernel and not the inputs"""
    worst = 0.0
    for (m, n) in W.SHAPES:
        for k in W.KS:
            for variant in W.VARIANTS:
                a, bt, c0, bias, _ = W.case_inputs(m, n, k, variant)
                ref64 = W.expected(m, n, k, variant, a, bt, c0, bias, np.float64)
                for sequential in (False, True):
                    got = W.expected(m, n, k, variant, a, bt, c0, bias, np.float32, sequential=sequential)
                    for key in ref64:
                        worst = max(worst, W.rel_frobenius(got[key], ref64[key]))
    print("largest float32 distance from float64 over the cases: %.3g" % worst)
    assert worst <= 2.5e-6, worst


def assert_rule(rec, what):
    """the rule of common.assert_as_close_to_float64_as_the_cpu_backend, on the distances the worker reports: within 1e-5
    (relative Frobenius) of the float64 result, or no further from it than twice numpy's float32 result"""
    for key, e_got in rec["err"].items():
        e_cpu = rec["cpu_err"][key]
        assert e_got <= max(1e-5, 2 * e_cpu), "%s %s: %.3g from the float64 result, numpy float32 %.3g" % (what, key, e_got, e_cpu)


def run_cases(spawn_ranks, env):
    res = spawn_ranks(1, ["tests/kgroups_worker.py"], env=env, timeout=280)
    assert res["rc"] == 0, res["outputs"][0][-3000:]
    recs = [json.loads(line) for line in res["outputs"][0].splitlines() if line.startswith("{")]
    assert recs and recs[-1] == {"done": len(W.SHAPES) * len(W.KS) * len(W.VARIANTS)}, recs[-1:]
    for rec in recs[:-1]:
        what = "M=%(m)d N=%(n)d K=%(k)d %(variant)s" % rec
        print(what, rec["err"], rec["cpu_err"])
        assert rec["repeat_equal"], what + ": two runs differ"
        assert rec["padding_untouched"], what + ": wrote beyond column N"
        assert_rule(rec, what)
    return {(rec["m"], rec["n"], rec["k"], rec["variant"]): rec["sha1"] for rec in recs[:-1]}


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_wave_private_loop_on_the_four_k_group_tile(hip, spawn_ranks):
    run_cases(spawn_ranks, {"LG_GEMM_TILE": "5"})


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_cooperative_loop_stays_selectable_and_both_loops_agree_bit_for_bit(hip, spawn_ranks):
    """a wave multiplies the same k-columns in the same order in both loops, and the K-group exchange adds in the same order: the
    results are the same bits"""
    coop = run_cases(spawn_ranks, {"LG_GEMM_TILE": "5", "LG_GEMM_KLOOP": "coop"})
    private = run_cases(spawn_ranks, {"LG_GEMM_TILE": "5"})
    differ = [case for case in coop if coop[case] != private[case]]
    assert not differ, differ
