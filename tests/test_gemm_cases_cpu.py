"""No GPU: the case table of the SGEMM tile sweep (tests/gemm_cases.py) covers the edges it claims to cover, and its two rules
measure a kernel and not the inputs - a float32 product of these operands, numpy's own and a one-k-after-the-other sum (the least
favourable order), passes both with room to spare."""
import numpy as np
import pytest
import gemm_cases as G


@pytest.mark.parametrize("child", sorted(G.CHILDREN))
def test_a_float32_product_of_the_inputs_passes_both_rules(child):
    """relative Frobenius distance from float64 at most 2.5e-6 (a quarter of the rule's 1e-5 floor, the margin of
    test_hip_gemm_kgroups.py) and every element inside the bound that holds for any order of summation"""
    worst_err, worst_ratio = 0.0, 0.0
    for case in G.cases(child):
        ref64 = G.reference(case, np.float64)
        for mode in ("matmul", "sequential"):
            rec = G.judge(case, G.reference(case, np.float32, mode), ref64)
            assert not rec["nan"], G.name(case)
            for key, e in rec["err"].items():
                assert e <= 2.5e-6, (G.name(case), mode, key, e)
                worst_err = max(worst_err, e)
            for key, r in rec["ratio"].items():
                assert r <= 1.0, (G.name(case), mode, key, r)
                worst_ratio = max(worst_ratio, r)
    print("child %s: largest float32 distance from float64 %.3g, largest share of the element bound %.3g" % (child, worst_err, worst_ratio))


def test_the_table_reaches_the_edges_it_is_made_for():
    for child, spec in G.CHILDREN.items():
        cases = G.cases(child)
        assert cases, child
        s, ks = spec["stage"], set(spec["ks"])
        split = "LG_GEMM_SLICES" in spec["env"]
        if not split:
            assert {s - 1, s, s + 1} <= ks, (child, "K around the k-values staged per step")
            assert {1, 2, 3, 4, 5} <= ks, (child, "fewer K-tiles than the prefetch ring holds, every tail of a float4")
        assert {k % 4 for k in ks} == {0, 1, 2, 3} or split, child
        assert any(k > 2 * s and k % s for k in ks), (child, "a last step that not every K-group / K-tile reaches")
        assert {c["k"] for c in cases if c["variant"] == "bias"} == set(spec["few"]), child
        tile = spec["tile"]
        for (m, n) in spec["shapes"]:
            bm, bn = G.expected_tile(dict(child=child, variant="plain", m=m, n=n))[:2]
            if spec["tile"] is None or G.is_skinny(m, n):
                continue                                                   # (the skinny tiles: M or N is the point, 1 .. 32)
            assert (m, n) == (64, 64) or (m % bm and n % bn), (child, m, n)
        if tile is not None:
            wide = [(m, n) for (m, n) in spec["shapes"] if not G.is_skinny(m, n)]
            assert any(m % tile[0] and n % tile[1] for (m, n) in wide), child
            assert any(m > tile[0] or n > tile[1] for (m, n) in wide), (child, "more than one workgroup")
        # both stagings of the virtual ones-column, all four layouts, every variant
        rows = [c for c in cases if c["variant"] == "rowsum" and not G.is_skinny(c["m"], c["n"])] or [c for c in cases if c["variant"] == "rowsum"]
        assert {c["n"] % 4 == 0 for c in rows} == {True, False}, child
        assert {(c["ta"], c["tb"]) for c in cases if c["variant"] == "plain"} == set(G.LAYOUTS), child
        seen = {c["variant"] for c in cases}
        assert set(G.FULL_K_VARIANTS) | set(G.FEW_K_VARIANTS) | {"multi3", "kseg3", "offset"} <= seen, (child, seen)
        assert (set(G.BATCHED_VARIANTS) <= seen) == (child in G.BATCHED_CHILDREN), child
        for variant in G.FULL_K_VARIANTS:
            for (m, n) in spec["shapes"]:
                for (ta, tb) in G.LAYOUTS:
                    got = {c["k"] for c in cases if (c["variant"], c["m"], c["n"], c["ta"], c["tb"]) == (variant, m, n, ta, tb)}
                    assert got == ks, (child, variant, m, n, ta, tb)


def test_forced_split_counts_follow_the_documented_rule():
    """LG_GEMM_SLICES=7 at the K of children c and h launches 2, 3, 4, 5, 7 and 4 slices: the fold of four slabs at a time sees a
    partial last batch, an exact batch and 4 + 3"""
    for child in ("c", "h"):
        m, n = G.CHILDREN[child]["shapes"][-1 if child == "h" else 0]
        counts = [G.expected_slices(dict(child=child, variant="plain", m=m, n=n, k=k))[0] for k in G.K_SPLIT]
        assert counts == [2, 3, 4, 5, 7, 4], (child, counts)
    assert G.expected_slices(dict(child="b", variant="plain", m=70, n=50, k=197)) is None
    assert G.expected_slices(dict(child="d", variant="plain", m=70, n=50, k=197)) == (1, 208)
    assert G.expected_slices(dict(child="i", variant="plain", m=300, n=513, k=33)) == (1, 64)


def test_buffers_guard_every_matrix_with_nan_and_keep_what_they_hold():
    inp = G.inputs(70, 50, 33, 1, 0, "offset")
    a = inp["A"]
    assert a.start == G.GUARD + 1 and np.isnan(a.buf[:a.start]).all() and np.isnan(a.buf[-G.GUARD:]).all()
    assert np.isnan(a.buf[~a.inside]).all() and not np.isnan(a.buf[a.inside]).any()
    np.testing.assert_array_equal(a.get()[0], inp["a"][0].T)                # transA: stored [K, M]
    c = G.c_buffer(dict(variant="accumulate", m=70, n=50), inp)
    assert (c.buf.view(np.uint32)[~c.inside] == G.PATTERN).all() and c.outside_untouched(c.buf.copy())
    np.testing.assert_array_equal(c.get(), inp["c0"])
    touched = c.buf.copy()
    touched[c.start + 50] = 0.0 if c.ld > 50 else touched[c.start + 50]     # the first padding column, where there is one
    assert c.outside_untouched(touched) == (c.ld == 50)
    batch = G.inputs(130, 77, 197, 0, 1, "batch3")
    assert batch["A"].stride > 130 * batch["A"].ld and batch["A"].count == 3
