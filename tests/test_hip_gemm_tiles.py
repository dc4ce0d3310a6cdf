"""Every SGEMM tile (csrc/gemm.hip: the skinny 64x32 / 32x64 tiles, 64x64 with and without the cross-workgroup K split, 32x32 with
four K-groups, 64x32 / 32x64 with two K-groups, 128x128 with and without the split, 256x256) in all four operand layouts through the
raw C ABI, at its K, M, N, leading-dimension and slice-count edges, against float64 - the table and the rules are
tests/gemm_cases.py.  One child process per configuration (tests/gemm_tile_worker.py): the library reads LG_GEMM_TILE /
LG_GEMM_SLICES once.

Per case: lg_gemm_last_plan names the tile the case is meant for, the layout and staging bits and - where LG_GEMM_SLICES forces the
split - the slice count of the documented rule; two runs give the same bits; every float of the output buffers outside the result
still holds the pattern it was filled with; no result is NaN although every float a kernel may fetch beyond its operands is NaN;
the relative Frobenius distance from float64 is at most max(1e-5, 2 x numpy float32's own); every element lies within the bound
that holds for ANY order of summing the K products."""
import json
import pytest
import gemm_cases as G


def check_records(child, lines):
    """the worker's output against the table: (failures, worst relative Frobenius error, worst share of the element bound)"""
    cases = G.cases(child)
    recs = [json.loads(line) for line in lines if line.startswith("{")]
    assert recs and recs[-1] == {"done": len(cases)}, recs[-1:]
    assert len(recs) == len(cases) + 1
    worst_err, worst_ratio, failures = 0.0, 0.0, []
    for case, rec in zip(cases, recs):
        what = G.name(case)
        assert all(rec[x] == case[x] for x in case), (what, rec)
        problems = []
        if tuple(rec["tile"]) != G.expected_tile(case):
            problems.append("ran on tile %s, meant for %s" % (rec["tile"], G.expected_tile(case)))
        if rec["flags"] != G.expected_flags(case):
            problems.append("plan flags %d, expected %d" % (rec["flags"], G.expected_flags(case)))
        if rec["route"] != "own":
            problems.append("route %s" % rec["route"])
        bk = rec["tile"][2]
        slices, per = rec["k_slices"], rec["k_per_slice"]
        want = G.expected_slices(case)
        if want is not None and (slices, per) != want:
            problems.append("%d slices of %d k, expected %s" % (slices, per, want))
        # whatever the cost model chose: whole K-steps per slice, no slice empty, K covered; a split only from 4 K-steps on
        if not (slices >= 1 and per % bk == 0 and (slices - 1) * per < case["k"] <= slices * per):
            problems.append("slices %d x %d do not tile K" % (slices, per))
        if slices > 1 and want is None and case["k"] < 4 * bk:
            problems.append("split below 4 K-steps")
        if not rec["repeat_equal"]:
            problems.append("two runs differ")
        if not rec["outside_untouched"]:
            problems.append("wrote outside the result")
        if rec["nan"]:
            problems.append("NaN in a result")
        for key, e in rec["err"].items():
            worst_err = max(worst_err, e)
            if not e <= max(1e-5, 2 * rec["cpu_err"][key]):
                problems.append("%s %.3g from the float64 result, numpy float32 %.3g" % (key, e, rec["cpu_err"][key]))
        for key, r in rec["ratio"].items():
            worst_ratio = max(worst_ratio, r)
            if not r <= 1.0:
                problems.append("%s: an element at %.3g times its bound" % (key, r))
        if case["variant"] == "gelu" and not rec["gelu_of_stored"]:
            problems.append("aux is not gelu of the stored pre-activation")
        if problems:
            failures.append(what + ": " + "; ".join(problems))
    return failures, worst_err, worst_ratio, len(cases)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("child", sorted(G.CHILDREN))
def test_tile_sweep(hip, spawn_ranks, tmp_path, child):
    records = tmp_path / "records.jsonl"                    # (the spawner returns only the end of the child's output)
    res = spawn_ranks(1, ["tests/gemm_tile_worker.py", child, str(records)], env=G.CHILDREN[child]["env"], timeout=280)
    assert res["rc"] == 0, res["outputs"][0][-3000:]
    assert res["outputs"][0].rstrip().endswith(json.dumps({"done": len(G.cases(child))})), res["outputs"][0][-300:]
    failures, worst_err, worst_ratio, n = check_records(child, records.read_text().splitlines())
    print("child %s: %d cases, worst relative Frobenius error %.3g, worst share of the element bound %.3g" % (child, n, worst_err, worst_ratio))
    assert not failures, "%d of %d cases:\n%s" % (len(failures), n, "\n".join(failures[:40]))
