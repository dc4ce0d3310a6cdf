"""tests/model_fuzz.py on the CPU backend alone: every program the GPU tests draw, float32 against the float64 tape through the
same `judge` (here `got` is the float32 run itself) - the generator's own test.  It proves what the GPU tests rely on: at most
15 % of either family is set aside by the float32-vs-float64 rule, the draw visits every ingredient and every pair of attention
features on both sides of 128 positions, and a program is a pure function of its seed."""
import collections
import itertools
import numpy as np
import pytest
from lightgrad_amd import CpuTensor
import model_fuzz as mf

TRANSFORMER_SEEDS, CNN_SEEDS = range(120), range(80)        # what tests/test_hip_model_fuzz.py runs, in blocks of ten
MAX_FILTERED = 0.15


def judged_on_the_cpu(draw, seeds):
    """(programs kept, programs filtered, worst distances) of float32 CpuTensor against the float64 tape"""
    kept, filtered, worst = 0, [], {}
    for seed in seeds:
        prog = draw(seed)
        ref64 = mf.run_program(CpuTensor, prog, dtype=np.float64)
        cpu32 = mf.run_program(CpuTensor, prog)
        verdict = mf.judge(ref64, cpu32, cpu32, prog)
        if verdict["status"] == "filtered":
            filtered.append(seed)
        else:
            kept += 1
            mf.merge_worst(worst, verdict["worst"])
    return kept, filtered, worst


@pytest.mark.parametrize("family", ["transformer", "cnn"])
def test_float32_against_float64_and_the_share_set_aside(family):
    draw, seeds = (mf.draw_transformer, TRANSFORMER_SEEDS) if family == "transformer" else (mf.draw_cnn, CNN_SEEDS)
    kept, filtered, worst = judged_on_the_cpu(draw, seeds)
    print("%s: %d programs kept, filtered %s" % (family, kept, filtered))
    for group, (e32, _) in sorted(worst.items()):
        print("  %-14s float32 CPU at most %.3g from float64" % (group, e32))
    assert kept >= (1 - MAX_FILTERED) * len(seeds), (kept, filtered)


def count(programs, key):
    return collections.Counter(key(p) for p in programs)


def test_the_transformer_draw_visits_everything():
    programs = [mf.draw_transformer(s) for s in TRANSFORMER_SEEDS]
    for name, key, values in (("S", lambda p: p["S"], mf.S_VALUES), ("mask", lambda p: p["mask"], mf.MASK_KINDS),
                              ("objective", lambda p: p["objective"], mf.OBJECTIVES), ("batch", lambda p: p["batch"], (1, 2, 3)),
                              ("heads", lambda p: p["heads"], (1, 2, 3)), ("d", lambda p: p["d"], (16, 32, 64)),
                              ("layers", lambda p: p["layers"], (1, 2)), ("vocab", lambda p: p["vocab"], (50, 61, 130)),
                              ("hidden_p", lambda p: p["hidden_p"], (0.0, 0.1, 0.5)), ("steps", lambda p: p["steps"], (0, 1, 2, 3)),
                              ("peek", lambda p: p["peek"], ("none", "logits", "probs")),
                              ("zero_grad", lambda p: p["zero_grad"], ("before_backward", "after_step", "never")),
                              ("token_types", lambda p: p["token_types"], (False, True)), ("eval", lambda p: p["eval_after"], (False, True)),
                              ("second_backward", lambda p: p["second_backward"], (False, True)),
                              ("decoder", lambda p: p["decoder_precision"], (None, "bf16")),
                              ("optimizer", lambda p: p["optimizer"], ("none", "adam", "adabelief"))):
        seen = count(programs, key)
        assert all(seen[v] >= 3 for v in values), (name, sorted(seen.items(), key=str))
    stepping = [p for p in programs if p["optimizer"] != "none"]
    forms = count(stepping, lambda p: p["form"])
    assert all(forms[f] >= 3 for f in mf.FORMS), forms
    recipes = [p["recipe"] for p in stepping if p["recipe"] is not None]
    assert sum(r["weight_decay"] > 0 for r in recipes) >= 3 and sum(r["max_grad_norm"] is not None for r in recipes) >= 3
    assert sum(r["schedule"] is not None for r in recipes) >= 3 and sum(r["decay_mask"] == "even" for r in recipes) >= 3
    assert any(p["intermediate"] % 32 for p in programs)
    # S > 128: at most a fifth of the programs, at batch 1
    long = [p for p in programs if p["S"] > 128]
    assert 0 < len(long) <= len(programs) / 5 and all(p["batch"] == 1 for p in long)
    # every pair of the four attention features together, on each side of 128 positions
    feature = {"mask": lambda p: p["mask"] != "none", "causal": lambda p: p["causal"],
               "attention dropout": lambda p: p["attention_p"] > 0, "hidden dropout": lambda p: p["hidden_p"] > 0}
    for a, b in itertools.combinations(feature, 2):
        for side, group in (("short", [p for p in programs if p["S"] <= 128]), ("long", long)):
            together = sum(1 for p in group if feature[a](p) and feature[b](p))
            assert together >= 3, (a, b, side, together)
    # what the HIP backend is expected to launch for them (tests/test_hip_model_fuzz.py looks at what it did launch)
    launches = count(programs, mf.attention_form)
    for family in ("plain", "tail", "long", "causal_short", "causal_long"):
        for drop in ("dropout", "nodropout"):
            assert launches["self_attention/%s/%s" % (family, drop)] >= 3, sorted(launches.items())
    assert launches["composite"] >= 3
    # a clm objective only where it is defined, a mask only where it can be what the issue asks for
    assert all(p["causal"] and p["S"] >= 2 for p in programs if p["objective"] == "clm")
    for p in programs:
        mask = mf.transformer_inputs(p)["mask"]
        if mask is not None:
            assert mask.dtype == np.float32 and mask.shape == ((1 if p["mask"] == "shared" else p["batch"]), p["S"]) and (mask[:, 0] == 1).all()
            if p["mask"] == "padding":
                lengths = [int(np.flatnonzero(row)[-1]) + 1 for row in mask]
                assert len(set(lengths)) == len(lengths) and all(n < p["S"] for n in lengths)
                assert sum(int((row[:n] == 0).sum()) for row, n in zip(mask, lengths)) == 1          # the one hole


def test_the_cnn_draw_visits_everything():
    programs = [mf.draw_cnn(s) for s in CNN_SEEDS]
    pairs = collections.Counter(pair for p in programs for pair in set(mf.stage_pairs(p)))
    for op in ("conv", "bn", "pool", "reshape"):           # a relu in front of and behind each of them
        assert pairs[("relu", op)] >= 3 and pairs[(op, "relu")] >= 3, (op, pairs)
    convs = [op for p in programs for op in p["ops"] if op["op"] == "conv"]
    for name, key, values in (("out", "cout", (2, 5, 8, 33)), ("kernel", "k", (1, 2, 3, 5)), ("stride", "stride", (1, 2, (2, 1))),
                              ("pad", "pad", (0, 1, 2)), ("bias", "bias", (False, True))):
        seen = collections.Counter(op[key] for op in convs)
        assert all(seen[v] >= 3 for v in values), (name, seen)
    ops = [op for p in programs for op in p["ops"]]
    assert sum(op["op"] == "bn" and op["affine"] for op in ops) >= 3 and sum(op["op"] == "bn" and not op["affine"] for op in ops) >= 3
    for kind in ("max_pool", "min_pool"):
        for kernel in ((2, 2), (2, 3)):
            assert sum(op["op"] == "pool" and op["kind"] == kind and tuple(op["kernel"]) == kernel for op in ops) >= 3, (kind, kernel)
    assert sum(op["op"] == "residual" for op in ops) >= 3 and sum(p["bn1d"] for p in programs) >= 3
    assert sum(op["op"] == "act" and op["kind"] == "tanh" for op in ops) >= 3
    for name, key, values in (("N", lambda p: p["x_shape"][0], (1, 2, 5)), ("C", lambda p: p["x_shape"][1], (1, 3)),
                              ("loss", lambda p: p["loss"], ("mse", "ce", "weighted")), ("stages", lambda p: sum(o["op"] == "begin" for o in p["ops"]), (1, 2, 3)),
                              ("linears", lambda p: p["hidden"] is None, (False, True)), ("steps", lambda p: p["steps"], (0, 1, 2, 3)),
                              ("form", lambda p: p["form"] if p["optimizer"] != "none" else "tape", mf.FORMS)):
        seen = count(programs, key)
        assert all(seen[v] >= 3 for v in values), (name, seen)
    assert sum(p["x_shape"][2] != p["x_shape"][3] for p in programs) >= 3
    assert all(6 <= p["x_shape"][2] <= 14 and 6 <= p["x_shape"][3] <= 14 for p in programs)
    assert sum(p["outs"] <= 16 and p["loss"] == "mse" for p in programs) >= 3           # skinny enough for the head kernels


def test_a_program_is_a_pure_function_of_its_seed():
    for draw, seeds in ((mf.draw_transformer, TRANSFORMER_SEEDS), (mf.draw_cnn, CNN_SEEDS)):
        for seed in seeds:
            np.random.seed(seed + 1)                       # the global stream is none of its inputs
            first = draw(seed)
            np.random.seed(seed + 2)
            assert draw(seed) == first and first["seed"] == seed
    a, b = mf.transformer_inputs(mf.draw_transformer(7)), mf.transformer_inputs(mf.draw_transformer(7))
    assert all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in a)
