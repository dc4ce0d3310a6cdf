"""Differential fuzzing of the HIP backend on whole models (tests/model_fuzz.py): random BertForMaskedLM and CNN training programs
over the ingredients the backend answers with something other than one kernel per op, each run on the float64 tape, on CpuTensor
in float32 and on HipTensor, and judged by the project's own yardsticks (model_fuzz.judge).  A failure names the seed and prints
the whole program: `mf.draw_transformer(seed)` / `mf.draw_cnn(seed)` gives it back, and `run_one` below runs it alone."""
import collections
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor, random as lrandom
import model_fuzz as mf
from test_hip_attention_dropout import _tape_nodes
from test_model_fuzz_cpu import TRANSFORMER_SEEDS, CNN_SEEDS, MAX_FILTERED

pytestmark = pytest.mark.gpu

BLOCK = 10
TAKEN = {}                      # (family, seed) -> the set of fused forms the HIP run of that program took
TALLY = {"transformer": collections.Counter(), "cnn": collections.Counter()}
WORST = {"transformer": {}, "cnn": {}}
ATTENTION_NODES = {"self_attention": "self_attention", "attention": "attention", "masked_attention": "attention", "long_attention": "attention"}


def _is_lazy_relu(t):
    return t._data is None and t._lazy_source is not None and t._lazy_source[0] == "relu"


def forms_taken(prog, out, loss):
    """what the tape behind `loss` (walked before anything is read) says the backend did for this program"""
    from lightgrad_amd.autograd.hip.ops import conv2d_last_plan, batchnorm_last_plan
    taken, relu_in_front = set(), {"conv2d": [], "batch_norm": []}
    for ctx in _tape_nodes(loss):
        name = type(ctx).__name__
        if name in ATTENTION_NODES:
            saved = ctx.get_saved_tensors()
            form, dropout = (saved[5], saved[6]) if name == "self_attention" else ({"attention": "plain", "masked_attention": "masked", "long_attention": "long"}[name], saved[6])
            if prog["causal"]:
                family = "causal_long" if form == "long" else "causal_short"
            else:
                family = {"plain": "plain", "masked": "tail", "long": "long"}[form]
            taken.add("%s/%s/%s" % (ATTENTION_NODES[name], family, "dropout" if dropout > 0 else "nodropout"))
        elif name == "feed_forward":
            taken.add("feed_forward/residual" if len(ctx._parents) > 5 and ctx._parents[5] is not None else "feed_forward/plain")
        elif name in ("dropout_add_layer_norm", "layer_norm_dropout", "embedding_sum"):
            taken.add(name)
        elif name == "softmax" and prog["family"] == "transformer":
            taken.add("composite")
            if ctx.get_saved_tensors()[2] != 1.0:
                taken.add("composite/scaled_softmax")
        elif name in relu_in_front:
            relu_in_front[name].append(_is_lazy_relu(ctx._parents[0]))
    # the launches' own record of the most recent call: the forward of the last convolution / BatchNorm of this pass
    for name, plan in (("conv2d", conv2d_last_plan), ("batch_norm", batchnorm_last_plan)):
        if relu_in_front[name] and any(relu_in_front[name]):
            taken.add(name + "/relu_x")
            if all(relu_in_front[name]):
                assert plan()["relu_x"], "seed %d: every %s reads a still-lazy relu, the last launch says relu_x = 0: %r" % (prog["seed"], name, plan())
    if loss._data is None and loss._lazy_source is not None and loss._lazy_source[0] == "mse_rows":
        taken.add("head")                                  # csrc/head.hip computed the output layer together with the loss
    return taken


def run_on_hip(hip, prog):
    """(observables, None), or (None, the contract's error text) where the optimizer form refuses the program by contract"""
    from lightgrad_amd.autograd.hip import HipError
    made, taken = [], set()
    inner = mf.prepare_for(prog)

    def prepare(model, make_opt, parameters):
        opt = inner(model, make_opt, parameters)
        made.append(opt)
        return opt

    def probe(out, loss):
        taken.update(forms_taken(prog, out, loss))
    refusable = prog["form"] == "in_backward" and prog["optimizer"] != "none" and (
        prog["second_backward"] or prog["zero_grad"] != "before_backward" or prog["recipe"] is not None)
    try:
        got = mf.run_program(hip, prog, prepare=prepare if inner is not None else None, probe=probe)
    except (HipError, AssertionError, RuntimeError) as e:
        text = [t for t in mf.REFUSAL_TEXTS if t in str(e)]
        if not (refusable and text):
            raise
        if made and made[0]._backward_update is not None:
            made[0]._backward_update.disarm()
        return None, text[0]
    TAKEN[(prog["family"], prog["seed"])] = taken
    if prog["family"] == "transformer":
        expected = mf.attention_form(prog)
        assert expected in taken, "seed %d: expected the attention of every layer as %s, the tape holds %s\nprogram: %r" % (
            prog["seed"], expected, sorted(taken), prog)
    return got, None


def run_one(hip, prog):
    """one program through the three runs and the judge: "refused" | "filtered" | "ok" """
    got, refused = run_on_hip(hip, prog)
    tally = TALLY[prog["family"]]
    if refused is not None:
        tally["refused"] += 1
        return "refused"
    ref64 = mf.run_program(CpuTensor, prog, dtype=np.float64)
    cpu32 = mf.run_program(CpuTensor, prog)
    verdict = mf.judge(ref64, cpu32, got, prog)
    tally[verdict["status"]] += 1
    mf.merge_worst(WORST[prog["family"]], verdict["worst"])
    return verdict["status"]


def run_block(hip, draw, seeds):
    outcome = collections.Counter(run_one(hip, draw(seed)) for seed in seeds)
    print("seeds %d..%d: %s" % (seeds[0], seeds[-1], dict(outcome)))
    assert outcome["filtered"] <= MAX_FILTERED * len(seeds), outcome
    assert outcome["ok"] + outcome["refused"] >= (1 - MAX_FILTERED) * len(seeds), outcome        # ran, or answered by contract


@pytest.mark.parametrize("block", range(len(TRANSFORMER_SEEDS) // BLOCK))
def test_transformer_programs(hip, block):
    run_block(hip, mf.draw_transformer, TRANSFORMER_SEEDS[block * BLOCK:(block + 1) * BLOCK])


@pytest.mark.parametrize("block", range(len(CNN_SEEDS) // BLOCK))
def test_cnn_programs(hip, block):
    run_block(hip, mf.draw_cnn, CNN_SEEDS[block * BLOCK:(block + 1) * BLOCK])


def graph_candidates(exact):
    """programs with nothing read on the host inside the step and a fused optimizer with its step number on the device.
    exact: the programs whose replay must give the bits of the eager steps - every CNN, and the transformers of at most 32
    tokens: an embedding row that receives more than 32 ids of a batch (token type 0, the padding or the mask token) is summed
    with float atomics ("Determinism": the one kernel whose bits may differ from run to run), and after one update
    every value follows; up to 32 tokens no row can.  Otherwise: transformers beyond that, one per stratum of the draw in turn"""
    picked = []
    for draw, seeds, want in ((mf.draw_transformer, TRANSFORMER_SEEDS, 9 if exact else 10), (mf.draw_cnn, CNN_SEEDS, 7 if exact else 0)):
        family = []
        for seed in seeds:
            prog = draw(seed)
            if prog["family"] == "transformer" and (prog["batch"] * prog["S"] <= 32) != exact:
                continue
            if not exact and prog.get("decoder_precision") == "bf16":
                continue                                   # (a last-place difference may cross a bfloat16 rounding boundary: model_fuzz.draw_transformer)
            flat = seed % 2 == 1
            variant = dict(prog, peek="none", second_backward=False, zero_grad="before_backward", eval_after=False, steps=5,
                           optimizer=prog["optimizer"] if prog["optimizer"] != "none" else "adam", form="flat" if flat else "device_step",
                           # (without flat buckets a recipe is the expression form, which reads the gradient norm on the host)
                           recipe=prog["recipe"] if flat and prog["optimizer"] != "none" else None)
            if variant.get("objective") != "mlm" or mf.masking_selects_something(variant):       # (five steps: five token maskings)
                family.append(variant)
        picked += family[:want]
    return picked


def eager_and_replayed(hip, prog):
    """(values after five eager steps, values after one eager step, one capture and four replays) of parameters and buffers;
    the random stream stands where five steps leave it either way (dropout and the token masking draw inside the recorded
    step, afresh at every replay)"""
    from lightgrad_amd.autograd.hip import GraphedStep
    what = "seed %d %r" % (prog["seed"], prog)
    light.manual_seed(prog["seed"])
    eager = mf.build(hip, prog, prepare=mf.prepare_for(prog))
    for _ in range(5):
        eager.iteration()
    want_state = lrandom.get_state("hip")
    want = [(n, t.numpy()) for n, t in list(eager.model.named_parameters()) + list(eager.model.named_buffers())]
    light.manual_seed(prog["seed"])
    graphed = mf.build(hip, prog, prepare=mf.prepare_for(prog))
    step = GraphedStep(graphed.iteration, optimizers=[graphed.opt], warmup=1)
    for _ in range(5):
        loss = step()
    assert np.isfinite(loss.item()), what
    assert lrandom.get_state("hip") == want_state, (lrandom.get_state("hip"), want_state, what)
    if prog["family"] == "transformer":
        assert want_state == (prog["seed"], 5 * mf.draws_per_forward(prog)), (want_state, what)
    have = [(n, t.numpy()) for n, t in list(graphed.model.named_parameters()) + list(graphed.model.named_buffers())]
    step.destroy()
    assert [n for n, _ in have] == [n for n, _ in want]
    return want, have, what


def test_programs_replayed_from_a_graph(hip):
    """one eager step, one capture, four replays: the bits of five eager HIP steps under the same seed - parameters, BatchNorm
    buffers and the random stream"""
    ran = 0
    for prog in graph_candidates(exact=True):
        want, have, what = eager_and_replayed(hip, prog)
        for (n, a), (_, b) in zip(have, want):
            np.testing.assert_array_equal(a, b, err_msg="%s of %s" % (n, what))
        ran += 1
    assert ran >= 12


def test_longer_programs_replayed_from_a_graph(hip):
    """the same for the transformers whose embedding gradient is summed with float atomics (more than 32 tokens: see
    graph_candidates): the replays are a second float32 run of the trajectory, held to the tolerances two float32 runs of one
    are held to everywhere here (tape_fuzz.compare); the random stream is exact"""
    ran = 0
    for prog in graph_candidates(exact=False):
        want, have, what = eager_and_replayed(hip, prog)
        mf.compare([(n, a.astype(np.float64)) for n, a in want], [(n, a.astype(np.float64)) for n, a in have], what=what)
        ran += 1
    assert ran >= 8


REQUIRED = ["self_attention/%s/%s" % (family, drop) for family in ("plain", "tail", "long", "causal_short", "causal_long")
            for drop in ("dropout", "nodropout")] + [
    "dropout_add_layer_norm", "layer_norm_dropout", "feed_forward/residual", "feed_forward/plain", "embedding_sum",
    "conv2d/relu_x", "batch_norm/relu_x", "head", "composite", "composite/scaled_softmax"]


def test_the_fused_nodes_were_taken(hip):
    """over the whole seed range every fused form ran in at least three programs - and so did the composite (d = 16): the
    programs above did not pass by quietly falling back.  Programs the tests above have not run in this session (a single test
    selected) get a forward pass here."""
    for draw, seeds in ((mf.draw_transformer, TRANSFORMER_SEEDS), (mf.draw_cnn, CNN_SEEDS)):
        for seed in seeds:
            prog = draw(seed)
            if (prog["family"], seed) not in TAKEN:
                light.manual_seed(seed)
                out, loss, _ = mf.build(hip, dict(prog, optimizer="none", steps=0)).forward(True)
                TAKEN[(prog["family"], seed)] = forms_taken(prog, out, loss)
    programs = collections.Counter(form for taken in TAKEN.values() for form in taken)
    for form, n in sorted(programs.items()):
        print("%-44s %3d programs" % (form, n))
    for family in ("transformer", "cnn"):
        print(family, dict(TALLY[family]))
        for group, (e_hip, e_cpu) in sorted(WORST[family].items()):
            print("  %-14s hip %.3g  float32 CPU %.3g from float64" % (group, e_hip, e_cpu))
    short = {form: programs[form] for form in REQUIRED if programs[form] < 3}
    assert not short, short
