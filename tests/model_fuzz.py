"""Differential fuzzing of whole models: the same randomly drawn transformer or CNN training program on CpuTensor in float64 (the
yardstick), on CpuTensor in float32 and on another backend, every observable compared.

Why: tests/tape_fuzz.py draws MLP programs only.  Most of the HIP backend's peepholes since then belong to the transformer
(`self_attention` in its five launch families, dropout of the probabilities inside them, `dropout_add_layer_norm`,
`layer_norm_dropout`, the one-node `feed_forward`, `embedding_sum`, the gathered `masked_positions` head, `ignore_index`
cross-entropy, the bf16 decoder, the AdamW / clipping / schedule recipe) and to the CNN (a lazy relu folded into `conv2d`,
`batch_norm` and pooling, BatchNorm's running statistics).  Each has a sweep of its own at the configuration it was built for;
examples/bert.py picks among a dozen branches per layer from the configuration, and a wrong answer that needs two features at
once - causal + padding mask + attention dropout at 129 positions, eval() after a step with hidden dropout, a lazy relu in front
of a BatchNorm that feeds a strided conv, a random-stream call count that differs once three dropout sites and the token masking
share it - is what a program here is made of.

    draw_transformer(seed) -> prog      draw_cnn(seed) -> prog        # plain dicts, numpy RandomState(seed) only
    run_program(T, prog, dtype=np.float32, prepare=None) -> [(label, float64 array)]
    judge(ref64, cpu32, got, prog)                                    # raises, naming seed, label and the three distances

The masked-LM objective is `mlm_forward_backward` of examples/bert.py spelled out (token masking at p = 0.3, prediction, the
ignoring cross-entropy): the example's own function names mask token 103 of the public vocabulary, which the vocabularies here
(50, 61, 130 tokens) do not all hold, and zeroes the gradients itself, which is one of the habits drawn here.  KV-cache `generate`
is not drawn: greedy choices at near-ties are nothing two correct backends must agree on (tests/test_hip_decode.py covers it).

Used by tests/test_model_fuzz_cpu.py (the generator itself, and the share of programs the float32-vs-float64 rule sets aside) and
tests/test_hip_model_fuzz.py (GPU)."""
import importlib.util
import os
import numpy as np
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor, random as lrandom
from common import float64_tape, rel_frobenius, assert_as_close_to_float64_as_the_cpu_backend
from tape_fuzz import compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("bert_example_model_fuzz", os.path.join(ROOT, "examples", "bert.py"))
bert = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bert)

S_SHORT, S_LONG = (1, 5, 31, 32, 33, 64, 100, 127, 128), (129, 160, 257)
S_VALUES = S_SHORT + S_LONG
MASK_KINDS = ("none", "padding", "shared", "ones")
OBJECTIVES = ("mlm", "positions", "clm", "sqlogits", "hidden")
FORMS = ("tape", "fused", "device_step", "flat", "in_backward")       # how the optimizer runs on the HIP backend
MLM_P, IGNORE = 0.3, -100
# error texts of the contracts a form refuses a program by (lightgrad_amd/optim.py, autograd/hip/tensor.py)
REFUSAL_TEXTS = ("again after its optimizer update was applied", "without zero_grad() + backward() before it",
                 "cannot ride in the backward kernels")


def _choice(rng, values, p=None):
    return values[int(rng.choice(len(values), p=p))]


# ---- transformer programs ---------------------------------------------------------------------------------------------------
def draws_per_forward(prog):
    """calls of the random stream in one training forward: the token masking, the dropout behind the embedding LayerNorm and the
    two of every layer, the dropout of every layer's attention probabilities"""
    layers = prog["layers"]
    return (1 if prog["objective"] == "mlm" else 0) + (1 + 2 * layers if prog["hidden_p"] > 0 else 0) + (layers if prog["attention_p"] > 0 else 0)


def training_forwards(prog):
    return max(1, prog["steps"]) * (2 if prog["second_backward"] else 1)


def attention_form(prog):
    """the node and launch family examples/bert.py and csrc/attention.hip (pick_form) take for this program on the HIP backend"""
    if prog["d"] == 16:
        return "composite"
    node = "self_attention" if (prog["heads"] * prog["d"]) % 64 == 0 else "attention"
    long = prog["S"] > 128
    if prog["causal"]:
        family = "causal_long" if long else "causal_short"
    elif long:
        family = "long"
    else:
        family = "plain" if prog["mask"] == "none" and prog["S"] % 32 == 0 else "tail"
    return "%s/%s/%s" % (node, family, "dropout" if prog["attention_p"] > 0 else "nodropout")


def transformer_inputs(prog):
    """ids (b, s) int32 with 0 = [PAD] at the padded positions, the attention mask (float32 or None), token types (int32 or None),
    the gathered form's flat positions and labels (static length, padded slots carry IGNORE), the weights of the hidden-state sum"""
    b, s, vocab = prog["batch"], prog["S"], prog["vocab"]
    rng = np.random.RandomState(prog["ids_seed"])
    ids = rng.randint(1, vocab - 1, (b, s)).astype(np.int32)             # vocab - 1 is the mask token, 0 the padding
    mask = None
    if prog["mask"] == "ones":
        mask = np.ones((b, s), np.float32)
    elif prog["mask"] in ("padding", "shared"):
        rows = b if prog["mask"] == "padding" else 1
        mask = np.ones((rows, s), np.float32)
        lengths = rng.permutation(np.arange(max(3, s // 2), s))[:rows]   # trailing padding of a different length per row
        for r, n in enumerate(lengths):
            mask[r, n:] = 0
        r = int(rng.randint(rows))
        mask[r, int(rng.randint(1, lengths[r] - 1))] = 0                 # one hole; key 0 is never masked
        ids = np.where(np.broadcast_to(mask, (b, s)) > 0, ids, 0).astype(np.int32)
    types = rng.randint(0, 2, (b, s)).astype(np.int32) if prog["token_types"] else None
    slots = max(1, int(np.ceil(0.3 * s)))
    positions, labels = np.zeros((b, slots), np.int32), np.full((b, slots), IGNORE, np.int64)
    masked_ids = ids.copy()
    for r in range(b):
        live = np.flatnonzero(ids[r] != 0)
        take = np.sort(rng.permutation(live)[:max(1, int(rng.randint(1, slots + 1)))])
        positions[r, :len(take)] = r * s + take
        labels[r, :len(take)] = ids[r, take]
        masked_ids[r, take] = vocab - 1
    weights = (rng.uniform(-1, 1, (b, s, prog["heads"] * prog["d"])) / (b * s)).astype(np.float32)
    return {"ids": ids, "mask": mask, "types": types, "positions": positions.reshape(-1), "position_labels": labels.reshape(-1),
            "masked_ids": masked_ids, "weights": weights}


def masking_selects_something(prog):
    """the draw's own check (CPU arithmetic only): every training forward's token masking selects at least one position"""
    ids, per = transformer_inputs(prog)["ids"], draws_per_forward(prog)
    for k in range(training_forwards(prog)):
        _, labels = lrandom.mlm_mask_words(prog["seed"], k * per, ids, MLM_P, prog["vocab"] - 1, prog["vocab"], special_ids=(0,), ignore_index=IGNORE)
        if not (labels != IGNORE).any():
            return False
    return True


def draw_transformer(seed):
    """the random choices of one BertForMaskedLM configuration and its training step, independent of the backend.  seed % 5 picks
    the stratum: 0 - a length and configuration the plain attention kernels take (no mask, not causal, 32 | S); 4 - beyond 128
    positions at batch 1 (a fifth of the programs); the others draw freely among the short lengths"""
    rng = np.random.RandomState(seed)
    stratum = seed % 5
    plain, long = stratum == 0, stratum == 4
    if long:
        S, batch = _choice(rng, S_LONG, [0.4, 0.35, 0.25]), 1
    elif plain:
        S, batch = _choice(rng, (32, 64, 128), [0.5, 0.3, 0.2]), _choice(rng, (1, 2, 3), [0.3, 0.5, 0.2])
    else:
        S = _choice(rng, S_SHORT, [0.1, 0.16, 0.14, 0.1, 0.16, 0.08, 0.1, 0.1, 0.06])
        batch = _choice(rng, (1, 2, 3), [0.3, 0.5, 0.2]) if S < 100 else _choice(rng, (1, 2), [0.5, 0.5])
    d = _choice(rng, (16, 32, 64), [0.15, 0.5, 0.35])
    heads = _choice(rng, (1, 2, 3), [0.3, 0.5, 0.2])
    causal = bool(rng.rand() < 0.5) and not plain
    attention_p = _choice(rng, (0.0, 0.1), [0.5, 0.5])
    if long:
        # two dozen programs have to visit the long and the causal long launches with and without dropout: the four
        # combinations in turn, at widths `self_attention` takes more often than not
        causal, attention_p = bool((seed // 5) % 2), (0.0, 0.1)[(seed // 10) % 2]
        d = _choice(rng, (32, 64), [0.3, 0.7])
        heads = _choice(rng, (1, 2, 3), [0.2, 0.6, 0.2]) if d == 32 else heads
    mask = "none" if plain else _choice(rng, MASK_KINDS, [0.3, 0.35, 0.2, 0.15])
    if S < 5 and mask in ("padding", "shared"):
        mask = "ones"                                          # one position: nothing to pad
    if mask == "padding" and batch > S - max(3, S // 2):
        mask = "shared"
    steps = _choice(rng, (0, 1, 2, 3), [0.2, 0.4, 0.25, 0.15])
    if long:
        steps = min(steps, 2)
    form = _choice(rng, FORMS, [0.15, 0.2, 0.2, 0.3, 0.15])
    objectives = ((0.2, 0.2, 0.35, 0.15, 0.1) if causal and S >= 2 else (0.35, 0.3, 0.0, 0.2, 0.15))
    prog = {
        "family": "transformer", "seed": int(seed), "batch": int(batch), "S": int(S), "heads": int(heads), "d": int(d),
        "layers": _choice(rng, (1, 2), [0.65, 0.35]), "intermediate": _choice(rng, (64, 128, 40, 100, 50)), "vocab": _choice(rng, (50, 61, 130)),
        "mask": mask, "causal": causal,
        "hidden_p": _choice(rng, (0.0, 0.1, 0.5), [0.4, 0.35, 0.25]), "attention_p": attention_p,
        "token_types": bool(rng.rand() < 0.4), "decoder_precision": "bf16" if rng.rand() < 0.12 and batch * S <= 100 else None,
        "objective": _choice(rng, OBJECTIVES, list(objectives)),
        "peek": _choice(rng, ("none", "logits", "probs"), [0.6, 0.2, 0.2]),       # a host read before backward
        "second_backward": bool(rng.rand() < 0.2),
        "zero_grad": _choice(rng, ("before_backward", "before_backward", "after_step", "never")),
        "steps": int(steps), "optimizer": _choice(rng, ("adam", "adabelief")) if steps else "none", "form": form,
        "recipe": None, "eval_after": bool(rng.rand() < 0.4),
    }
    if rng.rand() < 0.35:
        prog["recipe"] = {"weight_decay": _choice(rng, (0.0, 0.01, 0.01)), "decay_mask": _choice(rng, ("matrices", "even")),
                          "max_grad_norm": _choice(rng, (None, 0.5)), "schedule": _choice(rng, (None, (1, 4)))}
        if prog["recipe"]["weight_decay"] == 0 and prog["recipe"]["max_grad_norm"] is None and prog["recipe"]["schedule"] is None:
            prog["recipe"]["schedule"] = (1, 4)
    if prog["decoder_precision"] == "bf16":
        # rounding to bfloat16 is a step function of the operands: after an update the decoder's weights differ between two
        # correct float32 backends in the last place, an operand that crosses a rounding boundary moves a logit by 2^-9 of one
        # of its terms, and no yardstick here resolves that.  The bf16 programs are judged on what precedes the first update.
        prog.update(steps=0, optimizer="none", eval_after=False)
    if prog["optimizer"] == "none":
        prog["recipe"] = None
    if form == "in_backward" and rng.rand() < 0.6:
        prog.update(zero_grad="before_backward", second_backward=False, recipe=None)        # what that form's contract takes
    if prog["objective"] == "hidden":
        prog["decoder_precision"] = None                       # the head is absent
        if prog["peek"] == "logits":
            prog["peek"] = "probs"
    prog["ids_seed"] = int(rng.randint(1 << 30))
    if prog["objective"] == "mlm":
        for _ in range(50):
            if masking_selects_something(prog):
                break
            prog["ids_seed"] = int(rng.randint(1 << 30))
        else:
            prog["objective"] = "sqlogits"                     # (one token per row and 50 unlucky draws)
    return prog


def _hip_optimizer_kw(prog):
    return {"tape": {}, "fused": {"fused": True}}.get(prog["form"], {"fused": True, "device_step": True})


def prepare_for(prog):
    """run_program's `prepare` for the optimizer forms that need more than constructor arguments: flat buckets through
    DataParallel(..., SingleProcess(), flatten=True), and the update inside the backward kernels on top of them"""
    if prog["optimizer"] == "none" or prog["form"] not in ("flat", "in_backward"):
        return None

    def prepare(model, make_opt, parameters):
        from lightgrad_amd.dist import DataParallel, SingleProcess
        dp = DataParallel(parameters, SingleProcess(), flatten=True)
        opt = make_opt(parameters)
        dp.attach(opt)
        if prog["form"] == "in_backward":
            opt.fuse_update_into_backward()
        return opt
    return prepare


def _make_optimizer(T, prog, parameters, prepare, model):
    if prog["optimizer"] == "none":
        return None

    def make_opt(params):
        params = tuple(params)
        cls = light.optim.Adam if prog["optimizer"] == "adam" else light.optim.AdaBelief
        kw = {} if T is CpuTensor else _hip_optimizer_kw(prog)
        recipe = prog["recipe"]
        if recipe is not None:
            kw["weight_decay"] = recipe["weight_decay"]
            kw["decay_mask"] = None if recipe["decay_mask"] == "matrices" else [i % 2 == 0 for i in range(len(params))]
            kw["max_grad_norm"] = recipe["max_grad_norm"]
            kw["schedule"] = None if recipe["schedule"] is None else light.optim.WarmupLinear(*recipe["schedule"])
        return cls(params, lr=1e-2, eps=1e-3, **kw)
    return prepare(model, make_opt, parameters) if prepare is not None else make_opt(parameters)


def _to_backend(T, model):
    if T is not CpuTensor:
        model.map_parameters(lambda p: getattr(p, T.__module__.split(".")[-2])())        # p.hip()
    return model


def _initial_values(model, rng):
    """float32 start values: what the constructors drew, and the constants (LayerNorm / BatchNorm scale 1 and shift 0, the zero
    vocabulary bias) moved off their special values so that they matter"""
    values = []
    for n, p in model.named_parameters():
        a = p.numpy().astype(np.float32)
        if a.ndim == 1 and (np.all(a == 0) or np.all(a == 1)):
            a = (a + rng.uniform(-0.2, 0.2, a.shape)).astype(np.float32)
        values.append((n, a))
    return values


class _Program(object):
    """one program built on one backend: `iteration(see)` is one training step (`see` None: nothing is read on the host)"""


def build_transformer(T, prog, dtype=np.float32, prepare=None, probe=None):
    inputs = transformer_inputs(prog)
    b, s, vocab, hidden = prog["batch"], prog["S"], prog["vocab"], prog["heads"] * prog["d"]
    np.random.seed(prog["seed"])                     # the constructors draw from numpy's global stream
    model = bert.BertForMaskedLM(hidden_size=hidden, intermediate_size=prog["intermediate"], num_hidden_layers=prog["layers"],
                                 num_attention_heads=prog["heads"], vocab_size=vocab, max_position_embeddings=s, type_vocab_size=2,
                                 hidden_dropout_prob=prog["hidden_p"], attention_probs_dropout_prob=prog["attention_p"],
                                 causal=prog["causal"], decoder_precision=prog["decoder_precision"])
    model.load_parameters([(n, a.astype(dtype)) for n, a in _initial_values(model, np.random.RandomState(2000 + prog["seed"]))])
    assert all(p.dtype == dtype for p in model.parameters())
    _to_backend(T, model)
    trained = model.bert if prog["objective"] == "hidden" else model
    me = _Program()
    me.model, me.trained = model, trained
    me.opt = _make_optimizer(T, prog, list(trained.parameters()), prepare, model)

    def const(a, floating=False):
        return None if a is None else T.from_numpy(a.astype(dtype) if floating else a, requires_grad=False)
    ids, mask, types = const(inputs["ids"]), const(inputs["mask"], True), const(inputs["types"])
    masked_ids, positions, position_labels = const(inputs["masked_ids"]), const(inputs["positions"]), const(inputs["position_labels"])
    weights = const(inputs["weights"], True)

    def encode(tokens):
        """model.bert(...) layer by layer, so that the probabilities of layer 0 can be looked at"""
        h = model.bert.embeddings(tokens, token_type_ids=types)
        probs0 = None
        for k, layer in enumerate(model.bert.encoder.layer):
            h, probs = layer(h, attention_mask=mask)
            probs0 = probs if k == 0 else probs0
        return h, probs0

    def forward(training):
        """(output, loss or None, the probabilities of layer 0 or None)"""
        objective, probs0, labels = prog["objective"], None, None
        tokens = ids
        if objective == "mlm" and training:
            tokens, labels = light.data.mask_tokens(ids, MLM_P, vocab - 1, vocab, special_ids=(0,), ignore_index=IGNORE)
        elif objective == "positions":
            tokens = masked_ids
        gather = {"masked_positions": positions} if objective == "positions" else {}
        if objective == "hidden" or prog["peek"] == "probs":
            h, probs0 = encode(tokens)
            if objective == "hidden":
                return h, (h * weights).sum() if training else None, probs0
            if gather:
                h = h.reshape(-1, hidden)[positions]
            logits = model.head(h)
        else:
            logits = model(tokens, attention_mask=mask, token_type_ids=types, **gather)
        if not training:
            return logits, None, probs0
        if objective == "sqlogits":
            loss = (logits * logits).mean()
        else:
            if objective == "clm":
                labels = light.data.next_token_labels(ids, ignore_index=IGNORE)
            elif objective == "positions":
                labels = position_labels
            loss = light.loss.cross_entropy(logits.reshape(-1, vocab), labels.reshape(-1), ignore_index=IGNORE)
        return logits, loss, probs0
    me.forward = forward
    _add_iteration(me, prog, probe)
    return me


def _add_iteration(me, prog, probe):
    """the tape habits shared by both families: a host read before backward, a second forward / backward that accumulates,
    zero_grad before backward / after the step / never, the optimizer step"""
    parameters = list(me.trained.parameters())

    def zero_grad():
        if me.opt is not None:
            me.opt.zero_grad()
        else:
            for p in parameters:
                p.zero_grad()

    def iteration(see=None, tag=""):
        out, loss, probs0 = me.forward(True)
        if probe is not None:
            probe(out, loss)
        if see is not None and prog["peek"] == "logits":
            see(tag + "/peek/out", out)                # before backward: lazy tensors become real
        if see is not None and prog["peek"] == "probs" and probs0 is not None:
            see(tag + "/peek/attention_probs", probs0)
        if prog["zero_grad"] == "before_backward":
            zero_grad()
        loss.backward()
        if prog["second_backward"]:
            me.forward(True)[1].backward()             # parameter gradients accumulate over the two passes
        if see is not None:
            see(tag + "/loss", loss)
            see(tag + "/out", out)
            for n, p in me.trained.named_parameters():
                see("%s/grad/%s" % (tag, n), p.grad)
            if getattr(me, "x", None) is not None:
                see(tag + "/grad/x", me.x.grad)
        if me.opt is not None:
            me.opt.step()
        if prog["zero_grad"] == "after_step":
            zero_grad()
        if see is not None:
            if me.opt is not None:
                for n, p in me.trained.named_parameters():
                    see("%s/param/%s" % (tag, n), p)
            for n, t in me.model.named_buffers():
                see("%s/buffer/%s" % (tag, n), t)
        return loss
    me.iteration = iteration


# ---- CNN programs ------------------------------------------------------------------------------------------------------------
def _conv_out(h, w, k, stride, pad):
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    if k > h + 2 * pad or k > w + 2 * pad:                     # what conv_params (csrc/conv.hip) refuses
        return None
    return (h + 2 * pad - k) // sh + 1, (w + 2 * pad - k) // sw + 1


def draw_cnn(seed):
    """one to three stages of conv / batch norm / pooling / activation in a drawn order, a residual add where the shapes agree,
    reshape, one or two Linear layers.  A bias (or an affine BatchNorm) whose constant reaches a BatchNorm as a constant has a
    gradient of zero in exact arithmetic - rounding noise that no yardstick resolves and that an optimizer would normalise into
    steps: such a convolution or Linear has no bias and such a BatchNorm is not affine, as in any CNN with batch normalisation
    (the pass at the end of this function says what passes a constant on)"""
    rng = np.random.RandomState(seed)
    n, c = _choice(rng, (1, 2, 5), [0.2, 0.4, 0.4]), _choice(rng, (1, 3))
    h, w = int(rng.randint(6, 15)), int(rng.randint(6, 15))
    ops, shape = [], (c, h, w)
    x_shape = (n,) + shape
    for stage in range(int(rng.randint(1, 4))):
        kinds = ["conv"]
        if rng.rand() < 0.55:
            kinds.append("bn")
        if rng.rand() < 0.5:
            kinds.append("pool")
        act = _choice(rng, ("relu", "relu", "tanh", "none"))
        if act != "none":
            kinds.append("act")
        kinds = [kinds[i] for i in rng.permutation(len(kinds))]
        begin, first = shape, len(ops)
        ops.append({"op": "begin"})
        for kind in kinds:
            c, h, w = shape
            if kind == "conv":
                for _ in range(100):
                    out_c, k = _choice(rng, (2, 5, 8, 33), [0.3, 0.3, 0.3, 0.1]), _choice(rng, (1, 2, 3, 5), [0.2, 0.2, 0.4, 0.2])
                    stride, pad = _choice(rng, (1, 2, (2, 1)), [0.5, 0.3, 0.2]), _choice(rng, (0, 1, 2), [0.3, 0.5, 0.2])
                    size = _conv_out(h, w, k, stride, pad)
                    if size is not None and min(size) >= 1:
                        break
                else:
                    out_c, k, stride, pad, size = 5, 1, 1, 0, (h, w)
                ops.append({"op": "conv", "cin": c, "cout": out_c, "k": k, "stride": stride, "pad": pad, "bias": bool(rng.rand() < 0.75)})
                shape = (out_c,) + size
            elif kind == "bn":
                # statistics over a handful of values are noise, not a layer; behind a relu a channel with ONE live value among
                # a few is normalised to constants whatever the value, and its gradient is rounding noise
                before = next((o for o in reversed(ops) if o["op"] != "begin"), {"op": "input"})
                behind_relu = before["op"] == "act" and before["kind"] == "relu"
                if n * h * w >= (32 if behind_relu else 8):
                    ops.append({"op": "bn", "c": c, "affine": bool(rng.rand() < 0.7)})
            elif kind == "pool":
                kernel = _choice(rng, ((2, 2), (2, 3)))
                if kernel[0] <= h and kernel[1] <= w:
                    ops.append({"op": "pool", "kind": _choice(rng, ("max_pool", "max_pool", "min_pool")), "kernel": kernel})
                    shape = (c, h // kernel[0], w // kernel[1])
            else:
                ops.append({"op": "act", "kind": act})
        if shape == begin and len(ops) > first + 1 and rng.rand() < 0.7:
            ops.append({"op": "residual"})
    flat = shape[0] * shape[1] * shape[2]
    flat_act = _choice(rng, ("none", "relu"), [0.7, 0.3])              # an activation behind the reshape
    skinny = rng.rand() < 0.6
    outs = _choice(rng, (1, 2, 5, 10, 16)) if skinny else _choice(rng, (4, 24, 40))
    two = bool(rng.rand() < 0.6)
    hidden = _choice(rng, (8, 20, 32, 64)) if two else None
    bn1d = bool(two and n == 5 and rng.rand() < 0.4)
    prog = {
        "family": "cnn", "seed": int(seed), "x_shape": x_shape, "ops": ops, "flat": int(flat), "flat_act": flat_act,
        "hidden": hidden, "hidden_act": _choice(rng, ("relu", "relu", "tanh", "none")) if two else None, "bn1d": bn1d,
        "linear_bias": [bool(rng.rand() < 0.8) and not bn1d, bool(rng.rand() < 0.8)], "outs": int(outs),
        "loss": _choice(rng, ("mse", "mse", "ce", "weighted")) if outs >= 2 else "mse",
        "peek": _choice(rng, ("none", "logits"), [0.7, 0.3]), "second_backward": bool(rng.rand() < 0.2),
        "zero_grad": _choice(rng, ("before_backward", "before_backward", "after_step", "never")),
        "steps": _choice(rng, (0, 1, 2, 3), [0.15, 0.35, 0.3, 0.2]), "form": _choice(rng, FORMS, [0.15, 0.2, 0.2, 0.3, 0.15]),
        "recipe": None, "eval_after": True,
    }
    prog["optimizer"] = _choice(rng, ("adam", "adabelief")) if prog["steps"] else "none"
    if prog["form"] == "in_backward" and rng.rand() < 0.4:
        prog.update(zero_grad="before_backward", second_backward=False)                    # what that form's contract takes
    # a per-channel constant that reaches a BatchNorm as a per-channel constant takes no gradient: pooling, a convolution (all of it
    # without padding, all but its border with), the residual add and (into BatchNorm1d) reshape + Linear pass it on, and so
    # does tanh to first order at the small pre-activations of these networks (the float32 CPU run of such a bias gradient
    # is 3e-4 from the float64 one: cancellation, nothing to hold a second backend to); a relu does not
    chain = [op for op in ops if op["op"] not in ("begin", "residual")]

    def batch_norm_reached(j):
        """the BatchNorm a constant added behind op j - 1 reaches as a constant (True for the BatchNorm1d), or None"""
        while j < len(chain):
            if chain[j]["op"] == "bn":
                return chain[j]
            if chain[j]["op"] not in ("pool", "conv") and not (chain[j]["op"] == "act" and chain[j]["kind"] == "tanh"):
                return None
            j += 1
        return True if flat_act == "none" and bn1d else None
    # a BatchNorm also makes the weights in front of it scale-invariant: the gradient is orthogonal to them, and for a filter of
    # fewer than four weights that leaves (next to) nothing but rounding noise - such a BatchNorm is taken out of the program
    i = 0
    while i < len(chain):
        op, reached = chain[i], batch_norm_reached(i + 1)
        if op["op"] == "conv" and op["cin"] * op["k"] * op["k"] < 4 and isinstance(reached, dict):
            for ops_list in (chain, ops):
                del ops_list[next(j for j, o in enumerate(ops_list) if o is reached)]
            continue                                           # (the same convolution may reach the next BatchNorm now)
        i += 1
    for i, op in enumerate(chain):
        if op["op"] == "conv" and batch_norm_reached(i + 1) is not None:
            op["bias"] = False
        elif op["op"] == "bn" and batch_norm_reached(i + 1) is not None:
            op["affine"] = False
    return prog


def stage_pairs(prog):
    """the adjacent pairs of op kinds of a CNN program ("relu" and "tanh" for the activations, "reshape" at the end): where a
    still-lazy relu lands"""
    names = []
    for op in prog["ops"]:
        if op["op"] in ("begin", "residual"):
            continue
        names.append(op["kind"] if op["op"] == "act" else op["op"])
    names.append("reshape")
    if prog["flat_act"] != "none":
        names.append(prog["flat_act"])
    return list(zip(names[:-1], names[1:]))


class Cnn(nn.Module):
    def __init__(self, prog):
        nn.Module.__init__(self)
        self.spec = prog["ops"]
        made = []
        for op in self.spec:
            if op["op"] == "conv":
                layer = nn.Conv2d(op["cin"], op["cout"], kernelsize=op["k"], stride=op["stride"], pad=op["pad"], bias=op["bias"])
            elif op["op"] == "bn":
                layer = nn.BatchNorm2d(op["c"], affine=op["affine"])
            else:
                layer = nn.Module()
            made.append(layer)
        self.layers = nn.ModuleList(*made)
        first_out = prog["hidden"] if prog["hidden"] is not None else prog["outs"]
        self.l1 = nn.Linear(prog["flat"], first_out, bias=prog["linear_bias"][0])
        self.bn1 = nn.BatchNorm1d(first_out) if prog["bn1d"] else nn.Module()
        self.l2 = nn.Linear(prog["hidden"], prog["outs"], bias=prog["linear_bias"][1]) if prog["hidden"] is not None else nn.Module()
        self.flat, self.flat_act, self.hidden_act, self.two, self.bn1d = prog["flat"], prog["flat_act"], prog["hidden_act"], prog["hidden"] is not None, prog["bn1d"]

    def forward(self, x):
        h = begin = x
        for op, layer in zip(self.spec, self.layers):
            kind = op["op"]
            if kind == "begin":
                begin = h
            elif kind in ("conv", "bn"):
                h = layer(h)
            elif kind == "pool":
                h = getattr(h, op["kind"])(kernel=tuple(op["kernel"]))
            elif kind == "act":
                h = getattr(h, op["kind"])()
            else:
                h = h + begin
        h = h.reshape(-1, self.flat)
        if self.flat_act != "none":
            h = getattr(h, self.flat_act)()
        h = self.l1(h)
        if self.two:
            if self.bn1d:
                h = self.bn1(h)
            if self.hidden_act != "none":
                h = getattr(h, self.hidden_act)()
            h = self.l2(h)
        return h


def build_cnn(T, prog, dtype=np.float32, prepare=None, probe=None):
    rng = np.random.RandomState(1000 + prog["seed"])
    n, outs = prog["x_shape"][0], prog["outs"]
    np.random.seed(prog["seed"])
    model = Cnn(prog)
    model.load_parameters([(name, a.astype(dtype)) for name, a in _initial_values(model, np.random.RandomState(2000 + prog["seed"]))])
    model.load_buffers([(name, t.numpy().astype(dtype)) for name, t in model.named_buffers()])
    assert all(p.dtype == dtype for p in model.parameters())
    _to_backend(T, model)
    me = _Program()
    me.model = me.trained = model
    me.opt = _make_optimizer(T, prog, list(model.parameters()), prepare, model)
    x_np = rng.uniform(-1, 1, prog["x_shape"]).astype(dtype)
    target = T.from_numpy(rng.uniform(-1, 1, (n, outs)).astype(dtype), requires_grad=False)
    weights = T.from_numpy(rng.uniform(-1, 1, (n, outs)).astype(dtype), requires_grad=False)
    labels = T.from_numpy(rng.randint(0, outs, n).astype(np.int64), requires_grad=False)
    me.x = T.from_numpy(x_np, requires_grad=True)

    def forward(training):
        if not training:
            return model(me.x), None, None
        me.x.zero_grad()
        out = model(me.x)
        if prog["loss"] == "mse":
            loss = light.loss.mse(out, target)
        elif prog["loss"] == "ce":
            loss = light.loss.cross_entropy(out, labels)
        else:
            loss = (out * weights).sum()
        return out, loss, None
    me.forward = forward
    _add_iteration(me, prog, probe)
    return me


# ---- running and judging --------------------------------------------------------------------------------------------------------
def build(T, prog, dtype=np.float32, prepare=None, probe=None):
    return (build_cnn if prog["family"] == "cnn" else build_transformer)(T, prog, dtype, prepare, probe)


def backend_name(T):
    return "cpu" if T is CpuTensor else T.__module__.split(".")[-2]


def run_program(T, prog, dtype=np.float32, prepare=None, probe=None):
    """run `prog` on tensor class T (dtype float64: on the float64 tape); returns the ordered list of (label, float64 array) of
    everything observable, the last of them the backend's random-stream state after the run.
    prepare(model, optimizer_factory, parameters) -> optimizer lets a backend test choose an optimizer form (`prepare_for`);
    probe(output, loss) is called after every training forward, before anything is read (which kernels were taken)"""
    if np.dtype(dtype) == np.float64:
        assert T is CpuTensor
        with float64_tape():
            return _run(T, prog, np.float64, prepare, probe)
    return _run(T, prog, dtype, prepare, probe)


def _run(T, prog, dtype, prepare, probe):
    light.manual_seed(prog["seed"])
    me = build(T, prog, dtype, prepare, probe)
    out = []

    def see(label, t):
        out.append((label, np.array(t.numpy(), dtype=np.float64)))
    for step in range(max(1, prog["steps"])):
        me.iteration(see, "s%d" % step)
    state = lrandom.get_state(backend_name(T))
    if prog["family"] == "transformer":
        assert state == (prog["seed"], training_forwards(prog) * draws_per_forward(prog)), \
            "seed %d: the stream stands at %s after %d training forwards of %d calls each" % (
                prog["seed"], state, training_forwards(prog), draws_per_forward(prog))
    if prog["eval_after"]:
        me.model.eval()
        with light.no_grad():
            see("eval/out", me.forward(False)[0])
        me.model.train()
        moved = lrandom.get_state(backend_name(T))
        assert moved == state, "seed %d: a forward in eval() moved the random stream from %s to %s" % (prog["seed"], state, moved)
    out.append(("rng_state", np.array(state, dtype=np.float64)))
    return out


NOISE = ".key.bias"            # the key projection's bias: a gradient of zero in exact arithmetic (softmax is shift-invariant)


def observable_class(label, prog):
    """"rng" | "noise" (key biases: bounded absolutely) | "before" (values before the first update: judged against float64) |
    "after" (parameters, buffers and everything computed from updated parameters: judged against the float32 CPU run)"""
    if label == "rng_state":
        return "rng"
    if label.endswith(NOISE):
        return "noise"
    if prog["optimizer"] == "none":
        return "after" if "/buffer/" in label else "before"
    return "before" if label.startswith("s0/") and "/param/" not in label and "/buffer/" not in label else "after"


def judge(ref64, cpu32, got, prog):
    """the three runs of one program.  Raises AssertionError naming the seed, the label, the distances and the program;
    returns {"status": "ok" | "filtered", "worst": {class: (distance of got, distance of cpu32)}}.
      rng     the three stream states are equal
      noise   key-bias gradients below 1e-6 in float32 and 1e-12 in float64; their parameters within 1e-6 of the float32 CPU run
      -       a program whose float32 CPU run is not within HALF of compare()'s tolerances of the float64 run says nothing about
              another backend (float32 and float64 took different pool maxima or relu sides, or rounding alone comes near the
              tolerance): "filtered"
      before  within 1e-5 (relative Frobenius) of the float64 run, or no further from it than twice the float32 CPU run
      after   compare()'s tolerances against the float32 CPU run"""
    what = "seed %d" % prog["seed"]
    tail = "\nprogram: %r" % (prog,)
    names = [l for l, _ in ref64]
    assert names == [l for l, _ in cpu32] == [l for l, _ in got], "%s: the runs looked at different things:\n%s\n%s\n%s%s" % (
        what, names, [l for l, _ in cpu32], [l for l, _ in got], tail)
    kinds = [observable_class(l, prog) for l in names]
    rows = list(zip(names, kinds, (a for _, a in ref64), (a for _, a in cpu32), (a for _, a in got)))
    for label, kind, r, c, g in rows:
        assert r.shape == c.shape == g.shape, "%s %s: shapes %s / %s / %s%s" % (what, label, r.shape, c.shape, g.shape, tail)
        if kind == "rng":
            assert tuple(r) == tuple(c) == tuple(g), "%s: random-stream states float64 %s, cpu32 %s, got %s%s" % (what, r, c, g, tail)
    pick = lambda run, kept: [(l, a) for (l, a), k in zip(run, kinds) if k in kept]      # noqa: E731
    try:
        compare(pick(ref64, ("before", "after")), pick(cpu32, ("before", "after")), rtol=1e-4, atol=1e-5)
    except AssertionError:
        return {"status": "filtered", "worst": {}}
    worst = {}
    for label, kind, r, c, g in rows:
        if kind == "rng":
            continue
        e_got, e_cpu, apart = rel_frobenius(g, r), rel_frobenius(c, r), float(np.abs(g - c).max()) if g.size else 0.0
        where = "%s %s: got %.3g and cpu32 %.3g from the float64 run (relative Frobenius), got - cpu32 max %.3g" % (what, label, e_got, e_cpu, apart)
        if kind == "noise":
            if "/grad/" in label:
                assert np.abs(g).max() < 1e-6 and np.abs(c).max() < 1e-6 and np.abs(r).max() < 1e-12, \
                    "%s: max |.| got %.3g, cpu32 %.3g, float64 %.3g%s" % (where, np.abs(g).max(), np.abs(c).max(), np.abs(r).max(), tail)
            else:
                assert apart < 1e-6, where + tail
            continue
        try:
            if kind == "before":
                assert_as_close_to_float64_as_the_cpu_backend({label: g}, {label: c}, {label: r}, what=what)
            else:
                compare([(label, c)], [(label, g)], what=what)
        except AssertionError as e:
            raise AssertionError("%s\n%s%s" % (e, where, tail)) from None
        group = kind + ("/param" if "/param/" in label else "/buffer" if "/buffer/" in label else "/grad" if "/grad/" in label else "/value")
        merge_worst(worst, {group: (e_got, e_cpu)})
    return {"status": "ok", "worst": worst}


def merge_worst(total, worst):
    for group, (e_got, e_cpu) in worst.items():
        have = total.get(group, (0.0, 0.0))
        total[group] = (max(have[0], e_got), max(have[1], e_cpu))
    return total
