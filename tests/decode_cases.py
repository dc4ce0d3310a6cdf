"""What test_decode_cpu.py and test_hip_decode.py share: a small causal model, its float64 yardsticks (computed once per process
and never changed afterwards) and the teacher-forced / greedy runs through an nn.KVCache on any tensor class."""
import functools
import importlib.util
import os
import numpy as np
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from conftest import ROOT
from common import float64_tape

spec = importlib.util.spec_from_file_location("bert_example_decode", os.path.join(ROOT, "examples", "bert.py"))
bert = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bert)

# d = 32 per head: a shape the HIP decode kernel takes, so the same model runs on both backends
CFG = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, vocab_size=101,
           max_position_embeddings=48, type_vocab_size=2, causal=True)
B, S0, NEW = 2, 5, 10
CAPACITY = 17                           # >= S0 + NEW, <= max_position_embeddings, no multiple of anything
GAIN = 16.0
SEED = 2                                # model and ids; chosen on the CPU so that no greedy step is a near-tie (greedy_reference)
PROMPT_MASK = np.array([[1, 1, 0, 1, 1], [1, 0, 1, 1, 0]], np.float32)          # padding_mask-style holes, key 0 visible


@functools.lru_cache(maxsize=None)
def parameters(seed=SEED):
    """{name: float32 array} of a freshly initialised model, and (B, S0 + NEW) int32 ids"""
    np.random.seed(seed)
    model = bert.BertForMaskedLM(**CFG)
    # xavier draws are so small that such a model hardly looks at its input; every matrix and table is scaled up until attention
    # and the tokens matter (sequences then decode differently), LayerNorm parameters and biases stay as drawn
    params = {n: p.numpy().astype(np.float32) * (GAIN if p.numpy().ndim == 2 else 1.0) for n, p in model.named_parameters()}
    ids = np.random.randint(0, CFG["vocab_size"], (B, S0 + NEW)).astype(np.int32)
    return params, ids


def make_model(T, dtype=np.float32, seed=SEED):
    """the model with the parameters of `parameters(seed)` in `dtype` on tensor class T, in eval mode"""
    params, _ = parameters(seed)

    def build():
        model = bert.BertForMaskedLM(**CFG)
        model.load_parameters({n: a.astype(dtype) for n, a in params.items()})
        return model.eval()
    if np.dtype(dtype) == np.float64:
        assert T is CpuTensor
        with float64_tape():
            return build()
    model = build()
    if T is not CpuTensor:
        model.map_parameters(lambda p: T.from_numpy(p.numpy()))
    return model


def full_logits(model, ids, mask=None):
    """logits (b, s, vocab) of the full causal forward of a CpuTensor model over `ids` (ndarray), in the model's own dtype"""
    dtype = model.cls.predictions.bias.dtype
    m = None if mask is None else CpuTensor.from_numpy(mask.astype(dtype), requires_grad=False)
    with light.no_grad():
        if dtype == np.float64:
            with float64_tape():
                return model(CpuTensor.from_numpy(ids, requires_grad=False), attention_mask=m).numpy().copy()
        return model(CpuTensor.from_numpy(ids, requires_grad=False), attention_mask=m).numpy().copy()


def prefix_mask(n):
    """the prompt's key-padding mask extended with ones to n >= S0 positions"""
    return np.concatenate([PROMPT_MASK, np.ones((B, n - S0), np.float32)], axis=1)


@functools.lru_cache(maxsize=None)
def teacher_reference(masked):
    """(ref64, cpu32): {"prefill": logits (B, S0, vocab) of the prompt, "step<i>": logits (B, 1, vocab) of position S0 + i} from
    full causal forwards over each prefix, in float64 and on the float32 CPU backend"""
    _, ids = parameters()
    out = []
    for dtype in (np.float64, np.float32):
        model = make_model(CpuTensor, dtype)
        rows = {"prefill": full_logits(model, ids[:, :S0], prefix_mask(S0) if masked else None)}
        for i in range(NEW):
            n = S0 + i + 1
            rows["step%d" % i] = full_logits(model, ids[:, :n], prefix_mask(n) if masked else None)[:, -1:]
        out.append(rows)
    return tuple(out)


def teacher_forced(T, masked, model=None, dtype=np.float32):
    """the same rows through an nn.KVCache on tensor class T: the prompt once, then the NEW given tokens one at a time"""
    _, ids = parameters()
    model = make_model(T, dtype) if model is None else model
    width = CFG["hidden_size"]
    cache = nn.KVCache(CFG["num_hidden_layers"], B, CAPACITY, width, like=model.cls.predictions.bias)
    tensor = lambda a: T.from_numpy(a, requires_grad=False)          # noqa: E731
    prompt_mask = tensor(PROMPT_MASK.astype(dtype)) if masked else None
    cache_mask = tensor(prefix_mask(CAPACITY).astype(dtype)) if masked else None
    rows = {"prefill": model(tensor(ids[:, :S0]), attention_mask=prompt_mask, cache=cache).numpy().copy()}
    assert cache.length == S0
    for i in range(NEW):
        logits = model(tensor(ids[:, S0 + i:S0 + i + 1]), attention_mask=cache_mask, cache=cache)
        cache.advance()
        assert tuple(logits.shape) == (B, 1, CFG["vocab_size"]) and logits.ctx is None          # outside the tape
        rows["step%d" % i] = logits.numpy().copy()
    assert cache.length == S0 + NEW and int(cache.pos.numpy()[0]) == S0 + NEW
    return rows


@functools.lru_cache(maxsize=None)
def greedy_reference(seed=SEED, new=NEW):
    """greedy decoding by a full float64 recompute per token: (tokens (B, new), the smallest top-2 logit margin of any step, the
    largest deviation of the float32 full forward's last-row logits from the float64 ones over the same prefixes)"""
    _, ids = parameters(seed)
    model64, model32 = make_model(CpuTensor, np.float64, seed), make_model(CpuTensor, np.float32, seed)
    seq, margin, deviation = ids[:, :S0].copy(), np.inf, 0.0
    for _ in range(new):
        l64, l32 = full_logits(model64, seq)[:, -1], full_logits(model32, seq)[:, -1]
        top = np.sort(l64, axis=-1)
        margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
        deviation = max(deviation, float(np.abs(l32.astype(np.float64) - l64).max()))
        seq = np.concatenate([seq, l64.argmax(-1).astype(np.int32)[:, None]], axis=1)
    return seq[:, S0:], margin, deviation


def assert_margins_rule_out_ties(seed=SEED, new=NEW):
    tokens, margin, deviation = greedy_reference(seed, new)
    assert margin >= 100 * deviation, "seed %d: top-2 margin %.3g below 100 x the float32 deviation %.3g - pick another seed" % (seed, margin, deviation)
    return tokens


def greedy(T, new=NEW, seed=SEED, model=None, **options):
    """tokens (B, new) of `generate` on tensor class T"""
    _, ids = parameters(seed)
    model = make_model(T, seed=seed) if model is None else model
    out = bert.generate(model, T.from_numpy(ids[:, :S0], requires_grad=False), new, **options)
    assert tuple(out.shape) == (B, S0 + new)
    out = out.numpy()
    np.testing.assert_array_equal(out[:, :S0], ids[:, :S0])
    return out[:, S0:]
