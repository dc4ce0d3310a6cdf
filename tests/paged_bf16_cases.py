"""What test_paged_bf16_cpu.py and test_hip_paged_bf16.py share: the hand-written words of the bfloat16 rounding, the model of
decode_cases with r(.) behind every key and value projection (r = `bf16_round_array`) - a full forward of it attends to every key
and value as r of what the projection produced, which is what a bfloat16 cache promises -, the greedy continuation of every
prefixed prompt of paged_cases ALONE by a float64 full recompute per token with that model (computed once per process and never
changed afterwards), and the runs through `serve` over an nn.PagedKVCache(kv_dtype="bf16") on any tensor class."""
import functools
import numpy as np
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.cpu.ops import bf16_round_array
import decode_cases as dc
import serve_cases as sc
import paged_cases as pg

bert, CFG = dc.bert, dc.CFG

# (float32 word, the int16 word of a bfloat16 cache), written out by hand: nearest, ties to even in both directions, +-0, +-Inf,
# the largest finite float32 -> Inf, a carry out of the significand, NaNs (one with its payload in the low 16 bits only)
SPECIAL_WORDS = (
    (0x3F800000, 0x3F80),       # 1.0
    (0x3F808000, 0x3F80),       # a tie, the kept half even: down
    (0x3F818000, 0x3F82),       # a tie, the kept half odd: up
    (0x3F808001, 0x3F81),       # just above a tie: up
    (0x3F817FFF, 0x3F81),       # just below a tie: down
    (0xBF808000, 0xBF80),       # the same ties with the sign set
    (0xBF818000, 0xBF82),
    (0x3FFF8000, 0x4000),       # a tie that carries into the exponent: 2.0
    (0x00000000, 0x0000),       # +0
    (0x80000000, 0x8000),       # -0
    (0x7F800000, 0x7F80),       # +Inf
    (0xFF800000, 0xFF80),       # -Inf
    (0x7F7FFFFF, 0x7F80),       # the largest finite float32 -> +Inf
    (0xFF7FFFFF, 0xFF80),       # ... -> -Inf
    (0x7F7F7FFF, 0x7F7F),       # the largest bfloat16 and a bit less than half a step: stays finite
    (0x7FC00000, 0x7FC0),       # the quiet NaN
    (0x7F800001, 0x7FC0),       # a NaN whose payload lies in the low 16 bits only: still a NaN
    (0xFF80FFFF, 0xFFC0),
    (0x42F6E979, 0x42F7),       # 123.456
    (0x3DCCCCCD, 0x3DCD),       # 0.1
)


def special_values():
    """(float32 values, the int16 words a bfloat16 cache holds for them), 20 of each"""
    words = np.array([w for w, _ in SPECIAL_WORDS], np.uint32)
    return words.view(np.float32), np.array([b for _, b in SPECIAL_WORDS], np.uint16).view(np.int16)


class RoundedProjection(nn.Module):
    """a key or value projection followed by r: outside the tape, in the projection's own dtype (float64 rounds through float32)"""
    def __init__(self, inner):
        nn.Module.__init__(self)
        self.inner = inner

    def forward(self, x):
        y = self.inner(x)
        return type(y).from_numpy(bf16_round_array(y.numpy()), requires_grad=False)


def rounded_model(dtype):
    """decode_cases' CpuTensor model (serve_cases' seed) with every key and value rounded to bfloat16 where it is produced"""
    model = dc.make_model(CpuTensor, dtype, sc.SEED)
    for layer in model.bert.encoder.layer:
        attention = layer.attention.self
        attention.key, attention.value = RoundedProjection(attention.key), RoundedProjection(attention.value)
    return model


@functools.lru_cache(maxsize=None)
def rounded_reference(prefixed=True, new=sc.BUDGET):
    """paged_cases.prefixed_reference with K and V rounded through r: greedy decoding of each (prefixed) prompt ALONE by a full
    float64 recompute per token; the margin is that of the float64 rounded model, the deviation that of the float32 rounded one"""
    model64, model32 = rounded_model(np.float64), rounded_model(np.float32)
    tokens, margin, deviation = [], np.inf, 0.0
    for prompt in (pg.prefixed_prompts() if prefixed else sc.prompts()):
        seq = prompt[None, :].copy()
        for _ in range(new):
            l64, l32 = dc.full_logits(model64, seq)[:, -1], dc.full_logits(model32, seq)[:, -1]
            assert l64.dtype == np.float64 and l32.dtype == np.float32
            top = np.sort(l64, axis=-1)
            margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
            deviation = max(deviation, float(np.abs(l32.astype(np.float64) - l64).max()))
            seq = np.concatenate([seq, l64.argmax(-1).astype(np.int32)[:, None]], axis=1)
        tokens.append(seq[0, len(prompt):])
    return tokens, margin, deviation


def assert_rounded_margins_rule_out_ties(prefixed=True):
    """from the references alone: the top-2 margin of the float64 rounded reference >= 20 x the largest logit deviation of the
    float32 rounded model from it.  20 and not decode_cases' 100: a last-bit difference in a projection can flip a bfloat16
    rounding, so the float32 model deviates by more than its own arithmetic"""
    tokens, margin, deviation = rounded_reference(prefixed)
    print("%s prompts, K and V rounded to bfloat16: top-2 margin %.3g, float32 deviation %.3g, ratio %.0f" % (
        "prefixed" if prefixed else "plain", margin, deviation, margin / deviation))
    assert margin >= 20 * deviation, "top-2 margin %.3g below 20 x the float32 deviation %.3g of the rounded model - pick another seed" % (margin, deviation)
    return tokens


def run_serve(T, slots, chunk, num_blocks, model=None, budgets=sc.BUDGET, eos=sc.EOS, rows=None, **options):
    """paged_cases.run_serve over an nn.PagedKVCache(kv_dtype="bf16"): (out, out_len, stats, cache)"""
    model = dc.make_model(T, seed=sc.SEED) if model is None else model
    cache = nn.PagedKVCache(CFG["num_hidden_layers"], slots, num_blocks, pg.BLOCK, CFG["hidden_size"], pg.MAX_BLOCKS, like=model.cls.predictions.bias,
                            kv_dtype="bf16")
    assert cache.kv_dtype == "bf16" and all(np.dtype(t.dtype) == np.int16 and isinstance(t, T) for t in cache.k + cache.v)
    (out, out_len), stats = bert.serve(model, pg.prefixed_prompts() if rows is None else rows, budgets, slots=slots, chunk=chunk, eos_token_id=eos,
                                       pad_token_id=sc.PAD, cache=cache, **options)
    assert out.dtype == np.int32 and out_len.dtype == np.int32 and isinstance(out, T) and isinstance(out_len, T)
    assert stats["num_blocks"] == num_blocks and stats["block_size"] == pg.BLOCK and stats["kv_dtype"] == "bf16"
    assert stats["pool_bytes"] == cache.pool_bytes() == 2 * CFG["num_hidden_layers"] * num_blocks * pg.BLOCK * CFG["hidden_size"] * 2
    return out.numpy().copy(), out_len.numpy().copy(), stats, cache


def widened(pool):
    """the float32 values a tensor of bfloat16 words stands for"""
    return light.bf16_widen(pool.numpy())
