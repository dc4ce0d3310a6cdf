"""lg_attention_decode_gqa_f32 / _rows_f32 (csrc/decode_gqa.hip): one new token against a cache whose K/V heads are shared by
R = heads / kv_heads query heads each; `decode_attention(kv_heads=, split=True)`, `self_attention_decode(kv_heads=)` and the greedy
`generate` of an examples/bert.py model with num_key_value_heads.  The reference is a plain numpy float64 softmax over keys 0 .. t
with the K/V heads indexed by h // R; the bound is test_hip_decode_split.py's 1e-5 (relative Frobenius)."""
import math
import numpy as np
import pytest
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from lightgrad_amd import CpuTensor
from common import rel_frobenius, float64_tape
from test_hip_attention_dispatch import recorder  # noqa: F401  (fixture)
from test_hip_decode import bits
import decode_cases as dc

pytestmark = pytest.mark.gpu

CAPACITY = 768                                   # three slices of 256 keys
GROUPS = [(2, 1), (4, 2), (8, 1), (4, 4)]
T_VALUES = (0, 255, 256, 511, 600)               # alone in a slice, a slice's last row, the next one's first, two- and three-slice merges


def tensor(hip, a):
    return hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)


def operands(b, capacity, heads, kv_heads, d, seed=7):
    rng = np.random.RandomState(seed)
    k, v = (rng.uniform(-1.5, 1.5, (b, capacity, kv_heads * d)).astype(np.float32) for _ in range(2))
    q = rng.uniform(-1.5, 1.5, (b, 1, heads * d)).astype(np.float32)
    kn, vn = (rng.uniform(-1.5, 1.5, (b, 1, kv_heads * d)).astype(np.float32) for _ in range(2))
    return k, v, q, kn, vn


def repeat_heads(a, kv_heads, R):
    """(b, n, kv_heads * d) -> (b, n, kv_heads * R * d): head h of the result is K/V head h // R"""
    b, n, w = a.shape
    return np.repeat(a.reshape(b, n, kv_heads, w // kv_heads), R, axis=2).reshape(b, n, R * w)


def reference64(q, k, v, kn, vn, t, heads, kv_heads, mask=None):
    """(context (b, 1, heads * d), lse (b, heads)) over keys 0 .. t in float64"""
    R, b = heads // kv_heads, q.shape[0]
    k, v = (repeat_heads(np.concatenate([c[:, :t], new], axis=1).astype(np.float64), kv_heads, R) for c, new in ((k, kn), (v, vn)))
    d = q.shape[-1] // heads
    s = np.einsum("bhd,bjhd->bhj", q.astype(np.float64).reshape(b, heads, d), k.reshape(b, t + 1, heads, d)) / math.sqrt(d)
    if mask is not None:
        s = s + ((1.0 - np.broadcast_to(mask, (b, mask.shape[1]))[:, :t + 1].astype(np.float64)) * -10000.0)[:, None, :]
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    return np.einsum("bhj,bjhd->bhd", e / e.sum(-1, keepdims=True), v.reshape(b, t + 1, heads, d)).reshape(b, 1, heads * d), np.log(e.sum(-1)) + m[..., 0]


def decode(hip, q, kn, vn, k, v, t, heads, kv_heads, mask=None):
    """one launch on fresh device copies; t: an int or a position per row.  (the result with its .attention_lse, the two caches)"""
    d = q.shape[-1] // heads
    tk, tv, tq = tensor(hip, k), tensor(hip, v), tensor(hip, q)
    assert tq.decode_attention_supported(heads, k.shape[1], split=True, kv_heads=kv_heads)
    out = tq.decode_attention(tensor(hip, kn), tensor(hip, vn), tk, tv, tensor(hip, np.atleast_1d(np.asarray(t, np.int32))), heads=heads,
                              scale=math.sqrt(d) ** -1, mask=None if mask is None else tensor(hip, mask), split=True, lse=True, kv_heads=kv_heads)
    assert out.shape == q.shape and out.attention_lse.shape == (q.shape[0], heads)
    return out, tk, tv


def check(hip, d, heads, kv_heads, t, capacity=CAPACITY, b=2, mask=None):
    k, v, q, kn, vn = operands(b, capacity, heads, kv_heads, d)
    out, tk, tv = decode(hip, q, kn, vn, k, v, t, heads, kv_heads, mask)
    want, want_lse = reference64(q, k, v, kn, vn, t, heads, kv_heads, mask)
    what = "d %d, %d heads over %d, cap %d, t %d" % (d, heads, kv_heads, capacity, t)
    for name, got, ref in (("context", out.numpy(), want), ("lse", out.attention_lse.numpy(), want_lse)):
        err = rel_frobenius(got, ref)
        print("%s %s: %.3e" % (what, name, err))
        assert np.isfinite(got).all() and err <= 1e-5, (what, name, err)
    for before, after, new in ((k, tk.numpy(), kn), (v, tv.numpy(), vn)):         # row t is the new row, every other row keeps its bytes
        np.testing.assert_array_equal(bits(after[:, t:t + 1]), bits(new), err_msg=what)
        np.testing.assert_array_equal(bits(np.delete(after, t, axis=1)), bits(np.delete(before, t, axis=1)), err_msg=what)


@pytest.mark.parametrize("heads,kv_heads", GROUPS, ids=["%dover%d" % g for g in GROUPS])
@pytest.mark.parametrize("d", [32, 64])
def test_values_against_float64(hip, d, heads, kv_heads):
    for t in T_VALUES:
        check(hip, d, heads, kv_heads, t)


@pytest.mark.parametrize("heads,kv_heads", GROUPS, ids=["%dover%d" % g for g in GROUPS])
@pytest.mark.parametrize("d", [32, 64])
def test_the_bits_of_the_split_launch_on_repeated_heads(hip, d, heads, kv_heads):
    R = heads // kv_heads
    for t in T_VALUES:
        k, v, q, kn, vn = operands(2, CAPACITY, heads, kv_heads, d)
        out, _, _ = decode(hip, q, kn, vn, k, v, t, heads, kv_heads)
        wide = [tensor(hip, repeat_heads(a, kv_heads, R)) for a in (kn, vn, k, v)]
        split = tensor(hip, q).decode_attention(*wide, tensor(hip, np.array([t], np.int32)), heads=heads, scale=math.sqrt(d) ** -1, split=True, lse=True)
        np.testing.assert_array_equal(bits(out.numpy()), bits(split.numpy()), err_msg="t %d" % t)
        np.testing.assert_array_equal(bits(out.attention_lse.numpy()), bits(split.attention_lse.numpy()), err_msg="t %d" % t)


def test_a_position_per_row(hip):
    """rows 0 and 1 are their one-word launches bit for bit; row 2, at `capacity`, writes nothing and raises at the next synchronisation"""
    heads, kv_heads, d, pos = 4, 2, 32, (5, 300, CAPACITY)
    k, v, q, kn, vn = operands(3, CAPACITY, heads, kv_heads, d, seed=11)
    out, tk, tv = decode(hip, q, kn, vn, k, v, pos, heads, kv_heads)
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    for r in (0, 1):
        one, ok, ov = decode(hip, q[r:r + 1], kn[r:r + 1], vn[r:r + 1], k[r:r + 1], v[r:r + 1], pos[r], heads, kv_heads)
        for got, want in ((out.numpy(), one.numpy()), (out.attention_lse.numpy(), one.attention_lse.numpy()), (tk.numpy(), ok.numpy()), (tv.numpy(), ov.numpy())):
            np.testing.assert_array_equal(bits(got[r:r + 1]), bits(want))
    np.testing.assert_array_equal(bits(tk.numpy()[2]), bits(k[2]))
    np.testing.assert_array_equal(bits(tv.numpy()[2]), bits(v[2]))


@pytest.mark.parametrize("rows", [2, 1], ids=["mask-per-row", "one-mask-row"])
def test_a_fully_masked_slice_next_to_a_visible_one(hip, rows):
    mask = np.ones((rows, CAPACITY), np.float32)
    mask[:, :256] = 0                            # all of slice 0: w_s = +0 in the merge
    check(hip, 64, 4, 2, 300, mask=mask)


def test_the_widest_merge(hip):
    check(hip, 64, 8, 1, 16383, capacity=16384, b=1)


def test_self_attention_decode_is_decode_attention_on_the_projected_rows(hip, recorder):  # noqa: F811
    heads, kv_heads, d, hidden, b, t = 4, 2, 32, 64, 2, 300
    rng = np.random.RandomState(5)
    k, v, _, _, _ = operands(b, CAPACITY, heads, kv_heads, d)
    x = tensor(hip, rng.uniform(-1, 1, (b, 1, hidden)).astype(np.float32))
    ws = [tensor(hip, rng.uniform(-0.3, 0.3, (n * d, hidden)).astype(np.float32)) for n in (heads, kv_heads, kv_heads)]
    bs = [tensor(hip, rng.uniform(-0.3, 0.3, (n * d,)).astype(np.float32)) for n in (heads, kv_heads, kv_heads)]
    params = [p for pair in zip(ws, bs) for p in pair]
    q, kn, vn = ((x @ w.transpose(1, 0) + c).numpy() for w, c in zip(ws, bs))
    want, wk, wv = decode(hip, q, kn, vn, k, v, t, heads, kv_heads)
    pos, options = tensor(hip, np.array([t], np.int32)), dict(heads=heads, scale=math.sqrt(d) ** -1, split=True, lse=True, kv_heads=kv_heads)
    assert x.self_attention_decode_supported(ws[0], heads, CAPACITY, split=True, kv_heads=kv_heads)
    packed = hip.pack_qkv(*params)
    tk, tv = tensor(hip, k), tensor(hip, v)
    del recorder.calls[:]
    got = x.self_attention_decode(*params, tk, tv, pos, packed=packed, **options)
    assert recorder.calls == ["lg_attention_decode_gqa_f32"]
    graph = HipGraph()
    with graph.capture():
        captured = x.self_attention_decode(*params, tk, tv, pos, packed=packed, **options)
    assert graph.kernel_count() == 2                          # the product on the packed weights and the attention launch
    graph.replay()
    np.testing.assert_array_equal(bits(captured.numpy()), bits(got.numpy()))
    graph.destroy()
    unpacked = x.self_attention_decode(*params, tensor(hip, k), tensor(hip, v), pos, **options)
    np.testing.assert_array_equal(bits(got.numpy()), bits(unpacked.numpy()))
    for a, ref in ((got.numpy(), want.numpy()), (got.attention_lse.numpy(), want.attention_lse.numpy()), (tk.numpy()[:, t], wk.numpy()[:, t]),
                   (tv.numpy()[:, t], wv.numpy()[:, t])):
        assert rel_frobenius(a, ref) <= 1e-5
    with pytest.raises(AssertionError, match="self_attention_decode: kv_heads = 2 below heads = 4 .* needs split=True"):
        x.self_attention_decode(*params, tk, tv, pos, heads=heads, kv_heads=kv_heads)
    with pytest.raises(AssertionError, match="decode_attention: probs=True with split=True"):
        tensor(hip, q).decode_attention(tensor(hip, kn), tensor(hip, vn), tk, tv, pos, heads=heads, kv_heads=kv_heads, split=True, probs=True)


CFG = dict(dc.bert.TINY, num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=320, causal=True, attention_probs=False)
SEED, PROMPT, NEW = 3, 300, 8


def greedy_rows(T, params, ids, dtype=np.float32):
    """(tokens (2, NEW), the logits each was the argmax of) of greedy decoding through an nn.KVCache on tensor class T"""
    model = dc.bert.BertForMaskedLM(**CFG)
    model.load_parameters({n: a.astype(dtype) for n, a in params.items()})
    model = model.eval() if T is CpuTensor else model.eval().map_parameters(lambda p: T.from_numpy(p.numpy()))
    cache = dc.nn.KVCache(CFG["num_hidden_layers"], ids.shape[0], PROMPT + NEW, model.bert.encoder.layer[0].attention.self.kv_width,
                          like=model.cls.predictions.bias)
    rows, tokens = [], []
    logits = model(T.from_numpy(ids, requires_grad=False), cache=cache).numpy()[:, -1]
    for _ in range(NEW):
        rows.append(logits.copy())
        tokens.append(logits.argmax(-1).astype(np.int32))
        logits = model(T.from_numpy(tokens[-1][:, None], requires_grad=False), cache=cache).numpy()[:, 0]
        cache.advance()
    return np.stack(tokens, 1), np.stack(rows, 1)


def test_the_model_generates_the_cpu_runs_ids(hip, recorder):  # noqa: F811
    """seed 3, chosen on the CPU among 1 .. 5 (the only one whose tokens change along the run): the smallest top-2 margin of any
    float64 step is 1.8e-3 logits, 1.4e4 times the float32 CPU run's largest deviation from float64, 1.2e-7 (asserted below at
    decode_cases' factor of 100) - no step is a near-tie"""
    np.random.seed(SEED)
    params = {n: p.numpy().astype(np.float32) * (dc.GAIN if p.numpy().ndim == 2 else 1.0) for n, p in dc.bert.BertForMaskedLM(**CFG).named_parameters()}
    ids = np.random.randint(0, CFG["vocab_size"], (2, PROMPT)).astype(np.int32)
    with float64_tape():
        tokens64, logits64 = greedy_rows(CpuTensor, params, ids, np.float64)
    tokens32, logits32 = greedy_rows(CpuTensor, params, ids)
    top = np.sort(logits64, axis=-1)
    margin, deviation = float((top[..., -1] - top[..., -2]).min()), float(np.abs(logits32 - logits64).max())
    print("top-2 margin %.3g, float32 deviation %.3g" % (margin, deviation))
    assert margin >= 100 * deviation and (tokens32 == tokens64).all()
    model = dc.bert.BertForMaskedLM(**CFG)
    model.load_parameters(params)
    model.eval().map_parameters(lambda p: hip.from_numpy(p.numpy()))
    del recorder.calls[:]
    out = dc.bert.generate(model, tensor(hip, ids), NEW).numpy()
    np.testing.assert_array_equal(out[:, PROMPT:], tokens32)
    assert recorder.calls.count("lg_attention_decode_gqa_f32") == (NEW - 1) * CFG["num_hidden_layers"]
    assert not any("decode_split" in c for c in recorder.calls)
