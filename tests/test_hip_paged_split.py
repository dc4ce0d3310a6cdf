"""lg_attention_extend_paged_split_f32 / _bf16_f32 (csrc/paged_split.hip): the split-key extend launch with the caches reached
through a block table of up to 16384 positions; `extend_attention(count=, block_table=, block_size=, split=True)`,
lg_serve_commit_paged_wide_i32 and the paged `serve` of examples/bert.py beyond 512 positions.

"Bit for bit": context, log-sum-exp and the new pool rows equal those of `extend_attention(count=, split=True)` on a contiguous
cache that holds the same rows; every other pool word - NaN wherever no element has a row - keeps its bits.  Against float64 the
bound is the 1e-5 relative Frobenius contract of test_hip_extend_split.py."""
import math
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd.autograd.cpu.ops import bf16_round_array
from lightgrad_amd.autograd.hip import HipDevice
from lightgrad_amd.autograd.hip import lib as hiplib
from common import rel_frobenius
from test_hip_serve import recorder  # noqa: F401  (fixture)
from test_hip_decode_split import long_model, tensor, bits
from test_hip_extend import operands
from test_hip_extend_split import reference64, poisoned, hole_mask, slice_length, extend, SHAPES, SENTINEL
from test_hip_paged import tables_of, pools_expected
import decode_cases as dc

pytestmark = pytest.mark.gpu

LG_EINVAL, HEADS = -1, 2


def paged_case(capacity, slots, m, B, d, heads=HEADS, seed=5):
    """the contiguous operands (NaN in every cache row at or beyond an element's position) and the same rows in pools through
    shuffled tables, NaN in every other pool row - the blocks no table names included.  slots: (t, count) per element"""
    C = -(-capacity // B) * B
    pos, count = np.array([t for t, _ in slots], np.int32), np.array([n for _, n in slots], np.int32)
    k, v, q, kn, vn = poisoned(operands(len(slots), C, m, heads, d, seed=seed), pos)
    table, num_blocks = tables_of(slots, B, C // B, seed)
    kp, vp = (np.full((num_blocks, B, heads * d), np.nan, np.float32) for _ in range(2))
    for s, (t, _) in enumerate(slots):
        for j in range(t):
            kp[table[s, j // B], j % B], vp[table[s, j // B], j % B] = k[s, j], v[s, j]
    return dict(k=k, v=v, q=q, kn=kn, vn=vn, kp=kp, vp=vp, pos=pos, count=count, table=table, slots=slots, m=m, B=B, C=C, heads=heads)


def run_paged(hip, case, mask=None, kv_dtype=None):
    """one paged split launch on fresh device copies: (context, lse, k pool after, v pool after) as numpy"""
    tk, tv, tq = tensor(hip, case["kp"]), tensor(hip, case["vp"]), tensor(hip, case["q"])
    extra = {} if kv_dtype is None else {"kv_dtype": kv_dtype}
    assert tq.extend_attention_supported(case["heads"], case["C"], split=True, block_size=case["B"])
    with light.no_grad():
        out = tq.extend_attention(tensor(hip, case["kn"]), tensor(hip, case["vn"]), tk, tv, tensor(hip, case["pos"]), heads=case["heads"],
                                  scale=math.sqrt(case["q"].shape[2] // case["heads"]) ** -1, mask=None if mask is None else tensor(hip, mask),
                                  count=tensor(hip, case["count"]), block_table=tensor(hip, case["table"]), block_size=case["B"], split=True, lse=True, **extra)
    assert not hasattr(out, "attention_probs")
    return out.numpy(), out.attention_lse.numpy(), tk.numpy(), tv.numpy()


def check_float64(got, case, mask, what):
    for r, (t, n) in enumerate(case["slots"]):
        if n:
            want, want_lse = reference64(case["q"][r, :n], case["kn"][r, :n], case["vn"][r, :n], case["k"][r], case["v"][r], t, case["heads"],
                                         None if mask is None else mask[r])
            errors = rel_frobenius(got[0][r, :n], want), rel_frobenius(got[1][r, :, :n], want_lse)
            print("%s element %d t %d n %d: context %.3e, lse %.3e" % (what, r, t, n, *errors))
            assert np.isfinite(got[0][r]).all() and np.isfinite(got[1][r]).all() and max(errors) <= 1e-5, (what, r, errors)


def slots_of(case_index):
    """(capacity, slots, m) of SHAPES[case_index]: counts m, 1 and 0 - the full element, one row at the end of the cache, an idle one"""
    capacity, t, m = SHAPES[case_index](slice_length())
    return capacity, ((t, m), (capacity - 1, 1), (t // 2, 0)), m


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("B", [4, 16, 128])
@pytest.mark.parametrize("shape", range(4))
def test_bit_for_bit_the_contiguous_launch_and_within_the_contract_of_float64(hip, recorder, shape, B, d):  # noqa: F811
    capacity, slots, m = slots_of(shape)
    case = paged_case(capacity, slots, m, B, d, seed=5 + shape)
    for mask in (None, hole_mask(len(slots), case["C"])):
        what = "shape %d B %d d %d %s" % (shape, B, d, "nomask" if mask is None else "mask")
        want = extend(hip, tuple(case[n] for n in ("k", "v", "q", "kn", "vn")), case["pos"], HEADS, mask, count=case["count"])
        del recorder.calls[:]
        got = run_paged(hip, case, mask)
        assert recorder.attention() == ["lg_attention_extend_paged_split_f32"]
        np.testing.assert_array_equal(bits(got[0]), bits(want[0]), err_msg=what + ": context")
        np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg=what + ": lse")
        for pool, expected in zip(got[2:], pools_expected(case, want[2], want[3])):
            np.testing.assert_array_equal(bits(pool), bits(expected), err_msg=what + ": a pool (the new rows, every other word unchanged)")
        for r, (_, n) in enumerate(slots):
            assert (bits(got[0][r, n:]) == 0).all() and (bits(got[1][r, :, n:]) == 0).all(), what     # rows at or behind the count: +0.0
        check_float64(got, case, mask, what)
    HipDevice.synchronize()                                                   # no element raised the flag


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("shape", [1, 2])
def test_bf16_pools_equal_the_fp32_launch_on_the_rounded_operands(hip, recorder, shape, d):  # noqa: F811
    capacity, slots, m = slots_of(shape)
    case = paged_case(capacity, slots, m, 16, d, seed=11 + shape)
    ref = dict(case, kn=bf16_round_array(case["kn"]), vn=bf16_round_array(case["vn"]), kp=light.bf16_widen(light.bf16_bits(case["kp"])),
               vp=light.bf16_widen(light.bf16_bits(case["vp"])))
    mask = hole_mask(len(slots), case["C"])
    want = run_paged(hip, ref, mask)
    del recorder.calls[:]
    got = run_paged(hip, dict(case, kp=light.bf16_bits(case["kp"]), vp=light.bf16_bits(case["vp"])), mask, kv_dtype="bf16")
    assert recorder.attention() == ["lg_attention_extend_paged_split_bf16_f32"]
    np.testing.assert_array_equal(bits(got[0]), bits(want[0]))
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]))
    for pool, expected in zip(got[2:], want[2:]):                             # the whole int16 pools
        assert pool.dtype == np.int16
        np.testing.assert_array_equal(pool.view(np.uint16), light.bf16_bits(expected).view(np.uint16))


@pytest.mark.parametrize("B", [4, 128])
def test_the_largest_tables(hip, B):
    case = paged_case(16384, ((16384 - 128, 128),), 128, B, 64, heads=1, seed=3)
    assert case["table"].shape[1] == 16384 // B
    check_float64(run_paged(hip, case), case, None, "16384 positions in blocks of %d" % B)
    HipDevice.synchronize()


class Call(object):
    """elements `rows` of a case through the C ABI on sentinel outputs, every argument replaceable"""
    def __init__(self, hip, case, rows=slice(None), entry="lg_attention_extend_paged_split_f32"):
        self.lib, self.entry, self.case = hiplib.lib(), entry, case
        b, m, width = case["q"][rows].shape
        self.k, self.v = tensor(hip, case["kp"]), tensor(hip, case["vp"])
        self.q, self.kn, self.vn, self.pos, self.count, self.table = (tensor(hip, case[n][rows]) for n in ("q", "kn", "vn", "pos", "count", "table"))
        self.o, self.lse = tensor(hip, np.full((b, m, width), SENTINEL, np.float32)), tensor(hip, np.full((b, case["heads"], m), SENTINEL, np.float32))
        self.args = dict(q=self.q.ptr, ldq=width, sbq=m * width, k_new=self.kn.ptr, ldk=width, sbk=m * width, v_new=self.vn.ptr, ldv=width, sbv=m * width,
                         k_pool=self.k.ptr, v_pool=self.v.ptr, ldc=width, pos=self.pos.ptr, count=self.count.ptr, block_table=self.table.ptr, o=self.o.ptr,
                         ldo=width, sbo=m * width, lse=self.lse.ptr, batch=b, heads=case["heads"], m=m, max_blocks=case["C"] // case["B"],
                         num_blocks=case["kp"].shape[0], log2_block=case["B"].bit_length() - 1, D=width // case["heads"], scale=0.2, mask=None, sbm=0)

    def __call__(self, **override):
        return getattr(self.lib, self.entry)(*dict(self.args, **override).values())

    def results(self):
        return self.o.numpy(), self.lse.numpy(), self.k.numpy(), self.v.numpy()


def three_elements():
    L = slice_length()
    return paged_case(2 * L + 16, ((3, 2), (L + 5, 4), (2 * L, 2)), 4, 16, 32, seed=23)


@pytest.mark.parametrize("fault", ["word", "position"])
def test_a_bad_element_writes_nothing_the_others_are_computed_and_the_tickets_are_zero_again(hip, fault):
    """element 1 names no block for the first block of its SECOND slice (slice 0 of it sees only good words), or has t + n beyond
    the capacity: a bounds check, nothing here faults"""
    good = three_elements()
    bad = dict(good, table=good["table"].copy(), pos=good["pos"].copy())
    if fault == "word":
        bad["table"][1, slice_length() // 16] = good["kp"].shape[0]
    else:
        bad["pos"][1] = good["C"] - 3
    clean = Call(hip, good)
    assert clean() == 0
    HipDevice.synchronize()
    call = Call(hip, bad)
    assert call() == 0                                                        # the launch itself is fine: the kernel reads the words
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                                   # reported once
    o, lse, k, v = call.results()
    assert (o[1] == SENTINEL).all() and (lse[1] == SENTINEL).all()
    for r in (0, 2):                                                          # ... bit for bit what they are alone
        alone = Call(hip, good, rows=slice(r, r + 1))
        assert alone() == 0
        np.testing.assert_array_equal(bits(o[r]), bits(alone.o.numpy()[0]))
        np.testing.assert_array_equal(bits(lse[r]), bits(alone.lse.numpy()[0]))
    without = dict(good, slots=(good["slots"][0], (good["slots"][1][0], 0), good["slots"][2]))       # the pools: everything but element 1's rows
    after_k, after_v = good["k"].copy(), good["v"].copy()
    for s, (t, n) in enumerate(without["slots"]):
        after_k[s, t:t + n], after_v[s, t:t + n] = good["kn"][s, :n], good["vn"][s, :n]
    for pool, expected in zip((k, v), pools_expected(without, after_k, after_v)):
        np.testing.assert_array_equal(bits(pool), bits(expected))
    good_words = tensor(hip, good["table"]), tensor(hip, good["pos"])
    assert call(block_table=good_words[0].ptr, pos=good_words[1].ptr) == 0    # the same tensors: a ticket left non-zero would break this launch
    HipDevice.synchronize()
    for mine, theirs in zip(call.results(), clean.results()):
        np.testing.assert_array_equal(bits(mine), bits(theirs))


REFUSALS = [("positions16388", dict(log2_block=2, max_blocks=4097), b"unsupported"), ("m129", dict(m=129), b"unsupported"), ("D48", dict(D=48), b"unsupported"),
            ("pool-misaligned", dict(k_pool=4), b"16-byte aligned"), ("pool-in-k_new", dict(k_new="k_pool"), b"k_pool overlaps k_new"),
            ("table-in-pool", dict(block_table="v_pool"), b"v_pool overlaps block_table"), ("lse-in-o", dict(lse="o"), b"o overlaps lse")]


@pytest.mark.parametrize("name,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_refusals_launch_nothing(hip, name, change, message):
    call = Call(hip, three_elements())
    change = {key: call.args[value] if isinstance(value, str) else call.args[key] + value if key == "k_pool" else value for key, value in change.items()}
    assert call(**change) == LG_EINVAL, name
    error = call.lib.lg_last_error()
    assert b"lg_attention_extend_paged_split_f32:" in error and message in error, error
    HipDevice.synchronize()
    o, lse, k, v = call.results()
    assert (o == SENTINEL).all() and (lse == SENTINEL).all() and (bits(k) == bits(call.case["kp"])).all() and (bits(v) == bits(call.case["vp"])).all()


def test_the_predicate_the_keywords_and_the_wide_commit(hip):
    supported = hiplib.lib().lg_attention_extend_paged_split_supported
    assert supported(128, 4096, 2, 64) and supported(1, 128, 7, 32) and not supported(1, 4097, 2, 64) and not supported(129, 128, 7, 64)
    assert not supported(1, 8, 1, 64) and not supported(1, 8, 8, 64) and not supported(1, 8, 4, 48) and not supported(9, 2, 2, 64)
    case = three_elements()
    tk, tv, tq, tkn, tvn, tpos, tcount, ttable = (tensor(hip, case[n]) for n in ("kp", "vp", "q", "kn", "vn", "pos", "count", "table"))
    paged = dict(count=tcount, block_table=ttable, block_size=16, split=True)
    for keywords, message in ((dict(probs=True), "probs=True with split=True"), (dict(cu=tcount), "cu= with split=True"), (dict(m_max=2), "m_max= with split=True")):
        with pytest.raises(AssertionError, match="extend_attention: " + message):
            tq.extend_attention(tkn, tvn, tk, tv, tpos, heads=HEADS, **dict(paged, **keywords))
    with pytest.raises(AssertionError, match="block_table= with split=True takes an int32 HipTensor with block_size= and count="):
        tq.extend_attention(tkn, tvn, tk, tv, tpos, heads=HEADS, block_table=ttable, block_size=16, split=True)
    assert not tq.extend_attention_supported(HEADS, case["C"], block_size=16)                        # without split=: the 512-row launch


def test_the_model_serves_prompts_beyond_512_positions_from_a_pool(hip, recorder):  # noqa: F811
    L = slice_length()
    cfg = dict(dc.CFG, num_hidden_layers=1, max_position_embeddings=2 * L + 100, attention_probs=False, causal=True)
    np.random.seed(dc.SEED)
    params = {n: p.numpy().astype(np.float32) * (dc.GAIN if p.numpy().ndim == 2 else 1.0) for n, p in dc.bert.BertForMaskedLM(**cfg).named_parameters()}
    model = long_model(hip, cfg, params)
    rng = np.random.RandomState(7)
    prefix = rng.randint(0, cfg["vocab_size"], 40)
    prompts = [np.concatenate([prefix, rng.randint(0, cfg["vocab_size"], n)]) for n in (2 * L + 20, 9, 2 * L - 30, 70)]
    serve = lambda **kw: dc.bert.serve(model, prompts, 4, slots=2, chunk=32, **kw)[0][0].numpy()      # noqa: E731
    want = serve()                                                            # the contiguous nn.KVCache: lg_attention_extend_split_counts_f32
    for shared in (0, 40):
        del recorder.calls[:]
        np.testing.assert_array_equal(serve(num_blocks=80, block_size=16, shared_prefix=shared), want)
        assert set(recorder.attention()) == {"lg_attention_extend_paged_split_f32"}                  # the composite would launch none of it
        assert "lg_serve_commit_paged_wide_i32" in recorder.calls and "lg_serve_commit_paged_i32" not in recorder.calls
    with pytest.raises(AssertionError, match="chunk=129"):
        dc.bert.serve(model, prompts, 4, slots=2, chunk=129, num_blocks=80, block_size=16)
    assert nn.PagedKVCache(1, 1, 4, 128, 64, 5, like=model.cls.predictions.bias, split=True).capacity == 640
