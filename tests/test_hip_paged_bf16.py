"""The bfloat16 key / value pools of the paged cache on the GPU: lg_attention_extend_paged_bf16_f32 (csrc/paged_bf16.hip: the paged
launch with 2 bytes a pool element, fp32 tiles and MFMAs kept) and what stands on it - `extend_attention(..., kv_dtype="bf16")`,
`self_attention_extend`, and `serve` over an nn.PagedKVCache(kv_dtype="bf16"), eager and captured.

With r = `bf16_round_array`, bits = `light.bf16_bits` and widen = `light.bf16_widen`, "bit for bit" means: the context and the
probabilities equal those of lg_attention_extend_paged_f32 on (q, r(k_new), r(v_new), widen(pools)), and the int16 pools after
the launch equal the pools before it with bits(k_new) / bits(v_new) in the rows of the new positions - every other word as it was.
Every pool row no slot owns holds the NaN word 0x7FC0 and every token row >= count holds NaN: the launch reaches nothing it should
not.  The numerics of the float32 paged entry are the ground of test_hip_paged.py."""
import math
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.cpu.ops import bf16_round_array
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from common import assert_as_close_to_float64_as_the_cpu_backend, float64_tape
from test_hip_attention_masked import padding_mask
from test_hip_serve import recorder                                       # noqa: F401 (a fixture)
import test_hip_extend as he
import test_hip_paged as th
import decode_cases as dc
import serve_cases as sc
import paged_cases as pg
import paged_bf16_cases as pb

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
HEADS = th.HEADS
ENTRY = "lg_attention_extend_paged_bf16_f32"
bits = he.bits


def words(a):
    return np.ascontiguousarray(a).view(np.uint16)


def bf16_case(B, max_blocks, d, seed=13):
    """test_hip_paged.paged_operands with the pools as bfloat16 words (`kp16`, `vp16`: 0x7FC0 in every row no slot owns) and, as
    `ref`, the operands the float32 paged entry takes for the same result: r(k_new), r(v_new), the widened pools"""
    case = th.paged_operands(B, max_blocks, d, seed)
    case["kp16"], case["vp16"] = light.bf16_bits(case["kp"]), light.bf16_bits(case["vp"])
    owned = ~np.isnan(case["kp"])
    assert (words(case["kp16"])[~owned] == 0x7FC0).all() and (words(case["vp16"])[~owned] == 0x7FC0).all()
    case["ref"] = dict(case, kn=bf16_round_array(case["kn"]), vn=bf16_round_array(case["vn"]), kp=light.bf16_widen(case["kp16"]),
                       vp=light.bf16_widen(case["vp16"]))
    return case


def run16(hip, case, mask, rows=None, pools=None):
    """one launch of `extend_attention(count=, block_table=, kv_dtype="bf16")` on fresh device copies, of the slots `rows` (default:
    all): (context, probs, k pool after, v pool after) as numpy, the pools int16"""
    rows = slice(None) if rows is None else rows
    tensor = lambda a: hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)      # noqa: E731
    tq, tkn, tvn, tpos, tcount = (tensor(case[name][rows]) for name in ("q", "kn", "vn", "pos", "count"))
    tm = None if mask is None else tensor(mask[rows])
    d = case["q"].shape[-1] // HEADS
    tk, tv = (tensor(case["kp16"]), tensor(case["vp16"])) if pools is None else pools
    with light.no_grad():
        out = tq.extend_attention(tkn, tvn, tk, tv, tpos, heads=HEADS, scale=math.sqrt(d) ** -1, mask=tm, probs=True, count=tcount,
                                  block_table=tensor(case["table"][rows]), block_size=case["B"], kv_dtype="bf16")
    got = out.numpy(), out.attention_probs.numpy(), tk.numpy(), tv.numpy()
    assert got[2].dtype == np.int16 and got[3].dtype == np.int16
    return got


def pools16_expected(case):
    """the int16 pools after the launch: what they held, with bits(.) of rows 0 .. count - 1 of every slot's new tokens where its table says"""
    kp, vp, B = case["kp16"].copy(), case["vp16"].copy(), case["B"]
    for s, (t, n) in enumerate(case["slots"]):
        for i in range(n):
            at = (case["table"][s, (t + i) // B], (t + i) % B)
            kp[at], vp[at] = light.bf16_bits(case["kn"][s, i]), light.bf16_bits(case["vn"][s, i])
    return kp, vp


# ---- 1. the launch, bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("geometry", th.GEOMETRIES, ids=["B%dx%d" % g for g in th.GEOMETRIES])
def test_bf16_slots_equal_the_float_entry_on_rounded_rows_and_widened_pools(hip, recorder, geometry, d):
    case = bf16_case(*geometry, d)
    kp, vp = pools16_expected(case)
    for masked in (False, True):
        mask = padding_mask(len(case["pos"]), case["C"]) if masked else None
        want = th.run(hip, case["ref"], mask, paged=True)
        del recorder.calls[:]
        got = run16(hip, case, mask)
        assert recorder.attention() == [ENTRY]
        what = "B %d x %d D %d %s" % (geometry + (d, "mask" if masked else "nomask"))
        np.testing.assert_array_equal(bits(got[0]), bits(want[0]), err_msg=what + ": context")
        np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg=what + ": probs")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), what
        np.testing.assert_array_equal(words(got[2]), words(kp), err_msg=what + ": k pool (the new rows' words, and every other word untouched)")
        np.testing.assert_array_equal(words(got[3]), words(vp), err_msg=what + ": v pool")
        # ... which is what the float entry left in its pools, word for word
        np.testing.assert_array_equal(bits(light.bf16_widen(got[2])), bits(want[2]), err_msg=what + ": the widened k pool")
        np.testing.assert_array_equal(bits(light.bf16_widen(got[3])), bits(want[3]), err_msg=what + ": the widened v pool")
        for s, (t, n) in enumerate(case["slots"]):
            assert (bits(got[0][s, n:]) == 0).all() and (bits(got[1][s, :, n:]) == 0).all(), (what, s)
    HipDevice.synchronize()                                               # no slot raised the flag


# ---- 2. the store's rounding ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [32, 64])
def test_the_row_store_rounds_as_the_definition_on_the_special_values(hip, d):
    values, want = pb.special_values()
    B, width, m = 16, HEADS * d, 5
    tile = lambda a, shift: np.roll(np.tile(a, m * width // len(a) + 1), shift)[:m * width].reshape(1, m, width)       # noqa: E731
    kn, vn = tile(values, 0), tile(values, 7)
    case = dict(q=np.ones((1, m, width), np.float32), kn=kn, vn=vn, pos=np.array([B - 2], np.int32), count=np.array([m], np.int32),
                table=np.array([[2, 0, 1]], np.int32), B=B, kp16=np.full((3, B, width), 0x1234, np.int16), vp16=np.full((3, B, width), 0x1234, np.int16))
    _, _, k, v = run16(hip, case, None)
    HipDevice.synchronize()
    for pool, new, shift in ((k, kn, 0), (v, vn, 7)):
        flat = pool[[2, 0, 1]].reshape(3 * B, width)
        np.testing.assert_array_equal(words(flat[B - 2:B - 2 + m]), words(light.bf16_bits(new[0])))
        np.testing.assert_array_equal(words(flat[B - 2:B - 2 + m]).reshape(-1), words(tile(want, shift)).reshape(-1))       # ... the words by hand
        assert (flat[:B - 2] == 0x1234).all() and (flat[B - 2 + m:] == 0x1234).all()


# ---- 3. a key is r of it whichever call brought it in ---------------------------------------------------------------------------

def key_columns(t, m, i):
    """Kend of the workgroup that computes row i of a call of m rows at position t (csrc/extend_body.h): the key columns its chunk
    loops cover.  Two calls that give a row the same Kend split its keys over the waves of the context product alike"""
    q0 = 32 * (i // 32)
    return -(-(t + q0 + min(32, m - q0)) // 32) * 32


@pytest.mark.parametrize("d", [32, 64])
def test_the_result_does_not_depend_on_how_the_tokens_were_chunked(hip, d):
    """40 tokens of one slot in one call of m = 40, and in calls of 1, 7 and 32.  The pool words come out bitwise equal, and so do
    the probabilities, row by row: in the single call every key is the launch's own new row, in the pieces the keys of earlier
    pieces come from the pool - with new rows attended to unrounded the two would differ by a bfloat16 step, 4e-3 relative.

    The context rows are bitwise equal wherever the two schedules give the row's workgroup the same key columns (`key_columns`:
    rows 0 .. 7 and 32 .. 39 here - rows 32 .. 39 see keys 0 .. 7 from the pool in one schedule and from the launch in the other).
    Rows 8 .. 31 are computed over 32 key columns in the single call and over 64 in the third piece, and the context product splits
    its key columns over the waves: the float32 sums are folded in another order.  That is the float32 paged entry's own
    behaviour, kept by this launch on purpose (its contract is that entry's bits): measured on an MI355X, lg_attention_extend_paged_f32
    on the rounded rows differs between the two schedules in exactly these rows, by one unit in the last place (largest
    difference 1.19e-07), at D = 32 in rows 8 .. 31 and at D = 64 in rows 16 .. 31 - and the bfloat16 launch in the same rows by
    the same bits.  So for every row, in BOTH schedules, the context is asserted bitwise against the float32 paged entry run in
    that schedule on r(k_new), r(v_new) and float32 pools: whatever differs between the schedules is that entry's fold."""
    rng = np.random.RandomState(21)
    B, width, n = 16, HEADS * d, 40
    q, kn, vn = (rng.uniform(-1.5, 1.5, (1, n, width)).astype(np.float32) for _ in range(3))
    rk, rv = bf16_round_array(kn), bf16_round_array(vn)
    table = np.array([[3, 0, 2]], np.int32)
    tensor = lambda a: hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)      # noqa: E731
    schedules = ((40,), (1, 7, 32))
    results, columns = {}, {}
    for pieces in schedules:
        pools16 = tensor(np.full((4, B, width), 0x7FC0, np.int16)), tensor(np.full((4, B, width), 0x7FC0, np.int16))
        pools32 = tensor(np.full((4, B, width), np.nan, np.float32)), tensor(np.full((4, B, width), np.nan, np.float32))
        rows, probs, rows32, t, cols = [], [], [], 0, []
        for m in pieces:
            case = dict(q=q[:, t:t + m], kn=kn[:, t:t + m], vn=vn[:, t:t + m], pos=np.array([t], np.int32), count=np.array([m], np.int32), table=table, B=B)
            o, p, _, _ = run16(hip, case, None, pools=pools16)
            with light.no_grad():
                o32 = tensor(case["q"]).extend_attention(tensor(rk[:, t:t + m]), tensor(rv[:, t:t + m]), pools32[0], pools32[1], tensor(case["pos"]), heads=HEADS,
                                                         scale=math.sqrt(d) ** -1, count=tensor(case["count"]), block_table=tensor(table), block_size=B)
            rows.append(o[0])
            probs.append(p[0])
            rows32.append(o32.numpy()[0])
            cols += [key_columns(t, m, i) for i in range(m)]
            t += m
        results[pieces] = (np.concatenate(rows), np.concatenate(probs, axis=1), pools16[0].numpy(), pools16[1].numpy(), np.concatenate(rows32),
                           pools32[0].numpy())
        columns[pieces] = cols
    HipDevice.synchronize()
    one, three = (results[s] for s in schedules)
    np.testing.assert_array_equal(words(one[2]), words(three[2]))
    np.testing.assert_array_equal(words(one[3]), words(three[3]))
    assert (words(one[2][1]) == 0x7FC0).all() and np.isfinite(one[0]).all()
    np.testing.assert_array_equal(words(one[2][[3, 0, 2]].reshape(-1, width)[:n]), words(light.bf16_bits(kn[0])))
    same = [i for i in range(n) if columns[schedules[0]][i] == columns[schedules[1]][i]]
    assert same == list(range(8)) + list(range(32, 40))
    differing = [i for i in range(n) if (bits(one[0][i]) != bits(three[0][i])).any()]
    print("D %d: context rows that differ between the schedules: %s, largest difference %.3g; of the float32 entry: %s" % (
        d, differing, np.abs(one[0] - three[0]).max(), [i for i in range(n) if (bits(one[4][i]) != bits(three[4][i])).any()]))
    for i in range(n):
        np.testing.assert_array_equal(bits(one[1][:, i]), bits(three[1][:, i]), err_msg="probs row %d" % i)
        if i in same:
            np.testing.assert_array_equal(bits(one[0][i]), bits(three[0][i]), err_msg="context row %d" % i)
        for got in (one, three):                                          # ... and every row is the float32 entry's in the same schedule
            np.testing.assert_array_equal(bits(got[0][i]), bits(got[4][i]), err_msg="context row %d against the float32 paged entry" % i)
    # two orders of a float32 sum of n terms p_j * v_j with sum p_j = 1, |v_j| <= 1.5 differ by (n - 1) * 2 ** -24 * 1.5 at the most:
    # the fold's last bits, nowhere near a bfloat16 step (2 ** -8 relative)
    assert np.abs(one[0] - three[0]).max() <= (n - 1) * 2.0 ** -24 * 1.5
    for got in (one, three):
        np.testing.assert_array_equal(bits(light.bf16_widen(got[2])), bits(got[5]))


# ---- 4. projection + attention --------------------------------------------------------------------------------------------------

def test_rows_are_read_in_place_from_one_projection_buffer(hip, recorder):
    """x, weights and biases from {-1, 0, 1} with an inner size of 64: the projections are integers of at most 65 in size, exact
    in bfloat16 - so the bf16 route must give the float32 paged route's bits, and its pools widened are that route's pools"""
    case = bf16_case(16, 11, 32)
    rng = np.random.RandomState(3)
    b, m, width = case["q"].shape
    x = rng.randint(-1, 2, (b, m, 64)).astype(np.float32)
    ws = [rng.randint(-1, 2, (width, 64)).astype(np.float32) for _ in range(3)]
    bs = [rng.randint(-1, 2, width).astype(np.float32) for _ in range(3)]
    tensor = lambda a: hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)      # noqa: E731
    results = []
    for bf16 in (False, True):
        tk, tv = (tensor(case["kp16"]), tensor(case["vp16"])) if bf16 else (tensor(case["ref"]["kp"]), tensor(case["ref"]["vp"]))
        del recorder.calls[:]
        with light.no_grad():
            out = tensor(x).self_attention_extend(tensor(ws[0]), tensor(bs[0]), tensor(ws[1]), tensor(bs[1]), tensor(ws[2]), tensor(bs[2]), tk, tv,
                                                  tensor(case["pos"]), heads=HEADS, scale=0.125, probs=True, count=tensor(case["count"]),
                                                  block_table=tensor(case["table"]), block_size=16, **({"kv_dtype": "bf16"} if bf16 else {}))
        launches = [c for c in recorder.calls if c.startswith("lg_gemm") or c.startswith("lg_attention")]
        assert launches == ["lg_gemm_multi3_f32", ENTRY if bf16 else "lg_attention_extend_paged_f32"]
        results.append((out.numpy(), out.attention_probs.numpy(), tk.numpy(), tv.numpy()))
    HipDevice.synchronize()
    np.testing.assert_array_equal(bits(results[1][0]), bits(results[0][0]))
    np.testing.assert_array_equal(bits(results[1][1]), bits(results[0][1]))
    assert results[1][2].dtype == np.int16 and results[0][2].dtype == np.float32
    np.testing.assert_array_equal(bits(light.bf16_widen(results[1][2])), bits(results[0][2]))
    np.testing.assert_array_equal(bits(light.bf16_widen(results[1][3])), bits(results[0][3]))
    assert (words(results[1][2]) != words(case["kp16"])).any()


# ---- 5. against the definition --------------------------------------------------------------------------------------------------

class Fed(nn.Module):
    """a projection that returns what it was given when it was made: the composite's operands fed directly"""
    def __init__(self, tensor):
        nn.Module.__init__(self)
        self.fed = tensor

    def forward(self, x):
        return self.fed


def composite(case, mask, dtype):
    """`BertSelfAttention._paged_composite` on CpuTensor in `dtype` over an nn.PagedKVCache(kv_dtype="bf16") that holds the case's
    pools, with q, k_new, v_new fed in place of the projections: ({slot: real context rows}, {slot: real probability rows})"""
    b, m, width = case["q"].shape
    tensor = lambda a: CpuTensor.from_numpy(np.ascontiguousarray(a), requires_grad=False)          # noqa: E731
    clean = lambda a: np.nan_to_num(a, nan=0.25).astype(dtype)                                      # noqa: E731 (rows >= count: any number)
    attention = dc.bert.BertSelfAttention(width, HEADS, causal=True)
    attention.query, attention.key, attention.value = (Fed(tensor(clean(case[n]))) for n in ("q", "kn", "vn"))
    cache = nn.PagedKVCache(1, b, case["kp16"].shape[0], case["B"], width, case["table"].shape[1], like=tensor(np.zeros(1, dtype)), kv_dtype="bf16")
    cache.k[0][:], cache.v[0][:] = tensor(case["kp16"]), tensor(case["vp16"])
    cache.block_table[:] = tensor(case["table"])
    cache.pos[:] = tensor(case["pos"])
    with light.no_grad():
        context, probs = attention._paged_composite(tensor(np.zeros((b, m, width), dtype)), None if mask is None else tensor(mask.astype(dtype)), cache, 0,
                                                    tensor(case["count"]))
    context, probs = context.numpy(), probs.numpy()
    assert context.dtype == dtype
    named = {}
    for s, (t, n) in enumerate(case["slots"]):
        if n:
            named["context %d" % s], named["probs %d" % s] = context[s, :n], probs[s, :, :n, :t + n]
    return named, cache


@pytest.mark.parametrize("geometry,d", [((16, 11), 32), ((4, 6), 64)])
def test_the_bf16_launch_against_the_composite_on_identical_operands(hip, geometry, d):
    case = bf16_case(*geometry, d)
    kp, vp = pools16_expected(case)
    for masked in (False, True):
        mask = padding_mask(len(case["pos"]), case["C"]) if masked else None
        o, p, k, v = run16(hip, case, mask)
        got = {}
        for s, (t, n) in enumerate(case["slots"]):
            if n:
                got["context %d" % s], got["probs %d" % s] = o[s, :n], p[s, :, :n, :t + n]
        cpu32, cache32 = composite(case, mask, np.float32)
        with float64_tape():
            ref64, cache64 = composite(case, mask, np.float64)
        assert sorted(got) == sorted(ref64) and len(got) == 12
        assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, floor=1e-5, what="bf16 paged launch B %d x %d D %d" % (geometry + (d,)))
        # the three write the same words
        for cache in (cache32, cache64):
            np.testing.assert_array_equal(words(cache.k[0].numpy()), words(kp))
            np.testing.assert_array_equal(words(cache.v[0].numpy()), words(vp))
        np.testing.assert_array_equal(words(k), words(kp))
    HipDevice.synchronize()


# ---- 6. shared blocks -----------------------------------------------------------------------------------------------------------

def test_two_slots_share_blocks_below_both_positions(hip):
    """test_hip_paged's case on bfloat16 words: blocks 5 and 2 hold positions 0 .. 31 of BOTH slots; slot 0 goes on at 40 in blocks 7
    and 0, slot 1 at 33 in block 3.  Each slot equals the launch on it alone, and the shared blocks keep their words"""
    B, width = 16, HEADS * 32
    rng = np.random.RandomState(5)
    table = np.array([[5, 2, 7, 0], [5, 2, 3, -1]], np.int32)
    pos, count, m = np.array([40, 33], np.int32), np.array([9, 4], np.int32), 9
    kp, vp = (np.full((9, B, width), np.nan, np.float32) for _ in range(2))
    for block, rows in ((5, 16), (2, 16), (7, 8), (3, 1)):
        kp[block, :rows], vp[block, :rows] = rng.uniform(-1.5, 1.5, (2, rows, width)).astype(np.float32)
    q, kn, vn = (rng.uniform(-1.5, 1.5, (2, m, width)).astype(np.float32) for _ in range(3))
    case = dict(q=q, kn=kn, vn=vn, kp16=light.bf16_bits(kp), vp16=light.bf16_bits(vp), pos=pos, count=count, table=table, B=B)
    both = run16(hip, case, None)
    for s in range(2):
        alone = run16(hip, case, None, rows=slice(s, s + 1))
        np.testing.assert_array_equal(bits(both[0][s]), bits(alone[0][0]), err_msg="context of slot %d" % s)
        np.testing.assert_array_equal(bits(both[1][s]), bits(alone[1][0]), err_msg="probs of slot %d" % s)
        for own in table[s, 2:]:
            if own >= 0:
                np.testing.assert_array_equal(words(both[2][own]), words(alone[2][own]))
                np.testing.assert_array_equal(words(both[3][own]), words(alone[3][own]))
        assert np.isfinite(both[0][s, :count[s]]).all()
    for shared in (5, 2):
        np.testing.assert_array_equal(words(both[2][shared]), words(case["kp16"][shared]))
        np.testing.assert_array_equal(words(both[3][shared]), words(case["vp16"][shared]))
    for nobody in (1, 4, 6, 8):
        assert (words(both[2][nobody]) == 0x7FC0).all() and (words(both[3][nobody]) == 0x7FC0).all()
    HipDevice.synchronize()


# ---- 7. bounds, 8. refusals -----------------------------------------------------------------------------------------------------

class PagedCall16(th.PagedCall):
    """test_hip_paged.PagedCall - the (16, 2) launch case at D = 32 through the C ABI - with the pools as bfloat16 words"""
    def __init__(self, hip, table=None):
        th.PagedCall.__init__(self, hip, table)
        up = lambda a: hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)      # noqa: E731
        self.kp16, self.vp16 = light.bf16_bits(self.case["kp"]), light.bf16_bits(self.case["vp"])
        self.k, self.v = up(self.kp16), up(self.vp16)
        self.args.update(k_pool=self.k.ptr, v_pool=self.v.ptr)

    def __call__(self, **override):
        return self.lib.lg_attention_extend_paged_bf16_f32(*dict(self.args, **override).values())

    def untouched(self):
        return ((self.o.numpy() == he.SENTINEL).all() and (self.p.numpy() == he.SENTINEL).all()
                and (words(self.k.numpy()) == words(self.kp16)).all() and (words(self.v.numpy()) == words(self.vp16)).all())


@pytest.mark.parametrize("entry", ["-1", "num_blocks"])
def test_a_bad_table_word_is_reported_writes_nothing_and_the_others_are_computed(hip, entry):
    """slot 3 (t = 14, 5 new rows: it reaches both of its blocks) has a word that names no block.  Nothing here faults: the word
    never becomes an address"""
    good = PagedCall16(hip)
    assert good() == 0
    HipDevice.synchronize()
    want = good.results()
    table = good.case["table"].copy()
    table[3, 1] = -1 if entry == "-1" else good.case["kp"].shape[0]
    call = PagedCall16(hip, table=table)
    assert call() == 0                                                    # the launch itself is fine: the kernel reads the words
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    o, p, k, v = call.results()
    assert (o[3] == he.SENTINEL).all() and (p[3] == he.SENTINEL).all()
    others = [s for s in range(len(table)) if s != 3]
    np.testing.assert_array_equal(bits(o[others]), bits(want[0][others]))
    np.testing.assert_array_equal(bits(p[others]), bits(want[1][others]))
    # the pools: everything the good launch wrote but slot 3's rows
    B, (t, n) = 16, good.case["slots"][3]
    kp, vp = want[2].copy(), want[3].copy()
    for j in range(t, t + n):
        block = good.case["table"][3, j // B]
        kp[block, j % B], vp[block, j % B] = good.kp16[block, j % B], good.vp16[block, j % B]
    np.testing.assert_array_equal(words(k), words(kp))
    np.testing.assert_array_equal(words(v), words(vp))


def test_a_word_behind_the_reach_changes_nothing(hip):
    case = bf16_case(4, 6, 32)
    first = run16(hip, case, None)
    reach = [-(-(t + n) // 4) for t, n in case["slots"]]
    for filler in (-1, 0, 2 ** 31 - 1):
        other = dict(case, table=case["table"].copy())
        for s, r in enumerate(reach):
            other["table"][s, r:] = filler
        again = run16(hip, other, None)
        for name, a, c in zip(("context", "probs"), first[:2], again[:2]):
            np.testing.assert_array_equal(bits(a), bits(c), err_msg="%s with %d behind the reach" % (name, filler))
        for name, a, c in zip(("k pool", "v pool"), first[2:], again[2:]):
            np.testing.assert_array_equal(words(a), words(c), err_msg="%s with %d behind the reach" % (name, filler))
    HipDevice.synchronize()


def test_refusals_through_the_c_abi_launch_nothing(hip, recorder):
    call = PagedCall16(hip)
    handle = recorder._handle
    entry = lambda **o: handle.lg_attention_extend_paged_bf16_f32(*dict(call.args, **o).values())      # noqa: E731
    a = call.args
    del recorder.calls[:]
    for override, word in ((dict(k_pool=a["k_pool"] + 4), b"8-byte aligned"), (dict(v_pool=a["v_pool"] + 2), b"8-byte aligned"), (dict(k_pool=None), b"non-NULL"),
                           (dict(ldc=66), b"multiple of 4"), (dict(ldc=32), b"pitch"), (dict(ldc=60), b"pitch"),
                           (dict(block_table=a["k_pool"]), b"overlaps"), (dict(block_table=a["v_pool"] + 64), b"overlaps"), (dict(block_table=a["o"]), b"overlaps"),
                           (dict(block_table=a["p"] + 32), b"overlaps"), (dict(pos=a["k_pool"]), b"overlaps"), (dict(count=a["v_pool"] + 16), b"overlaps"),
                           (dict(count=a["pos"]), b"overlaps"), (dict(k_new=a["k_pool"]), b"overlaps"), (dict(v_new=a["v_pool"] + 128), b"overlaps"),
                           (dict(o=a["k_pool"]), b"overlaps"), (dict(p=a["v_pool"]), b"overlaps"), (dict(v_pool=a["k_pool"]), b"overlaps"),
                           (dict(o=a["p"]), b"overlaps"), (dict(block_table=None), b"non-NULL"), (dict(count=None), b"non-NULL"),
                           (dict(block_table=a["block_table"] + 2), b"aligned"), (dict(D=48), b"unsupported"), (dict(D=128), b"unsupported"), (dict(m=0), b"unsupported"),
                           (dict(m=33), b"unsupported"), (dict(log2_block=1), b"unsupported"), (dict(log2_block=8), b"unsupported"),
                           (dict(max_blocks=0), b"unsupported"), (dict(max_blocks=33), b"unsupported"), (dict(num_blocks=0), b"unsupported"), (dict(ldq=66), b"pitches")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and ENTRY.encode() in handle.lg_last_error(), (override, handle.lg_last_error())
    assert entry(batch=0) == 0
    HipDevice.synchronize()
    assert call.untouched() and [c for c in recorder.calls if c != "lg_sync"] == []
    # the overlaps are sized at 2 bytes a pool element: a table right behind the last pool word is apart from the pool (at 4 bytes
    # an element it would lie inside), one word earlier it overlaps
    case = call.case
    pool_words = case["kp"].size
    joined = np.concatenate([call.kp16.reshape(-1), case["table"].reshape(-1).view(np.int16)])
    both = hip.from_numpy(joined, requires_grad=False)
    assert both.ptr % 8 == 0 and (2 * pool_words) % 4 == 0
    assert entry(k_pool=both.ptr, block_table=both.ptr + 2 * pool_words - 4) == LG_EINVAL and b"overlaps" in handle.lg_last_error()
    HipDevice.synchronize()
    assert call.untouched()
    assert entry(k_pool=both.ptr, block_table=both.ptr + 2 * pool_words) == 0, handle.lg_last_error()
    HipDevice.synchronize()
    good = PagedCall16(hip)
    assert good() == 0
    HipDevice.synchronize()
    np.testing.assert_array_equal(bits(call.o.numpy()), bits(good.o.numpy()))
    after = both.numpy()
    np.testing.assert_array_equal(words(after[:pool_words].reshape(case["kp"].shape)), words(good.k.numpy()))
    np.testing.assert_array_equal(after[pool_words:].view(np.int32).reshape(case["table"].shape), case["table"])


def test_the_ops_refuse_the_other_form_of_pools_by_name(hip, recorder):
    case = bf16_case(16, 2, 32)
    tensor = lambda x: hip.from_numpy(np.ascontiguousarray(x), requires_grad=False)      # noqa: E731
    tq, tkn, tvn, tpos, tcount, ttable = (tensor(case[n]) for n in ("q", "kn", "vn", "pos", "count", "table"))
    k16, v16, k32, v32 = tensor(case["kp16"]), tensor(case["vp16"]), tensor(case["ref"]["kp"]), tensor(case["ref"]["vp"])
    w, bias = tensor(np.zeros((64, 64), np.float32)), tensor(np.zeros(64, np.float32))
    paged = dict(block_table=ttable, block_size=16, count=tcount)
    del recorder.calls[:]
    for pools, kw, error, match in (((k16, v16), paged, TypeError, "kv_dtype=\"bf16\""),                               # int16 pools without the keyword
                                    ((k32, v32), dict(paged, kv_dtype="bf16"), TypeError, "float32 pools go without"),  # the keyword with float32 pools
                                    ((k16, v32), dict(paged, kv_dtype="bf16"), TypeError, "float32 pools go without"),
                                    ((k16, v16), dict(paged, kv_dtype="fp8"), AssertionError, "kv_dtype"),
                                    ((k32, v32), dict(count=tcount, kv_dtype="bf16"), AssertionError, "kv_dtype.*paged")):
        for op in ("extend_attention", "self_attention_extend"):
            with pytest.raises(error, match=match), light.no_grad():
                if op.startswith("self"):
                    tq.self_attention_extend(w, bias, w, bias, w, bias, pools[0], pools[1], tpos, heads=HEADS, scale=0.2, **kw)
                else:
                    tq.extend_attention(tkn, tvn, pools[0], pools[1], tpos, heads=HEADS, scale=0.2, **kw)
    assert recorder.attention() == []
    np.testing.assert_array_equal(words(k16.numpy()), words(case["kp16"]))


# ---- 9. serve -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=sc.SEED)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", (1, 16))
@pytest.mark.parametrize("pool", ["generous", "tight"])
def test_bf16_serve_on_hip_gives_each_request_its_own_rounded_continuation(hip, model, slots, chunk, pool, captured):
    rows = pg.prefixed_prompts()
    want, want_len = sc.expected(pb.assert_rounded_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    lengths = [len(p) for p in rows]
    for prefix in (0, pg.PREFIX):
        F = 2 if prefix else 0
        num_blocks = F + slots * pg.MAX_BLOCKS if pool == "generous" else pg.tight_blocks(rows, sc.BUDGET, F)
        graph = HipGraph() if captured else None
        out, out_len, stats, cache = pb.run_serve(hip, slots, chunk, num_blocks, model=model, poll=1, graph=graph, shared_prefix=prefix)
        np.testing.assert_array_equal(out_len, want_len)
        np.testing.assert_array_equal(out, want)
        assert stats["prefix_blocks"] == F and stats["steps"] == pg.simulate(lengths, want_len, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, num_blocks, F)
        pg.assert_no_block_leaked(cache, F)
        if captured:
            assert graph.kernel_count() > 0
            graph.destroy()


def test_the_bf16_step_has_the_launches_of_the_float_paged_step_and_the_host_reads_the_poll_word_only(hip, model, recorder):
    rows = pg.prefixed_prompts()
    want, _ = sc.expected(pb.assert_rounded_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    want32, _ = sc.expected(pg.assert_prefixed_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    like = model.cls.predictions.bias

    def steps_of(kv_dtype, expected):
        cache = nn.PagedKVCache(sc.CFG["num_hidden_layers"], 3, 14, pg.BLOCK, sc.CFG["hidden_size"], pg.MAX_BLOCKS, like=like, kv_dtype=kv_dtype)
        del recorder.calls[:], recorder.reads[:]
        (out, out_len), stats = dc.bert.serve(model, rows, sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4)
        steps = stats["steps"]
        assert steps % 4 == 0 and recorder.reads == [4] * (steps // 4)    # one int32 word per poll, nothing else
        calls = [c for c in recorder.calls if c != "lg_sync"]
        np.testing.assert_array_equal(out.numpy(), expected)
        pg.assert_no_block_leaked(cache)
        per_step, step = [], []
        for name in calls:
            step.append(name)
            if name == "lg_serve_commit_paged_i32":
                per_step.append(step)
                step = []
        assert step == [] and len(per_step) == steps + 1                  # the admission commit, then a commit at the end of every step
        assert all(s == per_step[1] for s in per_step[2:]), "a step's launches depend on what the slots hold"
        # ... and the captured step holds as many kernels as entries were called
        graph = HipGraph()
        cache.reset()
        dc.bert.serve(model, rows, sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4, graph=graph)
        kernels = graph.kernel_count()
        graph.destroy()
        return per_step[1], kernels

    bf16_step, bf16_kernels = steps_of("bf16", want)
    float_step, float_kernels = steps_of(None, want32)
    assert bf16_step.count(ENTRY) == sc.CFG["num_hidden_layers"] and "lg_attention_extend_paged_f32" not in bf16_step
    assert [{ENTRY: "lg_attention_extend_paged_f32"}.get(c, c) for c in bf16_step] == float_step
    assert bf16_kernels == float_kernels > 0
    print("launch entries of one bf16 paged serving step: %d, kernels of the captured step: %d (float32 pools: %d, %d)" % (
        len(bf16_step), bf16_kernels, len(float_step), float_kernels))
