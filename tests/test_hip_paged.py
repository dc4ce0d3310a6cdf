"""The paged key / value cache on the GPU: lg_attention_extend_paged_f32 (csrc/paged.hip: the counts launch with the caches reached
through a block table), lg_serve_commit_paged_i32 (csrc/serve_paged.hip: the commit with a stack of free blocks) and what stands
on them - `extend_attention(count=, block_table=, block_size=)`, `Tensor.serve_commit_paged`, one model step against shuffled
tables and the paged `serve` of examples/bert.py, eager and captured, with a generous and a tight pool, with and without a shared
prefix.

"Bit for bit against the counts entry": the context, the probabilities and the bytes of the new rows in the pool equal those of
lg_attention_extend_counts_f32 on a contiguous (b, capacity, width) cache that holds the same rows below each slot's position.
Every pool row that holds no row of a slot holds NaN before the launch and its own bits after it: the launch reaches nothing it
should not.  The numerics of the counts entry are the ground of test_hip_serve.py / test_hip_extend.py."""
import math
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from common import assert_as_close_to_float64_as_the_cpu_backend
from test_hip_attention_masked import padding_mask
from test_hip_serve import recorder                                       # noqa: F401 (a fixture)
import test_hip_extend as he
import decode_cases as dc
import serve_cases as sc
import paged_cases as pg

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
HEADS = 2
bits = he.bits
GEOMETRIES = ((4, 6), (16, 2), (16, 11), (32, 5), (128, 2), (64, 8))      # (B, max_blocks): capacities 24 .. 512; (16, 11), (32, 5) cross a 128-key chunk inside a table


def slots_of(B, max_blocks):
    """(t, count) per slot and m: t = 0; a seam inside a block; a seam on a block boundary; new rows that cross a block boundary;
    count = 0; t + count = capacity, twice"""
    C = B * max_blocks
    m = min(33, C)
    half = min(m, C // 2)
    return ((0, min(m, B + 1)), (B + 1, 3), (B, 2), (B - 2, 5), (C // 2 + 1, 0), (C - half, half), (C - 1, 1)), m


def tables_of(slots, B, max_blocks, seed, spare=3):
    """(table (b, max_blocks), num_blocks): the blocks every slot reaches drawn from a shuffled pool, slot after slot for each table
    word in turn (neighbouring words of a row are far apart, neighbouring blocks belong to different slots); `spare` blocks are in
    no table; the words behind a slot's reach hold -1 (even slots) or a number far beyond the pool (odd slots)"""
    reach = [-(-(t + n) // B) for t, n in slots]
    num_blocks = sum(reach) + spare
    order = np.random.RandomState(seed).permutation(num_blocks).tolist()
    table = np.array([[-1 if s % 2 == 0 else 10 ** 6 + s] * max_blocks for s in range(len(slots))], np.int32)
    for n in range(max_blocks):
        for s in range(len(slots)):
            if n < reach[s]:
                table[s, n] = order.pop()
    return table, num_blocks


def paged_operands(B, max_blocks, d, seed=13):
    """a launch case: the contiguous operands of the counts entry (NaN in every cache row >= t and every token row >= count) and
    the same rows in pools through shuffled tables, NaN everywhere else"""
    slots, m = slots_of(B, max_blocks)
    C, width, b = B * max_blocks, HEADS * d, len(slots)
    rng = np.random.RandomState(seed)
    k, v = (rng.uniform(-1.5, 1.5, (b, C, width)).astype(np.float32) for _ in range(2))
    q, kn, vn = (rng.uniform(-1.5, 1.5, (b, m, width)).astype(np.float32) for _ in range(3))
    table, num_blocks = tables_of(slots, B, max_blocks, seed)
    kp, vp = (np.full((num_blocks, B, width), np.nan, np.float32) for _ in range(2))
    for s, (t, n) in enumerate(slots):
        k[s, t:], v[s, t:] = np.nan, np.nan
        q[s, n:], kn[s, n:], vn[s, n:] = np.nan, np.nan, np.nan
        for j in range(t):
            kp[table[s, j // B], j % B], vp[table[s, j // B], j % B] = k[s, j], v[s, j]
    pos, count = np.array([t for t, _ in slots], np.int32), np.array([n for _, n in slots], np.int32)
    return dict(k=k, v=v, q=q, kn=kn, vn=vn, kp=kp, vp=vp, pos=pos, count=count, table=table, slots=slots, m=m, B=B, C=C)


def run(hip, case, mask, paged, rows=None):
    """one launch of `extend_attention(count=)` - paged: with block_table= on the pools - on fresh device copies, of the slots `rows`
    (default: all): (context, probs, k after, v after) as numpy"""
    rows = slice(None) if rows is None else rows
    tensor = lambda a: hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)      # noqa: E731
    tq, tkn, tvn, tpos, tcount = (tensor(case[name][rows]) for name in ("q", "kn", "vn", "pos", "count"))
    tm = None if mask is None else tensor(mask[rows])
    d = case["q"].shape[-1] // HEADS
    if paged:
        tk, tv, extra = tensor(case["kp"]), tensor(case["vp"]), dict(block_table=tensor(case["table"][rows]), block_size=case["B"])
    else:
        tk, tv, extra = tensor(case["k"][rows]), tensor(case["v"][rows]), {}
    with light.no_grad():
        out = tq.extend_attention(tkn, tvn, tk, tv, tpos, heads=HEADS, scale=math.sqrt(d) ** -1, mask=tm, probs=True, count=tcount, **extra)
    return out.numpy(), out.attention_probs.numpy(), tk.numpy(), tv.numpy()


def pools_expected(case, ref_k, ref_v):
    """the pools after the launch: what they held, with rows t .. t + count - 1 of every slot where its table says"""
    kp, vp, B = case["kp"].copy(), case["vp"].copy(), case["B"]
    for s, (t, n) in enumerate(case["slots"]):
        for j in range(t, t + n):
            kp[case["table"][s, j // B], j % B], vp[case["table"][s, j // B], j % B] = ref_k[s, j], ref_v[s, j]
    return kp, vp


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["B%dx%d" % g for g in GEOMETRIES])
def test_paged_slots_equal_the_counts_entry_bit_for_bit(hip, recorder, geometry, d):
    case = paged_operands(*geometry, d)
    for masked in (False, True):
        mask = padding_mask(len(case["pos"]), case["C"]) if masked else None
        want = run(hip, case, mask, paged=False)
        del recorder.calls[:]
        got = run(hip, case, mask, paged=True)
        assert recorder.attention() == ["lg_attention_extend_paged_f32"]
        what = "B %d x %d D %d %s" % (geometry + (d, "mask" if masked else "nomask"))
        np.testing.assert_array_equal(bits(got[0]), bits(want[0]), err_msg=what + ": context")
        np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg=what + ": probs")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), what
        kp, vp = pools_expected(case, want[2], want[3])
        np.testing.assert_array_equal(bits(got[2]), bits(kp), err_msg=what + ": k pool (the new rows, and every other row untouched)")
        np.testing.assert_array_equal(bits(got[3]), bits(vp), err_msg=what + ": v pool")
        for s, (t, n) in enumerate(case["slots"]):                       # the new rows are the token rows' own bytes, the rest of the row is +0.0
            assert (bits(got[0][s, n:]) == 0).all() and (bits(got[1][s, :, n:]) == 0).all(), (what, s)
            for j in range(n):
                np.testing.assert_array_equal(bits(got[2][case["table"][s, (t + j) // case["B"]], (t + j) % case["B"]]), bits(case["kn"][s, j]))
    HipDevice.synchronize()                                               # no slot raised the flag


def test_rows_are_read_in_place_from_one_projection_buffer(hip, recorder):
    """`self_attention_extend(count=, block_table=)`: the projection launch and the paged launch, against the same call on the
    contiguous cache"""
    case = paged_operands(16, 11, 32)
    rng = np.random.RandomState(3)
    b, m, width = case["q"].shape
    x = rng.uniform(-1, 1, (b, m, 64)).astype(np.float32)
    ws = [rng.uniform(-0.3, 0.3, (width, 64)).astype(np.float32) for _ in range(3)]
    bs = [rng.uniform(-0.3, 0.3, width).astype(np.float32) for _ in range(3)]
    tensor = lambda a: hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)      # noqa: E731
    results = []
    for paged in (False, True):
        tk, tv = (tensor(case["kp" if paged else "k"]), tensor(case["vp" if paged else "v"]))
        extra = dict(block_table=tensor(case["table"]), block_size=16) if paged else {}
        del recorder.calls[:]
        with light.no_grad():
            out = tensor(x).self_attention_extend(tensor(ws[0]), tensor(bs[0]), tensor(ws[1]), tensor(bs[1]), tensor(ws[2]), tensor(bs[2]), tk, tv,
                                                  tensor(case["pos"]), heads=HEADS, scale=0.2, probs=True, count=tensor(case["count"]), **extra)
        launches = [c for c in recorder.calls if c.startswith("lg_gemm") or c.startswith("lg_attention")]
        assert launches == ["lg_gemm_multi3_f32", "lg_attention_extend_paged_f32" if paged else "lg_attention_extend_counts_f32"]
        results.append((out.numpy(), out.attention_probs.numpy(), tk.numpy(), tv.numpy()))
    np.testing.assert_array_equal(bits(results[1][0]), bits(results[0][0]))
    np.testing.assert_array_equal(bits(results[1][1]), bits(results[0][1]))
    kp, vp = pools_expected(case, results[0][2], results[0][3])
    np.testing.assert_array_equal(bits(results[1][2]), bits(kp))
    np.testing.assert_array_equal(bits(results[1][3]), bits(vp))


def test_two_slots_share_blocks_below_both_positions(hip):
    """blocks 5 and 2 hold positions 0 .. 31 of BOTH slots (a common prefix); slot 0 goes on at 40 in blocks 7 and 0, slot 1 at 33 in
    block 3.  Each slot equals the launch on it alone, and the shared blocks keep their bits"""
    B, d, width = 16, 32, HEADS * 32
    rng = np.random.RandomState(5)
    table = np.array([[5, 2, 7, 0], [5, 2, 3, -1]], np.int32)
    pos, count, m = np.array([40, 33], np.int32), np.array([9, 4], np.int32), 9
    kp, vp = (np.full((9, B, width), np.nan, np.float32) for _ in range(2))
    for block, rows in ((5, 16), (2, 16), (7, 8), (3, 1)):
        kp[block, :rows], vp[block, :rows] = rng.uniform(-1.5, 1.5, (2, rows, width)).astype(np.float32)
    q, kn, vn = (rng.uniform(-1.5, 1.5, (2, m, width)).astype(np.float32) for _ in range(3))
    case = dict(q=q, kn=kn, vn=vn, kp=kp, vp=vp, pos=pos, count=count, table=table, B=B)
    both = run(hip, case, None, paged=True)
    for s in range(2):
        alone = run(hip, case, None, paged=True, rows=slice(s, s + 1))
        np.testing.assert_array_equal(bits(both[0][s]), bits(alone[0][0]), err_msg="context of slot %d" % s)
        np.testing.assert_array_equal(bits(both[1][s]), bits(alone[1][0]), err_msg="probs of slot %d" % s)
        for own in table[s, 2:]:
            if own >= 0:
                np.testing.assert_array_equal(bits(both[2][own]), bits(alone[2][own]))
                np.testing.assert_array_equal(bits(both[3][own]), bits(alone[3][own]))
        assert np.isfinite(both[0][s, :count[s]]).all()
    for shared in (5, 2):
        np.testing.assert_array_equal(bits(both[2][shared]), bits(kp[shared]))
        np.testing.assert_array_equal(bits(both[3][shared]), bits(vp[shared]))
    for nobody in (1, 4, 6, 8):
        assert np.isnan(both[2][nobody]).all() and np.isnan(both[3][nobody]).all()
    HipDevice.synchronize()


class PagedCall(object):
    """the (16, 2) launch case at D = 32 on the device through the C ABI, every argument replaceable; o and p hold a sentinel"""
    def __init__(self, hip, table=None):
        from lightgrad_amd.autograd.hip import lib as L
        self.lib = L.lib()
        case = self.case = paged_operands(16, 2, 32)
        b, m, width = case["q"].shape
        up = lambda a: hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)      # noqa: E731
        self.k, self.v, self.q, self.kn, self.vn, self.pos, self.count = (up(case[n]) for n in ("kp", "vp", "q", "kn", "vn", "pos", "count"))
        self.table = up(case["table"] if table is None else table)
        self.o = up(np.full((b, m, width), he.SENTINEL, np.float32))
        self.p = up(np.full((b, HEADS, m, 32), he.SENTINEL, np.float32))
        self.args = dict(q=self.q.ptr, ldq=width, sbq=m * width, k_new=self.kn.ptr, ldk=width, sbk=m * width, v_new=self.vn.ptr, ldv=width, sbv=m * width,
                         k_pool=self.k.ptr, v_pool=self.v.ptr, ldc=width, pos=self.pos.ptr, count=self.count.ptr, block_table=self.table.ptr, o=self.o.ptr,
                         ldo=width, sbo=m * width, p=self.p.ptr, batch=b, heads=HEADS, m=m, max_blocks=2, num_blocks=case["kp"].shape[0], log2_block=4, D=32,
                         scale=math.sqrt(32) ** -1, mask=None, sbm=0)

    def __call__(self, **override):
        return self.lib.lg_attention_extend_paged_f32(*dict(self.args, **override).values())

    def results(self):
        return self.o.numpy(), self.p.numpy(), self.k.numpy(), self.v.numpy()

    def untouched(self):
        return ((self.o.numpy() == he.SENTINEL).all() and (self.p.numpy() == he.SENTINEL).all()
                and (bits(self.k.numpy()) == bits(self.case["kp"])).all() and (bits(self.v.numpy()) == bits(self.case["vp"])).all())


@pytest.mark.parametrize("entry", ["-1", "num_blocks"])
def test_a_bad_table_word_is_reported_writes_nothing_and_the_others_are_computed(hip, entry):
    """the bounds check of the launch: slot 3 (t = 14, 5 new rows: it reaches both of its blocks) has a word that names no block.
    Nothing here faults: the word never becomes an address"""
    good = PagedCall(hip)
    assert good() == 0
    HipDevice.synchronize()
    want = good.results()
    table = good.case["table"].copy()
    table[3, 1] = -1 if entry == "-1" else good.case["kp"].shape[0]
    call = PagedCall(hip, table=table)
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
        kp[block, j % B], vp[block, j % B] = good.case["kp"][block, j % B], good.case["vp"][block, j % B]
    np.testing.assert_array_equal(bits(k), bits(kp))
    np.testing.assert_array_equal(bits(v), bits(vp))


def test_a_word_behind_the_reach_changes_nothing(hip):
    """B = 4, tables of 6: every slot but the last two has words behind its reach - valid blocks of OTHER slots, -1 or numbers far
    beyond the pool give the same bits, in the outputs and in every pool row"""
    case = paged_operands(4, 6, 32)
    first = run(hip, case, None, paged=True)
    reach = [-(-(t + n) // 4) for t, n in case["slots"]]
    for filler in (-1, 0, 2 ** 31 - 1):
        other = dict(case, table=case["table"].copy())
        for s, r in enumerate(reach):
            other["table"][s, r:] = filler
        again = run(hip, other, None, paged=True)
        for name, a, c in zip(("context", "probs", "k pool", "v pool"), first, again):
            np.testing.assert_array_equal(bits(a), bits(c), err_msg="%s with %d behind the reach" % (name, filler))
    HipDevice.synchronize()


def test_paged_operands_that_overlap_are_refused_and_nothing_is_launched(hip, recorder):
    call = PagedCall(hip)
    handle = recorder._handle
    entry = lambda **o: handle.lg_attention_extend_paged_f32(*dict(call.args, **o).values())      # noqa: E731
    a = call.args
    for override, word in ((dict(block_table=a["k_pool"]), b"overlaps"), (dict(block_table=a["v_pool"] + 64), b"overlaps"), (dict(block_table=a["o"]), b"overlaps"),
                           (dict(block_table=a["p"] + 32), b"overlaps"), (dict(pos=a["k_pool"]), b"overlaps"), (dict(count=a["v_pool"] + 16), b"overlaps"),
                           (dict(count=a["pos"]), b"overlaps"), (dict(k_new=a["k_pool"]), b"overlaps"), (dict(v_new=a["v_pool"] + 128), b"overlaps"),
                           (dict(o=a["k_pool"]), b"overlaps"), (dict(p=a["v_pool"]), b"overlaps"), (dict(v_pool=a["k_pool"]), b"overlaps"),
                           (dict(o=a["p"]), b"overlaps"), (dict(block_table=None), b"non-NULL"), (dict(count=None), b"non-NULL"),
                           (dict(block_table=a["block_table"] + 2), b"aligned"), (dict(D=48), b"unsupported"), (dict(m=0), b"unsupported"),
                           (dict(m=33), b"unsupported"), (dict(log2_block=1), b"unsupported"), (dict(log2_block=8), b"unsupported"),
                           (dict(max_blocks=33), b"unsupported"), (dict(num_blocks=0), b"unsupported"), (dict(ldq=66), b"pitches"), (dict(ldc=32), b"pitch")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_attention_extend_paged_f32" in handle.lg_last_error(), override
    assert entry(batch=0) == 0
    HipDevice.synchronize()
    assert call.untouched()
    # through the ops: a table without a count or a block size, of another shape or dtype, next to cu=, pools of another block size
    case = call.case
    tensor = lambda x: hip.from_numpy(np.ascontiguousarray(x), requires_grad=False)      # noqa: E731
    tk, tv, tq, tkn, tvn, tpos, tcount, ttable = (tensor(case[n]) for n in ("kp", "vp", "q", "kn", "vn", "pos", "count", "table"))
    w, bias = tensor(np.zeros((64, 64), np.float32)), tensor(np.zeros(64, np.float32))
    del recorder.calls[:]
    for kw in (dict(block_table=ttable, block_size=16), dict(block_table=ttable, count=tcount), dict(block_size=16, count=tcount),
               dict(block_table=ttable, block_size=8, count=tcount), dict(block_table=ttable, block_size=12, count=tcount),
               dict(block_table=tensor(case["table"][:3]), block_size=16, count=tcount), dict(block_table=tensor(case["table"].astype(np.int64)), block_size=16, count=tcount),
               dict(block_table=ttable, block_size=16, count=tcount, cu=tensor(np.zeros(8, np.int32)))):
        for op in ("extend_attention", "self_attention_extend"):
            with pytest.raises(AssertionError, match="block_table|block_size|pools"), light.no_grad():
                if op.startswith("self"):
                    tq.self_attention_extend(w, bias, w, bias, w, bias, tk, tv, tpos, heads=HEADS, scale=0.2, **kw)
                else:
                    tq.extend_attention(tkn, tvn, tk, tv, tpos, heads=HEADS, scale=0.2, **kw)
    assert recorder.attention() == []
    np.testing.assert_array_equal(bits(tk.numpy()), bits(case["kp"]))


# ---- serve_commit_paged ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", (1, 3, 7, 64, 65, 70, 1024))
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("prefix_blocks", (0, 2))
def test_serve_commit_paged_against_the_words_by_hand(hip, recorder, b, eos, prefix_blocks):
    """the tables and the stack included: which block a slot gets is fixed by the definition.  64 slots fill a wave, 65 and 70
    cross into a second - the scans cross a wave -, 1024 fill the workgroup"""
    for spare in (0, 2, 500):
        for waiting in (0, 2, b + 100):
            state, nxt = pg.commit_state(b, waiting, 10 * b + waiting, prefix_blocks, spare, eos=eos)
            want, flag = pg.commit_by_hand(state, nxt, 4, prefix_blocks, eos)
            del recorder.calls[:]
            tensors, error = pg.commit_on(hip, state, nxt, 4, prefix_blocks, eos)
            assert error is None and not flag and recorder.calls == ["lg_serve_commit_paged_i32"]
            HipDevice.synchronize()
            for name in pg.NAMES:
                np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg="%s (spare %d, waiting %d)" % (name, spare, waiting))


def test_the_dry_pool_and_the_bounds_of_the_commit_on_hip(hip):
    state, nxt = pg.dry_pool_state()
    want, _ = pg.commit_by_hand(state, nxt, 4, 0, None)
    assert want["req"].tolist() == [0, -1, -1]                             # the third request does not overtake the second
    tensors, _ = pg.commit_on(hip, state, nxt, 4, 0, None)
    HipDevice.synchronize()
    for name in pg.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)
    # a bounds check, never a fault: the flag, count 0, the slot's other words as they were
    base, nxt = pg.commit_state(7, 4, 5, 0, 3, eos=3)
    for change in ("held", "entry", "stack", "need"):
        state = {k: v.copy() for k, v in base.items()}
        if change == "held":
            state["held"][3] = 7
        elif change == "entry":
            state["block_table"][4, 1] = len(state["free"]) - 1
        elif change == "stack":
            state["free"][0] = len(state["free"])
        else:
            state["budget"][state["queue"][0]] = 30
        want, flag = pg.commit_by_hand(state, nxt, 4, 0, 3)
        assert flag
        tensors, _ = pg.commit_on(hip, state, nxt, 4, 0, 3)
        with pytest.raises(IndexError):
            HipDevice.synchronize()
        HipDevice.synchronize()
        for name in pg.NAMES:
            np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg="%s (%s)" % (name, change))


def test_serve_commit_paged_refusals_launch_nothing(hip, recorder):
    state, nxt = pg.commit_state(3, 2, 0, 0, 4)
    i32 = lambda *shape: hip.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    for name, other in (("held", i32(4)), ("block_table", i32(2, 6)), ("free", hip.from_numpy(np.zeros(5, np.int64), requires_grad=False)), ("held", "count"),
                        ("free", "last"), ("req", i32(4))):
        tensors = sc.upload(hip, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="serve_commit"):
            hip.from_numpy(nxt.copy(), requires_grad=False).serve_commit_paged(*(tensors[k] for k in pg.NAMES), 4, 0)
    assert recorder.calls == []
    tensors = sc.upload(hip, state)
    t_nxt = hip.from_numpy(nxt.copy(), requires_grad=False)
    g = {k: t.ptr for k, t in tensors.items()}
    N, P, G = state["prompts"].shape[0], state["prompts"].shape[1], state["out"].shape[1]
    good = dict(nxt=t_nxt.ptr, np_=1, prompts=g["prompts"], pp=P, P=P, plen=g["prompt_len"], budget=g["budget"], out=g["out"], op=G, G=G,
                out_len=g["out_len"], queue=g["queue"], N=N, req=g["req"], pos=g["pos"], count=g["count"], ids=g["ids"], position_ids=g["position_ids"],
                last=g["last"], block_table=g["block_table"], held=g["held"], free=g["free"], slots=3, m=4, max_blocks=6, num_blocks=len(state["free"]) - 1,
                log2_block=2, prefix_blocks=0, eos=-1)
    handle = recorder._handle
    entry = lambda **o: handle.lg_serve_commit_paged_i32(*dict(good, **o).values())             # noqa: E731
    for override, word in ((dict(free=None), b"NULL"), (dict(held=g["pos"]), b"overlap"), (dict(free=g["block_table"] + 4), b"overlap"), (dict(block_table=g["ids"]), b"overlap"),
                           (dict(op=G - 1), b"pitch"), (dict(held=g["held"] + 2), b"aligned"), (dict(slots=1025), b"unsupported"), (dict(log2_block=1), b"unsupported"),
                           (dict(max_blocks=129), b"unsupported"), (dict(prefix_blocks=7), b"unsupported"), (dict(num_blocks=0), b"unsupported")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_serve_commit_paged_i32" in handle.lg_last_error(), override
    assert entry(slots=0) == 0
    HipDevice.synchronize()
    for name in pg.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), state[name], err_msg=name)
    assert entry() == 0
    HipDevice.synchronize()
    want, _ = pg.commit_by_hand(state, nxt, 4, 0, None)
    for name in pg.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)


# ---- one model step against a paged cache ---------------------------------------------------------------------------------------

def test_one_paged_step_on_hip_matches_each_sequence_alone(hip, recorder):
    ref64, cpu32 = sc.mixed_reference()
    got, cache = pg.mixed_step(hip)
    assert_as_close_to_float64_as_the_cpu_backend(sc.named(got), sc.named(cpu32), sc.named(ref64), floor=1e-5, what="paged step on HipTensor")
    assert set(recorder.attention()) == {"lg_attention_extend_paged_f32"} and len(recorder.attention()) == 2 * 4
    np.testing.assert_array_equal(cache.pos.numpy(), [t for t, _ in sc.MIXED])          # the caller moves the positions, not the forward


# ---- serve over a paged cache ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=sc.SEED)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
@pytest.mark.parametrize("pool", ["generous", "tight"])
def test_paged_serve_on_hip_gives_each_request_its_own_continuation(hip, model, slots, chunk, pool, captured):
    for prefix in (0, pg.PREFIX):
        rows = pg.prefixed_prompts() if prefix else sc.prompts()
        tokens = pg.assert_prefixed_margins_rule_out_ties() if prefix else sc.assert_margins_rule_out_ties()
        want, want_len = sc.expected(tokens, sc.BUDGET, sc.EOS)
        F = 2 if prefix else 0
        num_blocks = F + slots * pg.MAX_BLOCKS if pool == "generous" else pg.tight_blocks(rows, sc.BUDGET, F)
        graph = HipGraph() if captured else None
        out, out_len, stats, cache = pg.run_serve(hip, slots, chunk, num_blocks, model=model, rows=rows, poll=1, graph=graph, shared_prefix=prefix)
        np.testing.assert_array_equal(out_len, want_len)
        np.testing.assert_array_equal(out, want)
        lengths = [len(p) for p in rows]
        assert stats["prefix_blocks"] == F and stats["steps"] == pg.simulate(lengths, want_len, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, num_blocks, F)
        pg.assert_no_block_leaked(cache, F)
        if captured:
            assert graph.kernel_count() > 0
            graph.destroy()


def test_the_host_reads_the_poll_word_only_and_the_paged_step_has_the_launches_of_the_counted_step(hip, model, recorder):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)

    def steps_of(commit, cache):
        del recorder.calls[:], recorder.reads[:]
        (out, out_len), stats = dc.bert.serve(model, sc.prompts(), sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4)
        steps = stats["steps"]
        assert steps % 4 == 0 and recorder.reads == [4] * (steps // 4)    # one int32 word per poll, nothing else
        calls = [c for c in recorder.calls if c != "lg_sync"]
        np.testing.assert_array_equal(out.numpy(), want)
        per_step, step = [], []
        for name in calls:
            step.append(name)
            if name == commit:
                per_step.append(step)
                step = []
        assert step == [] and len(per_step) == steps + 1                  # the admission commit, then a commit at the end of every step
        assert all(s == per_step[1] for s in per_step[2:]), "a step's launches depend on what the slots hold"
        return per_step[1]

    like = model.cls.predictions.bias
    paged_cache = nn.PagedKVCache(sc.CFG["num_hidden_layers"], 3, 12, pg.BLOCK, sc.CFG["hidden_size"], pg.MAX_BLOCKS, like=like)
    plain_cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=like, per_row=True)
    paged_step = steps_of("lg_serve_commit_paged_i32", paged_cache)
    pg.assert_no_block_leaked(paged_cache)
    counted_step = steps_of("lg_serve_commit_i32", plain_cache)
    assert paged_step.count("lg_attention_extend_paged_f32") == sc.CFG["num_hidden_layers"]
    renamed = [{"lg_attention_extend_paged_f32": "lg_attention_extend_counts_f32", "lg_serve_commit_paged_i32": "lg_serve_commit_i32"}.get(c, c) for c in paged_step]
    assert renamed == counted_step and not any("decode" in c for c in paged_step)
    print("launch entries of one paged serving step: %d, of the counted step: %d" % (len(paged_step), len(counted_step)))
