"""lg_guide_rows_f32 (csrc/guide.hip) behind `HipTensor.guide_rows`, and guided decoding through examples/bert.py's
`serve(guide=)`.

The launch restates the definition (`guide.guide_logits`) and is store-only - -inf where the state's bit is clear, +0.0 at a forced
id, no logit read - so its results are the definition's BIT FOR BIT as uint32 words, NaN payloads and the sign of zero included,
with the state pairs equal, whatever the grid.  `serve` is held against the float64 run of every request ALONE through the
definition in the state its own automaton reaches (tests/guide_cases.py), whose near-ties are ruled out from the references
alone."""
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd import guide as lg_guide
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from lightgrad_amd.autograd.hip import lib as hiplib
from test_hip_serve import recorder                                       # noqa: F401 (a fixture)
from test_hip_sample_rows import steps_of
import decode_cases as dc
import guide_cases as gc
import paged_bf16_cases as pb
import paged_cases as pg
import serve_cases as sc
import serve_packed_cases as spc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1


def up(hip, a, dtype=None):
    return hip.from_numpy(np.ascontiguousarray(a, dtype), requires_grad=False)


def operands(hip, case):
    return [up(hip, case[k]) for k in gc.NAMES]


@pytest.fixture
def slices():
    """sets the slices of a row for the launches of a test, and the automatic grid back afterwards"""
    lib = hiplib.lib()
    yield lib.lg_guide_rows_slices
    lib.lg_guide_rows_slices(0)


# ---- bit for bit against the definition -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [0, 1, 3], ids=["auto", "a workgroup per row", "three slices"])
@pytest.mark.parametrize("V", gc.WIDTHS)
def test_every_kernel_case_bitwise(hip, slices, V, grid):
    case = gc.kernel_case(V)
    want, want_state, bad = lg_guide.guide_logits(**gc.operands(case))
    assert not bad.any() and want_state[:, 0].tolist() == case["reached"].tolist()
    slices(grid)
    logits, t = up(hip, case["logits"]), operands(hip, case)
    assert logits.guide_rows(*t) is logits
    HipDevice.synchronize()
    assert gc.same_words(logits.numpy(), want) and t[-1].numpy().tolist() == want_state.tolist()
    logits.guide_rows(*t)                                                 # a second call on the result changes nothing
    HipDevice.synchronize()
    assert gc.same_words(logits.numpy(), want) and t[-1].numpy().tolist() == want_state.tolist()


@pytest.mark.parametrize("V", [101, 30522])
def test_nine_rows_bitwise(hip, V):
    case = gc.nine_rows(V)
    want, want_state, bad = lg_guide.guide_logits(**gc.operands(case))
    assert bad.tolist() == gc.NINE_BAD
    logits, t = up(hip, case["logits"]), operands(hip, case)
    assert logits.guide_rows(*t) is logits
    with pytest.raises(IndexError):
        HipDevice.synchronize()                                           # the row beyond the table raised the flag ...
    HipDevice.synchronize()
    assert gc.same_words(logits.numpy(), want) and t[-1].numpy().tolist() == want_state.tolist()        # ... and every other row was computed


@pytest.mark.parametrize("grid", [0, 1, 5])
@pytest.mark.parametrize("V,offset", [(101, 3), (101, 1), (101, 2), (30522, 3), (1027, 1)])
def test_rows_of_a_wider_tensor_off_16_bytes(hip, slices, V, offset, grid):
    """rows that start 4, 8 or 12 bytes off a 16-byte address, a pitch of their own (V = 30522 with a pitch of V + 6 moves the
    offset from row to row): the same path, the bytes around the rows untouched"""
    case = gc.kernel_case(V)
    want, want_state, _ = lg_guide.guide_logits(**gc.operands(case))
    rows = want.shape[0]
    wide = np.full((rows, V + 6), -7.0, np.float32)
    wide[:, offset:offset + V] = case["logits"]
    t = up(hip, wide)
    from lightgrad_amd.autograd.hip.ops import _idx_view
    view = _idx_view(t, (slice(None), slice(offset, offset + V)))
    slices(grid)
    ops = operands(hip, case)
    with light.no_grad():                                                 # (a view asks for a gradient like any new tensor)
        assert view.guide_rows(*ops) is view
    HipDevice.synchronize()
    got = t.numpy()
    assert gc.same_words(got[:, offset:offset + V], want) and (got[:, :offset] == -7).all() and (got[:, offset + V:] == -7).all()
    assert ops[-1].numpy().tolist() == want_state.tolist()


def test_a_middle_axis_and_the_layouts_and_dtypes_that_are_refused(hip):
    case = gc.changed(gc.nine_rows(), dict(index=(6, gc.SPARE_REQUEST)))  # no bad row
    want, want_state, _ = lg_guide.guide_logits(**gc.operands(case))
    V = want.shape[1]
    logits, t = up(hip, case["logits"].reshape(9, 1, V)), operands(hip, case)
    assert logits.guide_rows(*t) is logits
    HipDevice.synchronize()
    assert gc.same_words(logits.numpy().reshape(9, V), want) and t[-1].numpy().tolist() == want_state.tolist()
    # a layout the launch cannot address is an error, never a copy; so is a tensor that asks for a gradient, and float64
    from lightgrad_amd.autograd.hip.ops import _idx_view
    wide, t = up(hip, np.zeros((9, 2 * V), np.float32)), operands(hip, case)
    with pytest.raises(AssertionError, match="contiguous"), light.no_grad():
        _idx_view(wide, (slice(None), slice(0, 2 * V, 2))).guide_rows(*t)
    with pytest.raises(AssertionError, match="gradient"):
        hip.from_numpy(case["logits"], requires_grad=True).guide_rows(*t)
    with pytest.raises(TypeError):
        up(hip, np.zeros((9, V), np.float64)).guide_rows(*t)
    for bad in (dict(allow=up(hip, case["allow"][:, :3])), dict(states=up(hip, case["states"][:, :3])), dict(index=up(hip, case["index"][:8])),
                dict(out_len=up(hip, case["out_len"], np.int64)), dict(state=up(hip, case["state"][:7]))):
        with pytest.raises(ValueError):
            up(hip, case["logits"]).guide_rows(**dict(dict(zip(gc.NAMES, t)), **bad))
    HipDevice.synchronize()
    assert t[-1].numpy().tolist() == case["state"].tolist()


@pytest.mark.parametrize("what", sorted(gc.bad_causes()))
def test_a_bad_row_raises_the_flag_keeps_its_bytes_and_its_state_and_the_others_are_right(hip, what):
    good = gc.changed(gc.nine_rows(), dict(index=(6, gc.SPARE_REQUEST)))
    case = gc.changed(good, gc.bad_causes()[what])                        # row 4 is the only bad one
    want, want_state, bad = lg_guide.guide_logits(**gc.operands(case))
    assert bad.tolist() == [r == gc.BAD_ROW for r in range(9)] and gc.same_words(want[gc.BAD_ROW], good["logits"][gc.BAD_ROW])
    assert want_state[gc.BAD_REQUEST].tolist() == case["state"][gc.BAD_REQUEST].tolist()
    logits, t = up(hip, case["logits"]), operands(hip, case)
    logits.guide_rows(*t)
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    assert gc.same_words(logits.numpy(), want) and t[-1].numpy().tolist() == want_state.tolist()


def test_the_c_abi_refuses_bad_arguments_before_anything_is_launched(hip):
    lib = hiplib.lib()
    case = gc.changed(gc.nine_rows(), dict(index=(6, gc.SPARE_REQUEST)))
    V = case["logits"].shape[1]
    x = up(hip, case["logits"])
    t = dict(zip(gc.NAMES, operands(hip, case)))
    S, E, (N, G) = case["states"].shape[0], case["edges"].shape[0], case["out"].shape
    good = dict(logits=x.ptr, rows=9, cols=V, row_pitch=V, allow=t["allow"].ptr, states=t["states"].ptr, S=S, edges=t["edges"].ptr, E=E, index=t["index"].ptr,
                out=t["out"].ptr, out_pitch=G, G=G, out_len=t["out_len"].ptr, state=t["state"].ptr, N=N)

    def call(**change):
        return lib.lg_guide_rows_f32(*dict(good, **change).values())
    last = x.ptr + 4 * (9 * V - 1)
    refused = [dict(logits=None), dict(allow=None), dict(states=None), dict(edges=None), dict(index=None), dict(out=None), dict(out_len=None), dict(state=None),
               dict(logits=x.ptr + 2), dict(allow=t["allow"].ptr + 2), dict(states=t["states"].ptr + 4), dict(states=t["states"].ptr + 8),
               dict(edges=t["edges"].ptr + 1), dict(index=t["index"].ptr + 1), dict(out=t["out"].ptr + 3), dict(out_len=t["out_len"].ptr + 2),
               dict(state=t["state"].ptr + 4), dict(state=t["state"].ptr + 2),
               dict(rows=-1), dict(rows=65536), dict(cols=0), dict(cols=1 << 31, row_pitch=1 << 31), dict(row_pitch=V - 1),
               dict(S=0), dict(S=-2), dict(E=0), dict(E=-1), dict(N=0), dict(N=-3), dict(G=0), dict(G=-1), dict(out_pitch=G - 1),
               # the logits overlap a table
               dict(allow=x.ptr), dict(states=x.ptr + 16), dict(edges=last - 4), dict(index=last), dict(out=x.ptr + 4 * V), dict(out_len=x.ptr + 400),
               dict(state=x.ptr + 8),
               # state overlaps another operand
               dict(state=t["allow"].ptr), dict(state=t["states"].ptr + 8), dict(state=t["edges"].ptr), dict(state=t["index"].ptr), dict(state=t["out"].ptr + 8),
               dict(state=t["out_len"].ptr)]
    for change in refused:
        assert call(**change) == LG_EINVAL and b"lg_guide_rows_f32" in lib.lg_last_error(), change
    HipDevice.synchronize()
    assert gc.same_words(x.numpy(), case["logits"]) and t["state"].numpy().tolist() == case["state"].tolist(), "a refused call wrote"
    assert call(rows=0, logits=None, cols=0, state=None) == 0             # no rows: LG_OK before anything else
    assert gc.same_words(x.numpy(), case["logits"])
    assert call() == 0
    HipDevice.synchronize()
    want, want_state, _ = lg_guide.guide_logits(**gc.operands(case))
    assert gc.same_words(x.numpy(), want) and t["state"].numpy().tolist() == want_state.tolist()


# ---- serve ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=sc.SEED)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_on_hip_gives_each_request_the_tokens_of_its_run_alone(hip, model, slots, chunk, mode, captured):
    want, want_len = gc.expected(mode)
    graph = HipGraph() if captured else None
    out, out_len, stats = sc.run_serve(hip, slots, chunk, model=model, poll=1, graph=graph, **gc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    gc.assert_consequences(mode, out, out_len)
    assert stats["guide"] is True and stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], want_len, slots, chunk)
    if captured:
        assert graph.kernel_count() > 0
        graph.destroy()


@pytest.mark.parametrize("mode", gc.MODES)
def test_serve_on_hip_token_packed_and_paged(hip, model, mode):
    want, want_len = gc.expected(mode)
    lengths = [len(p) for p in sc.prompts()]
    out, out_len, stats = sc.run_serve(hip, 3, 4, model=model, poll=1, token_budget=6, **gc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["guide"] is True and stats["steps"] == spc.simulate_packed(lengths, want_len, 3, 4, 6)
    if mode == "greedy":                                                  # the prefixed prompts behind their shared prefix (guide_cases.reference)
        want, want_len = gc.expected("greedy", True)
        out, out_len, stats, cache = pg.run_serve(hip, 3, 4, 2 + 3 * pg.MAX_BLOCKS, model=model, poll=1, rows=pg.prefixed_prompts(),
                                                  **gc.options(mode, shared_prefix=pg.PREFIX))
        assert stats["prefix_blocks"] == 2
        pg.assert_no_block_leaked(cache, 2)
    else:
        out, out_len, stats, cache = pg.run_serve(hip, 3, 4, 3 * pg.MAX_BLOCKS, model=model, poll=1, **gc.options(mode))
        pg.assert_no_block_leaked(cache)
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    gc.assert_consequences(mode, out, out_len)
    assert stats["guide"] is True


def test_the_bf16_paged_route_agrees_with_the_numpy_backend_schedule_for_schedule(hip, model):
    """its logits are the rounded model's: no reference equality, but the tokens of CpuTensor's run of the same schedule"""
    runs = [pb.run_serve(T, 3, 4, 3 * pg.MAX_BLOCKS, model=m, rows=sc.prompts(), poll=1, **gc.options("sampled")) for T, m in ((hip, model), (CpuTensor, None))]
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    gc.assert_consequences("sampled", runs[0][0], runs[0][1])
    assert runs[0][2]["steps"] == runs[1][2]["steps"] and runs[0][2]["guide"] is True


def test_kernel_counts_of_the_captured_step_and_the_host_reads_the_poll_word_only(hip, model, recorder):
    def serve(graph=None, **options):
        cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
        del recorder.calls[:], recorder.reads[:]
        (out, _), stats = dc.bert.serve(model, sc.prompts(), sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4,
                                        graph=graph, **options)
        return out, stats, list(recorder.calls), list(recorder.reads)
    for mode, entry in (("greedy", None), ("sampled", "lg_sample_rows_f32"), (gc.COMBINED, "lg_sample_rows_f32")):
        full = gc.options(mode)
        base = {k: v for k, v in full.items() if k != "guide"}
        out, stats, calls, reads = serve(**full)
        assert stats["steps"] % 4 == 0 and reads == [4] * (stats["steps"] // 4)          # one int32 word per poll, nothing else
        np.testing.assert_array_equal(out.numpy(), gc.expected(mode)[0])
        new = steps_of(calls)
        assert all(s == new[1] for s in new[2:]), "a step's launches depend on what the slots hold"
        plain, with_none = steps_of(serve(**base)[2]), steps_of(serve(**base, guide=[None] * 7)[2])
        assert plain[1] == with_none[1] and "lg_guide_rows_f32" not in plain[1]           # guide=None: launch for launch the old step
        at = new[1].index("lg_guide_rows_f32")
        assert new[1][:at] + new[1][at + 1:] == plain[1] and new[1].count("lg_guide_rows_f32") == 1
        print("%s: the step behind its head: %s" % (mode, new[1][at - 1:]))
        assert new[1][-1] == "lg_serve_commit_i32" and (entry is None or new[1][at + 1] == entry)                 # in front of the draw
        assert mode != gc.COMBINED or new[1][at - 1] == "lg_penalize_rows_f32"                                    # behind the penalties
        graphs = [HipGraph() for _ in range(3)]
        stats = [serve(graph=g, **o)[1] for g, o in zip(graphs, (base, dict(base, guide=None), full))]
        counts = [g.kernel_count() for g in graphs]
        print("%s: kernels of the captured step %d, with guide=None %d, with guides %d" % (mode, *counts))
        assert counts[0] == counts[1] and counts[2] == counts[0] + 1
        assert "guide" not in stats[0] and "guide" not in stats[1] and stats[2]["guide"] is True
        for g in graphs:
            g.destroy()
