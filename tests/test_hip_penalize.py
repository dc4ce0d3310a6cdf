"""lg_penalize_rows_f32 (csrc/penalize.hip) behind `HipTensor.penalize_rows`, and per-request penalties through
examples/bert.py's `serve(repetition_penalty=, presence_penalty=, frequency_penalty=, min_new_tokens=)`.

The launch restates the float32 definition (`random.penalize_logits`) operation for operation - one product or one correctly
rounded division, one product and two subtractions, nothing fused - so its results are the definition's BIT FOR BIT: compared as
uint32 words wherever the value is no NaN, a NaN for a NaN.  `serve` is held against the float64 run of every request ALONE
through the definition with its own history (tests/penalty_cases.py), whose near-ties are ruled out from the references alone."""
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from lightgrad_amd.autograd.hip import lib as hiplib
from test_hip_serve import recorder                                       # noqa: F401 (a fixture)
from test_hip_sample_rows import steps_of
import decode_cases as dc
import paged_bf16_cases as pb
import paged_cases as pg
import penalty_cases as pc
import serve_cases as sc
import serve_packed_cases as spc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
NAMES = ("table", "index", "prompts", "prompt_len", "out", "out_len")


def up(hip, a, dtype=None):
    return hip.from_numpy(np.ascontiguousarray(a, dtype), requires_grad=False)


def operands(hip, case):
    return [up(hip, case[k]) for k in NAMES]


# ---- bit for bit against the definition -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eos", [None, pc.NINE_EOS])
def test_nine_rows_bitwise(hip, eos):
    case = pc.nine_rows()
    want, bad = lg_random.penalize_logits(**case, eos=eos)
    assert bad.tolist() == pc.NINE_BAD
    logits = up(hip, case["logits"])
    assert logits.penalize_rows(*operands(hip, case), eos=eos) is logits
    with pytest.raises(IndexError):
        HipDevice.synchronize()                                           # the row beyond the table raised the flag ...
    HipDevice.synchronize()
    assert pc.same_bits(logits.numpy(), want)                             # ... kept its bytes, and every other row was computed


def test_nine_rows_of_a_wide_vocabulary_bitwise(hip):
    """V = 30522: the launch touches the ids of the history alone, whatever the width"""
    width = 30522
    case = pc.changed(pc.nine_rows(), {})
    rng = np.random.RandomState(8)
    wide = (3 * rng.standard_normal((9, width))).astype(np.float32)
    wide[:, :pc.V] = case["logits"]
    case["logits"] = wide
    case["prompts"][4, 0], case["out"][4, 0] = width - 1, width - 2      # request 4 (row 8): the last ids of the vocabulary
    want, bad = lg_random.penalize_logits(**case, eos=width - 3)
    assert bad.tolist() == pc.NINE_BAD and want[8, width - 3] == -np.inf and want[8, width - 1] == wide[8, width - 1]        # (rho = 1)
    logits = up(hip, wide).penalize_rows(*operands(hip, case), eos=width - 3)
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    assert pc.same_bits(logits.numpy(), want)


@pytest.mark.parametrize("L", pc.EDGES)
def test_every_history_length_bitwise(hip, L):
    case = pc.edge(L)
    want, bad = lg_random.penalize_logits(**case, eos=2)
    assert not bad.any()
    logits = up(hip, case["logits"]).penalize_rows(*operands(hip, case), eos=2)
    HipDevice.synchronize()
    assert pc.same_bits(logits.numpy(), want)


def test_rows_of_a_wider_tensor_and_a_middle_axis(hip):
    case = pc.changed(pc.nine_rows(), dict(index=(6, 2)))                 # no bad row
    want, _ = lg_random.penalize_logits(**case, eos=pc.NINE_EOS)
    wide = np.full((9, pc.V + 6), -7.0, np.float32)
    wide[:, 3:3 + pc.V] = case["logits"]
    t = up(hip, wide)
    from lightgrad_amd.autograd.hip.ops import _idx_view
    view = _idx_view(t, (slice(None), slice(3, 3 + pc.V)))                # rows off 16 bytes, a pitch of its own
    with light.no_grad():                                                 # (a view asks for a gradient like any new tensor)
        assert view.penalize_rows(*operands(hip, case), eos=pc.NINE_EOS) is view
    got = t.numpy()
    assert pc.same_bits(got[:, 3:3 + pc.V], want) and (got[:, :3] == -7).all() and (got[:, 3 + pc.V:] == -7).all()
    # (rows, 1, V)
    logits = up(hip, case["logits"].reshape(9, 1, pc.V))
    assert logits.penalize_rows(*operands(hip, case), eos=pc.NINE_EOS) is logits
    assert pc.same_bits(logits.numpy().reshape(9, pc.V), want)
    HipDevice.synchronize()
    # a layout the launch cannot address is an error, never a copy; so is a tensor that asks for a gradient
    with pytest.raises(AssertionError, match="contiguous"), light.no_grad():
        _idx_view(t, (slice(None), slice(0, 100, 2))).penalize_rows(*operands(hip, case))
    with pytest.raises(AssertionError, match="gradient"):
        hip.from_numpy(case["logits"], requires_grad=True).penalize_rows(*operands(hip, case))
    with pytest.raises(TypeError):
        up(hip, np.zeros((9, pc.V), np.float64)).penalize_rows(*operands(hip, case))


@pytest.mark.parametrize("rho", [0.8, 1.3, 1.5])
def test_2000_values_around_zero_bitwise(hip, rho):
    """pins the division (correctly rounded) and the missing fusion of x - beta * c: one row, every id once in the prompt, every
    second one also among the tokens, some of them twice"""
    width = 2000
    rng = np.random.RandomState(int(rho * 10))
    x = (rng.standard_normal((1, width)) * 10.0 ** rng.uniform(-6, 2, (1, width))).astype(np.float32)
    x[0, :8] = [0.0, -0.0, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38, 3.4e38, -3.4e38]          # zeros, subnormals, the smallest normal, near the largest
    tokens = np.r_[np.arange(0, width, 2), np.arange(0, width, 6)].astype(np.int32)
    case = dict(logits=x, table=lg_random.penalty_table(rho, 0.3, 0.7), index=np.array([0], np.int32), prompts=np.arange(width, dtype=np.int32)[None, :],
                prompt_len=np.array([width], np.int32), out=tokens[None, :], out_len=np.array([tokens.size], np.int32))
    want, _ = lg_random.penalize_logits(**case)
    assert (want != x).sum() >= width - 2
    logits = up(hip, x).penalize_rows(*operands(hip, case))
    HipDevice.synchronize()
    assert pc.same_bits(logits.numpy(), want)


@pytest.mark.parametrize("what", sorted(pc.bad_causes()))
def test_a_bad_row_raises_the_flag_keeps_its_bytes_and_the_others_are_right(hip, what):
    good = pc.nine_rows()
    case = pc.changed(good, dict(pc.bad_causes()[what], index=(6, 2)))    # row 4 is the only bad one
    want, bad = lg_random.penalize_logits(**case, eos=pc.NINE_EOS)
    assert bad.tolist() == [r == 4 for r in range(9)] and pc.same_bits(want[4], good["logits"][4])
    logits = up(hip, case["logits"]).penalize_rows(*operands(hip, case), eos=pc.NINE_EOS)
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    assert pc.same_bits(logits.numpy(), want)


def test_the_c_abi_refuses_bad_arguments_before_anything_is_launched(hip):
    lib = hiplib.lib()
    case = pc.changed(pc.nine_rows(), dict(index=(6, 2)))
    x = up(hip, case["logits"])
    t = dict(zip(NAMES, operands(hip, case)))
    P, G = case["prompts"].shape[1], case["out"].shape[1]
    good = dict(logits=x.ptr, rows=9, cols=pc.V, row_pitch=pc.V, table=t["table"].ptr, n=5, index=t["index"].ptr, prompts=t["prompts"].ptr, prompt_pitch=P, P=P,
                prompt_len=t["prompt_len"].ptr, out=t["out"].ptr, out_pitch=G, G=G, out_len=t["out_len"].ptr, eos=pc.NINE_EOS)
    big = up(hip, np.zeros(5 * 4200, np.int32))

    def call(**change):
        return lib.lg_penalize_rows_f32(*dict(good, **change).values())
    refused = [dict(logits=None), dict(table=None), dict(index=None), dict(prompts=None), dict(prompt_len=None), dict(out=None), dict(out_len=None),
               dict(logits=x.ptr + 2), dict(table=t["table"].ptr + 4), dict(table=t["table"].ptr + 8), dict(index=t["index"].ptr + 1),
               dict(prompts=t["prompts"].ptr + 2), dict(prompt_len=t["prompt_len"].ptr + 1), dict(out=t["out"].ptr + 3), dict(out_len=t["out_len"].ptr + 2),
               dict(rows=-1), dict(rows=65536), dict(cols=0), dict(cols=1 << 31, row_pitch=1 << 31), dict(row_pitch=pc.V - 1), dict(n=0), dict(n=-3),
               dict(P=0), dict(G=0), dict(P=-1), dict(prompt_pitch=P - 1), dict(out_pitch=G - 1),
               dict(prompts=big.ptr, P=4000, prompt_pitch=4000, G=97, out_pitch=97), dict(prompts=big.ptr, P=4096 - G + 1, prompt_pitch=4200),
               dict(eos=pc.V), dict(eos=-2), dict(eos=1 << 30),
               dict(table=x.ptr), dict(index=x.ptr + 4 * (9 * pc.V - 1)), dict(prompts=x.ptr + 4 * pc.V), dict(prompt_len=x.ptr),
               dict(out=x.ptr + 4 * 9 * pc.V - 4), dict(out_len=x.ptr + 400)]
    for change in refused:
        assert call(**change) == LG_EINVAL and b"lg_penalize_rows_f32" in lib.lg_last_error(), change
    assert call(prompts=big.ptr, P=4000, prompt_pitch=4000, G=97, out_pitch=97) == LG_EINVAL and b"4000 + 97" in lib.lg_last_error()
    HipDevice.synchronize()
    assert pc.same_bits(x.numpy(), case["logits"]), "a refused call wrote logits"
    assert call(rows=0, logits=None, cols=0) == 0                         # no rows: LG_OK before anything else
    assert pc.same_bits(x.numpy(), case["logits"])
    assert call() == 0
    HipDevice.synchronize()
    assert pc.same_bits(x.numpy(), lg_random.penalize_logits(**case, eos=pc.NINE_EOS)[0])
    # through the op: the history bound as an assertion with the numbers, other operands by name
    fresh = up(hip, case["logits"])
    with pytest.raises(AssertionError, match=r"4000 \+ 97"):
        fresh.penalize_rows(**dict(t, prompts=up(hip, np.zeros((5, 4000), np.int32)), out=up(hip, np.zeros((5, 97), np.int32))))
    for bad in (dict(table=up(hip, np.zeros((5, 8), np.int32))), dict(index=up(hip, np.zeros(8, np.int32))), dict(out_len=up(hip, np.zeros(5, np.int64))),
                dict(eos=pc.V), dict(eos=-1)):
        with pytest.raises(ValueError):
            fresh.penalize_rows(**dict(t, **bad))
    assert pc.same_bits(fresh.numpy(), case["logits"])


# ---- serve ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=sc.SEED)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_on_hip_gives_each_request_the_tokens_of_its_run_alone(hip, model, slots, chunk, mode, captured):
    want, want_len = pc.expected(mode)
    graph = HipGraph() if captured else None
    out, out_len, stats = sc.run_serve(hip, slots, chunk, model=model, poll=1, graph=graph, **pc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["penalties"] is True and stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], want_len, slots, chunk)
    if captured:
        assert graph.kernel_count() > 0
        graph.destroy()


@pytest.mark.parametrize("mode", pc.MODES)
def test_serve_on_hip_token_packed_and_paged(hip, model, mode):
    want, want_len = pc.expected(mode)
    lengths = [len(p) for p in sc.prompts()]
    out, out_len, stats = sc.run_serve(hip, 3, 4, model=model, poll=1, token_budget=6, **pc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["penalties"] is True and stats["steps"] == spc.simulate_packed(lengths, want_len, 3, 4, 6)
    if mode == "greedy":                                                  # the prefixed prompts behind their shared prefix (penalty_cases.reference)
        want, want_len = pc.expected("greedy", True)
        out, out_len, stats, cache = pg.run_serve(hip, 3, 4, 2 + 3 * pg.MAX_BLOCKS, model=model, poll=1, rows=pg.prefixed_prompts(),
                                                  **pc.options(mode, shared_prefix=pg.PREFIX))
        assert stats["prefix_blocks"] == 2
        pg.assert_no_block_leaked(cache, 2)
    else:
        out, out_len, stats, cache = pg.run_serve(hip, 3, 4, 3 * pg.MAX_BLOCKS, model=model, poll=1, **pc.options(mode))
        pg.assert_no_block_leaked(cache)
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["penalties"] is True


def test_the_bf16_paged_route_agrees_with_the_numpy_backend_schedule_for_schedule(hip, model):
    """its logits are the rounded model's: no reference equality, but the tokens of CpuTensor's run of the same schedule"""
    runs = [pb.run_serve(T, 3, 4, 3 * pg.MAX_BLOCKS, model=m, rows=sc.prompts(), poll=1, **pc.options("sampled")) for T, m in ((hip, model), (CpuTensor, None))]
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert runs[0][2]["steps"] == runs[1][2]["steps"] and runs[0][2]["penalties"] is True


def test_kernel_counts_of_the_captured_step_and_the_host_reads_the_poll_word_only(hip, model, recorder):
    def serve(graph=None, **options):
        cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
        del recorder.calls[:], recorder.reads[:]
        (out, _), stats = dc.bert.serve(model, sc.prompts(), sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4,
                                        graph=graph, **options)
        return out, stats, list(recorder.calls), list(recorder.reads)
    neutral = dict(repetition_penalty=1.0, presence_penalty=[0.0] * 7, frequency_penalty=0.0, min_new_tokens=0)
    for mode, entry in (("greedy", None), ("sampled", "lg_sample_rows_f32")):
        base = pc.options(mode)
        for k in pc.keywords():
            del base[k]
        out, stats, calls, reads = serve(**pc.options(mode))
        assert stats["steps"] % 4 == 0 and reads == [4] * (stats["steps"] // 4)          # one int32 word per poll, nothing else
        np.testing.assert_array_equal(out.numpy(), pc.expected(mode)[0])
        new = steps_of(calls)
        assert all(s == new[1] for s in new[2:]), "a step's launches depend on what the slots hold"
        plain, with_neutral = steps_of(serve(**base)[2]), steps_of(serve(**base, **neutral)[2])
        assert plain[1] == with_neutral[1] and "lg_penalize_rows_f32" not in plain[1]
        at = new[1].index("lg_penalize_rows_f32")
        assert new[1][:at] + new[1][at + 1:] == plain[1] and new[1].count("lg_penalize_rows_f32") == 1
        print("%s: the step behind its head: %s" % (mode, new[1][at - 1:]))
        assert new[1][-1] == "lg_serve_commit_i32" and (entry is None or new[1][at + 1] == entry)                 # in front of the draw
        graphs = [HipGraph() for _ in range(3)]
        stats = [serve(graph=g, **o)[1] for g, o in zip(graphs, (base, dict(base, **neutral), pc.options(mode)))]
        counts = [g.kernel_count() for g in graphs]
        print("%s: kernels of the captured step %d, with neutral keywords %d, with penalties %d" % (mode, *counts))
        assert counts[0] == counts[1] and counts[2] == counts[0] + 1
        assert "penalties" not in stats[0] and "penalties" not in stats[1] and stats[2]["penalties"] is True
        for g in graphs:
            g.destroy()
