"""Incremental decoding of the causal model without a device: the nn.KVCache, the cached forward of examples/bert.py on
CpuTensor (the composite over `cache[:, :length + 1]`, the only form the CPU backend and float64 tapes have), `generate`, the
host half of the decode entry of the C ABI, and the resources of the decode kernels.

The yardstick is the project's own (tests/common.py): a float32 result is judged by its distance to the SAME tape code run in
float64 - here full causal forwards over each prefix - and may be no further from it than twice the float32 full forward
("cpu32") is, with a floor of 1e-5.  hipcc cross-compiles without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.hip import lib as hiplib
from conftest import ROOT
from common import assert_as_close_to_float64_as_the_cpu_backend
import decode_cases as dc

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")
LG_ENOTINIT = -4


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "prompt-mask"])
def test_teacher_forced_logits_match_the_full_forward(masked):
    """a prompt of 5 tokens, then 10 given tokens one at a time through the cache: the logits of every step against the rows of
    a float64 full causal forward over the same prefix"""
    ref64, cpu32 = dc.teacher_reference(masked)
    got = dc.teacher_forced(CpuTensor, masked)
    assert sorted(got) == sorted(ref64) and len(got) == 1 + dc.NEW
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, floor=1e-5, what="cached forward on CpuTensor")


def test_teacher_forced_in_float64_is_the_full_forward():
    """the composite on a float64 tape (the other backend without a decode op): the cache changes the order of no sum by more
    than float64 rounding"""
    ref64, _ = dc.teacher_reference(True)
    from common import float64_tape, rel_frobenius
    with float64_tape():
        got = dc.teacher_forced(CpuTensor, True, model=dc.make_model(CpuTensor, np.float64), dtype=np.float64)
    for name in ref64:
        assert got[name].dtype == np.float64 and rel_frobenius(got[name], ref64[name]) < 1e-13, name


def test_generate_equals_a_full_recompute_per_token_in_float64():
    """greedy tokens, every step.  First, on the float64 reference alone: the top-2 logit margin of every step is at least 100
    times the largest deviation of the float32 full forward from the float64 one, so no step is a near-tie that could hide or
    fake a failure - the seed of tests/decode_cases.py was picked for that, no step is left out"""
    want = dc.assert_margins_rule_out_ties()
    assert want.shape == (dc.B, dc.NEW)
    np.testing.assert_array_equal(dc.greedy(CpuTensor), want)


def test_generate_with_a_prompt_mask_and_one_new_token():
    """a key-padding mask over the prompt reaches the prefill and (extended with ones) every decode step; max_new_tokens = 1
    is the prefill alone"""
    _, ids = dc.parameters()
    model64 = dc.make_model(CpuTensor, np.float64)
    seq = ids[:, :dc.S0].copy()
    for _ in range(3):
        last = dc.full_logits(model64, seq, dc.prefix_mask(seq.shape[1]))[:, -1]
        seq = np.concatenate([seq, last.argmax(-1).astype(np.int32)[:, None]], axis=1)
    mask = CpuTensor.from_numpy(dc.PROMPT_MASK, requires_grad=False)
    np.testing.assert_array_equal(dc.greedy(CpuTensor, new=3, attention_mask=mask), seq[:, dc.S0:])
    np.testing.assert_array_equal(dc.greedy(CpuTensor, new=1, attention_mask=mask), seq[:, dc.S0:dc.S0 + 1])


def test_kv_cache_position_and_capacity():
    like = CpuTensor.from_numpy(np.zeros(3, np.float32))
    cache = nn.KVCache(2, 3, 7, 8, like=like)
    assert len(cache.k) == len(cache.v) == 2 and all(tuple(t.shape) == (3, 7, 8) and t.dtype == np.float32 and not t.requires_grad
                                                     for t in cache.k + cache.v)
    assert len({id(t.numpy()) for t in cache.k + cache.v}) == 4          # four buffers, not one
    assert isinstance(cache.pos, CpuTensor) and cache.pos.dtype == np.int32 and tuple(cache.pos.shape) == (1,) and not cache.pos.requires_grad
    assert cache.length == 0 and cache.pos.numpy()[0] == 0
    storage = cache.pos.numpy()
    cache.advance()
    cache.advance()
    assert cache.length == 2 and cache.pos.numpy()[0] == 2 and cache.pos.numpy() is storage          # in place: a captured step sees it
    cache.set_length(5)
    assert cache.length == 5 and cache.pos.numpy()[0] == 5
    k = CpuTensor.from_numpy(np.arange(3 * 2 * 8, dtype=np.float32).reshape(3, 2, 8))
    cache.fill(1, k, k * 2.0)
    np.testing.assert_array_equal(cache.k[1].numpy()[:, :2], k.numpy())
    np.testing.assert_array_equal(cache.v[1].numpy()[:, :2], 2 * k.numpy())
    assert not cache.k[0].numpy().any() and not cache.k[1].numpy()[:, 2:].any()
    cache.reset()
    assert cache.length == 0 and cache.pos.numpy()[0] == 0
    with pytest.raises(AssertionError):
        cache.set_length(8)
    too_long = CpuTensor.from_numpy(np.zeros((3, 8, 8), np.float32))
    with pytest.raises(AssertionError):
        cache.fill(0, too_long, too_long)
    assert nn.KVCache(1, 1, 2, 4, like=CpuTensor.from_numpy(np.zeros(1, np.float64))).k[0].dtype == np.float64


def test_kv_cache_is_state_not_parameters():
    """a module that holds a cache shows it neither in parameters() nor in buffers(): it never reaches an optimizer"""
    model = dc.make_model(CpuTensor)
    before = [n for n, _ in model.named_parameters()], [n for n, _ in model.named_buffers()]
    model.cache = nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
    assert ([n for n, _ in model.named_parameters()], [n for n, _ in model.named_buffers()]) == before
    held = {id(t) for t in model.cache.k + model.cache.v + [model.cache.pos]}
    assert not held & {id(p) for p in model.parameters()} and not held & {id(p) for p in model.buffers()}
    assert not isinstance(model.cache, nn.Module)


def test_generate_checks_the_capacity_on_the_host():
    _, ids = dc.parameters()
    model = dc.make_model(CpuTensor)
    prompt = CpuTensor.from_numpy(ids[:, :dc.S0], requires_grad=False)
    layers, width, positions = dc.CFG["num_hidden_layers"], dc.CFG["hidden_size"], dc.CFG["max_position_embeddings"]
    like = model.cls.predictions.bias
    with pytest.raises(AssertionError, match="positions"):                           # s0 + new > capacity
        dc.bert.generate(model, prompt, 4, cache=nn.KVCache(layers, dc.B, dc.S0 + 3, width, like=like))
    with pytest.raises(AssertionError, match="position embeddings"):                 # capacity > max_position_embeddings
        dc.bert.generate(model, prompt, 4, cache=nn.KVCache(layers, dc.B, positions + 1, width, like=like))
    with pytest.raises(AssertionError, match="position embeddings"):                 # the cache made inside: s0 + new > max_position_embeddings
        dc.bert.generate(model, prompt, positions - dc.S0 + 1)
    exact = nn.KVCache(layers, dc.B, dc.S0 + 4, width, like=like)
    assert tuple(dc.bert.generate(model, prompt, 4, cache=exact).shape) == (dc.B, dc.S0 + 4) and exact.length == dc.S0 + 3
    with pytest.raises(AssertionError, match="causal=True"):
        np.random.seed(0)
        dc.bert.generate(dc.bert.BertForMaskedLM(**dict(dc.CFG, causal=False)), prompt, 2)


def test_a_second_prompt_needs_a_reset_cache():
    """with tokens in the cache the model takes one token per sequence; `reset()` makes room for a new prompt"""
    _, ids = dc.parameters()
    model = dc.make_model(CpuTensor)
    prompt = CpuTensor.from_numpy(ids[:, :dc.S0], requires_grad=False)
    cache = nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
    first = model(prompt, cache=cache).numpy().copy()
    with pytest.raises(AssertionError, match="one token per sequence"):
        model(prompt, cache=cache)
    cache.reset()
    np.testing.assert_array_equal(model(prompt, cache=cache).numpy(), first)


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------

def test_decode_supported_is_pure_host_code():
    handle = hiplib.load_library()
    for d in (16, 32, 48, 64, 128):
        for capacity in (0, 1, 512, 513):
            assert bool(handle.lg_attention_decode_supported(capacity, d)) == (d in (32, 64) and 1 <= capacity <= 512), (capacity, d)


def test_decode_entry_on_the_uninitialised_library():
    handle = hiplib.load_library()
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entry)
        fn = handle.lg_attention_decode_f32
        assert fn(None, 0, None, 0, None, 0, None, None, 64, 0, None, None, 0, None, 1, 1, 8, 64, 1.0, None, 0) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error()


def test_header_and_prototypes_name_the_decode_entries():
    """(tests/test_abi.py holds the two lists against each other; here: the new entries are in both, with 21 and 2 arguments)"""
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("lg_attention_decode_supported", 2), ("lg_attention_decode_f32", 21)):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(hiplib.PROTOTYPES[name][1]), name


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_decode_kernels_use_no_scratch(tmp_path):
    """csrc/decode.hip compiled for the device only: every attn_decode<D> instantiation has a private segment of 0 bytes (the
    kUnroll float4 in flight per lane stay in registers).  Only the kernels' resource directives are read.  The counts are
    printed: they are the rows of DESIGN.md's table."""
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    out = tmp_path / "decode.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), "decode.hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, body).group(1))        # noqa: E731
        found[name] = (field("private_segment_fixed_size"), field("next_free_vgpr"), field("next_free_sgpr"), field("group_segment_fixed_size"))
    decode = {n: v for n, v in found.items() if "attn_decode" in n}
    assert sorted(re.search(r"attn_decodeILi(\d+)E", n).group(1) for n in decode) == ["32", "64"], sorted(found)
    print("%-52s %8s %6s %6s %6s" % ("kernel", "scratch", "vgprs", "sgprs", "lds"))
    for name, row in sorted(decode.items()):
        print("%-52s %8d %6d %6d %6d" % ((name,) + row))
        assert row[0] == 0, "%s: %d bytes of scratch per lane" % (name, row[0])
        assert row[3] == (512 + 4 * 64 + 8) * 4, "%s: %d bytes of LDS" % (name, row[3])
