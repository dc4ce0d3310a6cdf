"""Appending several tokens to a filled nn.KVCache without a device: `model(ids, cache=cache, append=True)` of examples/bert.py
on CpuTensor (the composite over `cache[:, :length + m]` with an (m, length + m) causal bias), `generate(prefill_chunk=)`,
`generate(append=True)`, the host half of the extend entry of the C ABI, and the resources of the extend kernels.

The yardstick is that of test_decode_cpu.py: full causal forwards over each prefix in float64; a float32 result may be no
further from them than twice the float32 full forward is, with a floor of 1e-5.  hipcc cross-compiles without a GPU."""
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
from common import assert_as_close_to_float64_as_the_cpu_backend, float64_tape
import decode_cases as dc
import extend_cases as ec

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")
LG_ENOTINIT = -4


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "prompt-mask"])
def test_appended_pieces_in_float64_are_the_full_forward(masked):
    """a prompt of 5 tokens, then pieces of 3, 1 and 4 given tokens into a cache of 17: every logit row of every piece against
    the row of the full causal forward over the prefix that ends with the piece, under the rule of
    test_decode_cpu.py::test_teacher_forced_in_float64_is_the_full_forward - relative Frobenius distance below 1e-13.
    Not the rows' bits: the composite forms every sum over the same operands in the same order, but each product is numpy's
    matmul, and its BLAS rounds a row differently depending on how many rows the call has - a piece of 1 token is a
    matrix-vector product, and 3 rows onto the 101-word vocabulary differ from the same rows among 8.  Measured here: the
    attention's probabilities and context of a 3-token piece are the full forward's bit for bit, the logits differ by up to
    2.3e-15 absolute (a few units in the last place; relative Frobenius distance at most 5.5e-16), as numpy's own
    `x[5:8] @ w.T` differs from `(x @ w.T)[5:8]` for a (101, 64) w."""
    from common import rel_frobenius
    ref64, _ = ec.append_reference(masked)
    with float64_tape():
        got = ec.append_run(CpuTensor, masked, model=dc.make_model(CpuTensor, np.float64), dtype=np.float64)
    assert sorted(got) == sorted(ref64) and len(got) == 1 + len(ec.PIECES)
    for name in ref64:
        assert got[name].dtype == np.float64 and got[name].shape == ref64[name].shape, name
        print("%s: largest difference %.3e, relative Frobenius %.3e" % (name, np.abs(got[name] - ref64[name]).max(), rel_frobenius(got[name], ref64[name])))
        assert rel_frobenius(got[name], ref64[name]) < 1e-13, name


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "prompt-mask"])
def test_appended_pieces_in_float32_match_the_full_forward(masked):
    ref64, cpu32 = ec.append_reference(masked)
    got = ec.append_run(CpuTensor, masked)
    assert sorted(got) == sorted(ref64)
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, floor=1e-5, what="append forward on CpuTensor")


@pytest.mark.parametrize("chunk", [1, 2, 5, 7])
def test_chunked_prefill_gives_the_tokens_of_generate(chunk):
    """the prompt of 5 tokens in pieces of 1, 2, 5 (one piece through the append path) and 7 (more than the prompt)"""
    want = dc.assert_margins_rule_out_ties()
    np.testing.assert_array_equal(dc.greedy(CpuTensor, prefill_chunk=chunk), want)


def test_chunked_prefill_with_a_prompt_mask():
    mask = CpuTensor.from_numpy(dc.PROMPT_MASK, requires_grad=False)
    np.testing.assert_array_equal(dc.greedy(CpuTensor, new=3, attention_mask=mask, prefill_chunk=2), dc.greedy(CpuTensor, new=3, attention_mask=mask))


def test_two_turns_equal_a_full_recompute_per_token_in_float64():
    """prompt 5 -> 4 new tokens -> 3 given tokens appended -> 3 new tokens.  First, on the float64 reference alone: the top-2
    margin of every greedy step is at least 100 times the float32 deviation (the seed of tests/extend_cases.py was picked for
    that on the CPU), no step is left out"""
    first, second = ec.assert_two_turn_margins_rule_out_ties()
    assert first.shape == (dc.B, ec.TURN1) and second.shape == (dc.B, ec.TURN2)
    got1, got2 = ec.two_turns(CpuTensor)
    np.testing.assert_array_equal(got1, first)
    np.testing.assert_array_equal(got2, second)


def test_kv_cache_positions_follow_the_position():
    cache = nn.KVCache(1, 2, 9, 4, like=CpuTensor.from_numpy(np.zeros(1, np.float32)))
    p = cache.positions(3)
    assert isinstance(p, CpuTensor) and p.dtype == np.int32 and tuple(p.shape) == (3,) and not p.requires_grad
    np.testing.assert_array_equal(p.numpy(), [0, 1, 2])
    cache.advance(4)
    np.testing.assert_array_equal(cache.positions(3).numpy(), [4, 5, 6])
    np.testing.assert_array_equal(cache.positions(1).numpy(), [4])
    assert cache.pos.numpy()[0] == 4 and tuple(cache.pos.shape) == (1,)                 # the position itself is untouched


def test_the_append_path_checks_room_and_positions_on_the_host():
    _, ids = dc.parameters()
    model = dc.make_model(CpuTensor)
    layers, width, positions = dc.CFG["num_hidden_layers"], dc.CFG["hidden_size"], dc.CFG["max_position_embeddings"]
    like = model.cls.predictions.bias
    tensor = lambda a: CpuTensor.from_numpy(a, requires_grad=False)          # noqa: E731
    prompt = tensor(ids[:, :dc.S0])
    cache = nn.KVCache(layers, dc.B, dc.S0 + 3, width, like=like)
    model(prompt, cache=cache)
    with pytest.raises(AssertionError, match="do not fit"):                          # length + m > capacity
        model(tensor(ids[:, dc.S0:dc.S0 + 4]), cache=cache, append=True)
    assert tuple(model(tensor(ids[:, dc.S0:dc.S0 + 3]), cache=cache, append=True).shape) == (dc.B, 3, dc.CFG["vocab_size"])
    with pytest.raises(AssertionError, match="one token per sequence"):              # without append= a filled cache takes one token
        model(prompt, cache=cache)
    with pytest.raises(AssertionError, match="append=True goes with a cache"):
        model.bert(prompt, append=True)
    big = nn.KVCache(layers, dc.B, positions + 4, width, like=like)
    big.set_length(positions - 1)
    with pytest.raises(AssertionError, match="position embeddings"):                 # length + m > max_position_embeddings
        model(tensor(ids[:, :2]), cache=big, append=True)
    # generate: the tokens already in the cache count
    cache = nn.KVCache(layers, dc.B, dc.CAPACITY, width, like=like)
    dc.bert.generate(model, prompt, 4, cache=cache)                                  # 8 positions held
    with pytest.raises(AssertionError, match="positions"):
        dc.bert.generate(model, tensor(ids[:, :5]), dc.CAPACITY - 8 - 5 + 1, cache=cache, append=True)
    with pytest.raises(AssertionError, match="append=True continues a cache"):
        dc.bert.generate(model, prompt, 2, append=True)
    out = dc.bert.generate(model, tensor(ids[:, :5]), dc.CAPACITY - 8 - 5, cache=cache, append=True)
    assert tuple(out.shape) == (dc.B, dc.CAPACITY - 8) and cache.length == dc.CAPACITY - 1


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------

def test_extend_supported_is_pure_host_code():
    handle = hiplib.load_library()
    for d in (16, 32, 48, 64, 128):
        for capacity in (0, 1, 5, 512, 513):
            for m in (0, 1, 5, 6, 512, 513):
                want = d in (32, 64) and 1 <= m <= capacity <= 512
                assert bool(handle.lg_attention_extend_supported(m, capacity, d)) == want, (m, capacity, d)


def test_extend_entry_on_the_uninitialised_library():
    handle = hiplib.load_library()
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entry)
        fn = handle.lg_attention_extend_f32
        assert fn(None, 0, 0, None, 0, 0, None, 0, 0, None, None, 64, 0, None, None, 0, 0, None, 1, 1, 2, 8, 64, 1.0, None, 0) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error()


def test_header_and_prototypes_name_the_extend_entries():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("lg_attention_extend_supported", 3), ("lg_attention_extend_f32", 26)):
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(hiplib.PROTOTYPES[name][1]), name
    assert "extend.hip" in open(os.path.join(CSRC, "Makefile")).read()


# ---- the kernels' resources ---------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_extend_kernels_use_no_scratch(tmp_path):
    """csrc/extend.hip compiled for the device only: both attn_extend<D> instantiations have a private segment of 0 bytes (the
    chunk in flight and the softmax's row stay in registers) and no static LDS (the tiles are dynamic, sized by the capacity).
    Only the kernels' resource directives are read.  The counts are printed: they are the rows of DESIGN.md's table."""
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    out = tmp_path / "extend.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), "extend.hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, body).group(1))        # noqa: E731
        found[name] = (field("private_segment_fixed_size"), field("next_free_vgpr"), field("accum_offset"), field("next_free_sgpr"),
                       field("group_segment_fixed_size"))
    extend = {n: v for n, v in found.items() if "attn_extend" in n}
    assert sorted(re.search(r"attn_extendILi(\d+)E", n).group(1) for n in extend) == ["32", "64"], sorted(found)
    print("%-44s %8s %12s %12s %6s %6s" % ("kernel", "scratch", "vgprs+agprs", "accum_offset", "sgprs", "lds"))
    for name, row in sorted(extend.items()):
        print("%-44s %8d %12d %12d %6d %6d" % ((name,) + row))
        assert row[0] == 0, "%s: %d bytes of scratch per lane" % (name, row[0])
        assert row[4] == 0, "%s: %d bytes of static LDS" % (name, row[4])
