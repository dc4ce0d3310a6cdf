"""The paged cache beyond 512 positions without a device: nn.PagedKVCache(..., split=True), `serve(num_blocks=)` with requests
beyond 512 positions on the numpy backend, where `_paged_composite` and `CpuTensor.serve_commit_paged` are the definition."""
import numpy as np
import pytest
import lightgrad_amd.nn as nn
import decode_cases as dc
import paged_cases as pg

POSITIONS = 612


def test_the_cache_beyond_512_positions_is_an_opt_in():
    geometry = dict(layers=1, slots=1, num_blocks=4, block_size=128, width=64, max_blocks=5)
    with pytest.raises(AssertionError, match="PagedKVCache"):
        nn.PagedKVCache(**geometry)
    cache = nn.PagedKVCache(split=True, **geometry)
    assert cache.split and cache.capacity == 640 and not nn.PagedKVCache(**dict(geometry, max_blocks=4)).split
    with pytest.raises(AssertionError, match="16384"):
        nn.PagedKVCache(split=True, **dict(geometry, max_blocks=129))


def test_serve_beyond_512_positions_on_the_numpy_backend():
    cfg = dict(dc.CFG, num_hidden_layers=1, max_position_embeddings=POSITIONS, attention_probs=False, causal=True)
    np.random.seed(dc.SEED)
    model = dc.bert.BertForMaskedLM(**cfg)
    model.load_parameters({n: p.numpy().astype(np.float32) * (dc.GAIN if p.numpy().ndim == 2 else 1.0) for n, p in model.named_parameters()})
    model.eval()
    rng = np.random.RandomState(7)
    prefix = rng.randint(0, cfg["vocab_size"], 40)
    prompts = [np.concatenate([prefix, rng.randint(0, cfg["vocab_size"], n)]) for n in (532, 9, 482, 70)]
    lengths, B, slots, chunk = [len(p) for p in prompts], 16, 2, 32
    (want, want_len), _ = dc.bert.serve(model, prompts, 4, slots=slots, chunk=chunk)                  # the contiguous nn.KVCache
    for shared, F in ((0, 0), (40, 2)):
        cache = nn.PagedKVCache(1, slots, 80, B, cfg["hidden_size"], -(-(max(lengths) + 3) // B), like=model.cls.predictions.bias, split=True)
        assert cache.block_table.shape[1] * B > 512                           # what serve_commit_paged moves: a table beyond 512 positions
        (out, out_len), stats = dc.bert.serve(model, prompts, 4, slots=slots, chunk=chunk, cache=cache, shared_prefix=shared, poll=1)
        np.testing.assert_array_equal(out.numpy(), want.numpy())
        np.testing.assert_array_equal(out_len.numpy(), want_len.numpy())
        # the tables are those of the definition: the step count of the schedule it implies, and every block back on the stack
        assert stats["prefix_blocks"] == F and stats["steps"] == pg.simulate(lengths, out_len.numpy(), [4] * 4, slots, chunk, B, 80, F)
        pg.assert_no_block_leaked(cache, F)
    (out, _), stats = dc.bert.serve(model, prompts, 4, slots=slots, chunk=chunk, num_blocks=80, block_size=B)      # serve builds the cache itself
    np.testing.assert_array_equal(out.numpy(), want.numpy())
    with pytest.raises(AssertionError, match="chunk=129"):
        dc.bert.serve(model, prompts, 4, slots=slots, chunk=129, num_blocks=80, block_size=B)
    with pytest.raises(AssertionError, match="attention_probs=False"):
        dc.bert.serve(dc.bert.BertForMaskedLM(**dict(cfg, attention_probs=True)).eval(), prompts, 4, slots=slots, chunk=chunk, num_blocks=80, block_size=B)
