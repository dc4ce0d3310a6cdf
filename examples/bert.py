"""tiny-BERT for masked-LM (BASELINE config #5): model classes with the parameter naming of the public
BERT checkpoints (so `load_parameters` takes a HuggingFace-style state dict), written against the tensor
API only - they run on CpuTensor and on HipTensor.  Counterpart of the model half of the reference's
examples/bert.py:14-229; its tokenizer and `from_pretrained` need network access and are out of scope.

Differences from the reference, on purpose:
  * embeddings are looked up with `weight[ids]` on the tensor's own backend (the reference round-trips
    through the CPU and thereby drops the embedding gradient, bert.py:19-21);
  * `gelu` uses the backend's fused op when there is one (same expression, bert.py:12); so does the scaling of the
    attention scores in front of their softmax (bert.py:81-86) when there is no mask to add in between, and the two residual
    additions of a layer (bert.py:101, :117), spelled `dense(h, residual=r)` (nn.Linear adds r where the product is made);
  * dropout is real: `hidden_dropout_prob` after the embedding LayerNorm, the attention output projection and the feed-forward
    output projection, `attention_probs_dropout_prob` on the attention probabilities (the reference takes both arguments and
    then sets `self.dropout = lambda x: x`, bert.py:37, :67, :102, :124).  Both default to 0, and with 0 or in `model.eval()`
    every site takes exactly the path it took before.  Each hidden dropout sits next to a LayerNorm: where the backend has the
    one-launch forms (`layer_norm_dropout`, `dropout_add_layer_norm`) the pair is one node, with the same masks.

    python examples/bert.py [--cpu] [--batch 8]        # forward + backward of a random tiny-BERT
    python examples/bert.py --mlm [--graph]            # the masked-LM objective: token masking from the random stream (inside the
                                                       # capture with --graph), cross-entropy over the masked positions only
    python examples/bert.py --mlm --accuracy [--graph] # also counts the masked tokens predicted right (light.metrics.accuracy), on
                                                       # the device, over every step and replay: one host read at the end
    python examples/bert.py --clm [--graph] [--cpu]    # a causal language model of the same parameters: config key `causal=True`
                                                       # (query i sees keys j <= i, inside the fused attention launches) and the
                                                       # next-token objective (light.data.next_token_labels)
    python examples/bert.py --generate 16 [--graph] [--cpu]   # greedy decoding with a key / value cache (nn.KVCache): the prompt once through
                                                       # the causal forward, then one token per step against the cache - on HipTensor
                                                       # two launches of attention per layer (csrc/decode.hip), nothing read back until
                                                       # the ids are printed; --graph: the step is captured once and replayed
    python examples/bert.py --generate 16 --sample [--temperature T] [--top-k K] [--top-p P] [--seed S] [--graph] [--cpu]
                                                       # sampled decoding: every token is `logits.sample(T, K, P)` - one launch
                                                       # (csrc/sample.hip) in place of argmax + astype, drawn from the random stream
                                                       # after light.manual_seed(S); under --graph every replay draws fresh numbers
    python examples/bert.py --generate 16 --prefill-chunk 3 [--graph] [--cpu]
                                                       # the prompt goes into the cache in pieces of at most 3 tokens, each piece
                                                       # one attention launch per layer against the filled cache (csrc/extend.hip,
                                                       # `model(ids, cache=cache, append=True)`): the same tokens
    python examples/bert.py --generate 16 --ragged [--eos ID] [--graph] [--sample ...] [--cpu]
                                                       # a ragged batch in one run: prompts of different lengths, right-padded, every
                                                       # sequence at its own positions (nn.KVCache(per_row=True), `generate(lengths=)`);
                                                       # --eos ID: a row that draws ID stops, the others go on
    python examples/bert.py --serve 16 --slots 4 --chunk 16 [--eos ID] [--graph] [--sample ...] [--cpu]
                                                       # continuous batching: 16 requests of different lengths and budgets through 4
                                                       # cache slots (`serve`, nn.RequestPool) - a slot whose request has finished takes
                                                       # the next waiting prompt, in pieces of at most 16 tokens, while the other slots
                                                       # go on decoding; one attention launch per layer for all of them (a token count
                                                       # per slot, csrc/extend.hip), one launch of bookkeeping per step (csrc/serve.hip),
                                                       # one word read back every few steps; --graph: the step is captured once
    python examples/bert.py --serve 16 --slots 4 --chunk 16 --token-budget 24 [--graph] [--cpu]
                                                       # the same through TOKEN-PACKED steps: every step has 24 token rows for all slots
                                                       # together - one per decoding slot, the rest shared by the prefilling slots in
                                                       # pieces of at most 16 (`serve(token_budget=)`, csrc/serve_packed.hip)
    python examples/bert.py --serve 16 --sample --per-request [--seed S] [--graph] [--cpu]
                                                       # per-request sampling: request r has one of a short cycle of parameter sets
                                                       # (one of them greedy) and the random stream seeded S + r, so its tokens do not
                                                       # depend on slots, chunk or the other requests (`serve(seeds=)`,
                                                       # `logits.sample_rows`, csrc/sample_rows.hip)
    python examples/bert.py --serve 16 --repetition-penalty 1.3 --frequency-penalty 0.3 [--presence-penalty A] [--min-new-tokens M] [--graph] [--cpu]
                                                       # per-request penalties on the logits in front of the draw, from the request's
                                                       # own prompt and tokens: the randomly initialised model stops repeating one id
                                                       # (`serve(repetition_penalty=, ...)`, `logits.penalize_rows`, csrc/penalize.hip)
    python examples/bert.py --serve 16 --logprobs 3 [--graph] [--cpu]
                                                       # the log-probability of every token and the 3 most likely ids of its step,
                                                       # one launch a step behind the draw, nothing read back until the end
                                                       # (`serve(logprobs=)`, `logits.logprob_rows`, csrc/logprob.hip)
    python examples/bert.py --serve 16 --allow-only A,B,.. | --ban A,B,.. | --one-of "A B;C D E" | --stop-after "A B" [--eos E] [--graph] [--cpu]
                                                       # guided decoding: one token automaton for every request - an allowed set,
                                                       # banned ids, one of several sequences (then eos), or free text up to a
                                                       # stop sequence (`serve(guide=)`, `light.guide`, `logits.guide_rows`,
                                                       # csrc/guide.hip)
    python examples/bert.py --mlm --bf16-decoder       # the decoder onto the vocabulary (forward, dx, dW) on the bf16 matrix cores:
                                                       # config key `decoder_precision="bf16"`; tensors stay float32
"""
import math
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lightgrad_amd as light  # noqa: E402
import lightgrad_amd.nn as nn  # noqa: E402
from lightgrad_amd.autograd.cpu.ops import bf16_round_array  # noqa: E402

TINY = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
            vocab_size=30522, max_position_embeddings=512, type_vocab_size=2)


def gelu(x):
    if hasattr(x, "gelu"):
        return x.gelu()
    return 0.5 * x * (1.0 + (x * 0.7978845608 * (1.0 + 0.044715 * x * x)).tanh())


class Embedding(nn.Module):
    def __init__(self, embedding_dim, vocab_size):
        nn.Module.__init__(self)
        self.weight = light.xavier((vocab_size, embedding_dim))

    def forward(self, ids):
        return self.weight[ids]


class BertEmbedding(nn.Module):
    def __init__(self, hidden_size, vocab_size, max_position_embeddings, type_vocab_size, hidden_dropout_prob=0.0):
        nn.Module.__init__(self)
        self.dropout = nn.Dropout(hidden_dropout_prob)
        self.word_embeddings = Embedding(hidden_size, vocab_size)
        self.position_embeddings = Embedding(hidden_size, max_position_embeddings)
        self.token_type_embeddings = Embedding(hidden_size, type_vocab_size)
        self.LayerNorm = nn.LayerNorm(hidden_size)
        self._const_ids = {}        # (backend class, shape) -> constant id tensors, uploaded once

    def _constant_ids(self, cls, shape):
        key = (cls, tuple(shape))
        if key not in self._const_ids:
            self._const_ids[key] = (cls.from_numpy(np.zeros(shape, dtype=np.int32), requires_grad=False),
                                    cls.from_numpy(np.arange(shape[-1], dtype=np.int32), requires_grad=False))
            for t in self._const_ids[key]:
                if hasattr(t, "freeze"):
                    t.freeze()              # constants of the model: a backend may keep what it derives from them (and record it in graphs)
        return self._const_ids[key]

    def forward(self, input_ids, token_type_ids=None, token_position=None, token_positions=None):
        """`token_position`: an int32 tensor of one element on the ids' backend - the position of the ONE token per sequence that
        `input_ids` (b, 1) holds (a decode step: looked up where the tensor lives, no host read); `token_positions`: an int32 tensor
        (m,) on the ids' backend - the positions of the m tokens per sequence of `input_ids` (b, m), shared by the batch (an append
        to a filled cache: nn.KVCache.positions) - or (b, m): a position per token (a cache with a position per sequence; a
        `token_position` of shape (b,) with b > 1 is the (b, 1) case); neither: positions 0 .. s - 1"""
        zeros, position_ids = self._constant_ids(input_ids.__class__, input_ids.shape)
        if token_position is not None:
            assert input_ids.shape[-1] == 1, "a position goes with one token per sequence, got ids of shape %s" % (tuple(input_ids.shape),)
            position_ids = token_position
            if tuple(token_position.shape) == (input_ids.shape[0],) and input_ids.shape[0] > 1:
                position_ids = token_position.reshape(input_ids.shape[0], 1)           # a view: one position per sequence
                position_ids._requires_grad = False     # ids are state like the position: they go into lookups by keyword
        if token_positions is not None:
            assert token_position is None and tuple(token_positions.shape) in ((input_ids.shape[-1],), tuple(input_ids.shape)), \
                "position ids of shape %s do not go with ids of shape %s" % (tuple(token_positions.shape), tuple(input_ids.shape))
            position_ids = token_positions
        if token_type_ids is None:
            token_type_ids = zeros
        word, position, kind = self.word_embeddings.weight, self.position_embeddings.weight, self.token_type_embeddings.weight
        if hasattr(word, "embedding_sum"):
            # the backend's one-kernel form of the line below: three lookups and their sum
            e = word.embedding_sum(position, kind, ids0=input_ids, ids1=position_ids, ids2=token_type_ids)
        else:
            e = self.word_embeddings(input_ids) + self.position_embeddings(position_ids) + self.token_type_embeddings(token_type_ids)
        if self.training and self.dropout.p > 0 and hasattr(e, "layer_norm_dropout"):
            # the backend's one-launch form of the line below: the mask is drawn where the LayerNorm kernel stores its row
            return e.layer_norm_dropout(self.LayerNorm.weight, self.LayerNorm.bias, self.dropout.p, self.LayerNorm.eps)
        return self.dropout(self.LayerNorm(e))


def _bf16_refusal(cache):
    """what a refusal of a paged cache adds for one that holds bfloat16 words: the form the refused route does take"""
    if getattr(cache, "kv_dtype", None) != "bf16":
        return ""
    return " (kv_dtype=\"bf16\": a bf16 cache is a form of the paged one - this route takes a float32 nn.KVCache)"


class BertSelfAttention(nn.Module):
    def __init__(self, hidden_size, num_attention_heads, attention_probs_dropout_prob=0.0, causal=False):
        """`causal=True`: query i sees keys j <= i only - the decoder-style mask of a causal language model.  The values are those
        of the composite branch below: one more additive constant, `(1 - tril) * -10000`, behind the key-padding bias"""
        nn.Module.__init__(self)
        assert hidden_size % num_attention_heads == 0
        self.causal = bool(causal)
        self._tril = {}             # (backend class, s, dtype) -> the (1, 1, s, s) lower-triangular constant of ones
        self.dropout = nn.Dropout(attention_probs_dropout_prob)
        self.h, self.d = num_attention_heads, hidden_size // num_attention_heads
        self.query = nn.Linear(hidden_size, hidden_size)
        self.key = nn.Linear(hidden_size, hidden_size)
        self.value = nn.Linear(hidden_size, hidden_size)

    def _lower_triangle(self, like, s):
        key = (like.__class__, s, np.dtype(like.dtype))
        if key not in self._tril:
            t = like.__class__.from_numpy(np.tril(np.ones((1, 1, s, s), dtype=like.dtype)), requires_grad=False)
            if hasattr(t, "freeze"):
                t.freeze()                  # a constant of the model, like the position ids
            self._tril[key] = t
        return self._tril[key]

    def _decode(self, hidden, attention_mask, cache, index):
        """one new token per sequence against the cached keys and values: position t = the cache's position attends to keys 0 .. t
        - the row the causal forward computes for query t.  attention_mask: None or (b, capacity) over the cache's rows.  A cache
        with a position per sequence (per_row): the fused route passes `cache.pos` (b,) as it is - sequence r at its own t_r"""
        b = hidden.shape[0]
        scale = math.sqrt(self.d) ** -1
        k_cache, v_cache = cache.k[index], cache.v[index]
        mask_ok = attention_mask is None or (attention_mask.dtype == np.float32 and not attention_mask.requires_grad and
                                             tuple(attention_mask.shape) in ((b, cache.capacity), (1, cache.capacity)))
        if hasattr(hidden, "self_attention_decode") and mask_ok and hidden.self_attention_decode_supported(self.query.weight, self.h, cache.capacity):
            # the backend's one-node form: one launch for the three projections, one for the attention, which reads the position on
            # the device and writes the new key / value rows into the cache itself
            extra = {"mask": attention_mask} if attention_mask is not None else {}
            context = hidden.self_attention_decode(self.query.weight, self.query.bias, self.key.weight, self.key.bias, self.value.weight,
                                                   self.value.bias, k_cache, v_cache, cache.pos, heads=self.h, scale=scale, **extra)
            return context, None
        if getattr(cache, "per_row", False):
            return self._rows_composite(hidden, attention_mask, cache, index)
        # the same over the tensor API: the host mirror of the position slices the cache
        t = cache.length
        assert t < cache.capacity, "the cache holds %d positions: no room for position %d" % (cache.capacity, t)
        q, k, v = self.query(hidden), self.key(hidden), self.value(hidden)
        k_cache[:, t:t + 1] = k
        v_cache[:, t:t + 1] = v
        q = q.reshape(b, 1, self.h, self.d).transpose(0, 2, 1, 3)
        k = k_cache[:, :t + 1].reshape(b, t + 1, self.h, self.d).transpose(0, 2, 3, 1)
        v = v_cache[:, :t + 1].reshape(b, t + 1, self.h, self.d).transpose(0, 2, 1, 3)
        scores = (q @ k) / math.sqrt(self.d)
        if attention_mask is not None:
            mask = attention_mask[:, :t + 1]
            scores = scores + ((1.0 - mask.reshape(mask.shape[0], 1, 1, t + 1)) * -10000.0).detach()
        probs = scores.softmax(axis=-1)
        return (probs @ v).transpose(0, 2, 1, 3).reshape(b, 1, self.h * self.d), probs

    def _rows_composite(self, hidden, attention_mask, cache, index, count=None):
        """`_decode` (m = 1) and `_extend` over the tensor API for a cache with a position per sequence (nn.KVCache(per_row=True)):
        CpuTensor, float64 tapes and head sizes the kernels refuse.  Sequence r writes its m new rows at positions t_r .. t_r + m - 1
        and its query i sees keys 0 .. t_r + i; keys beyond - the other sequences' reach, and whatever the cache holds there - are
        hidden with the usual -10000 bias.  The positions are taken from the cache's host mirror while it is valid; otherwise
        they are READ from `cache.pos`: free on CpuTensor, a synchronising device read on any other backend.
        count (int32 (b,), READ like the positions): sequence r has count[r] real tokens among its m rows - only those are
        written to the cache (at t_r .. t_r + count[r] - 1: only they have to fit it), and the context rows of the others are 0."""
        if count is not None:
            return self._counted_composite(hidden, attention_mask, cache, index, count)
        b, m = hidden.shape[0], hidden.shape[1]
        k_cache, v_cache = cache.k[index], cache.v[index]
        t = cache.lengths if cache.lengths is not None else np.asarray(cache.pos.numpy(), np.int64)
        assert (t >= 0).all() and (t + m <= cache.capacity).all(), \
            "the cache holds %s of %d positions: no room for %d more in every row" % (t.tolist(), cache.capacity, m)
        n = int(t.max()) + m
        q, k, v = self.query(hidden), self.key(hidden), self.value(hidden)
        for r in range(b):
            k_cache[r:r + 1, int(t[r]):int(t[r]) + m] = k[r:r + 1]
            v_cache[r:r + 1, int(t[r]):int(t[r]) + m] = v[r:r + 1]
        q = q.reshape(b, m, self.h, self.d).transpose(0, 2, 1, 3)
        k = k_cache[:, :n].reshape(b, n, self.h, self.d).transpose(0, 2, 3, 1)
        v = v_cache[:, :n].reshape(b, n, self.h, self.d).transpose(0, 2, 1, 3)
        scores = (q @ k) / math.sqrt(self.d)
        if attention_mask is not None:
            mask = attention_mask[:, :n]
            scores = scores + ((1.0 - mask.reshape(mask.shape[0], 1, 1, n)) * -10000.0).detach()
        # (b, 1, m, n): key j is visible to query i of sequence r where j <= t_r + i
        visible = (np.arange(n)[None, None, :] <= (t[:, None, None] + np.arange(m)[None, :, None])).astype(scores.dtype)
        visible = scores.__class__.from_numpy(visible.reshape(b, 1, m, n), requires_grad=False)
        scores = scores + ((1.0 - visible) * -10000.0).detach()
        probs = scores.softmax(axis=-1)
        return (probs @ v).transpose(0, 2, 1, 3).reshape(b, m, self.h * self.d), probs

    def _counted_composite(self, hidden, attention_mask, cache, index, count, round_kv=False):
        """`_rows_composite` with a token count per sequence - the definition of `self_attention_extend(count=)`.  Positions and
        counts are read from the tensors (whoever moved them: `advance`, `serve_commit`).  round_kv (a bfloat16 cache,
        `_paged_composite`): the step's keys and values enter as r(key(hidden)), r(value(hidden)), r = `bf16_round_array` (a
        float64 tape rounds through float32, as r does); the queries are not rounded"""
        b, m = hidden.shape[0], hidden.shape[1]
        k_cache, v_cache = cache.k[index], cache.v[index]
        t, c = np.asarray(cache.pos.numpy(), np.int64), np.asarray(count.numpy(), np.int64)
        assert c.shape == (b,) and (c >= 0).all() and (c <= m).all() and (t >= 0).all() and (t + c <= cache.capacity).all(), \
            "the cache holds %s of %d positions: no room for %s more of the %d rows given" % (t.tolist(), cache.capacity, c.tolist(), m)
        n = max(int((t + c).max()), 1)
        q, k, v = self.query(hidden), self.key(hidden), self.value(hidden)
        if round_kv:
            # on the host, by the definition itself (the composite reads positions and pools there anyway): any backend, any float dtype
            k, v = (x.__class__.from_numpy(bf16_round_array(np.asarray(x.numpy())), requires_grad=False) for x in (k, v))
        for r in range(b):
            if c[r]:
                k_cache[r:r + 1, int(t[r]):int(t[r] + c[r])] = k[r:r + 1, :int(c[r])]
                v_cache[r:r + 1, int(t[r]):int(t[r] + c[r])] = v[r:r + 1, :int(c[r])]
        q = q.reshape(b, m, self.h, self.d).transpose(0, 2, 1, 3)
        k = k_cache[:, :n].reshape(b, n, self.h, self.d).transpose(0, 2, 3, 1)
        v = v_cache[:, :n].reshape(b, n, self.h, self.d).transpose(0, 2, 1, 3)
        scores = (q @ k) / math.sqrt(self.d)
        if attention_mask is not None:
            mask = attention_mask[:, :n]
            scores = scores + ((1.0 - mask.reshape(mask.shape[0], 1, 1, n)) * -10000.0).detach()
        # (b, 1, m, n): key j is visible to query i of sequence r where j <= t_r + i (a row without a token: as its last real one)
        reach = t[:, None, None] + np.minimum(np.arange(m)[None, :, None], np.maximum(c - 1, 0)[:, None, None])
        visible = (np.arange(n)[None, None, :] <= reach).astype(scores.dtype)
        visible = scores.__class__.from_numpy(visible.reshape(b, 1, m, n), requires_grad=False)
        scores = scores + ((1.0 - visible) * -10000.0).detach()
        probs = scores.softmax(axis=-1)
        real = (np.arange(m)[None, :] < c[:, None]).astype(scores.dtype)
        constant = lambda a: scores.__class__.from_numpy(np.ascontiguousarray(a), requires_grad=False)       # noqa: E731
        context = (probs @ v).transpose(0, 2, 1, 3).reshape(b, m, self.h * self.d)
        return context * constant(real.reshape(b, m, 1)), probs * constant(real.reshape(b, 1, m, 1))

    def _paged_composite(self, hidden, attention_mask, cache, index, count):
        """a step against an nn.PagedKVCache over the tensor API - the definition of `self_attention_extend(count=, block_table=,
        block_size=)`: every slot's rows below its position are gathered from the pool through its table into a contiguous
        (slots, capacity, width) cache, `_counted_composite` runs on it, and the new rows t .. t + count - 1 of every slot are
        scattered back to the pool.  Positions, counts and the table are READ from the tensors (whoever moved them:
        `serve_commit_paged`); a table word the slot reaches must name a block of the pool.
        A bfloat16 cache (`cache.kv_dtype == "bf16"`: int16 pools, the definition of `kv_dtype="bf16"`): the gather WIDENS
        (`light.bf16_widen`, into the dtype of `hidden`), the step's keys and values enter the counted composite as r(.) of what
        the projections produced, and the scatter writes `light.bf16_bits` - of values that are r(.) already, so exactly"""
        b, B, capacity = hidden.shape[0], cache.block_size, cache.capacity
        bf16 = getattr(cache, "kv_dtype", None) == "bf16"
        t, c = np.asarray(cache.pos.numpy(), np.int64), np.asarray(count.numpy(), np.int64)
        table = np.asarray(cache.block_table.numpy(), np.int64)
        assert c.shape == (b,) and (c >= 0).all() and (t >= 0).all() and (t + c <= capacity).all(), \
            "the paged cache holds %s of %d positions: no room for %s more" % (t.tolist(), capacity, c.tolist())
        reach = -(-(t + c) // B)
        for r in range(b):
            if not ((table[r, :reach[r]] >= 0) & (table[r, :reach[r]] < cache.num_blocks)).all():
                raise IndexError("slot %d reaches %d blocks and its table names %s: not blocks of a pool of %d" % (
                    r, reach[r], table[r, :reach[r]].tolist(), cache.num_blocks))
        cls = hidden.__class__
        pools = (cache.k[index], cache.v[index])
        rows = []
        for pool in pools:
            host = np.asarray(pool.numpy())
            if bf16:
                host = light.bf16_widen(host).astype(np.dtype(hidden.dtype))
            flat = np.zeros((b, capacity, cache.width), host.dtype)
            for r in range(b):
                if t[r]:
                    flat[r, :t[r]] = host[table[r, :-(-t[r] // B)]].reshape(-1, cache.width)[:t[r]]
            rows.append(cls.from_numpy(flat, requires_grad=False))

        class _Gathered(object):
            k, v, pos = [rows[0]], [rows[1]], cache.pos
        _Gathered.capacity = capacity
        context, probs = self._counted_composite(hidden, attention_mask, _Gathered, 0, count, round_kv=bf16)
        words = [cls.from_numpy(light.bf16_bits(np.asarray(flat.numpy())), requires_grad=False) for flat in rows] if bf16 else rows
        for r in range(b):
            for j in range(int(t[r]), int(t[r] + c[r])):
                block, at = int(table[r, j // B]), j % B
                for pool, flat in zip(pools, words):
                    pool[block:block + 1, at:at + 1] = flat[r:r + 1, j:j + 1]
        return context, probs

    def _packed_composite(self, hidden, attention_mask, cache, index, cu):
        """a TOKEN-PACKED step over the tensor API - the definition of `self_attention_extend(cu=)`: `hidden` (1, T, hidden) holds the
        step's tokens of all cache slots, slot s owns rows cu[s] .. cu[s + 1] - 1.  Every slot with a row is computed as
        `_rows_composite` computes it alone on its rows, against its own cache rows at its own position; the rows behind
        cu[slots], which belong to nobody, are 0 in the context.  Positions and cu are read from the tensors (whoever moved
        them: `serve_commit_packed`)"""
        T, slots = hidden.shape[1], cache.batch
        k_cache, v_cache = cache.k[index], cache.v[index]
        t, c = np.asarray(cache.pos.numpy(), np.int64), np.asarray(cu.numpy(), np.int64)
        n = np.diff(c)
        assert hidden.shape[0] == 1 and c.shape == (slots + 1,) and c[0] >= 0 and (n >= 0).all() and c[-1] <= T and (t >= 0).all() \
            and (t + n <= cache.capacity).all(), \
            "the cache holds %s of %d positions: no room for the rows %s of the %d given" % (t.tolist(), cache.capacity, c.tolist(), T)
        q, k, v = self.query(hidden), self.key(hidden), self.value(hidden)
        context = hidden.__class__.from_numpy(np.zeros((1, T, self.h * self.d), dtype=q.dtype), requires_grad=False)
        for s in range(slots):
            if n[s] == 0:
                continue
            lo, hi, ts, m = int(c[s]), int(c[s + 1]), int(t[s]), int(n[s])
            keys = ts + m
            k_cache[s:s + 1, ts:keys] = k[:, lo:hi]
            v_cache[s:s + 1, ts:keys] = v[:, lo:hi]
            qs = q[:, lo:hi].reshape(1, m, self.h, self.d).transpose(0, 2, 1, 3)
            ks = k_cache[s:s + 1, :keys].reshape(1, keys, self.h, self.d).transpose(0, 2, 3, 1)
            vs = v_cache[s:s + 1, :keys].reshape(1, keys, self.h, self.d).transpose(0, 2, 1, 3)
            scores = (qs @ ks) / math.sqrt(self.d)
            if attention_mask is not None:
                mask = attention_mask[s:s + 1, :keys] if attention_mask.shape[0] > 1 else attention_mask[:, :keys]
                scores = scores + ((1.0 - mask.reshape(1, 1, 1, keys)) * -10000.0).detach()
            # (1, 1, m, keys): key j is visible to query i where j <= t + i
            visible = (np.arange(keys)[None, :] <= (ts + np.arange(m))[:, None]).astype(scores.dtype)
            visible = scores.__class__.from_numpy(visible.reshape(1, 1, m, keys), requires_grad=False)
            scores = scores + ((1.0 - visible) * -10000.0).detach()
            context[:, lo:hi] = (scores.softmax(axis=-1) @ vs).transpose(0, 2, 1, 3).reshape(1, m, self.h * self.d)
        return context, None

    def _triangle_behind(self, like, t, m):
        """rows t .. t + m - 1 of the lower-triangular constant of t + m positions, (1, 1, m, t + m): query t + i sees keys 0 .. t + i"""
        key = (like.__class__, t, m, np.dtype(like.dtype))
        if key not in self._tril:
            tri = like.__class__.from_numpy(np.tril(np.ones((1, 1, m, t + m), dtype=like.dtype), k=t), requires_grad=False)
            if hasattr(tri, "freeze"):
                tri.freeze()
            self._tril[key] = tri
        return self._tril[key]

    def _extend(self, hidden, attention_mask, cache, index, count=None, cu=None):
        """m new tokens per sequence behind the cache's position t (any t >= 0): query row i at position t + i attends to keys
        0 .. t + i - the rows the causal forward computes for queries t .. t + m - 1.  attention_mask: None or (b, capacity) over
        the cache's rows.  count: None, or an int32 tensor (b,) next to a cache with a position per sequence - sequence r has
        count[r] real tokens among its m rows (a step that mixes decoding, prefilling and idle sequences): the fused route passes
        it to the launch as it is, the composite reads it.  cu: None, or an int32 tensor (slots + 1,) - the step is token-packed:
        `hidden` is (1, T, hidden), the tokens of all `cache.batch` slots, slot s owning rows cu[s] .. cu[s + 1] - 1
        (`_packed_composite` is the definition; the fused route is one projection launch on the T rows and one attention launch)"""
        counted = {} if count is None else {"count": count}
        assert count is None or getattr(cache, "per_row", False), "count= takes a cache with a position per sequence: nn.KVCache(..., per_row=True)"
        if isinstance(cache, nn.PagedKVCache):
            # the cache's rows lie in blocks of a pool: the fused route passes the table to the paged launch (still two launches
            # per layer), anything else gathers, runs the counted composite and scatters (`_paged_composite`, the definition)
            assert count is not None and cu is None, "an nn.PagedKVCache serves the count= append path only (not cu=, not a step without count=)" + \
                _bf16_refusal(cache)
            b = hidden.shape[0]
            mask_ok = attention_mask is None or (attention_mask.dtype == np.float32 and not attention_mask.requires_grad and
                                                 tuple(attention_mask.shape) in ((b, cache.capacity), (1, cache.capacity)))
            if hasattr(hidden, "self_attention_extend") and mask_ok and hidden.self_attention_extend_supported(self.query.weight, self.h, cache.capacity):
                extra = {"mask": attention_mask} if attention_mask is not None else {}
                if getattr(cache, "kv_dtype", None) is not None:
                    extra["kv_dtype"] = cache.kv_dtype          # int16 pools of bfloat16 words: the bf16 paged launch
                context = hidden.self_attention_extend(self.query.weight, self.query.bias, self.key.weight, self.key.bias, self.value.weight,
                                                       self.value.bias, cache.k[index], cache.v[index], cache.pos, heads=self.h,
                                                       scale=math.sqrt(self.d) ** -1, count=count, block_table=cache.block_table,
                                                       block_size=cache.block_size, **extra)
                return context, None
            return self._paged_composite(hidden, attention_mask, cache, index, count)
        if cu is not None:
            assert count is None, "cu= (token-packed rows) and count= (a count per batch row) exclude each other"
            assert getattr(cache, "per_row", False), "cu= takes a cache with a position per sequence: nn.KVCache(..., per_row=True)"
            assert hidden.shape[0] == 1 and tuple(cu.shape) == (cache.batch + 1,), \
                "cu= goes with token rows (1, T, hidden) and %d + 1 words, got %s and %s" % (cache.batch, tuple(hidden.shape), tuple(cu.shape))
            m_max = min(hidden.shape[1], cache.capacity)
            mask_ok = attention_mask is None or (attention_mask.dtype == np.float32 and not attention_mask.requires_grad and
                                                 tuple(attention_mask.shape) in ((cache.batch, cache.capacity), (1, cache.capacity)))
            if hasattr(hidden, "self_attention_extend") and mask_ok and \
                    hidden.self_attention_extend_supported(self.query.weight, self.h, cache.capacity, m_max):
                extra = {"mask": attention_mask} if attention_mask is not None else {}
                context = hidden.self_attention_extend(self.query.weight, self.query.bias, self.key.weight, self.key.bias, self.value.weight,
                                                       self.value.bias, cache.k[index], cache.v[index], cache.pos, heads=self.h,
                                                       scale=math.sqrt(self.d) ** -1, cu=cu, m_max=m_max, **extra)
                return context, None
            return self._packed_composite(hidden, attention_mask, cache, index, cu)
        b, m = hidden.shape[0], hidden.shape[1]
        scale = math.sqrt(self.d) ** -1
        k_cache, v_cache = cache.k[index], cache.v[index]
        mask_ok = attention_mask is None or (attention_mask.dtype == np.float32 and not attention_mask.requires_grad and
                                             tuple(attention_mask.shape) in ((b, cache.capacity), (1, cache.capacity)))
        if hasattr(hidden, "self_attention_extend") and mask_ok and hidden.self_attention_extend_supported(self.query.weight, self.h, cache.capacity):
            # the backend's one-node form: one launch for the three projections, one for the attention, which reads the position on
            # the device and writes the m new key / value rows into the cache itself
            extra = {"mask": attention_mask} if attention_mask is not None else {}
            context = hidden.self_attention_extend(self.query.weight, self.query.bias, self.key.weight, self.key.bias, self.value.weight,
                                                   self.value.bias, k_cache, v_cache, cache.pos, heads=self.h, scale=scale, **extra, **counted)
            return context, None
        if getattr(cache, "per_row", False):
            return self._rows_composite(hidden, attention_mask, cache, index, **counted)
        # the same over the tensor API: the host mirror of the position slices the cache
        t = cache.length
        n = t + m
        assert n <= cache.capacity, "the cache holds %d of %d positions: no room for %d more" % (t, cache.capacity, m)
        q, k, v = self.query(hidden), self.key(hidden), self.value(hidden)
        k_cache[:, t:n] = k
        v_cache[:, t:n] = v
        q = q.reshape(b, m, self.h, self.d).transpose(0, 2, 1, 3)
        k = k_cache[:, :n].reshape(b, n, self.h, self.d).transpose(0, 2, 3, 1)
        v = v_cache[:, :n].reshape(b, n, self.h, self.d).transpose(0, 2, 1, 3)
        scores = (q @ k) / math.sqrt(self.d)
        if attention_mask is not None:
            mask = attention_mask[:, :n]
            scores = scores + ((1.0 - mask.reshape(mask.shape[0], 1, 1, n)) * -10000.0).detach()
        scores = scores + ((1.0 - self._triangle_behind(scores, t, m)) * -10000.0).detach()
        probs = scores.softmax(axis=-1)
        return (probs @ v).transpose(0, 2, 1, 3).reshape(b, m, self.h * self.d), probs

    def forward(self, hidden, attention_mask=None, cache=None, index=None, append=False, count=None, cu=None):
        """cache (nn.KVCache) and index (this layer's): with tokens in the cache, `hidden` is one new token per sequence (`_decode`);
        with an empty one, the prompt takes the path below and its keys and values become the cache's first rows.  append=True:
        `hidden` is m >= 1 new tokens per sequence behind whatever the cache holds (`_extend`), count= its tokens per sequence, or
        - cu= - the token-packed rows of all cache slots"""
        assert (count is None and cu is None) or (cache is not None and append), "count= and cu= go with cache= and append=True"
        if cache is not None and append:
            assert self.causal, "appending to a cache takes a causal model"
            return self._extend(hidden, attention_mask, cache, index, **({} if count is None else {"count": count}), **({} if cu is None else {"cu": cu}))
        if cache is not None and cache.length > 0:
            assert self.causal and hidden.shape[1] == 1, "a decode step is one token per sequence of a causal model"
            return self._decode(hidden, attention_mask, cache, index)
        b, s, _ = hidden.shape
        # a padded batch (a mask) or a length the plain kernels do not take (no multiple of 32) goes to the backend's masked forms,
        # if it has them and the mask is what they read: a (b, s) or (1, s) float32 constant
        masked = attention_mask is not None or s % 32 != 0
        # beyond 128 positions (up to 512) the backend's long forms take over, with or without a mask, under the same conditions
        long = s > 128
        if masked or long:
            fused = hasattr(hidden, "long_attention" if long else "masked_attention") and (attention_mask is None or (
                attention_mask.dtype == np.float32 and not attention_mask.requires_grad and tuple(attention_mask.shape) in ((b, s), (1, s))))
            extra = {"long": True} if long else {"masked": True}
        else:
            fused, extra = hasattr(hidden, "self_attention"), {}
        scale = math.sqrt(self.d) ** -1
        # dropout of the probabilities sits between the softmax and the product with the values: the backends' one-launch forms
        # draw the composite's mask inside the kernel (one call of the stream); without `dropout=` they are the forms as they were
        drop = {"dropout": self.dropout.p} if self.training and self.dropout.p > 0 else {}
        # the causal mask is a flag of the same forms (their forward launch leaves the keys j > i out); without it, the calls of before
        if self.causal:
            extra["causal"] = True
            drop = dict(drop, causal=True)
        if fused and hidden.self_attention_supported(self.query.weight, self.h, **extra):
            # the backend's one-node form of this whole method: one launch for the three projections, one for the attention
            extra = {"mask": attention_mask} if attention_mask is not None else {}
            context = hidden.self_attention(self.query.weight, self.query.bias, self.key.weight, self.key.bias,
                                            self.value.weight, self.value.bias, heads=self.h, scale=scale, **extra, **drop)
            if cache is not None:
                # the projection launch's q | k | v buffer: its key and value columns go to the cache on the device
                width, qkv = self.h * self.d, context.attention_qkv
                cache.fill(index, qkv[:, :, width:2 * width], qkv[:, :, 2 * width:])
            return context, context.attention_probs
        q, k, v = self.query(hidden), self.key(hidden), self.value(hidden)
        if cache is not None:
            cache.fill(index, k, v)
        flag = {"causal": True} if self.causal else {}
        if fused and (q.long_attention_supported(self.h, **flag) if long else
                      q.masked_attention_supported(self.h, **flag) if masked else q.attention_supported(self.h, **flag)):
            # the backend's one-launch form of everything below (scores, scaling, softmax, context), forward and backward
            context = q.long_attention(k, v, heads=self.h, scale=scale, mask=attention_mask, **drop) if long else \
                q.masked_attention(k, v, heads=self.h, scale=scale, mask=attention_mask, **drop) if masked else \
                q.attention(k, v, heads=self.h, scale=scale, **drop)
            return context, context.attention_probs
        # head split: (b, s, h*d) -> (b, h, s, d) as stride permutations, no copies
        q = q.reshape(b, s, self.h, self.d).transpose(0, 2, 1, 3)
        k = k.reshape(b, s, self.h, self.d).transpose(0, 2, 3, 1)
        v = v.reshape(b, s, self.h, self.d).transpose(0, 2, 1, 3)
        scores = q @ k
        if attention_mask is None and not self.causal and hasattr(scores, "scaled_softmax"):
            # the backend's one-kernel form of the two lines below: the same x * sqrt(d)**-1, rounded to fp32, then softmax
            probs = scores.scaled_softmax(math.sqrt(self.d) ** -1)
        else:
            scores = scores / math.sqrt(self.d)
            if attention_mask is not None:
                # (b, s) -> (b, 1, 1, s); for batch 1 this is the reference's (1, 1, 1, s) (bert.py:82, which breaks for b > 1)
                mask = attention_mask.reshape(attention_mask.shape[0], 1, 1, attention_mask.shape[1])
                scores = scores + ((1.0 - mask) * -10000.0).detach()
            if self.causal:
                # the same line for the keys j > i of query i: exp underflows to exactly 0 there; -0.0 for a visible key changes no bit
                scores = scores + ((1.0 - self._lower_triangle(scores, s)) * -10000.0).detach()
            probs = scores.softmax(axis=-1)
        context = (self.dropout(probs) @ v).transpose(0, 2, 1, 3).reshape(b, s, self.h * self.d)
        return context, probs


class BertAttention(nn.Module):
    def __init__(self, hidden_size, num_attention_heads, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, causal=False):
        nn.Module.__init__(self)
        self.self = BertSelfAttention(hidden_size, num_attention_heads, attention_probs_dropout_prob, causal=causal)
        self.dropout = nn.Dropout(hidden_dropout_prob)
        self.output = nn.Module()
        self.output.dense = nn.Linear(hidden_size, hidden_size)
        self.output.LayerNorm = nn.LayerNorm(hidden_size)

    def forward(self, hidden_in, attention_mask=None, cache=None, index=None, append=False, count=None, cu=None):
        if cache is None:
            hidden, probs = self.self(hidden_in, attention_mask=attention_mask)
        elif append:
            hidden, probs = self.self(hidden_in, attention_mask=attention_mask, cache=cache, index=index, append=True,
                                      **({} if count is None else {"count": count}), **({} if cu is None else {"cu": cu}))
        else:
            hidden, probs = self.self(hidden_in, attention_mask=attention_mask, cache=cache, index=index)
        if self.training and self.dropout.p > 0:
            # dropout sits between the product and the residual addition, so the addition leaves the GEMM's epilogue
            norm = self.output.LayerNorm
            if hasattr(hidden, "dropout_add_layer_norm"):
                # the backend's one-launch form of dropout, addition and LayerNorm: the mask is drawn where the kernel loads its row
                return self.output.dense(hidden).dropout_add_layer_norm(hidden_in, norm.weight, norm.bias, self.dropout.p, norm.eps), probs
            hidden = self.dropout(self.output.dense(hidden), residual=hidden_in)
        else:
            hidden = self.output.dense(hidden, residual=hidden_in)                        # dense(hidden) + hidden_in
        return self.output.LayerNorm(hidden), probs


class BertLayer(nn.Module):
    def __init__(self, hidden_size, intermediate_size, num_attention_heads, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                 causal=False):
        nn.Module.__init__(self)
        self.attention = BertAttention(hidden_size, num_attention_heads, hidden_dropout_prob, attention_probs_dropout_prob, causal=causal)
        self.dropout = nn.Dropout(hidden_dropout_prob)
        self.intermediate = nn.Module()
        self.intermediate.dense = nn.Linear(hidden_size, intermediate_size)
        self.output = nn.Module()
        self.output.dense = nn.Linear(intermediate_size, hidden_size)
        self.output.LayerNorm = nn.LayerNorm(hidden_size)

    def forward(self, hidden, attention_mask=None, cache=None, index=None, append=False, count=None, cu=None):
        if cache is None:
            hidden, probs = self.attention(hidden, attention_mask)
        elif append:
            hidden, probs = self.attention(hidden, attention_mask, cache=cache, index=index, append=True, **({} if count is None else {"count": count}),
                                           **({} if cu is None else {"cu": cu}))
        else:
            hidden, probs = self.attention(hidden, attention_mask, cache=cache, index=index)
        if self.training and self.dropout.p > 0:
            if hasattr(hidden, "feed_forward") and hasattr(hidden, "dropout_add_layer_norm"):
                # the one-node feed-forward without its residual, then dropout, addition and LayerNorm in one launch
                up, down, norm = self.intermediate.dense, self.output.dense, self.output.LayerNorm
                out = hidden.feed_forward(up.weight, up.bias, down.weight, down.bias)
                return out.dropout_add_layer_norm(hidden, norm.weight, norm.bias, self.dropout.p, norm.eps), probs
            hidden = self.dropout(self.output.dense(gelu(self.intermediate.dense(hidden))), residual=hidden)
        elif hasattr(hidden, "feed_forward"):
            # the backend's one-node form of the line below: gelu and residual in the products' epilogues, four launches for six
            up, down = self.intermediate.dense, self.output.dense
            hidden = hidden.feed_forward(up.weight, up.bias, down.weight, down.bias, hidden)
        else:
            hidden = self.output.dense(gelu(self.intermediate.dense(hidden)), residual=hidden)  # hidden + dense(...)
        return self.output.LayerNorm(hidden), probs


class BertModel(nn.Module):
    def __init__(self, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, vocab_size,
                 max_position_embeddings, type_vocab_size, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, causal=False,
                 **unused):
        """`causal=True`: every layer's attention is causal - with the next-token objective (`clm_forward_backward`) a decoder-style
        language model of the same parameters"""
        nn.Module.__init__(self)
        self.embeddings = BertEmbedding(hidden_size, vocab_size, max_position_embeddings, type_vocab_size, hidden_dropout_prob)
        self.encoder = nn.Module()
        self.encoder.layer = nn.ModuleList(*[BertLayer(hidden_size, intermediate_size, num_attention_heads, hidden_dropout_prob,
                                                       attention_probs_dropout_prob, causal=causal)
                                             for _ in range(num_hidden_layers)])

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, cache=None, append=False, count=None, token_positions=None, cu=None):
        assert (count is None and token_positions is None and cu is None) or (cache is not None and append), \
            "count=, cu= and token_positions= go with cache= and append=True"
        if isinstance(cache, nn.PagedKVCache):
            assert append and count is not None and cu is None, \
                "an nn.PagedKVCache serves the count= append path only: model(ids, cache=paged, append=True, count=...) - not the prompt / one-token " \
                "decode route (no append=True) and not token-packed rows (cu=)" + _bf16_refusal(cache)
        if cache is not None:
            if append:
                if cu is not None:
                    return self._forward_packed(input_ids, attention_mask, token_type_ids, cache, count, token_positions, cu)
                return self._forward_append(input_ids, attention_mask, token_type_ids, cache, count, token_positions)
            return self._forward_cached(input_ids, attention_mask, token_type_ids, cache)
        assert not append, "append=True goes with a cache"
        hidden = self.embeddings(input_ids, token_type_ids=token_type_ids)
        for layer in self.encoder.layer:
            hidden, _ = layer(hidden, attention_mask=attention_mask)
        return hidden

    def _forward_append(self, input_ids, attention_mask, token_type_ids, cache, count=None, token_positions=None):
        """inference with an nn.KVCache that may hold tokens already, outside the tape: `input_ids` (b, m) are the next m >= 1
        tokens at the cache's position, whatever it is (attention_mask: None or (b, capacity) over the cache's rows, as a decode
        step reads it).  Their keys and values become the cache's next m rows and every one of the m rows comes back; the caller
        moves the position on with `cache.advance(m)`.
        count (int32 (b,), a cache with a position per sequence): sequence r has count[r] real tokens among its m rows - a step
        that mixes decoding (1), prefilling (up to m) and idle (0) sequences.  Only the real tokens' keys and values reach the
        cache and only they have to fit it; the rows behind them come back as whatever the layers make of an attention context
        of zeros - nobody reads them.  The caller moves the positions on (`cache.advance(count)`, or `serve_commit`).
        token_positions (int32 (b, m)): the position ids to embed at, in place of `cache.positions(m)` - nn.RequestPool's, which
        are 0 where a row holds no token and so never index past the position table"""
        b, m = input_ids.shape
        positions = self.embeddings.position_embeddings.weight.shape[0]
        assert cache.layers == len(self.encoder.layer) and cache.batch == b, "the cache was made for %d layers and a batch of %d" % (cache.layers, cache.batch)
        if count is not None or token_positions is not None:
            assert getattr(cache, "per_row", False), "count= / token_positions= take a cache with a position per sequence: nn.KVCache(..., per_row=True)"
            assert m >= 1 and cache.capacity <= positions and (token_positions is not None or cache.capacity + m - 1 <= positions), \
                "a cache of %d positions and rows of %d tokens reach position %d of %d position embeddings: pass token_positions=" % (
                    cache.capacity, m, cache.capacity + m - 1, positions)
            counted = {} if count is None else {"count": count}
            with light.no_grad():
                hidden = self.embeddings(input_ids, token_type_ids=token_type_ids,
                                         token_positions=cache.positions(m) if token_positions is None else token_positions)
                for index, layer in enumerate(self.encoder.layer):
                    hidden, _ = layer(hidden, attention_mask=attention_mask, cache=cache, index=index, append=True, **counted)
            return hidden
        if getattr(cache, "per_row", False):
            # a position per sequence: checked on the host where the mirror is valid, by the launches' own bounds checks otherwise
            assert m >= 1 and cache.capacity <= positions and (cache.lengths is None or (cache.lengths + m <= cache.capacity).all()), \
                "the cache holds %s of its %d positions: %d more tokens do not fit every row" % (
                    None if cache.lengths is None else cache.lengths.tolist(), cache.capacity, m)
        else:
            assert m >= 1 and cache.length + m <= cache.capacity, \
                "the cache holds %d of its %d positions: %d more tokens do not fit" % (cache.length, cache.capacity, m)
            assert cache.length + m <= positions, \
                "%d tokens behind the %d in the cache exceed the model's %d position embeddings" % (m, cache.length, positions)
        with light.no_grad():
            hidden = self.embeddings(input_ids, token_type_ids=token_type_ids, token_positions=cache.positions(m))
            for index, layer in enumerate(self.encoder.layer):
                hidden, _ = layer(hidden, attention_mask=attention_mask, cache=cache, index=index, append=True)
        return hidden

    def _forward_packed(self, input_ids, attention_mask, token_type_ids, cache, count, token_positions, cu):
        """`_forward_append` for a TOKEN-PACKED step: `input_ids` (1, T) are the step's tokens of all `cache.batch` slots and cu
        (int32 (slots + 1,)) says whose they are - slot s owns rows cu[s] .. cu[s + 1] - 1, behind its own position; rows
        >= cu[slots] belong to nobody.  token_positions (int32 (1, T)) are the position ids to embed at (nn.RequestPool's: 0 where
        a row holds no token).  Embeddings, Linears, LayerNorms and the feed-forward block run on T rows, whatever the slots
        hold; attention_mask: None, or (slots, capacity) over the cache's rows.  Every one of the T rows comes back; the caller
        moves the positions on (`serve_commit_packed`)"""
        assert count is None, "cu= (token-packed rows) and count= (a count per batch row) exclude each other"
        assert getattr(cache, "per_row", False), "cu= takes a cache with a position per sequence: nn.KVCache(..., per_row=True)"
        positions = self.embeddings.position_embeddings.weight.shape[0]
        assert len(input_ids.shape) == 2 and input_ids.shape[0] == 1 and input_ids.shape[1] >= 1, \
            "a token-packed step takes ids of shape (1, T), got %s" % (tuple(input_ids.shape),)
        assert cache.layers == len(self.encoder.layer) and tuple(cu.shape) == (cache.batch + 1,), \
            "the cache was made for %d layers and %d slots: cu has slots + 1 words, got %s" % (cache.layers, cache.batch, tuple(cu.shape))
        assert token_positions is not None and tuple(token_positions.shape) == tuple(input_ids.shape) and cache.capacity <= positions, \
            "a token-packed step takes token_positions= of the ids' shape (1, T), and a cache within the %d position embeddings" % positions
        with light.no_grad():
            hidden = self.embeddings(input_ids, token_type_ids=token_type_ids, token_positions=token_positions)
            for index, layer in enumerate(self.encoder.layer):
                hidden, _ = layer(hidden, attention_mask=attention_mask, cache=cache, index=index, append=True, cu=cu)
        return hidden

    def _forward_cached(self, input_ids, attention_mask, token_type_ids, cache):
        """inference with an nn.KVCache, outside the tape.  An empty cache: `input_ids` (b, s0) is the prompt - the causal forward
        as without a cache (attention_mask: None or (b, s0)), whose keys and values fill rows 0 .. s0 - 1 of every layer's cache
        on the device; the position becomes s0.  Otherwise `input_ids` (b, 1) is the token at the cache's position (attention_mask:
        None or (b, capacity) over the cache's rows); the caller moves the position on with `cache.advance()`"""
        b, s = input_ids.shape
        assert cache.layers == len(self.encoder.layer) and cache.batch == b, "the cache was made for %d layers and a batch of %d" % (cache.layers, cache.batch)
        prefill = cache.length == 0
        assert prefill or s == 1, "the cache holds %d positions: a decode step takes one token per sequence, got %d" % (cache.length, s)
        assert s <= cache.capacity, "a prompt of %d tokens does not fit a cache of %d positions" % (s, cache.capacity)
        with light.no_grad():
            if prefill:
                hidden = self.embeddings(input_ids, token_type_ids=token_type_ids)
            else:
                hidden = self.embeddings(input_ids, token_type_ids=token_type_ids, token_position=cache.pos)
            for index, layer in enumerate(self.encoder.layer):
                hidden, _ = layer(hidden, attention_mask=attention_mask, cache=cache, index=index)
            if prefill:
                # (a cache with a position per sequence: every row holds s tokens until the caller says otherwise - set_lengths)
                cache.set_length(s)
        return hidden


class BertForMaskedLM(nn.Module):
    def __init__(self, hidden_size, vocab_size, decoder_precision=None, **config):
        """`decoder_precision="bf16"`: the product onto the vocabulary and its two gradient products round their operands to
        bfloat16 on the way into the matrix cores (nn.Linear's `precision`); nothing else in the model changes"""
        nn.Module.__init__(self)
        self.bert = BertModel(hidden_size=hidden_size, vocab_size=vocab_size, **config)
        self.cls = nn.Module()
        self.cls.predictions = nn.Module()
        self.cls.predictions.transform = nn.Module()
        self.cls.predictions.transform.dense = nn.Linear(hidden_size, hidden_size)
        self.cls.predictions.transform.LayerNorm = nn.LayerNorm(hidden_size)
        self.cls.predictions.decoder = nn.Linear(hidden_size, vocab_size, bias=False, precision=decoder_precision)
        self.cls.predictions.bias = light.zeros(vocab_size)

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, masked_positions=None, cache=None, append=False, count=None,
                token_positions=None, cu=None):
        if cache is not None:
            # inference through an nn.KVCache (BertModel._forward_cached, append=True: _forward_append): the logits of every row
            # given, outside the tape
            extra = {"append": True} if append else {}
            if count is not None:
                extra["count"] = count
            if token_positions is not None:
                extra["token_positions"] = token_positions
            if cu is not None:
                extra["cu"] = cu
            h = self.bert(input_ids=input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, cache=cache, **extra)
            with light.no_grad():
                return self.head(h)
        h = self.bert(input_ids=input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids)
        if masked_positions is not None:
            # only the positions to predict go through the head: a constant int tensor of flat indices into the (b * s) token rows,
            # of static length (b * max_predictions; a padded slot may name any row - its label carries the loss's ignore_index).
            # The logits then have len(masked_positions) rows; the gather's backward scatter-adds into the hidden rows
            h = h.reshape(-1, h.shape[-1])[masked_positions]
        return self.head(h)

    def head(self, h):
        t = self.cls.predictions.transform
        h = t.LayerNorm(gelu(t.dense(h)))
        return self.cls.predictions.decoder(h) + self.cls.predictions.bias


def forward_backward(model, ids):
    logits = model(ids)
    loss = (logits * logits).mean()
    for p in model.parameters():
        p.zero_grad()
    loss.backward()
    return loss


MASK_TOKEN, SPECIAL_TOKENS = 103, (0, 100, 101, 102)          # [MASK]; [PAD], [UNK], [CLS], [SEP] of the public BERT vocabulary


def mlm_forward_backward(model, ids, p=0.15, accuracy_total=None):
    """one masked-LM step: mask the batch from the backend's random stream (on the device for HipTensors - inside a captured
    graph every replay masks a fresh batch), predict, and average the loss over the selected positions only.  With
    `accuracy_total` - an int64 tensor {correct, counted} - the step's masked tokens predicted right are added to it."""
    vocab = model.cls.predictions.decoder.weight.shape[0]
    masked, labels = light.data.mask_tokens(ids, p, MASK_TOKEN, vocab, special_ids=SPECIAL_TOKENS, ignore_index=-100)
    logits = model(masked)
    loss = light.loss.cross_entropy(logits.reshape(-1, vocab), labels.reshape(-1), ignore_index=-100)
    if accuracy_total is not None:
        light.metrics.accuracy(logits.reshape(-1, vocab), labels.reshape(-1), ignore_index=-100, into=accuracy_total)
    for q in model.parameters():
        q.zero_grad()
    loss.backward()
    return loss


def clm_forward_backward(model, ids):
    """one causal-LM step of a model built with `causal=True`: position i predicts token i + 1 from the tokens up to i; the last
    position has no label.  The labels are made on the ids' own backend (no host read: a captured step shifts what the ids hold
    at each replay)."""
    vocab = model.cls.predictions.decoder.weight.shape[0]
    labels = light.data.next_token_labels(ids, ignore_index=-100)
    logits = model(ids)
    loss = light.loss.cross_entropy(logits.reshape(-1, vocab), labels.reshape(-1), ignore_index=-100)
    for q in model.parameters():
        q.zero_grad()
    loss.backward()
    return loss


def decode_mask(attention_mask, capacity):
    """a key-padding mask (b, s0) over a prompt as a decode step reads it: (b, capacity) over the cache's rows, ones behind the
    prompt (a generated token is never padding); made on the mask's own backend"""
    if attention_mask is None:
        return None
    b, s0 = attention_mask.shape
    full = attention_mask.__class__.from_numpy(np.ones((b, capacity), dtype=attention_mask.dtype), requires_grad=False)
    full[:, :s0] = attention_mask
    return full


def next_token(logits, sampler=None, pool=None, eos=None):
    """(b, 1) int32 ids from (b, 1, vocab) logits: the argmax, or - sampler = (temperature, top_k, top_p) - one call of
    `logits.sample`, which draws from the backend's random stream (one launch in place of argmax + astype); or - a pool with a
    sampling table - one `logits.sample_rows`: slot s under the parameters and the seed of the request it holds, its counter the
    number of tokens that request has stored.  Nothing of the backend's stream is taken then.  A pool with a penalty table passes
    the logits through ONE `logits.penalize_rows` first, in place, whichever draw follows: slot s under the penalties and the
    history (prompt and stored tokens) of the request it holds; `eos` is the id its `min_new_tokens` keeps away.  A slot that is
    still prefilling draws a token nobody keeps: penalising its row is harmless and keeps the step one function.  A pool with
    `logprobs` scores the token behind whichever draw it was with ONE `logits.logprob_rows`, against the logits the draw read
    (penalised, in front of temperature, top-k and top-p), into column out_len[r] of the request r the slot holds - the caller's
    `pool.commit` moves out_len afterwards.  A prefilling slot writes column 0 of its request with a value nobody keeps: the
    request's first stored token overwrites it.  A pool with `guide` passes the logits through ONE `logits.guide_rows` behind the
    penalties and in front of whichever draw follows: the automaton of the request the slot holds absorbs the token that request
    stored last, the ids its state does not allow go to -inf and a forced id to +0.0 - so a forced end beats `min_new_tokens`, and
    `logprob_rows` scores the guided logits.  A prefilling slot has stored nothing: its state stays at the start"""
    if pool is not None and pool.penalties is not None:
        logits = logits.penalize_rows(pool.penalties, pool.req, pool.prompts, pool.prompt_len, pool.out, pool.out_len, eos=eos)
    if pool is not None and pool.guide is not None:
        logits = logits.guide_rows(*pool.guide, pool.req, pool.out, pool.out_len, pool.guide_state)
    if pool is not None and pool.sampling is not None:
        nxt = logits.sample_rows(pool.sampling, pool.req, pool.out_len)
    elif sampler is None:
        nxt = logits.argmax(-1).astype(np.int32)
    else:
        temperature, top_k, top_p = sampler
        nxt = logits.sample(temperature=temperature, top_k=top_k, top_p=top_p, dtype=np.int32)
    if pool is not None and pool.logprobs is not None:
        logits.logprob_rows(nxt, pool.logprobs, pool.req, pool.out_len, pool.logprob, pool.top_ids, pool.top_logprob)
    return nxt


def decode_step(model, cache, token, out_ids, mask=None, sampler=None):
    """one step, all on the ids' backend: the token (b, 1) at the cache's position goes through the model's decode forward
    and the head, the argmax of its logits (sampler=None: greedy) or a token sampled from them (sampler = (temperature, top_k,
    top_p)) is written back into `token` and into column position + 1 of `out_ids`, and the position moves on.  No host read,
    no value from the host: a captured step replays as it stands, and a sampling one draws fresh numbers at every replay."""
    logits = model(token, attention_mask=mask, cache=cache)                 # (b, 1, vocab)
    cache.advance()
    nxt = next_token(logits, sampler)                                       # (b, 1)
    token[:, :] = nxt
    out_ids[:, cache.pos] = nxt                                             # the column is the device position: s0 + steps done


def prefill_in_pieces(model, cache, ids32, mask, piece):
    """(b, s0) ids through the append path (`model.bert(..., cache=cache, append=True)`) in pieces of at most `piece` tokens,
    behind whatever the cache holds: each piece attends to the cache's rows and to itself, so the probabilities a layer holds at
    a time are (b, heads, piece, capacity), not (b, heads, s0, s0).  Returns the hidden row (b, 1, hidden) of the last token -
    the only one the head is asked about; the position has moved on by s0.  mask: None or (b, capacity) over the cache's rows"""
    b, s0 = ids32.shape
    hidden, n, buffers = None, 0, {}
    for lo in range(0, s0, piece):
        n = min(piece, s0 - lo)
        if n == s0:
            ids = ids32
        else:
            # an id buffer per piece length (ids are constants of a forward: a slice made under no_grad would not say so)
            if n not in buffers:
                buffers[n] = ids32.__class__.from_numpy(np.zeros((b, n), np.int32), requires_grad=False)
            ids = buffers[n]
            ids[:, :] = ids32[:, lo:lo + n]
        hidden = model.bert(ids, attention_mask=mask, cache=cache, append=True)
        cache.advance(n)
    return hidden[:, n - 1:n]


def decode_step_rows(model, cache, token, out_ids, done, mask=None, sampler=None, eos=None):
    """`decode_step` for a cache with a position per sequence: the token (b, 1) of every sequence goes through the decode forward
    at its own position, and ONE `decode_commit` does the bookkeeping per row - a live row's position moves on, its new token
    becomes its input and the next column of its ids, a row that drew `eos` is marked in `done`; a finished row is recomputed at
    its frozen position (the same cache row, the same bits) and nothing of it is written.  No host read, one shape whatever has
    finished: a captured step replays as it stands."""
    logits = model(token, attention_mask=mask, cache=cache)                 # (b, 1, vocab)
    next_token(logits, sampler).decode_commit(token, out_ids, cache.pos, done, eos=eos)
    cache.committed(1, eos=eos is not None)


def prefill_rows_in_pieces(model, cache, ids32, lengths, mask, piece):
    """`prefill_in_pieces` for right-padded rows: (b, s0) ids of which `lengths[r]` lead row r, behind whatever the cache holds
    in each row.  Every piece is (b, n) for all rows - what a row has no tokens for is padding whose keys and values land beyond
    the row's position, where nothing reads them - and the position moves on by the row's own tokens of the piece.  Returns the
    hidden row (b, 1, hidden) of each row's LAST token, gathered on the device from the piece that holds it."""
    b, s0 = ids32.shape
    last, buffers = None, {}
    for lo in range(0, s0, piece):
        n = min(piece, s0 - lo)
        if n == s0:
            ids = ids32
        else:
            if n not in buffers:
                buffers[n] = ids32.__class__.from_numpy(np.zeros((b, n), np.int32), requires_grad=False)
            ids = buffers[n]
            ids[:, :] = ids32[:, lo:lo + n]
        hidden = model.bert(ids, attention_mask=mask, cache=cache, append=True)
        if last is None:
            last = hidden.__class__.from_numpy(np.zeros((b, 1, hidden.shape[2]), hidden.dtype), requires_grad=False)
        for r in range(b):
            if lo < lengths[r] <= lo + n:
                i = int(lengths[r]) - 1 - lo
                last[r:r + 1] = hidden[r:r + 1, i:i + 1]
        cache.advance(np.clip(lengths - lo, 0, n))
    return last


class NgramDrafter(object):
    """the drafter of `generate(speculate=k)`: prompt lookup.  A row's guess at its next tokens is the continuation of the most
    recent earlier occurrence of its last n-gram (max_ngram down to min_ngram tokens) in its own ids - no second model, no second
    cache.  It sits inside `speculate_commit`, the launch that also accepts the last step's drafts.  A drafter is whatever has
    this `commit`: given the tokens `tgt` (b, m) drawn from the step's logits, it moves `state` on to the next step's inputs."""

    def __init__(self, draft, max_ngram=3, min_ngram=1):
        assert int(draft) == draft and draft >= 1 and int(max_ngram) == max_ngram and int(min_ngram) == min_ngram and 1 <= min_ngram <= max_ngram, \
            "speculate=k drafts k >= 1 tokens per step from n-grams of 1 <= min_ngram <= max_ngram tokens"
        self.draft, self.max_ngram, self.min_ngram = int(draft), int(max_ngram), int(min_ngram)

    def commit(self, tgt, state, cache, eos=None):
        tgt.speculate_commit(state["ids"], state["count"], state["position_ids"], state["out_ids"], cache.pos, state["end"], state["done"],
                             state["stats"], self.draft, max_ngram=self.max_ngram, min_ngram=self.min_ngram, eos=eos)


def speculate_step(model, cache, state, drafter, mask=None, sampler=None, eos=None):
    """one step of `generate(speculate=k)`, all on the ids' backend and one shape whatever the rows hold: each row's last token and
    its drafts - `count` real tokens among m = k + 1 - go through the append forward at the row's own positions, a token is drawn
    from EVERY one of the b * m rows of logits (the argmax, or one call of `sample`), and ONE `speculate_commit` keeps what the
    model agrees with and lays out the next step.  No host read, no value from the host: a captured step replays as it stands."""
    logits = model(state["ids"], cache=cache, append=True, count=state["count"], token_positions=state["position_ids"], attention_mask=mask)
    drafter.commit(next_token(logits, sampler), state, cache, eos=eos)


def speculate_rows(model, cache, out_ids, first, end, drafter, steps, mask, sampler, eos, graph, poll, info):
    """the decoding loop of `generate(speculate=k)` behind the prefill: `first` (b, 1) is the prompt's own first token, the
    cache's positions are those of each row's last prompt token, `end` (b,) the last column a row may write"""
    cls, b, m = out_ids.__class__, out_ids.shape[0], drafter.draft + 1
    i32 = lambda a: cls.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)       # noqa: E731
    state = dict(ids=i32(np.zeros((b, m))), count=i32(np.ones(b)), position_ids=i32(np.zeros((b, m))), out_ids=out_ids, end=i32(end),
                 done=i32(np.zeros(b)), stats=i32(np.zeros(3)))
    # stats[0] as a tensor of its own that shares the word (indexing a tensor copies: the poll would be a launch and a read)
    if isinstance(getattr(state["stats"], "data", None), np.ndarray):
        finished = cls.from_numpy(state["stats"].data[0:1], requires_grad=False)
    else:
        from lightgrad_amd.autograd.hip.ops import _idx_view
        finished = _idx_view(state["stats"], (slice(0, 1),))
    # the first new token goes the way of every later one: a step of one real token per row whose commit lands it in the column
    # behind the prompt and lays out the first speculative step
    tgt = i32(np.zeros((b, m)))
    tgt[:, 0:1] = first
    drafter.commit(tgt, state, cache, eos=eos)
    # the positions move on the device by what is accepted: the host keeps an upper bound only, as after an end-of-sequence run
    cache.lengths, cache.length = None, int(np.max(end))
    taken = 0

    def all_done():
        return taken % poll == 0 and int(finished.numpy()[0]) == b          # a host READ of one word every `poll` steps

    with light.no_grad():
        if graph is None or steps == 0:
            while taken < steps:
                speculate_step(model, cache, state, drafter, mask, sampler, eos)
                taken += 1
                if all_done():
                    break
        else:
            # one step eagerly (greedy: no call of the random stream) - it loads the kernels and fills the memory pool -, then back to
            # where the first commit left off: every int tensor the step writes is restored from a copy on the device (the ids too:
            # a greedy step may keep more drafts than the sampled one that takes its place)
            def clone(t):
                c = cls.from_numpy(np.zeros(tuple(t.shape), np.int32), requires_grad=False)
                c[tuple(slice(None) for _ in t.shape)] = t
                return c
            mutated = [state[k] for k in ("ids", "count", "position_ids", "out_ids", "done", "stats")] + [cache.pos]
            saved = [clone(t) for t in mutated]
            speculate_step(model, cache, state, drafter, mask, None, eos)
            for t, s in zip(mutated, saved):
                t[tuple(slice(None) for _ in t.shape)] = s
            with graph.capture():
                speculate_step(model, cache, state, drafter, mask, sampler, eos)         # recorded, not run
            while taken < steps:
                graph.replay()
                taken += 1
                if all_done():
                    break
    if info is not None:
        totals = state["stats"].numpy()
        info.update(steps=taken, drafted=int(totals[1]), accepted=int(totals[2]))


def generate_rows(model, ids, max_new_tokens, lengths, eos_token_id, pad_token_id, attention_mask, cache, graph, sampler, prefill_chunk,
                  append, drafter=None, poll=4, info=None):
    """the per-row path of `generate` (see there): right-padded prompts with a length per row, rows that stop at `eos_token_id`;
    with a drafter, the speculative loop behind the same prefill"""
    b, s0 = ids.shape
    cls = ids.__class__
    lengths = np.full(b, s0, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    assert lengths.shape == (b,) and (lengths >= 1).all() and (lengths <= s0).all(), \
        "lengths: %d ints within 1 .. %d, the real tokens that lead each right-padded row" % (b, s0)
    eos = None if eos_token_id is None else int(eos_token_id)
    positions = model.bert.embeddings.position_embeddings.weight.shape[0]
    layer0 = model.bert.encoder.layer[0].attention.self
    width = int(lengths.max()) + max_new_tokens                         # columns of the result
    if cache is None:
        cache = nn.KVCache(len(model.bert.encoder.layer), b, s0 + max_new_tokens, layer0.h * layer0.d,
                           like=model.bert.embeddings.word_embeddings.weight, per_row=True)
    assert cache.per_row, "lengths= / eos_token_id= take a cache with a position per sequence: nn.KVCache(..., per_row=True)"
    if append:
        if cache.lengths is None:
            # rows stopped where only the device knows (a run with an end-of-sequence id): one read brings the mirror back
            cache.lengths = np.asarray(cache.pos.numpy(), np.int64)
            cache.length = int(cache.lengths.max())
        start = cache.lengths.copy()                                    # tokens in front of `ids`, per row
        assert attention_mask is None or tuple(attention_mask.shape) in ((b, cache.capacity), (1, cache.capacity))
        mask = attention_mask
    else:
        assert attention_mask is None, "right-padded prompts need no mask: under the causal rule a real token never sees the padding behind it"
        cache.reset()
        start, mask = np.zeros(b, np.int64), None
    assert ((start + s0 <= cache.capacity) & (start + lengths + max_new_tokens <= cache.capacity)).all() and cache.capacity <= positions, \
        "rows of %s tokens in the cache, %d appended (%s real) and %d new ones do not fit a cache of %d positions and a model of %d position embeddings" % (
            start.tolist(), s0, lengths.tolist(), max_new_tokens, cache.capacity, positions)
    ids32 = ids if ids.dtype == np.int32 else ids.astype(np.int32)
    # a column per position of a row's sequence (the commit writes column = the row's device position), padding everywhere else
    columns = int(start.max()) + width
    out_ids = cls.from_numpy(np.full((b, columns), int(pad_token_id), np.int32), requires_grad=False)
    for r in range(b):
        out_ids[r:r + 1, int(start[r]):int(start[r] + lengths[r])] = ids32[r:r + 1, :int(lengths[r])]
    token = cls.from_numpy(np.zeros((b, 1), np.int32), requires_grad=False)        # the id buffer every step reads and writes
    done = cls.from_numpy(np.zeros(b, np.int32), requires_grad=False)              # 1 where a row has drawn the end-of-sequence id
    with light.no_grad():
        if append or prefill_chunk is not None:
            last = prefill_rows_in_pieces(model, cache, ids32, lengths, mask, s0 if prefill_chunk is None else int(prefill_chunk))
        else:
            hidden = model.bert(ids32, cache=cache)                                 # (b, s0, hidden); the padding's rows land beyond ...
            cache.set_lengths(lengths)                                              # ... each row's position
            rows = cls.from_numpy((np.arange(b) * s0 + lengths - 1).astype(np.int32), requires_grad=False)
            last = hidden.reshape(-1, hidden.shape[-1])[rows].reshape(b, 1, hidden.shape[-1])      # row lengths[r] - 1 of each sequence
        first = next_token(model.head(last), sampler)

    def result():
        if not append:
            return out_ids
        behind = cls.from_numpy(np.zeros((b, width), np.int32), requires_grad=False)        # row r from its own first appended column
        for r in range(b):
            behind[r:r + 1, :] = out_ids[r:r + 1, int(start[r]):int(start[r]) + width]
        return behind

    # the first new token goes the way of every later one: from position lengths - 1 the commit lands it in column lengths[r]
    cache.advance(-1)
    if drafter is not None:
        # row r may write the columns up to that of its last new token
        speculate_rows(model, cache, out_ids, first, start + lengths + max_new_tokens - 1, drafter, max_new_tokens - 1, mask, sampler, eos, graph,
                       int(poll), info)
        return result()
    first.decode_commit(token, out_ids, cache.pos, done, eos=eos)
    cache.committed(1, eos=eos is not None)

    steps = max_new_tokens - 1
    if graph is None or steps == 0:
        for _ in range(steps):
            decode_step_rows(model, cache, token, out_ids, done, mask, sampler, eos)
        return result()
    # as in `generate`: the first step once eagerly (greedy: no call of the random stream), then back to where the commit of the
    # first token left off - positions, flags and token are copies on the device, the host mirror a copy on the host
    def clone(t):
        c = cls.from_numpy(np.zeros(tuple(t.shape), np.int32), requires_grad=False)
        c[tuple(slice(None) for _ in t.shape)] = t
        return c
    saved = (clone(cache.pos), clone(done), clone(token), cache.length, None if cache.lengths is None else cache.lengths.copy())
    decode_step_rows(model, cache, token, out_ids, done, mask, None, eos)
    cache.pos[:] = saved[0]
    done[:] = saved[1]
    token[:, :] = saved[2]
    cache.length, cache.lengths = saved[3], saved[4]
    with graph.capture():
        decode_step_rows(model, cache, token, out_ids, done, mask, sampler, eos)    # recorded, not run: only the host mirror moved
    for i in range(steps):
        graph.replay()
        if i:
            cache.committed(1, eos=eos is not None)
    return result()


def beam_search_step(model, cache, state, num_beams, eos=None):
    """one step of `generate(num_beams=w)`, all on the ids' backend and one shape whatever the beams hold: the token (b * w, 1) of
    every beam goes through the decode forward at its own position (`decode_step_rows`' forward, at batch b * w), ONE `beam_step`
    keeps the best w continuations of every group of w beams - a finished beam competes as itself - and ONE `cache.reorder` makes
    the cache rows follow the beams that survived.  No host read, no value from the host: a captured step replays as it stands."""
    logits = model(state["token"], cache=cache)                             # (b * w, 1, vocab)
    logits.beam_step(state["scores"], state["parent"], state["token"], state["out_ids"], cache.pos, state["done"], state["stats"], num_beams, eos=eos)
    cache.reorder(state["parent"], num_beams)
    cache.committed(1, eos=True)


def generate_beams(model, ids, max_new_tokens, lengths, eos_token_id, pad_token_id, cache, graph, prefill_chunk, num_beams, length_penalty,
                   poll, beams):
    """the beam-search path of `generate` (see there): the beams of prompt g are rows g * w .. g * w + w - 1 of a per-row cache,
    best first.  The prompt is prefilled ONCE per prompt, at batch b, into a cache of b rows and exactly s0 positions; one strided
    copy per cache tensor takes it to the group leaders (rows g * w) of the big cache and one `cache.reorder` with every parent the
    leader to the other w - 1 rows."""
    b, s0 = ids.shape
    cls, w = ids.__class__, int(num_beams)
    rows = b * w
    lengths = np.full(b, s0, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    assert lengths.shape == (b,) and (lengths >= 1).all() and (lengths <= s0).all(), \
        "lengths: %d ints within 1 .. %d, the real tokens that lead each right-padded row" % (b, s0)
    eos = None if eos_token_id is None else int(eos_token_id)
    positions = model.bert.embeddings.position_embeddings.weight.shape[0]
    layer0 = model.bert.encoder.layer[0].attention.self
    weight = model.bert.embeddings.word_embeddings.weight
    layers, hidden_width = len(model.bert.encoder.layer), layer0.h * layer0.d
    assert weight.shape[0] >= w, "num_beams = %d exceeds the vocabulary of %d" % (w, weight.shape[0])
    columns = int(lengths.max()) + max_new_tokens                       # of the result, and of every beam's ids
    if cache is None:
        cache = nn.KVCache(layers, rows, s0 + max_new_tokens, hidden_width, like=weight, per_row=True)
    assert cache.per_row and cache.batch == rows, "num_beams = %d over %d prompts takes a per-row cache of %d rows: nn.KVCache(..., per_row=True)" % (w, b, rows)
    assert (lengths + max_new_tokens <= cache.capacity).all() and s0 <= cache.capacity <= positions, \
        "prompts of %s tokens (padded to %d) and %d new ones do not fit a cache of %d positions and a model of %d position embeddings" % (
            lengths.tolist(), s0, max_new_tokens, cache.capacity, positions)
    cache.reset()
    cache.num_beams = w
    ids32 = ids if ids.dtype == np.int32 else ids.astype(np.int32)
    i32 = lambda a: cls.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)       # noqa: E731
    leader = np.repeat(np.arange(b) * w, w)                             # the first row of each row's group
    scores0 = np.full((b, w), -np.inf, np.float32)
    scores0[:, 0] = 0.0                                                 # w copies of a prompt are one hypothesis: only the leader counts
    state = dict(token=i32(np.zeros((rows, 1))), out_ids=i32(np.full((rows, columns), int(pad_token_id))), done=i32(np.zeros(rows)),
                 parent=i32(leader), stats=i32(np.zeros(2)), scores=cls.from_numpy(scores0.reshape(rows), requires_grad=False))
    for g in range(b):                                                  # the prompt: the leader's row (a winner copies its parent's columns)
        state["out_ids"][g * w:g * w + 1, :int(lengths[g])] = ids32[g:g + 1, :int(lengths[g])]
    # stats[0] as a tensor of its own that shares the word (indexing a tensor copies: the poll would be a launch and a read)
    if isinstance(getattr(state["stats"], "data", None), np.ndarray):
        finished = cls.from_numpy(state["stats"].data[0:1], requires_grad=False)
    else:
        from lightgrad_amd.autograd.hip.ops import _idx_view
        finished = _idx_view(state["stats"], (slice(0, 1),))
    with light.no_grad():
        small = nn.KVCache(layers, b, s0, hidden_width, like=weight, per_row=True)
        if prefill_chunk is not None:
            last = prefill_rows_in_pieces(model, small, ids32, lengths, None, int(prefill_chunk))
        else:
            hidden = model.bert(ids32, cache=small)                                 # (b, s0, hidden), as in `generate_rows`
            at = cls.from_numpy((np.arange(b) * s0 + lengths - 1).astype(np.int32), requires_grad=False)
            last = hidden.reshape(-1, hidden.shape[-1])[at].reshape(b, 1, hidden.shape[-1])
        for layer in range(layers):
            cache.k[layer][0::w, :s0] = small.k[layer]
            cache.v[layer][0::w, :s0] = small.v[layer]
        cache.set_lengths(np.repeat(lengths, w))
        cache.reorder(state["parent"], w)                               # every row of a group holds its leader's prompt
        # the first new token goes the way of every later one: the head on the leader's row, once per beam, and a `beam_step` from
        # position lengths - 1 in which only the leaders' candidates are finite
        first = model.head(last.reshape(b, last.shape[-1])[i32(np.repeat(np.arange(b), w))].reshape(rows, 1, last.shape[-1]))
        cache.advance(-1)
        first.beam_step(state["scores"], state["parent"], state["token"], state["out_ids"], cache.pos, state["done"], state["stats"], w, eos=eos)
        cache.committed(1, eos=True)                                    # (no reorder: every row of a group holds the same prompt)
        steps, taken = max_new_tokens - 1, 0

        def all_done():
            return taken % poll == 0 and int(finished.numpy()[0]) == b          # a host READ of one word every `poll` steps

        if graph is None or steps == 0:
            while taken < steps:
                beam_search_step(model, cache, state, w, eos)
                taken += 1
                if all_done():
                    break
        else:
            # one step eagerly - it loads the kernels and fills the memory pool -, then back to where the first `beam_step` left
            # off: every tensor the step writes is restored from a copy on the device.  The cache rows need none: below each row's
            # position a group's rows are still equal, and a row's own position is rewritten by the forward of every step
            def clone(t):
                c = cls.from_numpy(np.zeros(tuple(t.shape), t.dtype), requires_grad=False)
                c[tuple(slice(None) for _ in t.shape)] = t
                return c
            mutated = [state[k] for k in ("scores", "parent", "token", "out_ids", "done", "stats")] + [cache.pos]
            saved, length = [clone(t) for t in mutated], cache.length
            beam_search_step(model, cache, state, w, eos)
            for t, s in zip(mutated, saved):
                t[tuple(slice(None) for _ in t.shape)] = s
            cache.length = length
            with graph.capture():
                beam_search_step(model, cache, state, w, eos)               # recorded, not run: only the host mirror moved
            while taken < steps:
                graph.replay()
                if taken:
                    cache.committed(1, eos=True)
                taken += 1
                if all_done():
                    break
        # the result: per prompt the beam with the largest scores / n ** length_penalty, n its new tokens (the end-of-sequence id
        # included) - the first of equals, like every argmax here
        n = (cache.pos + i32(-(np.repeat(lengths, w) - 1))).astype(np.float32)
        if length_penalty == 0:
            ranked = state["scores"]
        else:
            ranked = state["scores"] / (n if length_penalty == 1 else (n.log() * float(length_penalty)).exp())
        best = ranked.reshape(b, w).argmax(-1).astype(np.int32) + i32(np.arange(b) * w)
        # a slot keeps what it held beyond its beam's position (a finished beam may have moved into the slot of a longer one): the
        # result is padded there - mask = min(relu(pos + 1 - column), 1), in float32, which holds every id below 2^24 exactly
        chosen = state["out_ids"][best].astype(np.float32)
        reach = ((cache.pos[best] + 1).astype(np.float32).reshape(b, 1) - cls.from_numpy(np.arange(columns, dtype=np.float32), requires_grad=False)).relu()
        mask = 1.0 - (1.0 - reach).relu()
        result = (chosen * mask + (1.0 - mask) * float(int(pad_token_id))).astype(np.int32)
    if beams is not None:
        beams.update(sequences=state["out_ids"].reshape(b, w, columns), scores=state["scores"].reshape(b, w), steps=taken)
    return result


def generate(model, ids, max_new_tokens, attention_mask=None, cache=None, graph=None, temperature=None, top_k=0, top_p=1.0,
             prefill_chunk=None, append=False, lengths=None, eos_token_id=None, pad_token_id=0, speculate=None, max_ngram=3, min_ngram=1,
             poll=4, stats=None, num_beams=None, length_penalty=1.0, beams=None):
    """decoding of a model built with `causal=True`: (b, s0) prompt ids -> (b, s0 + max_new_tokens) int32 ids on the
    prompt's backend.  temperature=None is greedy; with a temperature every token - the prompt's own first one included - is
    `logits.sample(temperature, top_k, top_p)`, drawn from the backend's random stream (`light.manual_seed`): one call of the
    stream per token, eager or captured alike.  Guided decoding (`serve(guide=)`) is a keyword of `serve` alone: `generate`
    does not take it, and beams and speculation have no guides.
    The prompt is prefilled once through the causal forward, which fills an nn.KVCache (made here unless given: one of exactly
    s0 + max_new_tokens positions); every further token is one `decode_step` on the last position only.
    Nothing is read back to the host - the caller's `.numpy()` is the first read.  attention_mask: a key-padding mask (b, s0)
    over the prompt.  graph: an empty HipGraph (HipTensor only) - the decode step is captured into it once after the prefill
    and replayed for each of the max_new_tokens - 1 tokens behind the prompt's own.
    prefill_chunk=c: the prompt goes through the append path in pieces of at most c tokens (`prefill_in_pieces`) - the same
    tokens, with a layer's probabilities bounded by (b, heads, c, capacity).  append=True: `cache` (required) is NOT reset -
    `ids` are appended behind the `cache.length` tokens it already holds (a second turn of a conversation; one piece unless
    prefill_chunk is given) and decoding goes on from there; the result is the appended ids followed by the new ones, and
    attention_mask, if given, is (b, capacity) over the cache's rows as a decode step reads it.
    lengths= (a host sequence of b ints) or eos_token_id= select the per-row path, a ragged batch in one run: `ids` is (b, s0)
    RIGHT-padded and lengths[r] real tokens lead row r (default: s0 for every row).  The prompt goes through the causal forward
    without a mask - a real token never sees the padding behind it, and the padding's keys and values land in the cache beyond
    each row's position, where nothing reads them -, the head runs on row lengths[r] - 1 of each sequence, and every sequence
    is embedded and attends at its own positions (nn.KVCache(per_row=True); a cache given must be one): row r decodes as it does
    alone.  A row that draws eos_token_id stops: the result, (b, max(lengths) + max_new_tokens) filled with pad_token_id, holds
    each row's prompt, then its new tokens up to and including the end-of-sequence id.  A finished row keeps being recomputed at
    its frozen position (`decode_step_rows`), and the sampler draws for it too (one call of the stream per step): the step never
    changes shape and is captured once with graph=.  prefill_chunk= and append=True work as above, with pieces that are
    right-padded and a position that moves by `lengths` per row (append after a run with an end-of-sequence id reads the
    positions back once: only the device knows where the rows stopped).
    speculate=k >= 1 selects the per-row path too and decodes speculatively by prompt lookup: every step feeds a row's last token
    and up to k drafts - the continuation of the most recent earlier occurrence of the row's last n-gram (max_ngram down to
    min_ngram tokens) in its own ids - through ONE append forward of shape (b, k + 1) with a token count per row, draws a token
    from every row of logits, and ONE `speculate_commit` keeps the drafts the model agrees with plus one token of its own and looks
    up the next drafts (`speculate_step`, `NgramDrafter`): a row gains 1 .. k + 1 tokens per step.  The host reads one word every
    `poll` steps - the rows finished - and stops when it is b, or after max_new_tokens - 1 steps; graph= captures the step once.
    The result has the shape and padding of the per-row path; afterwards the cache's host mirror `lengths` is None and `length`
    an upper bound, as after an end-of-sequence run.  stats: a dict that receives `steps`, `drafted` and `accepted` (one more
    read, at the end).  Greedy, the tokens are those of the run without speculate= wherever no step is a near-tie (the (b, k + 1)
    forward rounds differently from the (b, 1) one).  Sampled, every one of the k + 1 rows is sampled and a draft is accepted when
    it EQUALS the sample: the drafts are a function of the prefix only, so every emitted token is a draw from the model's own
    distribution given its prefix and the output distribution is exact.  A sampled run repeats for a given seed, k and n-gram
    bounds (eager or captured); it does NOT reproduce the run without speculate=, because it takes one call of the random stream
    per step, not per token.
    num_beams=w (1 .. 8) selects beam search: b prompts occupy b * w rows of a per-row cache (a cache given must have that many),
    group g = rows g * w .. g * w + w - 1, best first.  The prompt is prefilled once per prompt at batch b and copied to its group;
    every step is the per-row decode forward at batch b * w, ONE `beam_step` that keeps the w best of the group's w * vocab
    continuations by cumulative log-probability (a beam that drew eos_token_id competes as itself and is never extended) and ONE
    `cache.reorder` that makes the cache rows follow the surviving beams (`beam_search_step`); graph= captures it once.  The host
    reads one word every `poll` steps - the groups whose beams have all finished - and stops when it is b, or after
    max_new_tokens - 1 steps.  The result has the shape and padding of the per-row path and holds, per prompt, the beam that
    maximises score / n ** length_penalty with n its new tokens (the end-of-sequence id included), the first of equals; it is
    picked on the device.  beams: a dict that receives `sequences` (b, w, columns) and `scores` (b, w) as tensors, and `steps`.
    lengths=, eos_token_id=, pad_token_id= and prefill_chunk= work as on the per-row path; temperature, speculate= and append=True
    are refused.  num_beams=1 is greedy decoding, up to near-ties (its scores come from a different launch than argmax's logits)."""
    assert not isinstance(cache, nn.PagedKVCache), "generate: an nn.PagedKVCache serves the count= append path only (serve): pass an nn.KVCache" + \
        _bf16_refusal(cache)
    if num_beams is not None:
        assert int(num_beams) == num_beams and 1 <= num_beams <= 8, "num_beams is an int within 1 .. 8 (got %s)" % (num_beams,)
        assert temperature is None, "beam search is deterministic: temperature= (sampling beams) is not supported with num_beams="
        assert speculate is None, "speculate= drafts for one sequence per row: it is not supported with num_beams="
        assert not append, "append=True (a second turn behind a filled cache) is not supported with num_beams="
        assert attention_mask is None, "right-padded prompts need no mask: pass lengths= with num_beams="
        assert max_new_tokens >= 1 and ids.shape[1] >= 1 and (prefill_chunk is None or prefill_chunk >= 1)
        assert model.bert.encoder.layer[0].attention.self.causal, "generate needs a model built with causal=True"
        assert int(poll) == poll and poll >= 1 and (beams is None or isinstance(beams, dict)), "poll is a number of steps >= 1, beams a dict"
        assert float(length_penalty) == length_penalty and length_penalty >= 0, "length_penalty is a number >= 0"
        return generate_beams(model, ids, max_new_tokens, lengths, eos_token_id, pad_token_id, cache, graph, prefill_chunk, int(num_beams),
                              float(length_penalty), int(poll), beams)
    if lengths is not None or eos_token_id is not None or speculate is not None:
        assert max_new_tokens >= 1 and ids.shape[1] >= 1 and (prefill_chunk is None or prefill_chunk >= 1)
        assert model.bert.encoder.layer[0].attention.self.causal, "generate needs a model built with causal=True"
        assert not append or cache is not None, "append=True continues a cache: pass the one that holds the tokens so far"
        sampler = None if temperature is None else (temperature, top_k, top_p)
        if speculate is None:
            return generate_rows(model, ids, max_new_tokens, lengths, eos_token_id, pad_token_id, attention_mask, cache, graph, sampler,
                                 prefill_chunk, append)
        assert int(poll) == poll and poll >= 1 and (stats is None or isinstance(stats, dict)), "poll is a number of steps >= 1, stats a dict"
        return generate_rows(model, ids, max_new_tokens, lengths, eos_token_id, pad_token_id, attention_mask, cache, graph, sampler,
                             prefill_chunk, append, drafter=NgramDrafter(speculate, max_ngram, min_ngram), poll=poll, info=stats)
    b, s0 = ids.shape
    positions = model.bert.embeddings.position_embeddings.weight.shape[0]
    layer0 = model.bert.encoder.layer[0].attention.self
    assert layer0.causal, "generate needs a model built with causal=True"
    assert max_new_tokens >= 1 and s0 >= 1
    assert prefill_chunk is None or prefill_chunk >= 1, "prefill_chunk is a number of tokens >= 1"
    assert not append or cache is not None, "append=True continues a cache: pass the one that holds the tokens so far"
    if cache is None:
        cache = nn.KVCache(len(model.bert.encoder.layer), b, s0 + max_new_tokens, layer0.h * layer0.d, like=model.bert.embeddings.word_embeddings.weight)
    start = cache.length if append else 0               # tokens in front of `ids`
    if append:
        assert start + s0 + max_new_tokens <= cache.capacity <= positions, \
            "%d tokens in the cache, %d appended and %d new ones need a cache of at least %d positions, and the model has %d position embeddings (cache: %d)" % (
                start, s0, max_new_tokens, start + s0 + max_new_tokens, positions, cache.capacity)
    else:
        assert s0 + max_new_tokens <= cache.capacity <= positions, \
            "a prompt of %d tokens and %d new ones need a cache of at least %d positions, and the model has %d position embeddings (cache: %d)" % (
                s0, max_new_tokens, s0 + max_new_tokens, positions, cache.capacity)
        cache.reset()
    end = start + s0                                    # the position of the first new token
    ids32 = ids if ids.dtype == np.int32 else ids.astype(np.int32)
    # a column per position of the cache's sequence (a step writes column = device position); what is returned starts at `ids`
    out_ids = ids.__class__.from_numpy(np.zeros((b, end + max_new_tokens), np.int32), requires_grad=False)
    out_ids[:, start:end] = ids32
    mask = attention_mask if append else decode_mask(attention_mask, cache.capacity)
    sampler = None if temperature is None else (temperature, top_k, top_p)
    # the prompt: every position at once; only its last row goes through the head
    token = ids.__class__.from_numpy(np.zeros((b, 1), np.int32), requires_grad=False)      # the id buffer every step reads and writes
    with light.no_grad():
        if append or prefill_chunk is not None:
            last = prefill_in_pieces(model, cache, ids32, mask, s0 if prefill_chunk is None else int(prefill_chunk))
        else:
            last = model.bert(ids32, attention_mask=attention_mask, cache=cache)[:, s0 - 1:s0]
        token[:, :] = next_token(model.head(last), sampler)                                 # the first new token, position `end`
    out_ids[:, end:end + 1] = token
    result = (lambda: out_ids[:, start:]) if start else (lambda: out_ids)       # taken when every column is written: a slice may be a copy
    steps = max_new_tokens - 1                        # the last new token is fed to nobody
    if graph is None or steps == 0:
        for _ in range(steps):
            decode_step(model, cache, token, out_ids, mask, sampler)
        return result()
    # the first step once eagerly - it loads the kernels, fills the memory pool and uploads the constants of a (b, 1) forward -,
    # then back to where the prefill left off: the recorded step writes the same row, token and column again.  This step is
    # greedy even when sampling (its token is overwritten): it must not take a call of the random stream, so that the replays
    # draw the calls the eager steps would; the prefill's own token has loaded the sampling kernel already
    decode_step(model, cache, token, out_ids, mask)
    cache.set_length(end)
    token[:, :] = out_ids[:, end:end + 1]
    with graph.capture():
        decode_step(model, cache, token, out_ids, mask, sampler)           # recorded, not run: the host mirror moved on, the device position not
    for i in range(steps):
        graph.replay()
        if i:
            cache.replayed()
    return result()


def serve_step(model, pool, sampler=None, eos=None):
    """one step of `serve`, all on the model's backend and the same function whatever the slots hold: the pool's (slots, chunk)
    ids go through the append forward with the pool's token count per slot - a decoding slot has 1 real token, a prefilling one
    up to `chunk`, an idle one none -, ONE gather takes each slot's last real row to the head, and ONE `serve_commit` stores the
    tokens drawn for the decoding slots, frees the slots whose request has finished, admits waiting requests to them and lays
    out the next step's ids.  No host read, no value from the host: a captured step replays as it stands.
    With a pool that has a token budget (`pool.cu`) the step is token-packed: the pool's (1, T) ids go through the append forward
    with `cu=`, T rows whatever the slots hold; gather, head, draw and commit (`serve_commit_packed`) follow as above."""
    if pool.cu is not None:
        hidden = model.bert(pool.ids, cache=pool.cache, append=True, cu=pool.cu, token_positions=pool.position_ids)
    else:
        hidden = model.bert(pool.ids, cache=pool.cache, append=True, count=pool.count, token_positions=pool.position_ids)
    width = hidden.shape[-1]
    rows = hidden.reshape(-1, width)[pool.last].reshape(pool.slots, 1, width)
    pool.commit(next_token(model.head(rows), sampler, pool, eos), eos=eos)


def fill_shared_prefix(model, pool, tokens):
    """the keys and values of the prefix every request shares, computed once: `tokens` (F * B of them) go through the paged append
    path itself in pieces of at most `pool.chunk` - as slot 0, whose table names blocks 0 .. F - 1 for the while; the other slots
    have no token.  Afterwards the table is -1 and the position 0 again: the blocks are in no table until `serve_commit_paged`
    gives them to every request it admits, they are not on the stack of free blocks, and nothing writes them again.  Host values
    are uploaded here, before the first step"""
    cache, slots, chunk = pool.cache, pool.slots, pool.chunk
    cls = type(cache.pos)
    i32 = lambda a: cls.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)        # noqa: E731
    table = np.full((slots, cache.max_blocks), -1, np.int32)
    table[0, :pool.prefix_blocks] = np.arange(pool.prefix_blocks)
    cache.block_table[:] = i32(table)
    for t in range(0, len(tokens), chunk):
        n = min(chunk, len(tokens) - t)
        ids, at, count, pos = (np.zeros((slots, chunk), np.int32), np.zeros((slots, chunk), np.int32), np.zeros(slots, np.int32), np.zeros(slots, np.int32))
        ids[0, :n], at[0, :n], count[0], pos[0] = tokens[t:t + n], t + np.arange(n), n, t
        cache.pos[:] = i32(pos)
        model.bert(i32(ids), cache=cache, append=True, count=i32(count), token_positions=i32(at))
    cache.block_table[:] = i32(np.full((slots, cache.max_blocks), -1))
    cache.pos.fill(0)


def serve(model, prompts, max_new_tokens, slots=8, chunk=32, eos_token_id=None, pad_token_id=0, graph=None, temperature=None, top_k=0,
          top_p=1.0, poll=8, lengths=None, cache=None, token_budget=None, num_blocks=None, block_size=16, shared_prefix=0, kv_dtype=None,
          seeds=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0, logprobs=None, guide=None):
    """continuous batching: N requests through `slots` cache slots, a finished slot refilled at once from the queue while the
    others go on decoding.  prompts: a list of N int sequences, or (N, P) right-padded ids (an array or a tensor) with lengths=;
    max_new_tokens: an int, or N ints - a budget per request.  Returns (out (N, G) int32 with G = the largest budget, filled with
    pad_token_id behind each request's tokens; out_len (N,) int32) on the model's backend, and a dict of statistics: `steps`.
    A request ends with eos_token_id (stored, then fed to nobody) or when its budget is used up.

    Every step is `serve_step`: prompts enter the cache in pieces of at most `chunk` tokens next to the slots that decode, one
    launch of attention per layer for all of them (csrc/extend.hip, a token count per slot), and the bookkeeping between two steps
    is one launch (csrc/serve.hip, `nn.RequestPool`).  The host reads ONE word every `poll` steps - the number of finished
    requests - and stops when it is N; nothing else is read back (the caller's `.numpy()` is the first read of the tokens).  Up
    to poll - 1 steps run after the last request has finished: every slot is idle then and nothing changes.  graph: an empty
    HipGraph - the first step runs eagerly (a real step), the second is captured and then replayed; no state is saved or
    restored, since every step is the same function of the device state.
    Greedy results depend on a request's own data only: not on slots, chunk or the order of admission.  With a temperature every
    step takes ONE call of the random stream for all slots, idle ones included, and a slot's numbers depend on its index: a
    sampled run is reproducible for a given seed, slots and chunk (eager or captured), but NOT independent of the schedule.
    The PER-REQUEST route IS independent of it: with seeds= (an int s - request r draws from the stream seeded (s + r) mod 2**64 -
    or N ints; seeds=None with a sequence among the parameters: s = the seed of the backend's generator, read once before the
    first step), or with temperature, top_k or top_p a sequence of N (scalars broadcast; a temperature of 0 is a greedy request),
    every request has its own parameters and its own random stream: its g-th token takes `random.sample_uniforms(seed, 0, g + 1)[g]`
    (`logits.sample_rows`, csrc/sample_rows.hip, driven by the pool's `req` and `out_len`).  A request's tokens are then
    `random.sample_tokens(seed, 0, its logits, T, k, p)` whatever slots, chunk, token_budget, num_blocks and the other requests
    are; the backend's generator is neither read by a step nor advanced; `stats` gains `per_request_sampling`.  A float
    temperature= without seeds= is the route above, unchanged.
    repetition_penalty, presence_penalty, frequency_penalty, min_new_tokens: each a scalar or one per request.  With any of them
    not neutral (1, 0, 0, 0) every step passes its logits through ONE `logits.penalize_rows` (csrc/penalize.hip) in front of the
    draw, driven by the pool's `req`, `prompts`, `prompt_len`, `out` and `out_len`; `stats` gains `penalties` and the step has
    exactly one kernel more.  The contract: the g-th token of request r is drawn from the logits behind its prompt and its first
    g tokens, passed through `random.penalize_logits` with that same history (the ids of prompt and tokens divided or multiplied
    by repetition_penalty, the tokens' logits lowered by frequency_penalty times their count and by presence_penalty, eos_token_id
    at -inf while fewer than min_new_tokens are stored).  So a request alone defines its tokens: they do not depend on slots,
    chunk, token_budget, num_blocks, block_size, shared_prefix or the other requests - for greedy and for per-request sampled
    requests; with kv_dtype="bf16" they are those of the rounded model, as before; the global temperature= route stays
    schedule-dependent, penalties or not.  min_new_tokens without eos_token_id is accepted and does nothing.  With every value
    neutral no table is built and the step is launch for launch what it was.
    logprobs: None, an int 0 .. 8 for every request, or one entry per request (None or -1: none for that request; 0: the
    log-probability of each of its tokens; k: also the k most likely ids of every step with theirs).  Every step then calls ONE
    `logits.logprob_rows` (csrc/logprob.hip) behind the draw - argmax, `sample` or `sample_rows`, penalised or not - and in front
    of the commit, driven by the pool's `req` and `out_len`: the step has exactly one kernel more and still no host read.
    `stats["logprobs"]` is a dict of three tensors on the model's backend, not read back: `token` float32 (N, G), `top_ids` int32
    (N, G, n) and `top` float32 (N, G, n) with n = max(the largest entry, 1); the returned tuple does not change.  The contract:
    column g < out_len[r] of request r holds `random.token_logprobs_rows` applied to the logits behind its prompt and its first
    g tokens - the logits the draw read: behind the penalties, in front of temperature, top-k and top-p -; columns from
    out_len[r] on, the entries behind a request's own k, and the rows of a request without log-probabilities hold the fills
    (+0.0, -1, +0.0).  The values do not depend on slots, chunk, token_budget, num_blocks, block_size or the other requests beyond
    the float32 rounding of the forward (with kv_dtype="bf16": of the rounded model); the ids in `top_ids` are exact wherever the
    gaps between the reference's ranks rule out a near-tie.  With logprobs=None nothing is built, `stats` has no such key and
    the step is launch for launch what it was.
    guide: None, one `light.guide.TokenAutomaton` for every request, or N entries that may include None - GUIDED DECODING: the
    automaton (`guide.allow_only`, `ban_sequences`, `one_of`, `stop_after`, or one built by hand) advances with every token the
    request stores, and the ids its state does not allow cannot be drawn; eos_token_id is allowed exactly in accepting states.
    `guide.compile_guides` lays the automata out once; every step then calls ONE `logits.guide_rows` (csrc/guide.hip) behind the
    penalties and in front of the draw - and so in front of `logprob_rows`, which scores the guided logits: the probabilities over
    the allowed ids - driven by the pool's `req`, `out`, `out_len` and `guide_state`; `stats` gains `guide` and the step has
    exactly one kernel more.  The contract: token g of request r is drawn from the logits behind its prompt and its first g
    tokens, passed through the penalties and then through `guide.guide_logits` in the state its own automaton reaches on those g
    tokens.  So a request alone defines its tokens, whatever slots, chunk, token_budget, num_blocks, block_size, shared_prefix and
    the other requests are (with kv_dtype="bf16": the tokens of the rounded model).  Hence `automaton.walk(tokens)` is never -1;
    a request that ended with eos has `automaton.accepts(tokens without the eos)`; a budget that ends it first leaves a valid
    prefix; an unguided request in a guided run has the tokens of the run without guide=.  A state that allows one id alone forces
    it (+0.0, log-probability 0.0), min_new_tokens or not.  An automaton of another vocabulary is refused by name, and so is one
    with a state that only an end can follow when no eos_token_id is given.  With guide=None nothing is built and the step is
    launch for launch what it was.  `generate` does not take the keyword.
    cache: an nn.KVCache(per_row=True) of `slots` rows to use (default: one whose capacity is the longest request's need).
    token_budget: None, or T >= slots - every step is TOKEN-PACKED: it has T token rows for all slots together in place of
    (slots, chunk) rows.  A decoding slot takes one row; the rows left go to the prefilling slots in slot order, in pieces of at
    most `chunk` (chunked prefill under a per-step token budget; csrc/serve_packed.hip, the packed launch of csrc/extend.hip).
    Eight decoding slots cost 8 rows of every Linear, not 8 * chunk.  Greedy results are the same tokens; `stats` gains
    `token_budget`.  Without it everything is as it was.
    num_blocks=N (or cache= an nn.PagedKVCache): the cache is PAGED - the keys and values lie in N blocks of `block_size` positions
    per layer, shared by all slots, in place of slots * capacity rows.  A request is admitted when the blocks of its whole life
    (prompt and budget) are free, holds exactly those, and returns them when it ends (csrc/serve_paged.hip; the attention launch
    reads the rows through the slot's table, csrc/paged.hip).  With few blocks fewer requests run at once - more steps, the same
    tokens.  N must hold the largest request.  shared_prefix=L declares that the first L tokens of every prompt are equal
    (asserted): their keys and values are computed ONCE, into F = min(L // block_size, (shortest prompt - 1) // block_size) full
    blocks that every slot's table names and nobody writes again, and every request starts at position F * block_size.  The step
    has the launches of the step without paging and is captured once with graph=; `stats` gains `num_blocks`, `block_size` and
    `prefix_blocks`.  token_budget= together with paging is refused.  Without num_blocks and a paged cache everything is as it was.
    kv_dtype="bf16" (with num_blocks=, or cache= an nn.PagedKVCache(kv_dtype="bf16")): the pools hold bfloat16 words, half the bytes
    (csrc/paged_bf16.hip).  Every key and value is attended to as r of what the projection produced (r = `bf16_round_array`),
    whichever step, chunk or shared prefix brought it in, so greedy tokens still depend on a request's own data only - but they
    are those of the rounded model, NOT promised to be the float32 run's.  `stats` gains `kv_dtype` and `pool_bytes` with any
    paged cache.  kv_dtype= without paging is refused: the contiguous nn.KVCache is float32."""
    weight = model.bert.embeddings.word_embeddings.weight
    cls = weight.__class__
    layer0 = model.bert.encoder.layer[0].attention.self
    assert layer0.causal, "serve needs a model built with causal=True"
    if lengths is None:
        rows = [np.asarray(p, np.int64).reshape(-1) for p in prompts]
        assert len(rows) >= 1 and all(len(p) >= 1 for p in rows), "serve: at least one prompt, each of at least one token"
        lengths = np.array([len(p) for p in rows], np.int64)
        padded = np.zeros((len(rows), int(lengths.max())), np.int32)
        for r, p in enumerate(rows):
            padded[r, :len(p)] = p
    else:
        padded, lengths = np.asarray(prompts.numpy() if hasattr(prompts, "numpy") else prompts), np.asarray(lengths, np.int64)
    n = padded.shape[0]
    budgets = np.full(n, max_new_tokens, np.int64) if np.ndim(max_new_tokens) == 0 else np.asarray(max_new_tokens, np.int64)
    assert budgets.shape == (n,) and (budgets >= 1).all(), "serve: max_new_tokens is an int >= 1 or one per request"
    assert int(poll) == poll and poll >= 1 and slots >= 1 and chunk >= 1
    positions = model.bert.embeddings.position_embeddings.weight.shape[0]
    paged, prefix_blocks = num_blocks is not None or isinstance(cache, nn.PagedKVCache), 0
    if paged:
        assert token_budget is None, "serve: token_budget= (token-packed steps) together with a paged cache (num_blocks= / nn.PagedKVCache) is not supported" + (
            " - kv_dtype=\"bf16\" included: the packed launch reads a float32 nn.KVCache" if kv_dtype == "bf16" or getattr(cache, "kv_dtype", None) == "bf16" else "")
        if cache is None:
            assert int(block_size) == block_size and block_size >= 1 and int(num_blocks) == num_blocks and num_blocks >= 1
            cache = nn.PagedKVCache(len(model.bert.encoder.layer), int(slots), int(num_blocks), int(block_size), layer0.h * layer0.d,
                                    int(-(-int((lengths + budgets - 1).max()) // int(block_size))), like=weight, kv_dtype=kv_dtype)
        assert isinstance(cache, nn.PagedKVCache), "serve: num_blocks= makes its own nn.PagedKVCache, or takes one as cache=, got a %s" % type(cache).__name__
        assert kv_dtype is None or cache.kv_dtype == kv_dtype, "serve: kv_dtype=%r and a cache= whose kv_dtype is %r" % (kv_dtype, cache.kv_dtype)
        shared = int(shared_prefix)
        assert shared == shared_prefix and 0 <= shared <= int(lengths.min()) and (padded[:, :shared] == padded[:1, :shared]).all(), \
            "serve: shared_prefix=%s declares the first tokens of every prompt equal: they are not, or a prompt is shorter" % (shared_prefix,)
        # full blocks only, and every request keeps a prompt token of its own
        prefix_blocks = min(shared // cache.block_size, (int(lengths.min()) - 1) // cache.block_size)
    else:
        assert not shared_prefix, "serve: shared_prefix= goes with a paged cache (num_blocks=)"
        assert kv_dtype is None, "serve: kv_dtype=%r goes with a paged cache (num_blocks=, or cache= an nn.PagedKVCache(kv_dtype=\"bf16\")): the contiguous " \
            "nn.KVCache is float32" % (kv_dtype,)
    if cache is None:
        cache = nn.KVCache(len(model.bert.encoder.layer), int(slots), int((lengths + budgets - 1).max()), layer0.h * layer0.d, like=weight, per_row=True)
    assert cache.batch == slots, "serve: the cache has %d rows for %d slots" % (cache.batch, slots)
    chunk = min(int(chunk), cache.capacity)                 # (a piece never exceeds the cache; the results do not depend on it)
    assert token_budget is None or (int(token_budget) == token_budget and token_budget >= slots), \
        "serve: token_budget is a number of token rows >= slots = %d (every decoding slot gets its token), got %s" % (slots, token_budget)
    packed = {} if token_budget is None else {"token_budget": int(token_budget)}
    if paged:
        packed = {"prefix_blocks": prefix_blocks}
    table = None
    if seeds is not None or any(np.ndim(v) for v in (temperature, top_k, top_p)):
        # per request: a row of parameters and a seed each (s + r for an int s; the backend generator's seed, read here, for None)
        assert temperature is not None, "serve: seeds= and per-request top_k / top_p go with temperature= (a float, or one per request; 0 is greedy)"
        if seeds is None:
            seeds = light.random.get_state("cpu" if cls is light.CpuTensor else "hip")[0]
        if np.ndim(seeds) == 0:
            seeds = [(int(seeds) + r) % (1 << 64) for r in range(n)]
        assert all(np.ndim(v) == 0 or len(v) == n for v in (temperature, top_k, top_p, seeds)), \
            "serve: temperature, top_k, top_p and seeds are scalars or one entry per request (%d)" % n
        table = light.random.sampling_table(temperature, top_k, top_p, seeds)
    penalties = None
    if any(np.ndim(v) or v != neutral for v, neutral in ((repetition_penalty, 1.0), (presence_penalty, 0.0), (frequency_penalty, 0.0), (min_new_tokens, 0))):
        assert all(np.ndim(v) == 0 or len(v) == n for v in (repetition_penalty, presence_penalty, frequency_penalty, min_new_tokens)), \
            "serve: repetition_penalty, presence_penalty, frequency_penalty and min_new_tokens are scalars or one entry per request (%d)" % n
        penalties = light.random.penalty_table(repetition_penalty, presence_penalty, frequency_penalty, min_new_tokens)
        penalties = np.ascontiguousarray(np.broadcast_to(penalties, (n, penalties.shape[1])))
        if (penalties == light.random.penalty_table()).all():
            penalties = None                                # sequences of neutral values: no table either
    want = None if logprobs is None else light.random.logprob_want(logprobs, n)
    eos = None if eos_token_id is None else int(eos_token_id)
    guides = None
    if guide is not None:
        vocab = weight.shape[0]
        entries = [guide] * n if isinstance(guide, light.guide.TokenAutomaton) else list(guide)
        assert len(entries) == n and all(a is None or isinstance(a, light.guide.TokenAutomaton) for a in entries), \
            "serve: guide= is None, one light.guide.TokenAutomaton, or one entry per request (%d), each an automaton or None" % n
        for r, a in enumerate(entries):
            assert a is None or a.vocab_size == vocab, "serve: the guide of request %d is over a vocabulary of %d ids, the model's has %d" % (r, a.vocab_size, vocab)
            assert a is None or eos is not None or not light.guide.needs_eos(a), \
                "serve: the guide of request %d has a state that only an end can follow: it needs eos_token_id" % r
        guides = light.guide.compile_guides(entries, n, eos, vocab_size=vocab)                # None if every entry is None
    pool = nn.RequestPool(cache, padded, lengths, budgets, chunk, pad_token_id=pad_token_id, max_positions=positions, sampling=table, penalties=penalties,
                          logprobs=want, guide=None if guides is None else tuple(guides), **packed)
    sampler = None if temperature is None or table is not None else (temperature, top_k, top_p)
    stats = {"steps": 0, "requests": n, "slots": int(slots), "chunk": chunk, **packed}
    if table is not None:
        stats["per_request_sampling"] = True
    if penalties is not None:
        stats["penalties"] = True
    if want is not None:
        stats["logprobs"] = {"token": pool.logprob, "top_ids": pool.top_ids, "top": pool.top_logprob}
    if guides is not None:
        stats["guide"] = True
    if paged:
        stats.update(num_blocks=cache.num_blocks, block_size=cache.block_size, kv_dtype=cache.kv_dtype, pool_bytes=cache.pool_bytes())

    def done():
        # the poll: one word read every `poll` steps, and at the step count no schedule exceeds (every request alone in turn)
        if stats["steps"] % poll and stats["steps"] < pool.max_steps:
            return False
        finished = pool.finished()
        assert finished == n or stats["steps"] < pool.max_steps, "serve: %d requests unfinished after the %d steps that every schedule ends within" % (
            n - finished, pool.max_steps)
        return finished == n

    with light.no_grad():
        if prefix_blocks:
            fill_shared_prefix(model, pool, padded[0, :prefix_blocks * cache.block_size])
        pool.admit(eos)
        serve_step(model, pool, sampler, eos)
        stats["steps"] = 1
        if graph is None:
            while not done():
                serve_step(model, pool, sampler, eos)
                stats["steps"] += 1
        elif not done():
            with graph.capture():
                serve_step(model, pool, sampler, eos)               # recorded, not run
            while True:
                graph.replay()
                stats["steps"] += 1
                if done():
                    break
    return (pool.out, pool.out_len), stats


if __name__ == "__main__":
    cpu = "--cpu" in sys.argv
    if "--serve" in sys.argv:
        option = lambda name, kind, default: kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default     # noqa: E731
        n_requests, n_slots, piece = option("--serve", int, 16), option("--slots", int, 4), option("--chunk", int, 16)
        np.random.seed(0)
        lm = BertForMaskedLM(**dict(TINY, causal=True)).eval()
        if not cpu:
            lm.map_parameters(lambda t: t.hip())
        requests = [np.random.randint(0, TINY["vocab_size"], np.random.randint(4, 48)) for _ in range(n_requests)]
        if "--shared-prefix" in sys.argv:
            # every prompt behind one common prefix (a system prompt) of that many tokens
            common = np.random.randint(0, TINY["vocab_size"], option("--shared-prefix", int, 0))
            requests = [np.concatenate([common, p]) for p in requests]
        new = [int(x) for x in np.random.randint(4, 32, n_requests)]
        recorded = None
        if "--graph" in sys.argv and not cpu:
            from lightgrad_amd.autograd.hip import HipGraph
            recorded = HipGraph()
        sampling = {}
        if "--sample" in sys.argv:
            sampling = dict(temperature=option("--temperature", float, 1.0), top_k=option("--top-k", int, 0), top_p=option("--top-p", float, 1.0))
            light.manual_seed(option("--seed", int, 0))
            if "--per-request" in sys.argv:
                # request r takes one of a short cycle of parameter sets (one of them greedy) and the stream seeded S + r
                cycle = ((0.0, 0, 1.0), (1.0, 0, 1.0), (0.8, 50, 0.95), (0.7, 5, 1.0), (1.3, 0, 0.9))
                sets = [cycle[r % len(cycle)] for r in range(n_requests)]
                sampling = dict(temperature=[s[0] for s in sets], top_k=[s[1] for s in sets], top_p=[s[2] for s in sets], seeds=option("--seed", int, 0))
        for flag, key, kind in (("--repetition-penalty", "repetition_penalty", float), ("--presence-penalty", "presence_penalty", float),
                                ("--frequency-penalty", "frequency_penalty", float), ("--min-new-tokens", "min_new_tokens", int)):
            if flag in sys.argv:
                sampling[key] = option(flag, kind, None)
        if "--logprobs" in sys.argv:
            sampling["logprobs"] = option("--logprobs", int, 0)
        ids_of = lambda text: [int(v) for v in text.replace(",", " ").split()]          # noqa: E731
        for flag, builder, many in (("--allow-only", light.guide.allow_only, False), ("--ban", light.guide.ban_sequences, True),
                                    ("--one-of", light.guide.one_of, True), ("--stop-after", light.guide.stop_after, True)):
            if flag in sys.argv:
                # one automaton for every request; sequences are separated by ";", ids by blanks or commas (--ban A,B,..: single ids)
                text = option(flag, str, "")
                if flag == "--ban" and ";" not in text and " " not in text.strip():
                    wanted = [[v] for v in ids_of(text)]
                else:
                    wanted = [ids_of(part) for part in text.split(";") if part.strip()] if many else ids_of(text)
                sampling["guide"] = builder(TINY["vocab_size"], wanted)
        t0 = time.perf_counter()
        if "--token-budget" in sys.argv:
            sampling["token_budget"] = option("--token-budget", int, None)
        if "--num-blocks" in sys.argv:
            sampling.update(num_blocks=option("--num-blocks", int, None), block_size=option("--block-size", int, 16),
                            shared_prefix=option("--shared-prefix", int, 0))
            if "--kv-dtype" in sys.argv:
                sampling["kv_dtype"] = option("--kv-dtype", str, None)           # bf16: the pools hold bfloat16 words, half the bytes
        (tokens, counts), info = serve(lm, requests, new, slots=n_slots, chunk=piece, eos_token_id=option("--eos", int, None), graph=recorded, **sampling)
        tokens, counts = tokens.numpy(), counts.numpy()             # the first read of anything but the poll word
        seconds = time.perf_counter() - t0
        print("%d requests (prompts of %d .. %d tokens, budgets of %d .. %d) through %d slots in pieces of %d%s: %d steps, %d tokens in %.1f ms (%s)" % (
            n_requests, min(map(len, requests)), max(map(len, requests)), min(new), max(new), n_slots, info["chunk"],
            " under a budget of %d token rows a step" % info["token_budget"] if "token_budget" in info else "", info["steps"], int(counts.sum()),
            1e3 * seconds, "step captured once, %d kernels" % recorded.kernel_count() if recorded else "eager steps"))
        if "num_blocks" in info:
            print("paged cache: %d blocks of %d positions per layer, %d of them a prefix shared by every request; %s pools of %d bytes" % (
                info["num_blocks"], info["block_size"], info["prefix_blocks"], info["kv_dtype"] or "float32", info["pool_bytes"]))
        for r in range(min(n_requests, 8)):
            print("request %d: %s" % (r, " ".join(str(i) for i in tokens[r, :counts[r]])))
        if "logprobs" in info:
            # request 0, token by token: its log-probability and what else the model considered
            scores, best, best_scores = (info["logprobs"][key].numpy() for key in ("token", "top_ids", "top"))
            print("request 0, log-probability %.4f over %d tokens (perplexity %.2f):" % (
                scores[0, :counts[0]].sum(), counts[0], np.exp(-scores[0, :counts[0]].mean())))
            for g in range(counts[0]):
                print("  token %6d  %9.4f   top: %s" % (tokens[0, g], scores[0, g], "  ".join(
                    "%d (%.4f)" % (i, v) for i, v in zip(best[0, g], best_scores[0, g]) if i >= 0)))
        sys.exit(0)
    if "--generate" in sys.argv:
        n_new = int(sys.argv[sys.argv.index("--generate") + 1])
        batch = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else 2
        np.random.seed(0)
        lm = BertForMaskedLM(**dict(TINY, causal=True)).eval()
        prompt = light.from_numpy(np.random.randint(0, TINY["vocab_size"], (batch, 8)).astype(np.int32), requires_grad=False)
        if not cpu:
            lm.map_parameters(lambda t: t.hip())
            prompt = prompt.hip(requires_grad=False)
        recorded = None
        if "--graph" in sys.argv and not cpu and n_new > 1:
            from lightgrad_amd.autograd.hip import HipGraph
            recorded = HipGraph()
        sampling = {}
        if "--sample" in sys.argv:
            option = lambda name, kind, default: kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default     # noqa: E731
            sampling = dict(temperature=option("--temperature", float, 1.0), top_k=option("--top-k", int, 0), top_p=option("--top-p", float, 1.0))
            light.manual_seed(option("--seed", int, 0))
        t0 = time.perf_counter()
        if "--prefill-chunk" in sys.argv:
            pieces = dict(prefill_chunk=int(sys.argv[sys.argv.index("--prefill-chunk") + 1]))
            print("prompt prefilled through the append path in pieces of at most %d tokens" % pieces["prefill_chunk"])
        else:
            pieces = {}
        if "--ragged" in sys.argv:
            # prompts of 8, 7, 6, .. tokens (at least 1): what lies behind a row's length is padding that nothing reads
            row_lengths = [max(1, 8 - r) for r in range(batch)]
            pieces = dict(pieces, lengths=row_lengths, eos_token_id=int(sys.argv[sys.argv.index("--eos") + 1]) if "--eos" in sys.argv else None)
            print("ragged batch: prompts of %s tokens%s" % (row_lengths, ", stopping at id %d" % pieces["eos_token_id"] if "--eos" in sys.argv else ""))
        counters = {}
        if "--speculate" in sys.argv:
            option = lambda name, kind, default: kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default     # noqa: E731
            if "--eos" in sys.argv:
                pieces = dict(pieces, eos_token_id=option("--eos", int, None))
            pieces = dict(pieces, speculate=option("--speculate", int, 3), max_ngram=option("--max-ngram", int, 3),
                          min_ngram=option("--min-ngram", int, 1), stats=counters)
        if "--num-beams" in sys.argv:
            option = lambda name, kind, default: kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default     # noqa: E731
            if "--eos" in sys.argv:
                pieces = dict(pieces, eos_token_id=option("--eos", int, None))
            pieces = dict(pieces, num_beams=option("--num-beams", int, 4), length_penalty=option("--length-penalty", float, 1.0))
            print("beam search: %d beams per prompt, length penalty %g" % (pieces["num_beams"], pieces["length_penalty"]))
        new_ids = generate(lm, prompt, n_new, graph=recorded, **sampling, **pieces).numpy()          # the only host read of the tokens
        if counters:
            print("speculative decoding by prompt lookup, up to %d drafts per step: %d steps, %d of %d drafts accepted" % (
                pieces["speculate"], counters["steps"], counters["accepted"], counters["drafted"]))
        if sampling:
            print("sampled: temperature %(temperature)g, top_k %(top_k)d, top_p %(top_p)g" % sampling)
        print("generated %d tokens per sequence in %.1f ms (%s)" % (
            n_new, 1e3 * (time.perf_counter() - t0),
            "decode step captured once, %d kernels, replayed %d times" % (recorded.kernel_count(), counters.get("steps", n_new - 1)) if recorded
            else "eager decode steps"))
        for r, row in enumerate(new_ids):
            print(" ".join(str(i) for i in row[pieces["lengths"][r] if "lengths" in pieces else 8:]))
        sys.exit(0)
    if "--mlm" in sys.argv:
        light.manual_seed(0)
        forward_backward = mlm_forward_backward            # the masked-LM objective in place of the stand-in loss below
    if "--clm" in sys.argv:
        assert "--mlm" not in sys.argv, "--clm and --mlm are two objectives"
        forward_backward = clm_forward_backward            # the next-token objective over causal attention
    batch = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else 8
    to_device = (lambda t: t) if cpu else (lambda t: t.hip())
    np.random.seed(0)
    config = dict(TINY, decoder_precision="bf16" if "--bf16-decoder" in sys.argv else None, causal="--clm" in sys.argv)
    model = BertForMaskedLM(**config).map_parameters(to_device)
    ids = to_device(light.from_numpy(np.random.randint(0, TINY["vocab_size"], (batch, 128)).astype(np.int32), requires_grad=False))
    total = None
    if "--accuracy" in sys.argv:
        assert "--mlm" in sys.argv, "--accuracy counts the masked tokens of the --mlm objective"
        total = to_device(light.from_numpy(np.zeros(2, np.int64), requires_grad=False))
        forward_backward = lambda m, i: mlm_forward_backward(m, i, accuracy_total=total)      # noqa: E731
    for it in range(3):
        t0 = time.perf_counter()
        value = forward_backward(model, ids).item()            # .item() synchronises
        print("iter %d: loss %.6f  fwd+bwd %.1f ms (eager tape)" % (it, value, 1e3 * (time.perf_counter() - t0)))
    if not cpu and "--graph" in sys.argv:
        # static shapes: record the ~400 launches of one forward+backward once, replay them with one host call
        from lightgrad_amd.autograd.hip import HipGraph, HipDevice
        graph = HipGraph()
        with graph.capture():
            loss = forward_backward(model, ids)
        replays = int(sys.argv[sys.argv.index("--replays") + 1]) if "--replays" in sys.argv else 3
        for it in range(replays):
            HipDevice.synchronize()
            t0 = time.perf_counter()
            graph.replay()
            value = loss.item()
            if it < 3 or it == replays - 1:
                print("replay %d: loss %.6f  fwd+bwd %.2f ms (hipGraph)" % (it, value, 1e3 * (time.perf_counter() - t0)))
    if total is not None:
        correct, counted = total.numpy()                       # the only host read of the counts
        print("masked-token accuracy %.4f (%d of %d masked tokens over every step and replay)" % (correct / max(counted, 1), correct, counted))
