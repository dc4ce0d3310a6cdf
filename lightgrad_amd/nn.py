"""Module system and the layers on the hot path (the callers of SURVEY.md §8 row a13).

Public surface = the reference's `lightgrad/nn.py` (same method names, argument meaning and iteration order, so a
training script written against lightgrad runs unchanged); the implementation is this repo's own:

  * a module keeps ONE ordered table of children (`_children`: attribute name -> tensor or Module) that attribute
    assignment maintains; every traversal is built on a single generator, `_leaves()`, which yields
    (owner module, attribute name, qualified name, tensor) with a module's own tensors before those of its
    sub-modules (the order of nn.py:31-45, which optimizers and the data-parallel bucket layout rely on);
  * `parameters`, `named_parameters`, `map_parameters` (nn.py:47-55: `model.map_parameters(lambda p: p.hip())` is how
    a model moves to a backend) and `load_parameters` (nn.py:57-76: tensors of any backend or ndarrays) are thin
    loops over `_leaves()` - no per-method recursion;
  * a tensor filed with `register_buffer` is a BUFFER (the running statistics of BatchNorm): the same table, the same traversal
    order, but `buffers` / `named_buffers` / `load_buffers` see it and the parameter methods do not; `map_parameters` maps both;
  * `Linear` / `LayerNorm` use a backend's fused tape op when the tensor class offers one (`linear`, `layer_norm` on
    HipTensor) and the reference's composite expression (nn.py:96, :117-124) otherwise - identical values.
"""
import numpy as np
from .autograd import Tensor, AbstractTensor


def _is_child(value) -> bool:
    return isinstance(value, (AbstractTensor, Module))


class Module(object):

    # training / evaluation switch (`train()`, `eval()`): layers that behave differently while training (Dropout) read it.
    # A plain attribute, not a child: it never shows in `parameters()`, `named_parameters()` or `load_parameters`.
    training = True

    def __init__(self):
        object.__setattr__(self, "_children", {})
        object.__setattr__(self, "_buffer_names", set())

    # ---- the call protocol ------------------------------------------------------------------------------------------

    def forward(self, *inputs):
        raise NotImplementedError("%s does not implement forward()" % type(self).__name__)

    def __call__(self, *inputs, **options):
        return self.forward(*inputs, **options)

    def train(self, mode: bool = True):
        """set `training` on this module and every sub-module; returns self"""
        self.training = bool(mode)
        for _, sub in self._own(Module):
            sub.train(mode)
        return self

    def eval(self):
        return self.train(False)

    # ---- bookkeeping ------------------------------------------------------------------------------------------------

    def __setattr__(self, name, value):
        if _is_child(value):
            self.register_param_or_module(name, value)
            if name in self._buffer_names and isinstance(value, AbstractTensor):
                value._requires_grad = False                         # a buffer stays one when it is replaced (map_parameters)
        object.__setattr__(self, name, value)

    def register_buffer(self, name, tensor):
        """file `tensor` under `name` as a BUFFER: state of the module that is no parameter (the running statistics of BatchNorm).
        It is an attribute, never requires a gradient, is absent from `parameters()` / `named_parameters()` / `load_parameters`
        and present in `buffers()` / `named_buffers()` / `load_buffers`; `map_parameters` maps it with the parameters"""
        if not isinstance(tensor, AbstractTensor):
            raise TypeError("register_buffer: %r must be a tensor, got %s" % (name, type(tensor).__name__))
        self._buffer_names.add(name)
        setattr(self, name, tensor)
        return tensor

    def register_param_or_module(self, name, value):
        """file a tensor / sub-module under `name` (re-assigning a name keeps its position in the table)"""
        if _is_child(value):
            self._children[name] = value
        return value

    def unregister_param_or_module(self, name):
        self._buffer_names.discard(name)
        return self._children.pop(name, None)

    def _own(self, kind):
        return [(n, c) for n, c in self._children.items() if isinstance(c, kind)]

    def _leaves(self, scope: str = "", sep: str = ".", buffers: bool = False):
        """every parameter (`buffers`: every buffer instead) below this module: (owner, attribute name, qualified name, tensor);
        own tensors first"""
        for name, tensor in self._own(AbstractTensor):
            if (name in self._buffer_names) == buffers:
                yield self, name, scope + name, tensor
        for name, sub in self._own(Module):
            yield from sub._leaves(scope + name + sep, sep, buffers)

    # ---- the reference's traversal API ------------------------------------------------------------------------------

    def parameters(self):
        return (leaf[3] for leaf in self._leaves())

    def named_parameters(self, prefix: str = "", separator: str = "."):
        scope = prefix + separator if prefix else ""
        return ((qualified, tensor) for _, _, qualified, tensor in self._leaves(scope, separator))

    def buffers(self):
        return (leaf[3] for leaf in self._leaves(buffers=True))

    def named_buffers(self, prefix: str = "", separator: str = "."):
        scope = prefix + separator if prefix else ""
        return ((qualified, tensor) for _, _, qualified, tensor in self._leaves(scope, separator, buffers=True))

    def map_parameters(self, fn):
        """replace every parameter AND every buffer p by fn(p): how a model moves to a backend"""
        for owner, name, _, tensor in list(self._leaves()) + list(self._leaves(buffers=True)):
            setattr(owner, name, fn(tensor))
        return self

    def load_parameters(self, param_dict, prefix: str = "", separator: str = ".") -> None:
        source = dict(param_dict)
        scope = prefix + separator if prefix else ""
        for owner, name, qualified, current in list(self._leaves(scope, separator)):
            if qualified not in source:
                raise AssertionError("no entry %r among the parameters to load (have: %s)" % (qualified, sorted(source)))
            setattr(owner, name, _as_tensor_like(current, source[qualified], qualified))

    def load_buffers(self, buffer_dict, prefix: str = "", separator: str = ".") -> None:
        """`load_parameters` for the buffers: every buffer of the module must have an entry"""
        source = dict(buffer_dict)
        scope = prefix + separator if prefix else ""
        for owner, name, qualified, current in list(self._leaves(scope, separator, buffers=True)):
            if qualified not in source:
                raise AssertionError("no entry %r among the buffers to load (have: %s)" % (qualified, sorted(source)))
            setattr(owner, name, _as_tensor_like(current, source[qualified], qualified))


def _as_tensor_like(current, incoming, what):
    """`incoming` (tensor of any backend, or ndarray) as a tensor of `current`'s class; shapes must agree"""
    if not isinstance(incoming, type(current)):
        array = incoming.numpy() if isinstance(incoming, AbstractTensor) else incoming
        if not isinstance(array, np.ndarray):
            raise AssertionError("cannot load %r from a %s" % (what, type(incoming).__name__))
        incoming = type(current).from_numpy(array)
    if tuple(incoming.shape) != tuple(current.shape):
        raise AssertionError("%r has shape %s, the value to load has %s" % (what, tuple(current.shape), tuple(incoming.shape)))
    return incoming


class ModuleList(Module, list):
    """a python list whose entries are registered under their index (nn.py:78-88)"""

    def __init__(self, *elements):
        Module.__init__(self)
        list.__init__(self, elements)
        for index, element in enumerate(elements):
            self.register_param_or_module(str(index), element)

    def __setitem__(self, index, element):
        if not -len(self) <= index < len(self):
            raise IndexError("ModuleList assignment index out of range")
        index %= len(self)
        # drop, then file again: like the reference (nn.py:84-88) a replaced entry moves to the END of the traversal
        # order, which the per-parameter step count of Adam / AdaBelief (optim.py:36, :48) makes observable
        self.unregister_param_or_module(str(index))
        self.register_param_or_module(str(index), element)
        list.__setitem__(self, index, element)


class Linear(Module):
    """y = x @ W^T + b with W of shape (out, in), both drawn by `xavier` (nn.py:90-96)"""

    def __init__(self, in_feats: int, out_feats: int, bias: bool = True, precision: str = None):
        """`precision` (extension of the reference): None = fp32 products; "bf16" = both operands of every product of this
        layer, forward and backward, rounded to bfloat16 on their way into the matrix cores, sums in fp32 (`linear_bf16`).
        Parameters, activations and gradients stay float32 either way."""
        Module.__init__(self)
        if precision not in (None, "bf16"):
            raise ValueError("Linear: precision must be None or 'bf16' (got %r)" % (precision,))
        self.precision = precision
        self.weight = Tensor.xavier((out_feats, in_feats))
        self.bias = Tensor.xavier((out_feats,)) if bias else None

    def forward(self, x, residual=None):
        """`residual` (extension of the reference's forward(x)): a tensor of the output's shape added to the result, as in
        `dense(h) + h_in` of a transformer block - a backend with a fused op adds it where the product is made"""
        if self.precision == "bf16":
            y = x.linear_bf16(self.weight) if self.bias is None else x.linear_bf16(self.weight, self.bias)
            return y if residual is None else y + residual
        fused = getattr(x, "linear", None)
        if fused is not None:        # one tape node, bias (and residual) added in the GEMM epilogue (HipTensor)
            if residual is not None:
                return fused(self.weight, self.bias, residual)
            return fused(self.weight) if self.bias is None else fused(self.weight, self.bias)
        y = x @ self.weight.T(1, 0)
        y = y if self.bias is None else y + self.bias
        return y if residual is None else y + residual


class Dropout(Module):
    """while training: x.dropout(p, residual=...) - each element zeroed with probability p, the others scaled by 1 / (1 - p),
    `+ residual` in the same kernel; in `eval()` or with p == 0: the input itself (or the plain sum with the residual).  Not a
    layer of the reference (its BERT example replaces dropout by the identity, examples/bert.py:37)."""

    def __init__(self, p: float = 0.5):
        Module.__init__(self)
        from .random import check_probability
        self.p = check_probability(p)

    def forward(self, x, residual=None):
        if self.training and self.p > 0:
            return x.dropout(self.p, residual=residual)
        return x if residual is None else x + residual


class Conv2d(Module):
    """valid 2-d convolution, zero padding of kernelsize // 2 unless told otherwise (nn.py:98-107; CNN tail of §8f)"""

    def __init__(self, in_channels: int, out_channels: int, kernelsize: int = 3, stride: int = 1, pad: int = None, bias: bool = True):
        Module.__init__(self)
        self.w = Tensor.xavier((out_channels, in_channels, kernelsize, kernelsize))
        self.b = Tensor.xavier((1, out_channels, 1, 1)) if bias else None
        self.s = stride
        self.p = kernelsize // 2 if pad is None else pad

    def forward(self, x):
        return x.conv2d(self.w, self.b, stride=self.s, pad=self.p)


class LayerNorm(Module):
    """normalise over the trailing `shape` axes, then scale and shift (nn.py:109-124)"""

    def __init__(self, shape: tuple, eps: float = 1e-5):
        Module.__init__(self)
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        self.eps = eps
        self.weight = Tensor.ones(self.shape)
        self.bias = Tensor.zeros(self.shape)

    def forward(self, x):
        k = len(self.shape)
        if tuple(x.shape[-k:]) != self.shape:
            raise AssertionError("LayerNorm over %s applied to an input of shape %s" % (self.shape, tuple(x.shape)))
        fused = getattr(x, "layer_norm", None)
        if k == 1 and fused is not None:          # the composite below as one kernel (HipTensor)
            return fused(self.weight, self.bias, eps=self.eps)
        axes = tuple(range(len(x.shape) - k, len(x.shape)))
        centred = x - x.mean(axis=axes, keepdims=True)
        variance = (centred * centred).mean(axis=axes, keepdims=True)
        return centred / (variance + self.eps).pow(1 / 2) * self.weight + self.bias


class _BatchNorm(Module):
    """y = (x - mean_c) / sqrt(var_c + eps) * weight_c + bias_c over every axis but the channel axis 1.  While training: the
    statistics of the batch (`batch_norm`), and the running statistics - buffers, not parameters - follow them with `momentum`
    (running_var takes the unbiased variance, PyTorch's convention).  In `eval()`: the running statistics (`batch_norm_infer`),
    which stay as they are.  Each data-parallel rank normalises its own batch.  Not a layer of the reference."""

    _ranks = ()

    def __init__(self, channels: int, eps: float = 1e-5, momentum: float = 0.1, affine: bool = True):
        Module.__init__(self)
        if not 0.0 < momentum <= 1.0:
            raise ValueError("%s: momentum must lie in (0, 1], got %r" % (type(self).__name__, momentum))
        self.channels, self.eps, self.momentum = int(channels), eps, momentum
        self.weight = Tensor.ones((self.channels,)) if affine else None
        self.bias = Tensor.zeros((self.channels,)) if affine else None
        self.register_buffer("running_mean", Tensor.zeros((self.channels,), requires_grad=False))
        self.register_buffer("running_var", Tensor.ones((self.channels,), requires_grad=False))

    def forward(self, x):
        if len(x.shape) not in self._ranks or x.shape[1] != self.channels:
            raise AssertionError("%s over %d channels applied to an input of shape %s" % (type(self).__name__, self.channels, tuple(x.shape)))
        if self.training:
            return x.batch_norm(self.weight, self.bias, self.running_mean, self.running_var, momentum=self.momentum, eps=self.eps)
        return x.batch_norm_infer(self.weight, self.bias, self.running_mean, self.running_var, eps=self.eps)


class BatchNorm1d(_BatchNorm):
    """batch normalisation of (N, C) or (N, C, L) inputs"""
    _ranks = (2, 3)


class BatchNorm2d(_BatchNorm):
    """batch normalisation of (N, C, H, W) inputs"""
    _ranks = (4,)


class KVCache(object):
    """the keys and values of the tokens a causal model has seen, per layer: `k[i]`, `v[i]` of shape (batch, capacity, width) on
    the backend (and in the dtype) of `like`, and the position of the NEXT token - `pos`, an int32 tensor of one element on that
    backend, which the backend's decode attention and the position lookup read on the device, and `length`, its mirror on the
    host for the backends that have no decode op (they slice the cache with it).  `advance()` adds 1 on the device with the
    in-place int32 add - inside a hipGraph capture it is recorded like any kernel, and every replay moves the position on.
    State, not parameters: not a Module, so it is in no `parameters()` / `buffers()` and never reaches an optimizer.  Not a
    class of the reference (its model has no decoder).

    `per_row=True`: every sequence of the batch has a position of its own (a ragged batch: prompts of different lengths, rows
    that stop at an end-of-sequence token).  `pos` then has shape (batch,) - the backend's attention launches read word r for
    sequence r -, `positions(m)` is (batch, m), `set_lengths` takes a length per row and `advance` an int or a length per row.
    The host mirror is `lengths`, an int64 array: valid only while every change came from the host, None once the device moved
    the positions by values the host has not seen (`committed` with an end-of-sequence id).  `length` is then an upper bound of
    every row's position - what the routing between prefill and decode step and the capacity checks need, never an index.
    Rejected drafts (speculative decoding: `speculate_commit`) leave key and value rows in the cache beyond the new position.
    Nothing reads beyond the position, and the next step overwrites them.
    Beam search keeps the beams of a prompt in `num_beams` neighbouring rows (a group; `num_beams` is an attribute, 1 unless the
    caller sets it, and `batch` is a multiple of it).  `reorder(parent)` makes the rows follow the beams that survived a
    `beam_step`: row n of a group becomes the old row parent[n] (an absolute row index inside the same group; duplicates are the
    normal case) at the positions below the group's largest `pos`; what lies at or beyond it is not touched, and nothing reads it.
    Without `per_row` every attribute, shape and launch is as it was."""

    def __init__(self, layers: int, batch: int, capacity: int, width: int, like=None, per_row: bool = False):
        cls = Tensor if like is None else type(like)
        dtype = np.dtype(np.float32 if like is None else like.dtype)
        assert layers >= 1 and batch >= 1 and capacity >= 1 and width >= 1
        self.layers, self.batch, self.capacity, self.width = int(layers), int(batch), int(capacity), int(width)
        shape = (self.batch, self.capacity, self.width)          # (an array of its own each: CpuTensor.from_numpy adopts what it is given)
        self.k = [cls.from_numpy(np.zeros(shape, dtype), requires_grad=False) for _ in range(self.layers)]
        self.v = [cls.from_numpy(np.zeros(shape, dtype), requires_grad=False) for _ in range(self.layers)]
        self.per_row = bool(per_row)
        self.pos = cls.from_numpy(np.zeros(self.batch if self.per_row else 1, np.int32), requires_grad=False)
        self.length = 0
        self.lengths = np.zeros(self.batch, np.int64) if self.per_row else None
        self._arange = {}           # m -> the int32 constant 0 .. m - 1 on the cache's backend
        self.num_beams = 1          # rows per group of `reorder`

    def reorder(self, parent, num_beams=None) -> None:
        """per_row: the rows follow their beams.  parent: int32 (batch,) on the cache's backend; for every layer and for both k and v,
        row n of each group of `num_beams` rows (default: the attribute) becomes the old row parent[n] at the cache positions
        j < max(pos) of the group - the positions as they are now, after `beam_step`; positions beyond are not touched.  One op of
        the backend for all 2 * layers tensors (`kv_reorder`: on HipTensor one launch, in place).  Neither the positions nor the
        host mirror change."""
        assert self.per_row, "KVCache.reorder goes with per_row=True"
        w = self.num_beams if num_beams is None else int(num_beams)
        assert 1 <= w <= 8 and self.batch % w == 0, "KVCache.reorder: %d rows are no groups of num_beams = %d (1 .. 8)" % (self.batch, w)
        type(self.pos).kv_reorder(self.k + self.v, parent, self.pos, w)

    def positions(self, m: int):
        """the int32 position ids `pos + arange(m)` of the next m tokens, shape (m,): one broadcast add on the cache's backend -
        no host read, and inside a hipGraph capture it is recorded like any kernel (a replay reads the position as it is then).
        per_row: shape (batch, m), `pos[:, None] + arange(m)` - still one broadcast add"""
        m = int(m)
        assert m >= 1
        if m not in self._arange:
            t = type(self.pos).from_numpy(np.arange(m, dtype=np.int32), requires_grad=False)
            if hasattr(t, "freeze"):
                t.freeze()          # a constant, like a model's position ids
            self._arange[m] = t
        ids = (self.pos.reshape(self.batch, 1) if self.per_row else self.pos) + self._arange[m]
        ids._requires_grad = False  # ids are state like `pos`: they go into lookups by keyword and take no gradient
        return ids

    def advance(self, n=1) -> None:
        """the next token's position, + n: on the device, and in the host mirror.  per_row: n is an int for every row, or a
        length per row - a host sequence / array of `batch` ints (uploaded; the mirror stays valid) or an int32 tensor (batch,)
        on the cache's backend (nothing is read back: the mirror stays valid only where reading is free, on the numpy backend)"""
        if self.per_row and not isinstance(n, (int, np.integer)):
            if hasattr(n, "shape") and not isinstance(n, np.ndarray):
                assert tuple(n.shape) == (self.batch,) and np.dtype(n.dtype) == np.int32, "KVCache.advance: a tensor of lengths is int32 (batch,)"
                step, host = n, (np.asarray(n.data, np.int64) if isinstance(getattr(n, "data", None), np.ndarray) else None)
            else:
                host = np.asarray(n, np.int64)
                assert host.shape == (self.batch,) and (host >= 0).all(), "KVCache.advance: %d lengths >= 0, one per row" % self.batch
                step = type(self.pos).from_numpy(host.astype(np.int32), requires_grad=False)
            self.pos += step
            self.lengths = None if host is None or self.lengths is None else self.lengths + host
            if self.lengths is not None:
                self.length = int(self.lengths.max())
            else:               # the upper bound moves by the largest step the host knows of
                self.length = self.capacity if host is None else min(self.capacity, self.length + int(host.max()))
            return
        self.pos += int(n)
        self.length += int(n)
        if self.lengths is not None:
            self.lengths = self.lengths + int(n)

    def committed(self, n: int = 1, eos: bool = False) -> None:
        """per_row: `decode_commit` moved the positions on the device n times (eagerly, or as replays of a captured step): the host
        follows.  Without an end-of-sequence id every row moved; with one (eos=True) which rows moved is known on the device
        only - `lengths` is None from here on and `length` stays the upper bound"""
        assert self.per_row, "KVCache.committed goes with per_row=True"
        self.length += int(n)
        self.lengths = None if eos or self.lengths is None else self.lengths + int(n)

    def set_lengths(self, lengths) -> None:
        """per_row: rows 0 .. lengths[r] - 1 of sequence r have been filled: its next token's position is lengths[r]"""
        assert self.per_row, "KVCache.set_lengths goes with per_row=True (set_length: one position for the batch)"
        host = np.asarray(lengths, np.int64)
        assert host.shape == (self.batch,) and (host >= 0).all() and (host <= self.capacity).all(), \
            "KVCache: %d lengths within 0 .. %d, one per row, got %s" % (self.batch, self.capacity, lengths)
        self.pos[:] = type(self.pos).from_numpy(host.astype(np.int32), requires_grad=False)
        self.lengths, self.length = host.copy(), int(host.max())

    def replayed(self, n: int = 1) -> None:
        """a captured step that holds `advance()` was replayed n more times: the device position moved, the host mirror follows"""
        self.length += int(n)
        if self.lengths is not None:
            self.lengths = self.lengths + int(n)

    def set_length(self, n: int) -> None:
        """rows 0 .. n - 1 have been filled (a prompt): the next token's position is n"""
        assert 0 <= n <= self.capacity, "KVCache: %d positions do not fit a capacity of %d" % (n, self.capacity)
        self.pos.fill(int(n))
        self.length = int(n)
        if self.per_row:
            self.lengths = np.full(self.batch, int(n), np.int64)

    def reset(self) -> None:
        """forget every token: the position goes back to 0 (the rows stay as they are - nothing reads beyond the position)"""
        self.set_length(0)

    def fill(self, layer: int, k, v) -> None:
        """the keys / values (batch, s, width) of a prompt become rows 0 .. s - 1 of a layer, on the tensors' own backend"""
        s = k.shape[1]
        assert tuple(k.shape) == tuple(v.shape) == (self.batch, s, self.width) and s <= self.capacity, \
            "KVCache: keys / values of shape %s / %s do not fit (%d, <= %d, %d)" % (tuple(k.shape), tuple(v.shape), self.batch, self.capacity, self.width)
        self.k[layer][:, :s] = k
        self.v[layer][:, :s] = v


class PagedKVCache(object):
    """the keys and values of a serving loop in fixed-size BLOCKS drawn from one pool, in place of `capacity` contiguous rows per
    slot (KVCache): `k[i]`, `v[i]` are pools of shape (num_blocks, block_size, width) on the backend (and in the dtype) of `like`,
    and `block_table`, int32 (slots, max_blocks), says where a slot's rows are - word n of row s is the pool block that holds
    positions n * B .. n * B + B - 1 of slot s (B = block_size), -1 = none.  `held` (slots,) counts the blocks a slot's table
    names; `free` (num_blocks + 1,) is the allocator, a stack on the device: word 0 the number n of free blocks, words 1 .. n their
    indices, the top at word n.  `pos` (slots,) is the position of each slot's next token (`per_row` is True, `batch` = slots),
    `positions(m)` what KVCache.positions is, `capacity` = max_blocks * block_size the most a slot can hold.  A slot holds the
    blocks its request needs, not the worst request's; blocks below the positions of every slot that names them may be SHARED
    (a common prompt prefix: `reset(prefix_blocks=F)` keeps blocks 0 .. F - 1 off the stack for it) - the attention launch never
    writes below a slot's position.  block_size is a power of two, 4 <= B <= 128 (small blocks reach multi-block tables at tiny
    shapes), and capacity <= 512, the extend kernel's limit.  Tables and stack are moved by ONE op per step,
    `serve_commit_paged` (nn.RequestPool); the cache serves the `count=` append path only: `reorder`, the one-token decode route,
    token-packed steps (`cu=`) and `generate` refuse it.  State, not parameters, like KVCache.  Not a class of the reference.
    kv_dtype="bf16": the pools are int16 tensors of the same shape that hold BFLOAT16 words - `light.bf16_bits` of every key and
    value, half the bytes (`pool_bytes`).  Every key and value is then attended to as r of what the projection produced
    (r = `bf16_round_array`), whichever step brought it in; `kv_dtype` says which form the cache holds (None: the dtype of `like`)."""

    per_row = True
    num_beams = 1

    def __init__(self, layers: int, slots: int, num_blocks: int, block_size: int, width: int, max_blocks: int, like=None, kv_dtype=None):
        cls = Tensor if like is None else type(like)
        assert kv_dtype in (None, "bf16"), "PagedKVCache: kv_dtype is None (the pools in the dtype of `like`) or \"bf16\", got %r" % (kv_dtype,)
        self.kv_dtype = kv_dtype
        dtype = np.dtype(np.int16) if kv_dtype == "bf16" else np.dtype(np.float32 if like is None else like.dtype)
        assert layers >= 1 and slots >= 1 and num_blocks >= 1 and width >= 1 and max_blocks >= 1
        assert int(block_size) == block_size and 4 <= block_size <= 128 and block_size & (block_size - 1) == 0, \
            "PagedKVCache: block_size is a power of two within 4 .. 128, got %s" % (block_size,)
        assert max_blocks * block_size <= 512, "PagedKVCache: max_blocks * block_size = %d positions exceed the 512 of the extend kernel" % (max_blocks * block_size)
        self.layers, self.batch, self.slots, self.width = int(layers), int(slots), int(slots), int(width)
        self.num_blocks, self.block_size, self.max_blocks = int(num_blocks), int(block_size), int(max_blocks)
        self.capacity = self.max_blocks * self.block_size
        shape = (self.num_blocks, self.block_size, self.width)
        self.k = [cls.from_numpy(np.zeros(shape, dtype), requires_grad=False) for _ in range(self.layers)]
        self.v = [cls.from_numpy(np.zeros(shape, dtype), requires_grad=False) for _ in range(self.layers)]
        i32 = lambda a: cls.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)        # noqa: E731
        self.block_table, self.held = i32(np.full((self.batch, self.max_blocks), -1)), i32(np.zeros(self.batch))
        self.free, self.pos = i32(np.zeros(self.num_blocks + 1)), i32(np.zeros(self.batch))
        self.prefix_blocks = 0
        self.length, self.lengths = 0, np.zeros(self.batch, np.int64)
        self._arange = {}
        self.reset()

    positions = KVCache.positions
    advance = KVCache.advance           # (tests and tools move the positions by hand; `serve` leaves it to serve_commit_paged)

    def reset(self, prefix_blocks: int = 0) -> None:
        """forget every token and every block: positions 0, tables -1, held 0, and the stack holds blocks num_blocks - 1 down to
        `prefix_blocks` - block `prefix_blocks` is popped first; blocks 0 .. prefix_blocks - 1 stay off it (the pools stay as they are)"""
        F = int(prefix_blocks)
        assert 0 <= F <= min(self.num_blocks, self.max_blocks), \
            "PagedKVCache.reset: prefix_blocks within 0 .. min(num_blocks, max_blocks) = %d, got %s" % (min(self.num_blocks, self.max_blocks), prefix_blocks)
        stack = np.zeros(self.num_blocks + 1, np.int32)
        stack[0] = self.num_blocks - F
        stack[1:1 + self.num_blocks - F] = np.arange(self.num_blocks - 1, F - 1, -1)
        i32 = lambda a: type(self.pos).from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)        # noqa: E731
        self.free[:] = i32(stack)
        self.block_table[:] = i32(np.full((self.batch, self.max_blocks), -1))
        self.held.fill(0)
        self.pos.fill(0)
        self.prefix_blocks = F
        self.length, self.lengths = 0, np.zeros(self.batch, np.int64)

    def reorder(self, parent, num_beams=None) -> None:
        if self.kv_dtype == "bf16":
            raise NotImplementedError("PagedKVCache.reorder: a bf16 cache (kv_dtype=\"bf16\") serves the count= append path only; beams copy rows "
                                      "between the slots of a float32 nn.KVCache")
        raise NotImplementedError("PagedKVCache.reorder: beams copy rows between slots; the paged cache serves the count= append path only")

    def pool_bytes(self) -> int:
        """bytes of the key and value pools of every layer"""
        return 2 * self.layers * self.num_blocks * self.block_size * self.width * np.dtype(self.k[0].dtype).itemsize


class RequestPool(object):
    """the requests of a serving loop and the state of the cache slots that work through them (continuous batching): N prompts
    wait in a queue, each of the cache's `batch` slots holds one request at a time, and a slot whose request has finished takes
    the next one while the other slots go on.  Everything is an int32 tensor on the cache's backend, moved by ONE op per step,
    `serve_commit` (the numpy backend's is the definition: autograd/cpu/ops.py) - nothing is read back:
        prompts (N, P) right-padded, prompt_len (N,), budget (N,) new tokens per request,
        out (N, G) the generated tokens (pre-filled with `pad_token_id`), out_len (N,),
        queue (2,) = {next request to admit, requests finished},
        req (b,) the request each slot holds, -1 = free; `cache.pos` (b,); count (b,) the real new tokens of the step;
        ids, position_ids (b, chunk) the step's inputs; last (b,) the row of the flattened (b * chunk) hidden rows for the head.
    `cache` must be per_row.  A request needs lengths[r] + budgets[r] - 1 cache rows (its last token is fed to nobody): checked
    here, on the host, against the capacity.  State, not parameters, like the cache.  Not a class of the reference."""

    def __init__(self, cache, prompts, lengths, budgets, chunk: int, pad_token_id: int = 0, max_positions=None, token_budget=None, prefix_blocks: int = 0,
                 sampling=None, penalties=None, logprobs=None, guide=None):
        """max_positions: the model's position embeddings, if the caller knows them - the capacity must not exceed them.
        token_budget: None, or T >= slots - the steps are TOKEN-PACKED: ids and position_ids are (1, T), the step's tokens of all
        slots in one flat buffer, `cu` (slots + 1,) says which rows are whose, `last` names rows of the T, and `commit` is
        `serve_commit_packed`: a decoding slot takes one row, the prefilling slots share the rest in pieces of at most `chunk`.
        `count` stays (pos + count is the commit's t).  Without it `cu` is None and everything is as it was.
        cache: an nn.PagedKVCache in place of a KVCache - `commit` is `serve_commit_paged`, which also moves the cache's tables
        and its stack of free blocks; prefix_blocks: the blocks 0 .. F - 1 every request shares (they hold the first F * B tokens
        of every prompt already; the pool resets the cache with them off the stack)
        sampling: None, or an int32 (N, 8) numpy table of `random.sampling_table` - parameters and a seed per REQUEST, uploaded once
        as `self.sampling`; a step then draws with `logits.sample_rows(pool.sampling, pool.req, pool.out_len)`: slot s under the row
        of the request it holds, with the number of tokens that request has stored as its counter.  Both are the pool's own
        state and right when the step draws (the previous commit laid the step out for req[s]; out_len[r] moves only when a
        token is stored), so no commit changes.  None: `self.sampling` is None and everything is as it was.
        penalties: None, or an int32 (N, 4) numpy table of `random.penalty_table` - repetition, presence and frequency penalty and
        the minimum of new tokens per REQUEST, uploaded once as `self.penalties`; a step then passes its logits through
        `logits.penalize_rows(pool.penalties, pool.req, pool.prompts, pool.prompt_len, pool.out, pool.out_len, eos=)` in front of
        the draw.  The history is the pool's own state and right when the step draws, for the reason above; the launch keeps it
        in LDS, so P + G <= 4096 is asserted here.  None: `self.penalties` is None and everything is as it was.
        logprobs: None, or N ints per REQUEST (`random.logprob_want`): -1 = none for it, 0 = the log-probability of each of its
        tokens, k in 1 .. 8 = also the k most likely ids of every step.  They are uploaded once as `self.logprobs`, next to
        `self.logprob` float32 (N, G), `self.top_ids` int32 (N, G, n) and `self.top_logprob` float32 (N, G, n) with n = max(k, 1),
        filled with +0.0, -1 and +0.0; a step then calls `logits.logprob_rows(nxt, pool.logprobs, pool.req, pool.out_len,
        pool.logprob, pool.top_ids, pool.top_logprob)` behind the draw and in front of `commit`, which moves out_len: token g of
        request r is scored in column g.  None: the four attributes are None and everything is as it was.
        guide: None, or the tables of `guide.compile_guides` for the N requests (allow, states, edges, start) - the token automata
        that restrict what each REQUEST may generate.  The three tables are uploaded once as `self.guide` (a tuple), next to
        `self.guide_state` int32 (N, 2), initialised to (start[r], 0): the state of request r's automaton and the number of stored
        tokens it has absorbed.  A step then passes its logits through `logits.guide_rows(*pool.guide, pool.req, pool.out,
        pool.out_len, pool.guide_state)` behind the penalties and in front of the draw; the launch lets the state catch up with
        `out_len` first, so no commit changes.  None: both attributes are None and everything is as it was."""
        assert isinstance(cache, (KVCache, PagedKVCache)) and cache.per_row, \
            "RequestPool takes a cache with a position per sequence: nn.KVCache(..., per_row=True) or nn.PagedKVCache"
        self.paged = isinstance(cache, PagedKVCache)
        assert not self.paged or token_budget is None, "RequestPool: token_budget= (token-packed steps) does not go with a PagedKVCache%s" % (
            " (kv_dtype=\"bf16\": the packed launch reads a float32 nn.KVCache)" if getattr(cache, "kv_dtype", None) == "bf16" else "")
        assert max_positions is None or cache.capacity <= max_positions, \
            "RequestPool: a cache of %d positions exceeds the model's %s position embeddings" % (cache.capacity, max_positions)
        cls = type(cache.pos)
        prompts = np.asarray(prompts.numpy() if hasattr(prompts, "numpy") else prompts)
        assert prompts.ndim == 2 and prompts.shape[0] >= 1 and prompts.shape[1] >= 1 and np.issubdtype(prompts.dtype, np.integer), \
            "RequestPool: prompts are (N, P) right-padded integer ids, got %s %s" % (prompts.dtype, prompts.shape)
        n = prompts.shape[0]
        lengths, budgets = np.asarray(lengths, np.int64), np.asarray(budgets, np.int64)
        assert lengths.shape == budgets.shape == (n,) and (lengths >= 1).all() and (lengths <= prompts.shape[1]).all() and (budgets >= 1).all(), \
            "RequestPool: %d lengths within 1 .. %d and %d budgets >= 1, one per request" % (n, prompts.shape[1], n)
        assert int(chunk) == chunk and chunk >= 1, "RequestPool: chunk is a number of tokens >= 1"
        assert (lengths + budgets - 1 <= cache.capacity).all(), \
            "RequestPool: a request of %d prompt tokens and %d new ones does not fit a cache of %d positions" % (
                int(lengths[np.argmax(lengths + budgets)]), int(budgets[np.argmax(lengths + budgets)]), cache.capacity)
        if self.paged:
            # a request reserves the blocks of its whole life when it is admitted: each must fit a table, and the pool once the
            # running requests have ended (the head of the queue is then always admitted); its own tokens start behind the prefix
            B, F = cache.block_size, int(prefix_blocks)
            need = -(-(lengths + budgets - 1) // B) - F
            assert 0 <= F <= min(cache.max_blocks, cache.num_blocks), "RequestPool: prefix_blocks within 0 .. %d, got %s" % (min(cache.max_blocks, cache.num_blocks), prefix_blocks)
            assert (need + F <= cache.max_blocks).all(), "RequestPool: a request needs %d blocks of %d positions, a table of the PagedKVCache has %d" % (
                int(need.max()) + F, B, cache.max_blocks)
            assert (need <= cache.num_blocks - F).all(), "RequestPool: a request needs %d blocks behind the %d shared ones, the pool of the PagedKVCache has %d in all" % (
                int(need.max()), F, cache.num_blocks)
            assert (F * B < lengths).all(), "RequestPool: a shared prefix of %d blocks of %d tokens leaves a prompt of %d tokens none of its own" % (F, B, int(lengths.min()))
            self.prefix_blocks = F
        else:
            assert not prefix_blocks, "RequestPool: prefix_blocks= goes with a PagedKVCache"
        self.cache, self.requests, self.slots, self.chunk, self.pad_token_id = cache, n, cache.batch, int(chunk), int(pad_token_id)
        tensor = lambda a: cls.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)        # noqa: E731
        self.prompts, self.prompt_len, self.budget = tensor(prompts), tensor(lengths), tensor(budgets)
        self.out = tensor(np.full((n, int(budgets.max())), int(pad_token_id)))
        self.out_len, self.queue = tensor(np.zeros(n)), tensor(np.zeros(2))
        self.req, self.count, self.last = tensor(np.full(self.slots, -1)), tensor(np.zeros(self.slots)), tensor(np.zeros(self.slots))
        self._no_tokens = tensor(np.zeros(self.slots))
        self.sampling = None
        if sampling is not None:
            sampling = np.asarray(sampling)
            assert sampling.dtype == np.int32 and sampling.shape == (n, 8), \
                "RequestPool: sampling= is the int32 (%d, 8) table of random.sampling_table, a row per request (got %s %s)" % (n, sampling.dtype, sampling.shape)
            self.sampling = tensor(sampling)
        self.penalties = None
        if penalties is not None:
            from .random import PENALTY_MAX_HISTORY, PENALTY_WORDS
            penalties = np.asarray(penalties)
            assert penalties.dtype == np.int32 and penalties.shape == (n, PENALTY_WORDS), \
                "RequestPool: penalties= is the int32 (%d, %d) table of random.penalty_table, a row per request (got %s %s)" % (
                    n, PENALTY_WORDS, penalties.dtype, penalties.shape)
            assert prompts.shape[1] + int(budgets.max()) <= PENALTY_MAX_HISTORY, \
                "RequestPool: penalties= keeps a request's history in LDS: P + G = %d + %d ids exceed %d" % (
                    prompts.shape[1], int(budgets.max()), PENALTY_MAX_HISTORY)
            self.penalties = tensor(penalties)
        self.logprobs = self.logprob = self.top_ids = self.top_logprob = None
        if logprobs is not None:
            from .random import logprob_want
            want = logprob_want(list(logprobs), n)
            cells = (n, int(budgets.max()), max(int(want.max()), 1))
            self.logprobs, self.top_ids = tensor(want), tensor(np.full(cells, -1))
            self.logprob = cls.from_numpy(np.zeros(cells[:2], np.float32), requires_grad=False)
            self.top_logprob = cls.from_numpy(np.zeros(cells, np.float32), requires_grad=False)
        self.guide = self.guide_state = None
        if guide is not None:
            allow, states, edges, start = (np.asarray(a) for a in guide)
            assert all(a.dtype == np.int32 for a in (allow, states, edges, start)) and allow.ndim == 2 and allow.shape[0] >= 1 and \
                states.shape == (allow.shape[0], 4) and edges.ndim == 2 and edges.shape[0] >= 1 and edges.shape[1] == 2 and start.shape == (n,) and \
                (start >= -1).all() and (start < allow.shape[0]).all(), \
                "RequestPool: guide= is the int32 tables of guide.compile_guides - allow (S, W), states (S, 4), edges (E, 2), start (%d,) within -1 .. S - 1 " \
                "(got %s)" % (n, [(str(a.dtype), a.shape) for a in (allow, states, edges, start)])
            self.guide = (tensor(allow), tensor(states), tensor(edges))
            self.guide_state = tensor(np.stack([start, np.zeros(n, np.int32)], axis=1))
        # queue[1] as a tensor of its own that shares the word (indexing a tensor copies: the poll would be a launch and a read)
        if isinstance(getattr(self.queue, "data", None), np.ndarray):
            self._finished = cls.from_numpy(self.queue.data[1:2], requires_grad=False)
        else:
            from .autograd.hip.ops import _idx_view
            self._finished = _idx_view(self.queue, (slice(1, 2),))
        self.token_budget, self.cu = None, None
        if token_budget is None:
            self.ids, self.position_ids = tensor(np.zeros((self.slots, self.chunk))), tensor(np.zeros((self.slots, self.chunk)))
            self.max_steps = int((-(-lengths // self.chunk) + budgets).sum())      # every request alone in turn: no schedule takes longer
        else:
            assert int(token_budget) == token_budget and token_budget >= self.slots, \
                "RequestPool: token_budget is a number of token rows >= the %d slots, got %s" % (self.slots, token_budget)
            self.token_budget = int(token_budget)
            self.ids, self.position_ids = tensor(np.zeros((1, self.token_budget))), tensor(np.zeros((1, self.token_budget)))
            self.cu = tensor(np.zeros(self.slots + 1))
            self.max_steps = int((lengths + budgets).sum())                        # a prompt token a step at the least: no schedule takes longer
        if self.paged:
            cache.reset(prefix_blocks=self.prefix_blocks)
        else:
            cache.reset()
        cache.lengths = None            # the positions move on the device from here on: the host mirror is an upper bound only
        cache.length = cache.capacity

    @property
    def pos(self):
        return self.cache.pos

    def commit(self, nxt, eos=None) -> None:
        """one `serve_commit`: `nxt` (slots,) or (slots, 1) int32 are the tokens the step has just drawn (ignored for slots that
        are free or prefilling); with a token budget, one `serve_commit_packed`; with a paged cache, one `serve_commit_paged`"""
        if self.paged:
            c = self.cache
            nxt.serve_commit_paged(self.prompts, self.prompt_len, self.budget, self.out, self.out_len, self.queue, self.req, c.pos, self.count,
                                   self.ids, self.position_ids, self.last, c.block_table, c.held, c.free, c.block_size, self.prefix_blocks, eos=eos)
            return
        if self.cu is not None:
            nxt.serve_commit_packed(self.prompts, self.prompt_len, self.budget, self.out, self.out_len, self.queue, self.req, self.cache.pos,
                                    self.count, self.cu, self.ids, self.position_ids, self.last, self.cache.capacity, self.chunk, eos=eos)
            return
        nxt.serve_commit(self.prompts, self.prompt_len, self.budget, self.out, self.out_len, self.queue, self.req, self.cache.pos, self.count,
                         self.ids, self.position_ids, self.last, self.cache.capacity, eos=eos)

    def admit(self, eos=None) -> None:
        """the first admissions: one commit with every slot free (what it is given as `nxt` is ignored)"""
        self.commit(self._no_tokens, eos=eos)

    def finished(self) -> int:
        """requests finished so far: a host READ of one word, queue[1]"""
        return int(self._finished.numpy()[0])
