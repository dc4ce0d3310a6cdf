"""which lg_attention_* entry a fused attention op takes, and what the eight launch entries share through the C ABI: an empty
batch, and the first error of a call that is wrong in two ways.  The numerics of every entry are the ground of
test_hip_attention_masked.py, test_hip_attention_long.py, test_hip_attention_dropout.py and test_hip_bert.py; here only the
routing: a plain call through a tail or dropout kernel would give the same bits from a slower launch."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import random as lrandom
from test_hip_dropout import LG_EINVAL

pytestmark = pytest.mark.gpu

PLAIN, MASKED, LONG, DROPOUT = ((stem + "fwd_f32", stem + "bwd_f32") for stem in
                                ("lg_attention_", "lg_attention_masked_", "lg_attention_long_", "lg_attention_dropout_"))


class Recorder:
    """the loaded library, noting every attention launch entry that is called (a lookup alone is none)"""
    def __init__(self, handle):
        self._handle, self.calls = handle, []

    def __getattr__(self, name):
        entry = getattr(self._handle, name)
        if not (name.startswith("lg_attention_") and name.endswith("_f32")):
            return entry

        def noted(*args):
            self.calls.append(name)
            return entry(*args)
        return noted


@pytest.fixture
def recorder(hip, monkeypatch):
    from lightgrad_amd.autograd.hip import lib as L
    rec = Recorder(L.lib())
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


def tensors(hip, *shapes, seed=3):
    rng = np.random.RandomState(seed)
    return [hip.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)) for shape in shapes]


def mask_of(hip, s):
    m = np.ones((1, s), np.float32)
    m[0, s - 2:] = 0
    return hip.from_numpy(m, requires_grad=False)


OPS = [("attention", 32, False, 0.0, PLAIN), ("attention", 32, False, 0.5, DROPOUT),
       ("masked_attention", 5, False, 0.0, MASKED), ("masked_attention", 32, True, 0.0, MASKED), ("masked_attention", 5, True, 0.5, DROPOUT),
       ("long_attention", 131, False, 0.0, LONG), ("long_attention", 131, False, 0.5, DROPOUT)]


@pytest.mark.parametrize("op,s,masked,dropout,entries", OPS, ids=["%s-%d-%s-p%g" % (c[0], c[1], "mask" if c[2] else "nomask", c[3]) for c in OPS])
def test_entries_of_the_three_ops(hip, recorder, op, s, masked, dropout, entries):
    light.manual_seed(1)
    q, k, v = tensors(hip, *[(1, s, 32)] * 3)
    kwargs = {"dropout": dropout}
    if masked:
        kwargs["mask"] = mask_of(hip, s)
    out = getattr(q, op)(k, v, heads=1, scale=32 ** -0.5, **kwargs)
    out.backward(allow_fill=True)
    assert recorder.calls == list(entries)
    assert all(np.isfinite(t.grad.numpy()).all() for t in (q, k, v))


NODE = [(32, False, 0.0, PLAIN), (32, True, 0.0, MASKED), (20, False, 0.0, MASKED), (160, False, 0.0, LONG),
        (32, False, 0.5, DROPOUT), (160, False, 0.5, DROPOUT)]


@pytest.mark.parametrize("s,masked,dropout,entries", NODE, ids=["%d-%s-p%g" % (c[0], "mask" if c[1] else "nomask", c[2]) for c in NODE])
def test_entries_of_self_attention(hip, recorder, s, masked, dropout, entries):
    light.manual_seed(1)
    hidden, heads = 64, 2
    x, wq, bq, wk, bk, wv, bv = tensors(hip, (1, s, hidden), (hidden, hidden), (hidden,), (hidden, hidden), (hidden,), (hidden, hidden), (hidden,))
    kwargs = {"dropout": dropout}
    if masked:
        kwargs["mask"] = mask_of(hip, s)
    out = x.self_attention(wq, bq, wk, bk, wv, bv, heads=heads, scale=(hidden // heads) ** -0.5, **kwargs)
    out.backward(allow_fill=True)
    assert recorder.calls == list(entries)
    assert all(np.isfinite(t.grad.numpy()).all() for t in (x, wq, bq, wk, bk, wv, bv))


SENTINEL = 3.0


def c_abi_calls(hip, s, d=32, heads=1):
    """(forward, backward) callers of every family over operands of ONE batch element - `batch` is what the caller says - and the
    tensors they would write"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    w = heads * d
    q, k, v, g = tensors(hip, *[(1, s, w)] * 4)
    o, dq, dk, dv = (hip.from_numpy(np.full((1, s, w), SENTINEL, np.float32)) for _ in range(4))
    pr = hip.from_numpy(np.full((1, heads, s, s), SENTINEL, np.float32))
    base = hip.from_numpy(np.zeros(1, np.uint64))
    keep = (q, k, v, g, o, dq, dk, dv, pr, base)

    def forward(entry, batch=1, S=s, q_ptr=None):
        tail = () if entry == PLAIN[0] else (None, 0)
        if entry == DROPOUT[0]:
            tail += (0.5, base.ptr)
        return getattr(lib, entry)(q.ptr if q_ptr is None else q_ptr, w, s * w, k.ptr, w, s * w, v.ptr, w, s * w, o.ptr, w, s * w, pr.ptr,
                                   batch, heads, S, d, 0.2, *tail)

    def backward(entry, batch=1):
        tail = (0.5, base.ptr) if entry == DROPOUT[1] else ()
        return getattr(lib, entry)(q.ptr, w, s * w, k.ptr, w, s * w, v.ptr, w, s * w, g.ptr, w, s * w, pr.ptr, dq.ptr, w, s * w,
                                   dk.ptr, w, s * w, dv.ptr, w, s * w, batch, heads, s, d, 0.2, *tail)
    return lib, forward, backward, (o, dq, dk, dv, pr), keep


@pytest.mark.parametrize("s,families", [(32, (PLAIN, MASKED, DROPOUT)), (160, (LONG, DROPOUT))], ids=["s32", "s160"])
def test_empty_batch(hip, s, families):
    lib, forward, backward, written, _keep = c_abi_calls(hip, s)
    light.manual_seed(4)
    before = lrandom.get_state("hip")
    for fwd, bwd in families:
        if fwd == DROPOUT[0]:
            assert forward(fwd, batch=0) == LG_EINVAL                    # an empty batch draws nothing: refused, not skipped
            message = lib.lg_last_error()
            assert fwd.encode() in message and b"batch" in message, message
        else:
            assert forward(fwd, batch=0) == 0, fwd
        assert backward(bwd, batch=0) == 0, bwd
    assert lrandom.get_state("hip") == before
    for t in written:
        assert (t.numpy() == SENTINEL).all()


@pytest.mark.parametrize("entry,bad_s", [(PLAIN[0], 48), (MASKED[0], 129), (LONG[0], 128), (DROPOUT[0], 513)],
                         ids=["plain", "masked", "long", "dropout"])
def test_first_error_wins(hip, entry, bad_s):
    """an unsupported length AND a misaligned q: the length is what the message names"""
    lib, forward, _backward, written, keep = c_abi_calls(hip, 32)
    assert forward(entry, S=bad_s, q_ptr=keep[0].ptr + 4) == LG_EINVAL
    message = lib.lg_last_error()
    assert b"unsupported" in message and entry.encode() + b":" in message, message
    for t in written:
        assert (t.numpy() == SENTINEL).all()
