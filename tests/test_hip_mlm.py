"""The masked-LM objective on the GPU: the ignoring cross-entropy at the smallest shape of every dispatch path against the float64
reference and the numpy backend, `mlm_mask` bit for bit against the numpy backend, and a captured step that masks a fresh batch
at every replay."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor, random as lrandom
from test_dropout_cpu import BERT_CFG, BERT_IDS, build_bert
from test_mlm_cpu import (RTOL, ATOL, MASK, VOCAB, SPECIAL, reference_cross_entropy, ignoring_case, loss_and_grad,
                          assert_gathered_form_equals_all_positions)

pytestmark = pytest.mark.gpu

# rows kernel with a partly empty last block; held 8 x 1024; held 16 x 1024; held 60 x 512 with unaligned row starts; wide
SHAPES = [(7, 33), (5, 4097), (5, 8200), (5, 30522), (3, 30700)]


def check_against_reference(hip, logits, labels, ignore_index, reference_logits=None):
    want_loss, want_grad = reference_cross_entropy(logits if reference_logits is None else reference_logits, labels, ignore_index)
    loss, grad = loss_and_grad(hip, logits, labels, ignore_index=ignore_index)
    print("loss %.9g want %.9g, max gradient error %.3g" % (loss, want_loss, np.abs(grad - want_grad).max()))
    np.testing.assert_allclose(loss, want_loss, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad, want_grad, rtol=RTOL, atol=ATOL)
    zero_rows = grad[labels == ignore_index]
    assert np.array_equal(zero_rows, np.zeros_like(zero_rows)) and not np.signbit(zero_rows).any()      # +0.0, sign bit included
    return loss, grad


@pytest.mark.parametrize("shape", SHAPES)
def test_ignore_index_on_every_dispatch_path(hip, shape):
    logits, labels = ignoring_case(*shape, -100, np.int64)
    assert labels[0] == labels[-1] == -100 and (labels != -100).sum() >= 1
    loss, grad = check_against_reference(hip, logits, labels, -100)
    cpu_loss, cpu_grad = loss_and_grad(CpuTensor, logits, labels, ignore_index=-100)
    np.testing.assert_allclose(loss, cpu_loss, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad, cpu_grad, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64])
@pytest.mark.parametrize("shape", [(7, 33), (5, 4097)])
def test_ignore_index_label_dtypes(hip, shape, dtype):
    for ignore_index in (-100, 0):
        check_against_reference(hip, *ignoring_case(*shape, ignore_index, dtype), ignore_index)


@pytest.mark.parametrize("shape", SHAPES)
def test_ignored_rows_may_hold_nan_or_infinity(hip, shape):
    clean, labels = ignoring_case(*shape, -100, np.int32)
    logits = clean.copy()
    logits[0] = np.nan
    logits[-1, ::3] = np.inf
    logits[-1, 1] = -np.inf
    loss, grad = check_against_reference(hip, logits, labels, -100, reference_logits=clean)
    assert np.isfinite(loss) and np.isfinite(grad).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_all_rows_ignored(hip, shape):
    logits = np.random.RandomState(3).standard_normal(shape).astype(np.float32)
    loss, grad = loss_and_grad(hip, logits, np.full(shape[0], -100, np.int64), ignore_index=-100)
    assert np.isnan(loss)
    assert np.array_equal(grad, np.zeros(shape, np.float32)) and not np.signbit(grad).any()
    from lightgrad_amd.autograd.hip import HipDevice
    HipDevice.synchronize()                                               # raises if a kernel has set a status flag


@pytest.mark.parametrize("shape", SHAPES)
def test_no_row_ignored_is_the_plain_loss(hip, shape):
    rng = np.random.RandomState(4)
    logits, labels = (rng.standard_normal(shape) * 2).astype(np.float32), rng.randint(0, shape[1], shape[0]).astype(np.int64)
    plain = loss_and_grad(hip, logits, labels)
    again = loss_and_grad(hip, logits, labels, ignore_index=None)
    assert plain[0].tobytes() == again[0].tobytes() and plain[1].tobytes() == again[1].tobytes()       # None: the old call's bits
    got = loss_and_grad(hip, logits, labels, ignore_index=-100)
    np.testing.assert_allclose(got[0], plain[0], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got[1], plain[1], rtol=RTOL, atol=ATOL)


def test_without_the_hook_there_is_no_host_fallback(hip, monkeypatch):
    logits, labels = ignoring_case(7, 33, -100, np.int64)
    y3 = hip.from_numpy(logits.reshape(7, 3, 11))
    with pytest.raises(NotImplementedError, match="fused hook"):
        light.loss.cross_entropy(y3, hip.from_numpy(labels, requires_grad=False), ignore_index=-100)
    monkeypatch.setattr(hip, "_fused_cross_entropy", None)
    with pytest.raises(NotImplementedError, match="switched off"):
        light.loss.cross_entropy(hip.from_numpy(logits), hip.from_numpy(labels, requires_grad=False), ignore_index=-100)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("shape", [(4, 16), (3, 129), (1,), (0, 4)])
def test_mlm_mask_equals_the_numpy_backend(hip, shape, dtype):
    ids = np.random.RandomState(7).randint(0, VOCAB, shape).astype(dtype)
    seed = 11
    light.manual_seed(seed)
    for call in range(2):
        want = CpuTensor.from_numpy(ids, requires_grad=False).mlm_mask(0.5, MASK, VOCAB, special_ids=SPECIAL)
        got = hip.from_numpy(ids, requires_grad=False).mlm_mask(0.5, MASK, VOCAB, special_ids=SPECIAL)
        assert lrandom.get_state("hip") == lrandom.get_state("cpu") == (seed, call + 1)
        for g, w in zip(got, want):
            assert g.dtype == dtype and tuple(g.shape) == tuple(shape) and not g.requires_grad
            np.testing.assert_array_equal(g.numpy(), w.numpy())


def test_gathered_positions_give_the_all_positions_loss(hip):
    assert_gathered_form_equals_all_positions(hip, lambda p: p.hip())


def test_captured_step_masks_a_fresh_batch_at_every_replay(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    seed, p = 21, 0.3
    cpu_model = build_bert()
    hip_model = build_bert().map_parameters(lambda q: q.hip())

    def make(T, model):
        ids = T.from_numpy(BERT_IDS, requires_grad=False)

        def step():
            masked, labels = ids.mlm_mask(p, MASK, BERT_CFG["vocab_size"], special_ids=SPECIAL)
            loss = light.loss.cross_entropy(model(masked).reshape(-1, BERT_CFG["vocab_size"]), labels.reshape(-1), ignore_index=-100)
            for q in model.parameters():
                q.zero_grad()
            loss.backward()
            return masked, loss
        return step

    light.manual_seed(seed)
    cpu_step = make(CpuTensor, cpu_model)
    expected = [[t.numpy().copy() for t in cpu_step()] for _ in range(3)]
    assert lrandom.get_state("cpu") == (seed, 3)
    assert not np.array_equal(expected[0][0], expected[1][0]) and not np.array_equal(expected[1][0], expected[2][0])
    assert all(np.isfinite(e[1]) for e in expected)

    step = make(hip, hip_model)
    step()                                                                # eager once: pool, kernels
    graph = HipGraph()
    with graph.capture():
        masked, loss = step()
    light.manual_seed(seed)                                               # after the capture: a replay reads the state from memory
    for k in range(3):
        graph.replay()
        np.testing.assert_array_equal(masked.numpy(), expected[k][0], err_msg="replay %d" % k)
        got, want = loss.item(), float(expected[k][1])
        print("replay %d: loss %.7f, numpy backend %.7f" % (k, got, want))
        assert abs(got - want) <= 1e-5 * abs(want), (k, got, want)
    assert lrandom.get_state("hip") == (seed, 3)
    graph.destroy()


def test_vocabulary_width_loss_is_one_launch_more(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    logits, labels = ignoring_case(5, 30522, -100, np.int64)
    y, lab = hip.from_numpy(logits), hip.from_numpy(labels.clip(0), requires_grad=False)
    counts = {}
    for name, kwargs in (("plain", {}), ("ignoring", {"ignore_index": -100})):
        light.loss.cross_entropy(y, lab, **kwargs)
        graph = HipGraph()
        with graph.capture():
            light.loss.cross_entropy(y, lab, **kwargs)
        counts[name] = graph.kernel_count()
        graph.destroy()
    assert 0 < counts["plain"] and counts["ignoring"] <= counts["plain"] + 1, counts
