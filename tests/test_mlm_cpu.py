"""The masked-LM objective on the numpy backend: `loss.cross_entropy(..., ignore_index=)` against a float64 reference written
here, `Tensor.mlm_mask` against the three-threshold rule evaluated from `random.words`, and the gathered form of the model."""
import os
import re
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor, random as lrandom
from conftest import ROOT
from test_dropout_cpu import BERT_CFG, BERT_IDS, build_bert

RTOL, ATOL = 2e-5, 1e-9                   # tests/test_hip_fused.py's for this loss against float64


def reference_cross_entropy(logits, labels, ignore_index):
    """float64: (loss, gradient of the logits) of the ignoring form; the ignored rows' logits are never looked at"""
    labels = np.asarray(labels).astype(np.int64)
    valid = labels != ignore_index
    n = int(valid.sum())
    grad = np.zeros(logits.shape, np.float64)
    x = logits[valid].astype(np.float64)
    picked = np.where(labels[valid] < 0, labels[valid] + logits.shape[1], labels[valid])
    z = x - x.max(axis=1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    if n == 0:
        return np.float64("nan"), grad
    nll = -np.log(p[np.arange(n), picked])
    p[np.arange(n), picked] -= 1.0
    grad[valid] = p / n
    return nll.sum() / n, grad


def ignoring_case(rows, cols, ignore_index, dtype, seed=0):
    """logits, labels with about half the rows ignored, the first and the last among them"""
    rng = np.random.RandomState(seed + rows * 7 + cols)
    logits = (rng.standard_normal((rows, cols)) * 3).astype(np.float32)
    low = 1 if ignore_index == 0 else 0
    labels = rng.randint(low, min(cols, 30000), rows).astype(dtype)
    ignored = np.zeros(rows, bool)
    ignored[[0, rows - 1]] = True
    ignored[rng.permutation(np.arange(1, rows - 1))[:(rows - 2) // 2]] = True
    labels[ignored] = ignore_index
    return logits, labels


def loss_and_grad(T, logits, labels, **kwargs):
    y = T.from_numpy(logits)
    loss = light.loss.cross_entropy(y, T.from_numpy(labels, requires_grad=False), **kwargs)
    y.zero_grad()
    loss.backward()
    return loss.numpy(), y.grad.numpy()


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64])
@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("shape", [(7, 33), (5, 4097)])
def test_ignore_index_against_float64(shape, ignore_index, dtype):
    logits, labels = ignoring_case(*shape, ignore_index, dtype)
    assert (labels == ignore_index).sum() >= 2 and (labels != ignore_index).sum() >= 2
    want_loss, want_grad = reference_cross_entropy(logits, labels, ignore_index)
    loss, grad = loss_and_grad(CpuTensor, logits, labels, ignore_index=ignore_index)
    assert loss.dtype == np.float32 and grad.dtype == np.float32
    np.testing.assert_allclose(loss, want_loss, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad, want_grad, rtol=RTOL, atol=ATOL)
    zero_rows = grad[labels == ignore_index]
    assert np.array_equal(zero_rows, np.zeros_like(zero_rows)) and not np.signbit(zero_rows).any()


def test_ignored_rows_may_hold_nan():
    logits, labels = ignoring_case(7, 33, -100, np.int64)
    want_loss, want_grad = reference_cross_entropy(logits, labels, -100)
    logits = logits.copy()
    logits[0] = np.nan
    logits[6, 3] = np.inf
    with np.errstate(invalid="ignore"):
        loss, grad = loss_and_grad(CpuTensor, logits, labels, ignore_index=-100)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    np.testing.assert_allclose(loss, want_loss, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad, want_grad, rtol=RTOL, atol=ATOL)
    assert not np.signbit(grad[[0, 6]]).any() and not grad[[0, 6]].any()


def test_no_valid_row_gives_nan_and_a_zero_gradient():
    logits = np.random.RandomState(1).standard_normal((5, 9)).astype(np.float32)
    loss, grad = loss_and_grad(CpuTensor, logits, np.full(5, -100, np.int32), ignore_index=-100)
    assert np.isnan(loss)
    assert np.array_equal(grad, np.zeros((5, 9), np.float32)) and not np.signbit(grad).any()


def test_ignore_index_none_is_the_call_without_it():
    rng = np.random.RandomState(2)
    logits, labels = rng.standard_normal((7, 33)).astype(np.float32), rng.randint(0, 33, 7).astype(np.int64)
    a, b = loss_and_grad(CpuTensor, logits, labels), loss_and_grad(CpuTensor, logits, labels, ignore_index=None)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_a_valid_label_is_wrapped_after_the_comparison():
    """-1 is the last class unless it is the ignore_index itself"""
    logits = np.random.RandomState(3).standard_normal((4, 6)).astype(np.float32)
    labels = np.array([-1, 2, -100, -6], np.int64)
    want_loss, want_grad = reference_cross_entropy(logits, labels, -100)
    loss, grad = loss_and_grad(CpuTensor, logits, labels, ignore_index=-100)
    np.testing.assert_allclose(loss, want_loss, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad, want_grad, rtol=RTOL, atol=ATOL)
    labels = np.array([-1, 2, -3, -6], np.int64)
    want_loss, want_grad = reference_cross_entropy(logits, labels, -1)
    loss, grad = loss_and_grad(CpuTensor, logits, labels, ignore_index=-1)
    np.testing.assert_allclose(loss, want_loss, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(grad, want_grad, rtol=RTOL, atol=ATOL)
    assert not grad[0].any() and grad[2, 3] < 0


# ---- token masking ---------------------------------------------------------------------------------------------------
MASK, VOCAB, SPECIAL = 49, 50, (0, 3)
MLM_SEED = 11
MLM_IDS = np.random.RandomState(9).randint(0, VOCAB, (4, 16))


def rule(seed, draw, ids, p, mask=MASK, vocab=VOCAB, special=SPECIAL, ignore=-100):
    """element by element, from the stream's words: (masked, labels, kind) with kind 0 unselected, 1 [MASK], 2 random, 3 unchanged"""
    flat = ids.reshape(-1)
    w = lrandom.words(seed, draw, 4 * flat.size).reshape(flat.size, 4)
    masked, labels, kind = flat.copy(), np.full_like(flat, ignore), np.zeros(flat.size, int)
    for i in range(flat.size):
        if int(flat[i]) in special or not int(w[i, 0]) < lrandom.threshold(p):
            continue
        labels[i] = flat[i]
        if int(w[i, 1]) < 3435973836:
            masked[i], kind[i] = mask, 1
        elif int(w[i, 1]) < 3865470566:
            masked[i], kind[i] = (int(w[i, 2]) * vocab) >> 32, 2
        else:
            kind[i] = 3
    return masked.reshape(ids.shape), labels.reshape(ids.shape), kind


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_mlm_mask_follows_the_three_threshold_rule(dtype):
    ids = MLM_IDS.astype(dtype)
    p = 0.5                                # enough selected elements among 64 for every kind to occur
    kinds = rule(MLM_SEED, 0, ids, p)[2]
    assert set(kinds) == {0, 1, 2, 3}, "the seed must produce every kind: %s" % np.bincount(kinds)
    assert np.isin(ids, SPECIAL).any()
    light.manual_seed(MLM_SEED)
    t = CpuTensor.from_numpy(ids, requires_grad=False)
    for draw in range(2):
        masked, labels = t.mlm_mask(p, MASK, VOCAB, special_ids=SPECIAL)
        assert lrandom.get_state("cpu") == (MLM_SEED, draw + 1)
        want_masked, want_labels, _ = rule(MLM_SEED, draw, ids, p)
        assert masked.dtype == labels.dtype == dtype and masked.shape == labels.shape == ids.shape
        assert not masked.requires_grad and not labels.requires_grad
        np.testing.assert_array_equal(masked.numpy(), want_masked)
        np.testing.assert_array_equal(labels.numpy(), want_labels)
        assert (labels.numpy()[np.isin(ids, SPECIAL)] == -100).all()            # specials are never selected
        assert (masked.numpy()[np.isin(ids, SPECIAL)] == ids[np.isin(ids, SPECIAL)]).all()
    first = rule(MLM_SEED, 0, ids, p)
    assert not np.array_equal(first[1] != -100, rule(MLM_SEED, 1, ids, p)[1] != -100)     # another call number, another mask
    light.manual_seed(MLM_SEED)
    again = light.data.mask_tokens(t, p, MASK, VOCAB, special_ids=SPECIAL)
    np.testing.assert_array_equal(again[0].numpy(), first[0])
    np.testing.assert_array_equal(again[1].numpy(), first[1])
    np.testing.assert_array_equal(lrandom.mlm_mask_words(MLM_SEED, 0, ids, p, MASK, VOCAB, SPECIAL)[0], first[0])


def test_mlm_mask_of_nothing_is_still_one_call():
    light.manual_seed(5)
    masked, labels = CpuTensor.from_numpy(np.zeros((0, 4), np.int32), requires_grad=False).mlm_mask(0.15, MASK, VOCAB)
    assert masked.shape == labels.shape == (0, 4) and lrandom.get_state("cpu") == (5, 1)
    CpuTensor.from_numpy(np.zeros((3,), np.int64), requires_grad=False).mlm_mask(0.15, MASK, VOCAB, ignore_index=-1)
    assert lrandom.get_state("cpu") == (5, 2)


def test_mlm_mask_refuses_what_it_cannot_do():
    ids = CpuTensor.from_numpy(np.zeros((3,), np.int32), requires_grad=False)
    with pytest.raises(ValueError):
        ids.mlm_mask(1.0, MASK, VOCAB)
    with pytest.raises(ValueError):
        ids.mlm_mask(0.15, MASK, VOCAB, special_ids=range(9))
    with pytest.raises(ValueError):
        ids.mlm_mask(0.15, MASK, VOCAB, ignore_index=-(1 << 40))
    with pytest.raises(TypeError):
        CpuTensor.from_numpy(np.zeros((3,), np.float32)).mlm_mask(0.15, MASK, VOCAB)


def test_selection_rate():
    """2^16 elements, p = 0.15: the binomial standard deviation of the share is 0.0014, the bound seven of them"""
    light.manual_seed(1234)
    ids = CpuTensor.from_numpy(np.random.RandomState(0).randint(5, 30522, 1 << 16).astype(np.int32), requires_grad=False)
    masked, labels = ids.mlm_mask(0.15, 103, 30522, special_ids=(0, 101, 102))
    selected = labels.numpy() != -100
    assert abs(selected.mean() - 0.15) <= 0.01, selected.mean()
    share = (masked.numpy()[selected] == 103).mean()
    assert abs(share - 0.8) <= 0.03, share
    assert 0 <= masked.numpy().min() and masked.numpy().max() < 30522


# ---- the gathered form of the model -----------------------------------------------------------------------------------
def gathered_problem():
    """the tiny batch, labels with 5 live positions, and their flat indices padded to 8 slots (the padding names row 0)"""
    labels = np.full(BERT_IDS.size, -100, np.int64)
    live = np.array([1, 4, 6, 9, 15])
    labels[live] = BERT_IDS.reshape(-1)[live]
    positions = np.concatenate([live, np.zeros(3, int)]).astype(np.int32)
    gathered = np.concatenate([labels[live], np.full(3, -100)]).astype(np.int64)
    return labels, positions, gathered


def model_loss_and_grads(T, model, labels, positions=None):
    ids = T.from_numpy(BERT_IDS, requires_grad=False)
    extra = {} if positions is None else {"masked_positions": T.from_numpy(positions, requires_grad=False)}
    logits = model(ids, **extra)
    loss = light.loss.cross_entropy(logits.reshape(-1, BERT_CFG["vocab_size"]), T.from_numpy(labels, requires_grad=False), ignore_index=-100)
    for p in model.parameters():
        p.zero_grad()
    loss.backward()
    return logits.shape, loss.item(), {n: p.grad.numpy().astype(np.float64) for n, p in model.named_parameters()}


def assert_gathered_form_equals_all_positions(T, to_backend):
    labels, positions, gathered = gathered_problem()
    model = build_bert().map_parameters(to_backend)
    shape_all, loss_all, grads_all = model_loss_and_grads(T, model, labels)
    shape_g, loss_g, grads_g = model_loss_and_grads(T, model, gathered, positions)
    assert tuple(shape_all) == (2, 8, 50) and tuple(shape_g) == (8, 50)
    assert abs(loss_g - loss_all) <= 1e-5 * abs(loss_all), (loss_g, loss_all)
    for n in grads_all:
        err = np.linalg.norm(grads_g[n] - grads_all[n]) / np.linalg.norm(grads_all[n])
        assert err <= 1e-5, (n, err)


def test_gathered_positions_give_the_all_positions_loss():
    assert_gathered_form_equals_all_positions(CpuTensor, lambda p: p)


def test_header_declares_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("lg_cross_entropy_ignore_f32", "lg_mlm_mask"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
