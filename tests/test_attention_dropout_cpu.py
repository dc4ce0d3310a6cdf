"""attention with dropout inside the fused kernels as far as it can be seen without a GPU: the library exports the three entry
points, the host-only predicate answers, the prototype table carries them, and the model on the CPU backend still takes the
composite - one call of the stream per attention, four per forward of a one-layer model"""
import ctypes
import numpy as np
import lightgrad_amd as light
from lightgrad_amd import CpuTensor, random as lrandom
from lightgrad_amd.autograd.hip import lib as hiplib
from test_bert_cpu import bert

SYMBOLS = ("lg_attention_dropout_supported", "lg_attention_dropout_fwd_f32", "lg_attention_dropout_bwd_f32")


def test_the_library_exports_the_dropout_forms():
    handle = ctypes.CDLL(hiplib.LIB_PATH)
    for name in SYMBOLS:
        assert getattr(handle, name) is not None, name


def test_the_supported_table_needs_no_device():
    fits = hiplib.load_library().lg_attention_dropout_supported
    assert all(fits(s, d) == 1 for s in range(1, 513) for d in (32, 64))
    assert all(fits(s, d) == 0 for s in (0, -3, 513) for d in (32, 64))
    assert all(fits(s, d) == 0 for s in (1, 128, 512) for d in (16, 48, 128))


def test_the_prototype_table_carries_them():
    masked_fwd, masked_bwd = hiplib.PROTOTYPES["lg_attention_masked_fwd_f32"], hiplib.PROTOTYPES["lg_attention_masked_bwd_f32"]
    assert hiplib.PROTOTYPES["lg_attention_dropout_supported"] == (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64])
    # the argument lists of the masked forms, then the probability and the word that holds the call's number
    tail = [ctypes.c_double, ctypes.c_void_p]
    assert hiplib.PROTOTYPES["lg_attention_dropout_fwd_f32"] == (masked_fwd[0], masked_fwd[1] + tail)
    assert hiplib.PROTOTYPES["lg_attention_dropout_bwd_f32"] == (masked_bwd[0], masked_bwd[1] + tail)


def _model(positions):
    np.random.seed(5)
    model = bert.BertForMaskedLM(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, vocab_size=60,
                                 max_position_embeddings=positions, type_vocab_size=2, hidden_dropout_prob=0.1,
                                 attention_probs_dropout_prob=0.1)
    assert model.training
    return model


def test_the_cpu_backend_still_takes_the_composite():
    assert not any(hasattr(CpuTensor, name) for name in ("attention", "masked_attention", "long_attention", "self_attention"))
    rng = np.random.RandomState(1)
    for s, masked in ((20, True), (160, False)):
        model = _model(s)
        ids = CpuTensor.from_numpy(rng.randint(0, 60, (2, s)).astype(np.int32), requires_grad=False)
        mask = None
        if masked:
            m = np.ones((2, s), np.float32)
            m[0, 15:] = 0
            m[1, 9:] = 0
            mask = CpuTensor.from_numpy(m, requires_grad=False)
        light.manual_seed(77)
        for forward in (1, 2):
            logits = model(ids, attention_mask=mask)
            # embeddings, probabilities, attention output, layer output: four calls of the stream per forward of one layer
            assert lrandom.get_state("cpu") == (77, 4 * forward)
        assert logits.shape == (2, s, 60) and np.isfinite(logits.numpy()).all()
        logits.sum().backward()
        assert lrandom.get_state("cpu") == (77, 8)                     # the backward draws nothing
        assert all(p.grad is not None and np.isfinite(p.grad.numpy()).all() for p in model.parameters())
