"""the long attention forms (129 .. 512 positions) as far as they can be seen without a GPU: the library exports them, the
host-only predicate answers, the prototype table carries them, and the model on the CPU backend still takes the composite"""
import ctypes
import numpy as np
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.hip import lib as hiplib
from test_bert_cpu import bert

SYMBOLS = ("lg_attention_long_supported", "lg_attention_long_fwd_f32", "lg_attention_long_bwd_f32")


def test_the_library_exports_the_long_forms():
    handle = ctypes.CDLL(hiplib.LIB_PATH)
    for name in SYMBOLS:
        assert getattr(handle, name) is not None, name


def test_the_supported_table_needs_no_device():
    handle = hiplib.load_library()
    fits = handle.lg_attention_long_supported
    assert fits(128, 32) == 0 and fits(129, 32) == 1 and fits(512, 32) == 1 and fits(513, 32) == 0
    assert fits(128, 64) == 0 and fits(129, 64) == 1 and fits(512, 64) == 1 and fits(513, 64) == 0
    assert fits(256, 48) == 0 and fits(256, 16) == 0 and fits(256, 128) == 0 and fits(0, 64) == 0 and fits(-200, 64) == 0
    # every length in between, and the short forms keep their own ground
    assert all(fits(s, d) == 1 for s in range(129, 513) for d in (32, 64))
    assert handle.lg_attention_supported(256, 64) == 0 and handle.lg_attention_masked_supported(129, 32) == 0


def test_the_prototype_table_carries_them():
    masked_fwd, masked_bwd = hiplib.PROTOTYPES["lg_attention_masked_fwd_f32"], hiplib.PROTOTYPES["lg_attention_masked_bwd_f32"]
    assert hiplib.PROTOTYPES["lg_attention_long_supported"] == (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64])
    # the argument lists of the masked forms, mask and its batch pitch included
    assert hiplib.PROTOTYPES["lg_attention_long_fwd_f32"] == masked_fwd
    assert hiplib.PROTOTYPES["lg_attention_long_bwd_f32"] == masked_bwd


def test_the_cpu_backend_still_takes_the_composite():
    assert not hasattr(CpuTensor, "long_attention") and not hasattr(CpuTensor, "self_attention")
    np.random.seed(5)
    model = bert.BertForMaskedLM(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, vocab_size=60,
                                 max_position_embeddings=160, type_vocab_size=2)
    rng = np.random.RandomState(1)
    s = 160
    ids = CpuTensor.from_numpy(rng.randint(0, 60, (2, s)).astype(np.int32), requires_grad=False)
    mask = np.ones((2, s), np.float32)
    mask[0, 150:] = 0
    mask[1, 97:] = 0
    logits = model(ids, attention_mask=CpuTensor.from_numpy(mask, requires_grad=False))
    assert logits.shape == (2, s, 60) and np.isfinite(logits.numpy()).all()
    logits.sum().backward()
    assert all(p.grad is not None and np.isfinite(p.grad.numpy()).all() for p in model.parameters())
