"""lg_gemm_bf16_f32 and the ops on it (dot_bf16, linear_bf16, bf16_round, nn.Linear(precision="bf16")) on the GPU.

Yardsticks: the float64 product of the `bf16_round`ed operands (relative Frobenius <= 1e-5 plus an elementwise bound), EXACT
cases (small integers, a product with the identity) that any fragment, index or edge mistake breaks whatever the summation
order, and the CPU backend on identical inputs."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from common import assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius
from bf16_cases import (SHAPES, K_SWEEP, LAYOUTS, TOL, round_np, product64, operands, integer_operands, rel, assert_close_to_product,
                        TwoLayer, two_layer_problem, load_bert_example, tiny_bert, bert_mlm_step, bert_cpu_yardsticks)

pytestmark = pytest.mark.gpu

LG_EINVAL = -1


def _lib():
    from lightgrad_amd.autograd.hip import lib as L
    return L.lib()


def _stored(x, trans):
    """the host array whose row-major bytes hold x in the layout `trans` asks for"""
    return np.ascontiguousarray(x.T) if trans else np.ascontiguousarray(x)


def gemm(hip, tA, tB, a, b, bias=None, c0=None, accumulate=0, pad=0, shift=0):
    """C = r(a) @ r(b) through the raw C ABI.  `pad` widens every buffer by that many columns and `shift` moves the operands'
    first column inside it (leading dimensions larger than the extents, base addresses off the 16-byte grid)."""
    (M, K), N = a.shape, b.shape[1]
    sa, sb = _stored(a, tA), _stored(b, tB)
    rng = np.random.RandomState(1)

    def widen(x):
        wide = rng.uniform(-3, 3, (x.shape[0], x.shape[1] + pad)).astype(np.float32)
        wide[:, shift:shift + x.shape[1]] = x
        return wide
    wa, wb = widen(sa), widen(sb)
    wc = widen(c0 if c0 is not None else np.full((M, N), -7.0, np.float32))
    ta, tb, tc = hip.from_numpy(wa), hip.from_numpy(wb), hip.from_numpy(wc)
    tbias = hip.from_numpy(bias) if bias is not None else None
    rc = _lib().lg_gemm_bf16_f32(tA, tB, M, N, K, ta.ptr + 4 * shift, wa.shape[1], tb.ptr + 4 * shift, wb.shape[1],
                                 tc.ptr + 4 * shift, wc.shape[1], tbias.ptr if tbias is not None else None, accumulate)
    assert rc == 0, _lib().lg_last_error()
    out = tc.numpy()
    untouched = np.ones(out.shape, bool)
    untouched[:, shift:shift + N] = False
    np.testing.assert_array_equal(out[untouched], wc[untouched])               # nothing outside C is written
    return out[:, shift:shift + N]


@pytest.mark.parametrize("mnk", SHAPES + [(40, 72, k) for k in K_SWEEP], ids=lambda s: "x".join(map(str, s)))
def test_all_layouts_against_float64(hip, mnk):
    M, N, K = mnk
    a, b, ref = operands(M, N, K)
    for tA, tB, tag in LAYOUTS:
        assert_close_to_product(gemm(hip, tA, tB, a, b), ref, K, (tag, mnk))


@pytest.mark.parametrize("mnk", [(33, 31, 35), (129, 127, 33), (40, 72, 17), (16, 24, 3000)], ids=lambda s: "x".join(map(str, s)))
def test_column_slices_of_wider_buffers(hip, mnk):
    """ld > extent and base addresses 4, 8 and 12 bytes off the 16-byte grid, operands and C alike"""
    M, N, K = mnk
    a, b, ref = operands(M, N, K)
    for (tA, tB, tag), shift in zip(LAYOUTS, (1, 2, 3, 1)):
        assert_close_to_product(gemm(hip, tA, tB, a, b, pad=5, shift=shift), ref, K, (tag, mnk, "shift", shift))


@pytest.mark.parametrize("mnk", [(1, 1, 1), (3, 5, 2), (65, 129, 67), (129, 127, 33), (40, 72, 256), (257, 130, 8), (128, 128, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_small_integers_are_exact(hip, mnk):
    a, b, want = integer_operands(*mnk)
    for tA, tB, tag in LAYOUTS:
        np.testing.assert_array_equal(gemm(hip, tA, tB, a, b), want, err_msg=tag)
        np.testing.assert_array_equal(gemm(hip, tA, tB, a, b, pad=3, shift=1), want, err_msg=tag + " sliced")


def test_identity_returns_the_rounded_operand(hip):
    """r(A) @ I == r(A) and I @ r(B) == r(B) bit for bit with an asymmetric operand: a swapped row / column map cannot pass"""
    a = np.random.RandomState(5).uniform(-1, 1, (192, 160)).astype(np.float32)
    ra = round_np(a)
    for tA, tB, tag in LAYOUTS:
        np.testing.assert_array_equal(gemm(hip, tA, tB, a, np.eye(160, dtype=np.float32)), ra, err_msg=tag)
        np.testing.assert_array_equal(gemm(hip, tA, tB, np.eye(192, dtype=np.float32), a), ra, err_msg=tag)


def test_bf16_round_on_the_device(hip):
    x = np.array([1.00390625, 1.01171875, 3.3895314e38, 3.4e38, -3.4e38, 0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    got = light.bf16_round(hip.from_numpy(x))
    assert not got.requires_grad and got.ctx is None
    np.testing.assert_array_equal(got.numpy().view(np.uint32)[:-1], round_np(x).view(np.uint32)[:-1])
    assert np.isnan(got.numpy()[-1])
    bits = np.random.RandomState(2).randint(0, 2 ** 32, 70001, dtype=np.uint64).astype(np.uint32).view(np.float32)
    bits = bits[np.isfinite(bits) & (np.abs(bits) >= np.float32(2.0 ** -126))].reshape(-1, 1)[:60000].reshape(300, 200)
    np.testing.assert_array_equal(light.bf16_round(hip.from_numpy(bits)).numpy().view(np.uint32), round_np(bits).view(np.uint32))
    view = hip.from_numpy(bits).transpose(1, 0)                                # a strided view is gathered first
    np.testing.assert_array_equal(light.bf16_round(view).numpy(), round_np(bits).T)


def test_nan_and_inf_land_where_they_should(hip):
    M, N, K = 70, 40, 37
    a, b, _ = operands(M, N, K)
    a, b = a.copy(), b.copy()
    a[3, 36] = np.nan                # behind the first 32-deep step, inside a float4 that K cuts
    b[7, 2] = np.inf
    for tA, tB, tag in LAYOUTS:
        c = gemm(hip, tA, tB, a, b)
        nan, inf = np.zeros((M, N), bool), np.zeros((M, N), bool)
        nan[3, :] = True
        inf[:, 2] = True
        inf[3, 2] = False
        np.testing.assert_array_equal(np.isnan(c), nan, err_msg=tag)
        np.testing.assert_array_equal(np.isinf(c), inf, err_msg=tag)
        np.testing.assert_array_equal(np.sign(c[inf]), np.sign(round_np(a)[:, 7][inf[:, 2]]), err_msg=tag)


def test_c_abi_accumulate_bias_and_empty_extents(hip):
    lib = _lib()
    M, N, K = 70, 50, 40
    a, b, ref = operands(M, N, K)
    c0 = np.random.RandomState(3).uniform(-1, 1, (M, N)).astype(np.float32)
    bias = np.random.RandomState(4).uniform(-1, 1, (N,)).astype(np.float32)
    plain = gemm(hip, 0, 0, a, b)
    np.testing.assert_array_equal(gemm(hip, 0, 0, a, b, c0=c0, accumulate=1), c0 + plain)          # C_old + (fp32 sum): one rounding
    np.testing.assert_array_equal(gemm(hip, 0, 1, a, b, bias=bias), plain + bias)                  # (fp32 sum) + bias
    # the chunks along K (one tile, K = 3000) fold into the same epilogue
    a2, b2, ref2 = operands(16, 24, 3000)
    c2 = np.random.RandomState(5).uniform(-1, 1, (16, 24)).astype(np.float32)
    long_plain = gemm(hip, 0, 0, a2, b2)
    np.testing.assert_array_equal(gemm(hip, 0, 0, a2, b2, c0=c2, accumulate=1, pad=4, shift=1), c2 + long_plain)
    np.testing.assert_array_equal(gemm(hip, 1, 0, a2, b2, bias=bias[:24]), gemm(hip, 1, 0, a2, b2) + bias[:24])
    ta, tb, tc, tbias = hip.from_numpy(a), hip.from_numpy(b), hip.from_numpy(c0), hip.from_numpy(bias)
    assert lib.lg_gemm_bf16_f32(0, 0, M, N, K, ta.ptr, K, tb.ptr, N, tc.ptr, N, tbias.ptr, 1) == LG_EINVAL     # bias + accumulate
    assert b"bias" in lib.lg_last_error()
    assert lib.lg_gemm_bf16_f32(0, 0, M, N, K, ta.ptr, K - 1, tb.ptr, N, tc.ptr, N, None, 0) == LG_EINVAL       # lda < K
    assert lib.lg_gemm_bf16_f32(0, 0, M, N, K, ta.ptr, K, tb.ptr, N, tc.ptr, N - 1, None, 0) == LG_EINVAL       # ldc < N
    assert lib.lg_gemm_bf16_f32(0, 0, M, N, K, None, K, tb.ptr, N, tc.ptr, N, None, 0) == LG_EINVAL
    assert lib.lg_gemm_bf16_f32(0, 0, -1, N, K, ta.ptr, K, tb.ptr, N, tc.ptr, N, None, 0) == LG_EINVAL
    np.testing.assert_array_equal(tc.numpy(), c0)                                                  # a refused call writes nothing
    assert lib.lg_gemm_bf16_f32(0, 0, 0, N, K, ta.ptr, K, tb.ptr, N, tc.ptr, N, None, 0) == 0      # M = 0, N = 0: nothing happens
    assert lib.lg_gemm_bf16_f32(0, 0, M, 0, K, ta.ptr, K, tb.ptr, N, tc.ptr, N, None, 0) == 0
    assert lib.lg_gemm_bf16_f32(0, 0, M, N, 0, ta.ptr, K, tb.ptr, N, tc.ptr, N, None, 1) == 0      # K = 0, accumulate: C stays
    np.testing.assert_array_equal(tc.numpy(), c0)
    assert lib.lg_gemm_bf16_f32(0, 0, M, N, 0, ta.ptr, K, tb.ptr, N, tc.ptr, N, None, 0) == 0      # K = 0: the empty sum
    np.testing.assert_array_equal(tc.numpy(), np.zeros((M, N), np.float32))
    # K = 0 with a bias: C = 0 + bias, no operand is read (NULL operands are fine) - also into a padded C and for a 1 x 1 result
    wide = hip.from_numpy(np.full((M, N + 3), -7.0, np.float32))
    assert lib.lg_gemm_bf16_f32(0, 1, M, N, 0, None, 0, None, 0, wide.ptr + 4, N + 3, tbias.ptr, 0) == 0, lib.lg_last_error()
    expect = np.full((M, N + 3), -7.0, np.float32)
    expect[:, 1:1 + N] = bias
    np.testing.assert_array_equal(wide.numpy(), expect)
    one = hip.from_numpy(np.full((1, 1), -7.0, np.float32))
    assert lib.lg_gemm_bf16_f32(0, 0, 1, 1, 0, ta.ptr, 1, tb.ptr, 1, one.ptr, 1, tbias.ptr, 0) == 0
    np.testing.assert_array_equal(one.numpy(), bias[:1].reshape(1, 1))


@pytest.mark.parametrize("mnk", [(129, 127, 33), (16, 24, 3000)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_give_the_same_bits(hip, mnk):
    a, b, _ = operands(*mnk)
    for tA, tB, tag in LAYOUTS:
        np.testing.assert_array_equal(gemm(hip, tA, tB, a, b), gemm(hip, tA, tB, a, b), err_msg=tag)


# ---- the ops --------------------------------------------------------------------------------------------------------------

def _grads(T, fn, arrays, upstream, wants):
    tensors = [T.from_numpy(x.copy(), requires_grad=w) for x, w in zip(arrays, wants)]
    y = fn(*tensors)
    (y * T.from_numpy(upstream, requires_grad=False)).backward(allow_fill=True)
    return y.numpy(), [t.grad.numpy() if w else t.grad for t, w in zip(tensors, wants)]


@pytest.mark.parametrize("a_shape", [(65, 67), (2, 3, 33, 67)], ids=["2d", "tall"])
def test_dot_bf16_against_the_cpu_backend_and_float64(hip, a_shape):
    rng = np.random.RandomState(6)
    a, b = rng.uniform(-1, 1, a_shape).astype(np.float32), rng.uniform(-1, 1, (67, 129)).astype(np.float32)
    g = rng.uniform(-1, 1, a_shape[:-1] + (129,)).astype(np.float32)
    fn = lambda x, y: x.dot_bf16(y)           # noqa: E731
    y_hip, (ga, gb) = _grads(hip, fn, (a, b), g, (True, True))
    y_cpu, (ga_cpu, gb_cpu) = _grads(CpuTensor, fn, (a, b), g, (True, True))
    a2, g2 = a.reshape(-1, 67), g.reshape(-1, 129)
    for got, cpu, ref, what in [(y_hip, y_cpu, product64(a2, b), "y"), (ga, ga_cpu, product64(g2, b.T), "dA"), (gb, gb_cpu, product64(a2.T, g2), "dB")]:
        assert got.shape == cpu.shape, what
        assert rel(got, cpu) <= TOL and rel(got.reshape(ref.shape), ref) <= TOL, (what, rel(got, cpu), rel(got.reshape(ref.shape), ref))
    # a transposed view as the right operand is consumed in place: the same values
    bt = hip.from_numpy(np.ascontiguousarray(b.T)).transpose(1, 0)
    np.testing.assert_array_equal(hip.from_numpy(a).dot_bf16(bt).numpy(), y_hip)


@pytest.mark.parametrize("x_shape", [(33, 35), (2, 17, 35)], ids=["2d", "bsh"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no-bias"])
@pytest.mark.parametrize("x_grad", [True, False], ids=["dx", "no-dx"])
def test_linear_bf16_against_the_cpu_backend_and_float64(hip, x_shape, with_bias, x_grad):
    rng = np.random.RandomState(7)
    x, w = rng.uniform(-1, 1, x_shape).astype(np.float32), rng.uniform(-1, 1, (31, 35)).astype(np.float32)
    bias = rng.uniform(-1, 1, (31,)).astype(np.float32)
    g = rng.uniform(-1, 1, x_shape[:-1] + (31,)).astype(np.float32)
    arrays, wants = ((x, w, bias), (x_grad, True, True)) if with_bias else ((x, w), (x_grad, True))
    fn = lambda t, *rest: t.linear_bf16(*rest)           # noqa: E731
    y_hip, grads = _grads(hip, fn, arrays, g, wants)
    y_cpu, grads_cpu = _grads(CpuTensor, fn, arrays, g, wants)
    x2, g2 = x.reshape(-1, 35), g.reshape(-1, 31)
    refs = [product64(g2, w).reshape(x_shape), product64(g2.T, x2), g2.astype(np.float64).sum(axis=0)]
    assert rel(y_hip, y_cpu) <= TOL and rel(y_hip.reshape(-1, 31), product64(x2, w.T) + (bias if with_bias else 0.0)) <= TOL
    for got, cpu, ref, want, what in zip(grads, grads_cpu, refs, wants, ("dx", "dW", "db")):
        if not want:
            assert got is None, what
            continue
        assert got.shape == ref.shape and rel(got, cpu) <= TOL and rel(got, ref) <= TOL, (what, rel(got, cpu), rel(got, ref))


def test_a_lazy_relu_in_front_is_computed_first(hip):
    rng = np.random.RandomState(8)
    x, w = rng.uniform(-1, 1, (40, 24)).astype(np.float32), rng.uniform(-1, 1, (10, 24)).astype(np.float32)
    g = rng.uniform(-1, 1, (40, 10)).astype(np.float32)
    fn = lambda t, u: t.relu().linear_bf16(u)           # noqa: E731
    y_hip, (dx, dw) = _grads(hip, fn, (x, w), g, (True, True))
    y_cpu, (dx_cpu, dw_cpu) = _grads(CpuTensor, fn, (x, w), g, (True, True))
    assert rel(y_hip, product64(np.maximum(x, 0), w.T)) <= TOL
    assert rel(y_hip, y_cpu) <= TOL and rel(dx, dx_cpu) <= TOL and rel(dw, dw_cpu) <= TOL


def test_rank_and_dtype_errors(hip):
    f = lambda *s: hip.from_numpy(np.ones(s, np.float32))      # noqa: E731
    for a, b in [(f(4), f(4, 3)), (f(2, 4), f(4)), (f(2, 4), f(2, 4, 3)), (f(2, 3, 4), f(2, 4, 5))]:
        with pytest.raises(ValueError):
            a.dot_bf16(b)
    with pytest.raises(ValueError, match="do not align"):
        f(2, 5).dot_bf16(f(4, 3))
    with pytest.raises(ValueError):
        f(4).linear_bf16(f(3, 4))
    for other in (hip.from_numpy(np.ones((4, 3), np.int32)), hip.from_numpy(np.ones((4, 3), np.float64))):
        with pytest.raises(TypeError):
            f(2, 4).dot_bf16(other)
        with pytest.raises(TypeError):
            f(2, 3).linear_bf16(other)
    with pytest.raises(TypeError):
        light.bf16_round(hip.from_numpy(np.ones((4,), np.int32)))
    with pytest.raises(ValueError, match="bias"):
        f(2, 4).linear_bf16(f(3, 4), f(4))


# ---- a small model under the three forms of the optimizer step ------------------------------------------------------------------

STEPS = 3


def _two_layer(hip, precision, form):
    from lightgrad_amd.dist import DataParallel, SingleProcess
    w0, x, target = two_layer_problem()
    model = TwoLayer(precision)
    model.load_parameters(w0)
    model.map_parameters(lambda p: p.hip())
    if form == "plain":
        opt = light.optim.Adam(model.parameters(), lr=1e-2, fused=True, device_step=True)
    else:
        dp = DataParallel(model.parameters(), SingleProcess(), flatten=True)
        # the bound is never reached: the coefficient is exactly 1, the forms stay comparable
        opt = light.optim.Adam(model.parameters(), lr=1e-2, fused=True, device_step=True, **(dict(max_grad_norm=1e9) if form == "clip" else {}))
        dp.attach(opt)
        if form == "in_backward":
            opt.fuse_update_into_backward()
    tx, tt = hip.from_numpy(x, requires_grad=False), hip.from_numpy(target, requires_grad=False)

    def step():
        loss = light.loss.mse(model(tx), tt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    return model, opt, step


def _weights(model):
    return {n: p.numpy().copy() for n, p in model.named_parameters()}


@pytest.fixture(scope="module")
def three_forms(hip):
    out = {}
    for precision in (None, "bf16"):
        for form in ("plain", "clip", "in_backward"):
            model, opt, step = _two_layer(hip, precision, form)
            losses = [step().item() for _ in range(STEPS)]
            out[precision, form] = (losses, _weights(model))
    return out


def test_two_layer_model_three_forms_agree_where_the_fp32_model_agrees(three_forms):
    forms = ("plain", "clip", "in_backward")
    compared = 0
    for i, f in enumerate(forms):
        for h in forms[i + 1:]:
            for n in three_forms[None, f][1]:
                if np.array_equal(three_forms[None, f][1][n], three_forms[None, h][1][n]):
                    np.testing.assert_array_equal(three_forms["bf16", f][1][n], three_forms["bf16", h][1][n], err_msg="%s vs %s: %s" % (f, h, n))
                    compared += 1
    print("weights compared bit for bit: %d of %d" % (compared, 3 * 4))
    assert compared > 0
    w0 = two_layer_problem()[0]
    for form in forms:
        losses, weights = three_forms["bf16", form]
        assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]
        for n in weights:
            assert not np.array_equal(weights[n], w0[n]), (form, n)                            # every parameter was updated
        assert not np.array_equal(weights["l1.weight"], three_forms[None, form][1]["l1.weight"])       # ... by bf16 products


def test_two_layer_model_first_step_against_the_cpu_backend(hip):
    """one forward + backward of the model: loss and gradients against the CPU backend on the same inputs"""
    w0, x, target = two_layer_problem()
    got = {}
    for T, to in ((hip, lambda p: p.hip()), (CpuTensor, lambda p: p)):
        model = TwoLayer("bf16")
        model.load_parameters(w0)
        model.map_parameters(to)
        loss = light.loss.mse(model(T.from_numpy(x, requires_grad=False)), T.from_numpy(target, requires_grad=False))
        for p in model.parameters():
            p.zero_grad()
        loss.backward()
        got[T] = dict({n: p.grad.numpy() for n, p in model.named_parameters()}, loss=np.asarray(loss.item()))
    for n in got[hip]:
        assert rel(got[hip][n], got[CpuTensor][n]) <= TOL, (n, rel(got[hip][n], got[CpuTensor][n]))


def test_replayed_graph_gives_the_eager_bits(hip, three_forms):
    from lightgrad_amd.autograd.hip import GraphedStep
    model, opt, step = _two_layer(hip, "bf16", "plain")
    graphed = GraphedStep(step, optimizers=[opt], warmup=1)
    losses = [graphed().item() for _ in range(STEPS)]                  # one eager step, then the capture and two replays
    np.testing.assert_array_equal(losses, three_forms["bf16", "plain"][0])
    for n, w in _weights(model).items():
        np.testing.assert_array_equal(w, three_forms["bf16", "plain"][1][n], err_msg=n)
    graphed.destroy()


# ---- tiny-BERT with the decoder on the bf16 matrix cores ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bert():
    return load_bert_example()


def test_tiny_bert_masked_lm_step_against_the_float64_tape(hip, bert):
    """examples/bert.py with decoder_precision="bf16", batch 2, one masked-LM step: the loss and every parameter gradient within
    1e-5 (relative Frobenius) of the float64 run of the same tape in the same bf16 mode, or no further from it than twice the
    float32 CPU backend.  A rounding tie of an operand can flip on a 1e-7 difference upstream, so no tighter bound is derived;
    the CPU distances measured when this was written are in profiles/bf16_matmul.md.  The key projections' biases have a
    gradient of exactly zero in exact arithmetic and are bounded as rounding noise, like tests/test_hip_bert.py does."""
    values, cpu32, ref64 = bert_cpu_yardsticks(bert)
    model = tiny_bert(bert, "bf16")
    model.load_parameters(values)
    model.map_parameters(lambda p: p.hip())
    got = bert_mlm_step(bert, model, hip)
    noise = [n for n in ref64 if n.endswith(".key.bias")]
    for n in noise:
        assert np.abs(got[n]).max() < 1e-6 and np.abs(cpu32[n]).max() < 1e-6 and np.abs(ref64[n]).max() < 1e-12
    for n in ref64:
        print("%-60s hip %.2e  cpu32 %.2e" % (n, rel_frobenius(got[n], ref64[n]), rel_frobenius(cpu32[n], ref64[n])))
    rest = {n: a for n, a in ref64.items() if n not in noise}
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, rest, what="tiny-BERT, bf16 decoder")


def _tape_names(t):
    seen, names, stack = set(), [], [t.ctx]
    while stack:
        c = stack.pop()
        if c is None or id(c) in seen:
            continue
        seen.add(id(c))
        names.append(type(c).__name__)
        stack.extend(p.ctx for p in c.parent_tensors)
    return sorted(names)


def test_tiny_bert_without_the_switch_is_the_model_as_it_was(hip, bert):
    """decoder_precision=None: the tape, the logits, the loss and the parameter gradients bit for bit, and the captured step's
    kernel count, of a model built without the key; with "bf16" exactly one node of the tape changes.  (Both models run this
    build: that the path is also the PARENT's rests on nn.Linear.forward, which `precision=None` leaves as it was.)  One gradient is
    compared to 1e-6 (relative Frobenius) instead: the token-type table.  All 256 positions hold token type 0, and an id that
    occurs more than 32 times is scatter-added by several chunk leaders with float atomics (csrc/tail_jobs.h), in an order that
    is not fixed - two runs of the SAME model differ in its last bits (fp32 sums of 8 partial sums in another order).  Every other
    id of this batch occurs at most twice (word ids are drawn from 29 522 values, each position id twice) and takes the ordered,
    atomic-free path; the table is a leaf, so nothing else depends on it."""
    from lightgrad_amd.autograd.hip import HipGraph
    ids = hip.from_numpy(np.random.RandomState(1).randint(1000, 30522, (2, 128)).astype(np.int32), requires_grad=False)
    results = {}
    for tag, config in (("absent", dict(bert.TINY)), ("none", dict(bert.TINY, decoder_precision=None)), ("bf16", dict(bert.TINY, decoder_precision="bf16"))):
        np.random.seed(42)
        model = bert.BertForMaskedLM(**config).map_parameters(lambda p: p.hip())
        logits = model(ids)
        names, logits = _tape_names(logits), logits.numpy()
        light.manual_seed(3)
        loss = bert.mlm_forward_backward(model, ids)
        grads = {n: p.grad.numpy() for n, p in model.named_parameters()}
        graph = HipGraph()
        with graph.capture():
            bert.mlm_forward_backward(model, ids)
        results[tag] = (names, float(loss.item()), grads, graph.kernel_count(), logits)
        graph.destroy()
    absent, none, low = results["absent"], results["none"], results["bf16"]
    assert none[0] == absent[0] and "linear_bf16" not in none[0]
    assert none[1] == absent[1] and none[3] == absent[3]
    np.testing.assert_array_equal(none[4], absent[4])
    assert max(np.unique(np.asarray(ids.numpy()), return_counts=True)[1]) <= 32          # no hot word id: the ordered scatter-add
    for n in absent[2]:
        if n.endswith("token_type_embeddings.weight"):
            assert rel(none[2][n], absent[2][n]) <= 1e-6, n
        else:
            np.testing.assert_array_equal(none[2][n], absent[2][n], err_msg=n)
    assert low[0].count("linear_bf16") == 1
    assert abs(low[1] - none[1]) < 1e-2            # (the loss itself may not move by an fp32 ulp: the logits below do)
    assert rel(low[4], none[4]) > 1e-4
