"""Hidden dropout inside the LayerNorm launches (csrc/rowwise.hip, lg_dropout_layernorm_*; ops `dropout_add_layer_norm` and
`layer_norm_dropout`): bit equality with the two-launch forms, where the mask lands, the stream's bookkeeping, graph replay, what
lies outside the operands through the C ABI, and argument checks.

Shapes are (rows, cols): one wave owns a row and lane l takes columns l, l + 64, ...; the stream's groups of four elements
straddle rows wherever cols is no multiple of 4."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import random as lrandom
from test_hip_dropout import SEEDS, LG_EINVAL
from test_hip_attention_dropout import burn

pytestmark = pytest.mark.gpu

# rows not divisible by 4 (a workgroup holds four); cols 1, below 64, no multiple of 4, no multiple of 64, above 256; one 3-D input
SHAPES = [(1, 1), (5, 3), (3, 65), (4, 128), (9, 130), (2, 300), (7, 768), (2, 5, 64)]
PROBS = (0.1, 0.5, 0.9)
SEED = SEEDS[1]


def ident(shape):
    return "x".join(str(d) for d in shape)


def operands(shape, seed=3):
    """x, residual, out_grad of `shape`, weight and bias of its last axis - continuous distributions, nothing exactly zero"""
    rng = np.random.RandomState(seed)
    x, r, g = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    w = rng.uniform(0.5, 1.5, shape[-1:]).astype(np.float32)
    b = rng.standard_normal(shape[-1:]).astype(np.float32)
    return x, r, g, w, b


def two_launches_add(x, r, w, b, p):
    return (x.dropout(p) if r is None else x.dropout(p, residual=r)).layer_norm(w, b)


def one_launch_add(x, r, w, b, p):
    return x.dropout_add_layer_norm(r, w, b, p)


def two_launches_after(x, r, w, b, p):
    return x.layer_norm(w, b).dropout(p)


def one_launch_after(x, r, w, b, p):
    return x.layer_norm_dropout(w, b, p)


def run(hip, form, arrays, p, residual, seed=SEED, draw=0):
    """{y, dx, dres, dw, db} of one forward and a backward from the random out_grad, at call number `draw` of the stream"""
    xa, ra, ga, wa, ba = arrays
    x, w, b = hip.from_numpy(xa), hip.from_numpy(wa), hip.from_numpy(ba)
    r = hip.from_numpy(ra) if residual else None
    light.manual_seed(seed)
    burn(hip, draw)
    y = form(x, r, w, b, p)
    (y * hip.from_numpy(ga, requires_grad=False)).backward(allow_fill=True)
    assert lrandom.get_state("hip") == (seed, draw + 1)
    out = {"y": y.numpy(), "dx": x.grad.numpy(), "dw": w.grad.numpy(), "db": b.grad.numpy()}
    if residual:
        out["dres"] = r.grad.numpy()
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_bit_equality_with_the_two_launch_form(hip, shape):
    arrays = operands(shape)
    for p in PROBS:
        for name, two, one, residual in (("dropout, add, normalise", two_launches_add, one_launch_add, True),
                                         ("dropout, normalise", two_launches_add, one_launch_add, False),
                                         ("normalise, dropout", two_launches_after, one_launch_after, False)):
            want, got = run(hip, two, arrays, p, residual), run(hip, one, arrays, p, residual)
            assert sorted(got) == sorted(want)
            for key in want:
                assert got[key].shape == want[key].shape
                np.testing.assert_array_equal(got[key], want[key], err_msg="%s, p = %.1f: %s" % (name, p, key))


# (5, 3) has 15 elements: the call number is one at which the reference mask alone drops and keeps something for every p
PLACEMENT = [((5, 3), 1), ((3, 65), 3), ((9, 130), 3), ((2, 5, 64), 3)]


@pytest.mark.parametrize("shape,draw", PLACEMENT, ids=[ident(s) for s, _ in PLACEMENT])
def test_the_mask_lands_where_the_stream_puts_it(hip, shape, draw):
    arrays = operands(shape, seed=8)
    xa, _, _, wa, ba = arrays
    n = xa.size
    with light.no_grad():
        plain = hip.from_numpy(xa).layer_norm(hip.from_numpy(wa), hip.from_numpy(ba)).numpy()
    for p in PROBS:
        keep = lrandom.keep_mask(SEED, draw, n, p).reshape(shape)
        assert 1 <= keep.sum() <= n - 1, (shape, p, int(keep.sum()))          # the reference alone: the check is not vacuous
        # mode 0 without a residual: x's gradient is exactly +0.0 at the dropped positions and nowhere else
        got = run(hip, one_launch_add, arrays, p, False, draw=draw)
        np.testing.assert_array_equal(got["dx"] == 0, ~keep, err_msg="dropout, normalise: p = %.1f" % p)
        assert not np.signbit(got["dx"][~keep]).any()
        # mode 1: the plain LayerNorm's value times s, rounded once, at the kept positions; +0.0 at the others
        got = run(hip, one_launch_after, arrays, p, False, draw=draw)
        np.testing.assert_array_equal(got["y"], np.where(keep, plain * lrandom.scale(p), np.float32(0)), err_msg="normalise, dropout: p = %.1f" % p)
        assert not np.signbit(got["y"][~keep]).any()


def test_bookkeeping(hip):
    seed = SEEDS[0]
    xa, ra, ga, wa, ba = operands((9, 130))
    x, r, w, b = (hip.from_numpy(a) for a in (xa, ra, wa, ba))
    light.manual_seed(seed)
    y = x.dropout_add_layer_norm(r, w, b, 0.0)
    z = x.layer_norm_dropout(w, b, 0.0)
    assert lrandom.get_state("hip") == (seed, 0)                          # p == 0: no new node, nothing drawn
    assert type(y.ctx).__name__ == type(z.ctx).__name__ == "layer_norm"
    np.testing.assert_array_equal(y.numpy(), (x + r).layer_norm(w, b).numpy())
    np.testing.assert_array_equal(z.numpy(), x.layer_norm(w, b).numpy())
    np.testing.assert_array_equal(x.dropout_add_layer_norm(None, w, b, 0.0).numpy(), z.numpy())
    draws = 0
    for form, res in ((one_launch_add, r), (one_launch_add, None), (one_launch_after, None)):
        y = form(x, res, w, b, 0.5)
        draws += 1
        assert lrandom.get_state("hip") == (seed, draws)                  # one call of the stream per forward
        (y * hip.from_numpy(ga, requires_grad=False)).backward(allow_fill=True)
        assert lrandom.get_state("hip") == (seed, draws)                  # the backward draws nothing
    # no rows: one workgroup still advances the stream
    empty = hip.from_numpy(np.ones((0, 130), np.float32))
    for form, res in ((one_launch_add, empty), (one_launch_add, None), (one_launch_after, None)):
        out = form(empty, res, w, b, 0.5)
        draws += 1
        assert out.shape == (0, 130) and lrandom.get_state("hip") == (seed, draws)
    # 1030 rows are 258 workgroups: eight first-level ticket groups of 32 and a short ninth
    xa, ra, _, wa, ba = operands((1030, 8))
    x, r, w, b = (hip.from_numpy(a) for a in (xa, ra, wa, ba))
    with light.no_grad():
        for form, res in ((one_launch_add, r), (one_launch_after, None)):
            first = form(x, res, w, b, 0.5).numpy()
            assert lrandom.get_state("hip") == (seed, draws + 1)
            second = form(x, res, w, b, 0.5).numpy()
            draws += 2
            assert lrandom.get_state("hip") == (seed, draws)
            assert not np.array_equal(first, second)
        light.manual_seed(seed)
        burn(hip, draws - 1)
        np.testing.assert_array_equal(one_launch_after(x, None, w, b, 0.5).numpy(), second)
        keep = lrandom.keep_mask(seed, draws - 1, xa.size, 0.5).reshape(xa.shape)
        np.testing.assert_array_equal(second != 0, keep)


@pytest.mark.parametrize("mode", [0, 1], ids=["dropout-add-normalise", "normalise-dropout"])
def test_graph_replay_draws_a_fresh_mask(hip, mode):
    from lightgrad_amd.autograd.hip import GraphedStep
    p = 0.5
    xa, ra, ga, wa, ba = operands((8, 64), seed=31)
    x, r, w, b = (hip.from_numpy(a) for a in (xa, ra, wa, ba))
    g = hip.from_numpy(ga, requires_grad=False)

    def once():
        y = one_launch_add(x, r, w, b, p) if mode == 0 else one_launch_after(x, None, w, b, p)
        for t in (x, r, w, b):
            t.zero_grad()
        (y * g).backward(allow_fill=True)
        return (y, x.grad, w.grad, b.grad) + ((r.grad,) if mode == 0 else ())

    expected = []
    for draw in range(3):
        light.manual_seed(SEED)
        burn(hip, draw)
        expected.append([t.numpy().copy() for t in once()])
    step = GraphedStep(once, warmup=1)
    step()
    light.manual_seed(SEED)
    for draw in range(3):
        got = [t.numpy() for t in step()]
        assert lrandom.get_state("hip") == (SEED, draw + 1)
        for name, a, e in zip(("y", "dx", "dw", "db", "dres"), got, expected[draw]):
            np.testing.assert_array_equal(a, e, err_msg="replay %d %s" % (draw, name))
    assert step._graph is not None and step._graph.kernel_count() > 0
    assert not np.array_equal(expected[0][0], expected[1][0]) and not np.array_equal(expected[1][0], expected[2][0])
    step.destroy()


@pytest.mark.parametrize("shape", [(5, 3), (3, 65)], ids=ident)
@pytest.mark.parametrize("mode", [0, 1], ids=["dropout-add-normalise", "normalise-dropout"])
def test_nothing_outside_the_operands_is_read_or_written(hip, mode, shape):
    """through the C ABI: every input lies between bands of NaN, every output between bands of a marker; the results are the bits
    of the run on exact buffers and every band is as it was"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    rows, cols = shape
    xa, ra, ga, wa, ba = operands(shape, seed=11)
    marker, p, eps, band = np.float32(-777.25), 0.5, 1e-5, 7

    def launch(wide):
        lead = band if wide else 0

        def banded(a, fill):
            side = np.full(lead, fill, np.float32)
            return hip.from_numpy(np.concatenate([side, np.asarray(a, np.float32).reshape(-1), side]), requires_grad=False)

        def at(t):
            return t.ptr + 4 * lead

        def body(t, n, check):
            a = t.numpy()
            assert check(a[:lead]).all() and check(a[lead + n:]).all()
            return a[lead:lead + n].copy()

        n = rows * cols
        x, r, g, w, b = ins = [banded(a, np.nan) for a in (xa, ra, ga, wa, ba)]
        y, xhat, dx, dres, gdrop = (banded(np.full(n, marker), marker) for _ in range(5))
        rstd = banded(np.full(rows, marker), marker)
        base = hip.from_numpy(np.full(3, 99, np.uint64))
        light.manual_seed(SEED)
        burn(hip, 2)
        L.check(lib.lg_dropout_layernorm_fwd_f32(at(x), at(r) if mode == 0 else None, at(w), at(b), at(y), at(xhat), at(rstd), rows, cols,
                                                 eps, p, mode, base.ptr + 8))
        outs = [(y, n), (xhat, n), (rstd, rows)]
        # the backward reads what the forward saved from banded inputs of its own
        saved_xhat, saved_rstd = banded(body(xhat, n, np.isfinite), np.nan), banded(body(rstd, rows, np.isfinite), np.nan)
        L.check(lib.lg_dropout_layernorm_bwd_f32(at(g), at(w), at(saved_xhat), at(saved_rstd), at(dx), at(dres) if mode == 0 else None,
                                                 at(gdrop) if mode == 1 else None, rows, cols, p, mode, base.ptr + 8))
        outs += [(dx, n), (dres, n) if mode == 0 else (gdrop, n)]
        assert lrandom.get_state("hip") == (SEED, 3)
        np.testing.assert_array_equal(base.numpy(), [99, 2, 99])
        for t, a in zip(ins, (xa, ra, ga, wa, ba)):
            np.testing.assert_array_equal(body(t, a.size, np.isnan), a.reshape(-1))
        untouched = gdrop if mode == 0 else dres
        assert (untouched.numpy() == marker).all()
        return [body(t, k, lambda a: a == marker) for t, k in outs]

    dense, wide = launch(False), launch(True)
    for name, a, c in zip(("y", "xhat", "rstd", "dx", "dres / gdrop"), wide, dense):
        assert np.isfinite(a).all() and (a != marker).all(), name
        np.testing.assert_array_equal(a, c, err_msg=name)


def test_argument_checks(hip):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    rows, cols = 5, 3
    xa, ra, ga, wa, ba = operands((rows, cols))
    x, r, g, w, b = (hip.from_numpy(a) for a in (xa, ra, ga, wa, ba))
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            x.dropout_add_layer_norm(r, w, b, bad)
        with pytest.raises(ValueError):
            x.layer_norm_dropout(w, b, bad)
    half = hip.from_numpy(xa.astype(np.float16))
    for call in (lambda: half.dropout_add_layer_norm(None, w, b, 0.5), lambda: x.dropout_add_layer_norm(half, w, b, 0.5),
                 lambda: half.layer_norm_dropout(w, b, 0.5), lambda: x.layer_norm_dropout(w, hip.from_numpy(ba.astype(np.float16)), 0.5)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        x.dropout_add_layer_norm(hip.from_numpy(ra[:4]), w, b, 0.5)       # a residual of another shape
    with pytest.raises(TypeError):
        x.dropout_add_layer_norm(ra, w, b, 0.5)                           # ... of another class

    light.manual_seed(4)
    before = lrandom.get_state("hip")
    outs = y, xhat, dx, dres, gdrop = [hip.from_numpy(np.full((rows, cols), 3.0, np.float32)) for _ in range(5)]
    rstd = hip.from_numpy(np.full(rows, 3.0, np.float32))
    base = hip.from_numpy(np.zeros(1, np.uint64))

    def fwd(p=0.5, mode=0, res=r.ptr, base_ptr=base.ptr, x_ptr=x.ptr, y_ptr=y.ptr, rstd_ptr=rstd.ptr, n_rows=rows, n_cols=cols):
        return lib.lg_dropout_layernorm_fwd_f32(x_ptr, res, w.ptr, b.ptr, y_ptr, xhat.ptr, rstd_ptr, n_rows, n_cols, 1e-5, p, mode, base_ptr)

    def bwd(p=0.5, mode=0, dres_ptr=dres.ptr, gdrop_ptr=None, base_ptr=base.ptr, g_ptr=g.ptr, dx_ptr=dx.ptr, n_rows=rows, n_cols=cols):
        return lib.lg_dropout_layernorm_bwd_f32(g_ptr, w.ptr, xhat.ptr, rstd.ptr, dx_ptr, dres_ptr, gdrop_ptr, n_rows, n_cols, p, mode,
                                                base_ptr)

    cases = [(fwd, b"lg_dropout_layernorm_fwd_f32", kwargs, word) for kwargs, word in (
        ({"p": -0.1}, b"p ="), ({"p": 1.0}, b"p ="), ({"p": float("nan")}, b"p ="), ({"mode": 2}, b"mode = 2"), ({"mode": -1}, b"mode = -1"),
        ({"mode": 1}, b"residual"), ({"base_ptr": None}, b"NULL"), ({"x_ptr": None}, b"NULL"), ({"y_ptr": None}, b"NULL"),
        ({"rstd_ptr": None}, b"NULL"), ({"n_rows": -1}, b"shape"), ({"n_cols": 0}, b"shape"), ({"n_rows": 2**26 + 1, "n_cols": 1}, b"rows"))]
    cases += [(bwd, b"lg_dropout_layernorm_bwd_f32", kwargs, word) for kwargs, word in (
        ({"p": -0.1}, b"p ="), ({"p": 1.0}, b"p ="), ({"p": float("nan")}, b"p ="), ({"mode": 2}, b"mode = 2"),
        ({"mode": 1, "gdrop_ptr": gdrop.ptr}, b"dres"), ({"mode": 1, "dres_ptr": None}, b"gdrop"), ({"base_ptr": None}, b"NULL"),
        ({"g_ptr": None}, b"NULL"), ({"dx_ptr": None}, b"NULL"), ({"n_rows": -1}, b"shape"), ({"n_cols": 0}, b"shape"))]
    for call, name, kwargs, word in cases:
        assert call(**kwargs) == LG_EINVAL, (name, kwargs)
        message = lib.lg_last_error()
        assert name in message and word in message, message
    assert lrandom.get_state("hip") == before
    for t in outs + [rstd]:
        assert (t.numpy() == 3.0).all()                                   # the refused calls wrote nothing
    assert fwd(res=None) == 0 and bwd(dres_ptr=None) == 0                 # residual and dres may be NULL in mode 0
    assert lrandom.get_state("hip") == (4, 1)
