"""Worker of tests/test_hip_gemm_kgroups.py: the K-group tile's cases through the raw C ABI, in a process of its own because the
library reads LG_GEMM_TILE / LG_GEMM_KLOOP once.  Prints one JSON line per case and a last line {"done": n}."""
import hashlib
import json
import sys
import numpy as np

KS = (1, 3, 16, 17, 63, 64, 65, 196, 197, 784)
SHAPES = ((70, 50), (130, 77))                 # M, N: neither a multiple of 32, both beyond the skinny tiles
VARIANTS = ("plain", "accumulate", "bias", "bias_relu", "relu_accumulate", "rowsum")


def case_inputs(m, n, k, variant):
    """operands of one case (float32): A [m, lda >= k], B^T [n, ldb >= k], old C, bias - the same on every call"""
    rng = np.random.RandomState(1000 * k + 10 * m + VARIANTS.index(variant))
    lda, ldb, ldc = k + (3 if k % 2 else 0), k + (1 if variant == "bias" else 0), n + (5 if variant == "accumulate" else 0)
    a = rng.uniform(-1, 1, (m, lda)).astype(np.float32)
    bt = rng.uniform(-1, 1, (n, ldb)).astype(np.float32)
    c0 = rng.uniform(-1, 1, (m, ldc)).astype(np.float32)
    bias = rng.uniform(-1, 1, n).astype(np.float32)
    return a, bt, c0, bias, (lda, ldb, ldc)


def expected(m, n, k, variant, a, bt, c0, bias, dtype, sequential=False):
    """what the case computes, in `dtype`; sequential: one k after the other (the least favourable float32 order)"""
    x = a[:, :k].astype(dtype)
    w = bt[:, :k].astype(dtype)
    if "relu" in variant:
        x = np.maximum(x, 0)
    if sequential:
        prod = np.zeros((m, n), dtype)
        for j in range(k):
            prod += np.outer(x[:, j], w[:, j])
    else:
        prod = x @ w.T
    out = {}
    c = c0.astype(dtype).copy()
    if "accumulate" in variant:
        c[:, :n] += prod
    elif "bias" in variant:
        c[:, :n] = prod + bias.astype(dtype)
    else:
        c[:, :n] = prod
    out["c"] = c
    if variant == "rowsum":
        out["rowsum"] = x.sum(axis=1)
    return out


def rel_frobenius(got, ref64):
    d = np.linalg.norm(got.astype(np.float64) - ref64)
    s = np.linalg.norm(ref64)
    return float(d / s) if s > 0 else float(d)


def main():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from lightgrad_amd.autograd.hip import HipTensor
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    count = 0
    for (m, n) in SHAPES:
        for k in KS:
            for variant in VARIANTS:
                a, bt, c0, bias, (lda, ldb, ldc) = case_inputs(m, n, k, variant)
                ta, tb, tbias = HipTensor.from_numpy(a), HipTensor.from_numpy(bt), HipTensor.from_numpy(bias)
                runs = []
                for _ in range(2):
                    tc = HipTensor.from_numpy(c0)
                    trs = HipTensor.from_numpy(np.full(m, 7.0, np.float32))
                    acc = 1 if "accumulate" in variant else 0
                    if variant in ("plain", "accumulate"):
                        L.check(lib.lg_gemm_f32(0, 1, m, n, k, ta.ptr, lda, 0, tb.ptr, ldb, 0, tc.ptr, ldc, 0, 1, acc))
                    elif variant == "bias":
                        L.check(lib.lg_gemm_bias_f32(0, 1, m, n, k, ta.ptr, lda, 0, tb.ptr, ldb, 0, tc.ptr, ldc, 0, 1, tbias.ptr))
                    elif variant == "bias_relu":
                        L.check(lib.lg_gemm_fused_f32(0, 1, m, n, k, ta.ptr, lda, tb.ptr, ldb, tc.ptr, ldc, 0, tbias.ptr, None, 0, 1, 0))
                    elif variant == "relu_accumulate":
                        L.check(lib.lg_gemm_fused_f32(0, 1, m, n, k, ta.ptr, lda, tb.ptr, ldb, tc.ptr, ldc, 1, None, None, 0, 1, 0))
                    else:
                        L.check(lib.lg_gemm_fused_f32(0, 1, m, n, k, ta.ptr, lda, tb.ptr, ldb, tc.ptr, ldc, 0, None, trs.ptr, 0, 0, 0))
                    runs.append({"c": tc.numpy().copy(), "rowsum": trs.numpy().copy()})
                ref64 = expected(m, n, k, variant, a, bt, c0, bias, np.float64)
                cpu32 = expected(m, n, k, variant, a, bt, c0, bias, np.float32)
                rec = {"m": m, "n": n, "k": k, "variant": variant,
                       "repeat_equal": all(np.array_equal(runs[0][key], runs[1][key]) for key in runs[0]),
                       "padding_untouched": bool(np.array_equal(runs[0]["c"][:, n:], c0[:, n:])),
                       "sha1": hashlib.sha1(b"".join(runs[0][key].tobytes() for key in sorted(runs[0]))).hexdigest(),
                       "err": {key: rel_frobenius(runs[0][key], ref64[key]) for key in ref64},
                       "cpu_err": {key: rel_frobenius(cpu32[key], ref64[key]) for key in ref64}}
                print(json.dumps(rec), flush=True)
                count += 1
    print(json.dumps({"done": count}), flush=True)


if __name__ == "__main__":
    main()
