"""Worker of tests/test_hip_gemm_tiles.py: the cases of ONE child of tests/gemm_cases.py through the raw C ABI, in a process of its
own because the library reads LG_GEMM_TILE / LG_GEMM_SLICES once.  `python gemm_tile_worker.py <child> [<file>]` prints one JSON line
per case and a last line {"done": n}, and writes the same lines to <file>: the spawner hands back only the end of a child's output,
and a child has up to 2213 cases."""
import ctypes
import hashlib
import json
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as G                                                     # noqa: E402


def main(child, copy_to=None):
    copy = open(copy_to, "w") if copy_to else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if copy:
            copy.write(line + "\n")
            copy.flush()

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from lightgrad_amd.autograd.hip import HipTensor
    from lightgrad_amd.autograd.hip import lib as L
    from lightgrad_amd.autograd.hip import ops as H
    lib = L.lib()

    def dev(matrix):
        return HipTensor.from_numpy(matrix.buf, requires_grad=False)

    def at(tensor, matrix):
        return tensor.ptr + 4 * matrix.start

    ptr3 = lambda *ps: (ctypes.c_void_p * 3)(*ps)                          # noqa: E731
    on_device = {}                                                         # the operands of the current product, uploaded once
    count = 0
    for case in G.cases(child):
        m, n, k, ta, tb, variant = (case[x] for x in ("m", "n", "k", "ta", "tb", "variant"))
        key = (m, n, k, ta, tb, G.kind_of(variant))
        inp = G.inputs(*key)
        if on_device.get("key") != key:
            bs = inp["B"] if isinstance(inp["B"], list) else [inp["B"]]
            on_device = {"key": key, "A": dev(inp["A"]), "B": [dev(b) for b in bs], "addend": dev(inp["addend"]),
                         "bias": HipTensor.from_numpy(inp["bias"], requires_grad=False)}
        A, B0 = inp["A"], (inp["B"][0] if isinstance(inp["B"], list) else inp["B"])
        pa, pbs = at(on_device["A"], A), [at(t, b) for t, b in zip(on_device["B"], inp["B"] if isinstance(inp["B"], list) else [inp["B"]])]
        pbias = on_device["bias"].ptr
        C = G.c_buffer(case, inp)
        RS = G.Matrix(inp["rs0"] if variant == "rowsum_acc" else np.zeros((1, 1, m), np.float32), 0, fill=G.PATTERN)
        if variant != "rowsum_acc":
            RS.blank()
        AUX = G.Matrix(inp["pre"].get(), inp["pads"][4], fill=G.PATTERN)   # gelu: written; gelu-backward: the pre-activation, read
        if variant == "gelu":
            AUX.blank()
        runs, plans = [], []
        for _ in range(2):
            tc, trs, taux = dev(C), dev(RS), dev(AUX)
            pc, prs, paux = at(tc, C), at(trs, RS), at(taux, AUX)
            acc = 1 if "acc" in variant else 0
            if variant in ("plain", "offset", "accumulate"):
                rc = lib.lg_gemm_f32(ta, tb, m, n, k, pa, A.ld, 0, pbs[0], B0.ld, 0, pc, C.ld, 0, 1, acc)
            elif variant in ("batched", "batched_accumulate"):
                rc = lib.lg_gemm_f32(ta, tb, m, n, k, pa, A.ld, A.stride, pbs[0], B0.ld, B0.stride, pc, C.ld, C.stride, 3, acc)
            elif variant == "batched_bias":
                rc = lib.lg_gemm_bias_f32(ta, tb, m, n, k, pa, A.ld, A.stride, pbs[0], B0.ld, B0.stride, pc, C.ld, C.stride, 3, pbias)
            elif variant == "batched2":                                    # matrix (o, i) at o * 2 * stride + i * stride
                rc = lib.lg_gemm_batched2_f32(ta, tb, m, n, k, pa, A.ld, 2 * A.stride, A.stride, pbs[0], B0.ld, 2 * B0.stride, B0.stride,
                                              pc, C.ld, 2 * C.stride, C.stride, 2, 2, 0)
            elif variant == "bias":
                rc = lib.lg_gemm_bias_f32(ta, tb, m, n, k, pa, A.ld, 0, pbs[0], B0.ld, 0, pc, C.ld, 0, 1, pbias)
            elif variant == "addend":
                rc = lib.lg_gemm_addend_f32(ta, tb, m, n, k, pa, A.ld, pbs[0], B0.ld, pc, C.ld, pbias,
                                            at(on_device["addend"], inp["addend"]), inp["addend"].ld)
            elif variant in ("relu_a", "relu_b"):
                rc = lib.lg_gemm_fused_f32(ta, tb, m, n, k, pa, A.ld, pbs[0], B0.ld, pc, C.ld, 0, None, None, 0,
                                           1 if variant == "relu_a" else 0, 1 if variant == "relu_b" else 0)
            elif variant in ("rowsum", "rowsum_acc"):
                rc = lib.lg_gemm_rowsum_f32(ta, tb, m, n, k, pa, A.ld, pbs[0], B0.ld, pc, C.ld, acc, prs, acc)
            elif variant == "gelu":
                rc = lib.lg_gemm_act_f32(ta, tb, m, n, k, pa, A.ld, pbs[0], B0.ld, pc, C.ld, pbias, L.ACT_GELU, paux, AUX.ld)
            elif variant == "gelu_bwd":
                rc = lib.lg_gemm_act_f32(ta, tb, m, n, k, pa, A.ld, pbs[0], B0.ld, pc, C.ld, None, L.ACT_GELU_BWD, paux, AUX.ld)
            elif variant == "multi3":
                rc = lib.lg_gemm_multi3_f32(ta, tb, m, n, k, pa, A.ld, ptr3(*pbs), B0.ld, ptr3(pc, pc + 4 * n, pc + 8 * n), C.ld,
                                            ptr3(pbias, pbias + 4 * n, pbias + 8 * n))
            elif variant == "kseg3":
                rc = lib.lg_gemm_kseg3_f32(ta, tb, m, n, k // 3, pa, A.ld, ptr3(*pbs), B0.ld, pc, C.ld, 0, None, 0)
            else:
                raise ValueError(variant)
            L.check(rc)
            plans.append(H.gemm_last_plan())
            runs.append({"c": tc.numpy(), "rowsum": trs.numpy(), "aux": taux.numpy()})
        first = runs[0]
        got = {"c": C.get(first["c"])}
        if variant == "multi3":
            got["c"] = got["c"].reshape(m, 3, n).transpose(1, 0, 2)
        if variant.startswith("rowsum"):
            got["rowsum"] = RS.get(first["rowsum"])
        if variant == "gelu":
            got["aux"] = AUX.get(first["aux"])
        ref64 = G.reference(case, np.float64)
        rec = G.judge(case, got, ref64)
        cpu32 = G.reference(case, np.float32)
        plan = plans[0]
        rec.update(case)
        rec.update({
            "repeat_equal": all(np.array_equal(runs[0][x].view(np.uint32), runs[1][x].view(np.uint32)) for x in first) and plans[0] == plans[1],
            "outside_untouched": C.outside_untouched(first["c"]) and RS.outside_untouched(first["rowsum"]) and AUX.outside_untouched(first["aux"])
                                 and (variant.startswith("rowsum") or bool(np.array_equal(first["rowsum"].view(np.uint32), RS.buf.view(np.uint32))))
                                 and (variant == "gelu" or bool(np.array_equal(first["aux"].view(np.uint32), AUX.buf.view(np.uint32)))),
            "cpu_err": {x: G.rel_frobenius(cpu32[x], ref64[x]) for x in ref64},
            "tile": [plan["tile"][0], plan["tile"][1], plan["bk"], plan["kg"]], "k_slices": plan["k_slices"], "k_per_slice": plan["k_per_slice"],
            "flags": (plan["a_kc"] * 1) | (plan["b_kc"] * 2) | (plan["va"] * 4) | (plan["vb"] * 8) | (plan["wave_private"] * 16),
            "route": plan["route"],
            "sha1": hashlib.sha1(b"".join(first[x].tobytes() for x in sorted(first))).hexdigest()})
        if variant == "gelu":                                              # aux = gelu of the pre-activation as STORED
            want = G.gelu(got["c"].astype(np.float64))
            rec["gelu_of_stored"] = bool(np.allclose(got["aux"], want, rtol=2e-6, atol=1e-7))
        emit(rec)
        count += 1
    emit({"done": count})


if __name__ == "__main__":
    main(*sys.argv[1:3])
