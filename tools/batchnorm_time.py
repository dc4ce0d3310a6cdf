"""Time batch normalisation on its kernels (csrc/batchnorm.hip) against the composite of autograd/ops.py run on HipTensor, which is
built from the ops the package had before these kernels.  Everything timed is a captured graph, replayed back to back between two
HIP events (WINDOW replays per window, WARMUP replays first, the median of REPS windows, the cases alternating inside every
repetition), so the device and not the host sets the pace.

  (a) per op at (1024, 8, 26, 26), (1024, 16, 11, 11) and (1024, 512): training forward, backward (dx, dw, db) and evaluation, in two
      cache states.  `cache`: one set of tensors, replayed: everything stays in the 256 MiB Infinity Cache.  `hbm`: the graph holds
      the op on SETS different sets of tensors in turn, at least 512 MiB in all, so every replay finds its operands evicted; the
      time is per op.  Next to each: the launch count, and the traffic floor - the bytes the launches must move (forward 3, backward
      5, evaluation 2 passes over the activation) over the 6.29 TB/s copy ceiling.
  (b) the step of examples/mnist.py --cnn --batchnorm --graph at batch 1024: kernel launches per replay, us per replayed step and
      what the forward pass keeps alive (HipDevice.pool_stats), for the kernels and for the same model on the composite.

    python tools/batchnorm_time.py [--batch 1024] [--out FILE.json]
"""
import argparse
import ctypes
import importlib.util
import json
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, REPS, WINDOW = 5, 15, 10
COPY_CEILING = 6.29e12          # bytes / s: the stream copy the project records (tools/stream_bench.hip)
HBM_FOOTPRINT = 512 << 20       # bytes a rotating graph touches at least: twice the Infinity Cache
MAX_SETS = 128
PASSES = {"fwd": 3, "bwd": 5, "eval": 2}


def time_graphs(lib, graphs):
    """graphs: [(name, HipGraph)] -> {name: {median, p10, p90}} in us per replay"""
    def event():
        e = ctypes.c_void_p()
        assert lib.lg_event_create(ctypes.byref(e)) == 0
        return e
    samples = {name: [] for name, _ in graphs}
    for _, g in graphs:
        for _ in range(WARMUP):
            g.replay()
    assert lib.lg_sync() == 0
    for _ in range(REPS):
        for name, g in graphs:
            e0, e1 = event(), event()
            assert lib.lg_event_record(e0) == 0
            for _ in range(WINDOW):
                g.replay()
            assert lib.lg_event_record(e1) == 0
            ms = ctypes.c_float()
            assert lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)) == 0        # waits: the next case starts on an idle device
            samples[name].append(1e3 * ms.value / WINDOW)
            lib.lg_event_destroy(e0), lib.lg_event_destroy(e1)
    out = {}
    for name, v in samples.items():
        v = np.sort(v)
        out[name] = {"median": float(np.median(v)), "p10": float(v[len(v) // 10]), "p90": float(v[(9 * len(v)) // 10])}
    return out


def op_numbers(shapes):
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, lib as L
    from lightgrad_amd.autograd.hip import ops as H
    lib = L.lib()
    rng = np.random.RandomState(2)
    u = lambda *s, **kw: HipTensor.from_numpy(rng.standard_normal(s).astype(np.float32), **kw)      # noqa: E731
    paths = {"kernel": (HipTensor.batch_norm, HipTensor.batch_norm_infer),
             "composite": (H._batch_norm_composite, H._batch_norm_infer_composite)}
    graphs, meta, keep = [], {}, []
    for shape in shapes:
        c, nbytes = shape[1], 4 * int(np.prod(shape))
        sets = {"cache": 1, "hbm": min(MAX_SETS, -(-HBM_FOOTPRINT // (2 * nbytes)))}
        tensors = [dict(x=u(*shape), g=u(*shape, requires_grad=False), w=u(c), b=u(c), rm=u(c, requires_grad=False),
                        rv=HipTensor.from_numpy(rng.uniform(0.5, 2, c).astype(np.float32), requires_grad=False)) for _ in range(sets["hbm"])]
        for path, (train, infer) in paths.items():
            def fwd(t):
                return train(t["x"], t["w"], t["b"], t["rm"], t["rv"])

            def bwd(t):
                return t["y"].ctx._backpropagate(t["g"])          # the node's backward and the add_grad into x, w, b

            def evaluate(t):
                return infer(t["x"], t["w"], t["b"], t["rm"], t["rv"])
            for t in tensors:
                t["y"] = fwd(t)                                   # eager once: pool, kernels; the tape the backward graphs replay
                evaluate(t)
                bwd(t)
            for kind, fn in (("fwd", fwd), ("bwd", bwd), ("eval", evaluate)):
                for state, n in sets.items():
                    graph = HipGraph()
                    with graph.capture():
                        keep.append([fn(t) for t in tensors[:n]])
                    key = "%s %s %s %s" % ("x".join(map(str, shape)), kind, state, path)
                    meta[key] = {"kernels": graph.kernel_count() // n, "sets": n, "floor_us": 1e6 * PASSES[kind] * nbytes / COPY_CEILING}
                    graphs.append((key, graph))
            keep.append([t.pop("y") for t in tensors])
    us = time_graphs(lib, graphs)
    return {k: dict(meta[k], **{s: v / meta[k]["sets"] for s, v in us[k].items()}) for k in us}


def step_numbers(batch):
    import lightgrad_amd as light
    import lightgrad_amd.nn as nn
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, HipDevice, lib as L
    from lightgrad_amd.autograd.hip import ops as H
    spec = importlib.util.spec_from_file_location("mnist_example", os.path.join(ROOT, "examples", "mnist.py"))
    mnist = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mnist)

    class CompositeNorm(nn.BatchNorm2d):
        def forward(self, x):
            return H._batch_norm_composite(x, self.weight, self.bias, self.running_mean, self.running_var, momentum=self.momentum, eps=self.eps)

    def composite_model():
        model = mnist.CNN(batchnorm=True)
        model.n1, model.n2 = CompositeNorm(8), CompositeNorm(16)
        return model
    lib = L.lib()
    rng = np.random.RandomState(1)
    x = HipTensor.from_numpy(rng.uniform(0, 1, (batch, 1, 28, 28)).astype(np.float32))
    t = HipTensor.from_numpy(np.eye(10, dtype=np.float32)[rng.randint(0, 10, batch)])
    out, graphs, keep = {}, [], []
    for name, make in (("composite", composite_model), ("kernel", lambda: mnist.CNN(batchnorm=True)), ("no batchnorm", mnist.CNN)):
        np.random.seed(0)
        model = make().map_parameters(lambda p: p.hip())
        opt = light.optim.AdaBelief(model.parameters(), lr=0.001, fused=True, device_step=True)

        def step():
            l = light.loss.mse(model(x), t)
            opt.zero_grad()
            l.backward()
            opt.step()
            return l
        for _ in range(3):
            step()
        HipDevice.synchronize()
        before = HipDevice.pool_stats()["in_use_bytes"]
        l = light.loss.mse(model(x), t)
        l.item()
        out[name] = {"forward_in_use_bytes": int(HipDevice.pool_stats()["in_use_bytes"] - before)}
        del l
        graph = HipGraph()
        with graph.capture():
            loss = step()
        opt.t -= len(opt.parameters)
        out[name]["kernels_per_step"] = graph.kernel_count()
        graphs.append((name, graph))
        keep.append((model, opt, loss))
    for name, us in time_graphs(lib, graphs).items():
        out[name]["step_us"] = us
    for name, (_, _, loss) in zip(out, keep):
        assert np.isfinite(loss.item()), name
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"batch": args.batch, "windows": REPS, "replays_per_window": WINDOW}
    result["step"] = step_numbers(args.batch)
    result["ops"] = op_numbers([(args.batch, 8, 26, 26), (args.batch, 16, 11, 11), (args.batch, 512)])
    for name, r in result["step"].items():
        print("step %-13s %3d kernels  %9.1f us (p10 %9.1f, p90 %9.1f)  forward keeps %7.1f MB" % (
            name, r["kernels_per_step"], r["step_us"]["median"], r["step_us"]["p10"], r["step_us"]["p90"], r["forward_in_use_bytes"] / 1e6))
    for name, r in result["ops"].items():
        print("%-38s %2d kernels  %8.1f us (p10 %8.1f, p90 %8.1f)  floor %6.1f us  %3d sets" % (
            name, r["kernels"], r["median"], r["p10"], r["p90"], r["floor_us"], r["sets"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
