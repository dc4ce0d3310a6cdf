"""Time the CNN example on the conv2d / pooling kernels (csrc/conv.hip) against the composites they replace.  Everything timed is a
captured graph, replayed back to back between two HIP events (WINDOW replays per window, WARMUP replays first, the median of REPS
windows, the cases alternating inside every repetition), so the device and not the host sets the pace.

  (a) the step of examples/mnist.py --cnn --graph at batch 1024: kernel launches per replay and us per replayed step, for this
      build (`fused`) and for the model spelled with the composites, `x.pad(p).conv(w) + b` and `pool(k).max(0)` (`composite`).
      With --parent-tree DIR the composite model ALSO runs on the parent commit, checked out and built in a directory of its own:
      first, in a child process that imports the package from that directory and so loads only that library.  The composites
      are the parent's code, unchanged by the kernels.
  (b) per op at the example's shapes, (1024,1,28,28) -> 8 and (1024,8,13,13) -> 16 channels, 3x3: forward, and forward + backward,
      of conv2d against x.conv(w), and of max_pool against pool((2,2)).max(0) on (1024,8,26,26) and (1024,16,11,11).  Same build.
  (c) HipDevice.pool_stats()["in_use_bytes"] gained by the forward pass of one eager step (what the tape keeps alive), per model.

    python tools/conv_time.py [--parent-tree DIR] [--batch 1024] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS, WINDOW = 5, 15, 10
CHILD_LIMIT = 300         # seconds for the parent library's process


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


def cnn_models():
    import lightgrad_amd.nn as nn

    class Fused(nn.Module):                                      # examples/mnist.py: CNN
        def __init__(self):
            nn.Module.__init__(self)
            self.c1 = nn.Conv2d(1, 8, kernelsize=3, bias=False, pad=0)
            self.c2 = nn.Conv2d(8, 16, kernelsize=3, bias=False, pad=0)
            self.l1 = nn.Linear(5 * 5 * 16, 10)

        def forward(self, x):
            y = self.c1(x).max_pool().relu()
            y = self.c2(y).max_pool().relu()
            return self.l1(y.reshape(-1, 5 * 5 * 16))

    class Composite(Fused):                                      # the same model as the parent commit runs it
        def forward(self, x):
            y = x.conv(self.c1.w, strides=1).pool(kernel=(2, 2)).max(axis=0).relu()
            y = y.conv(self.c2.w, strides=1).pool(kernel=(2, 2)).max(axis=0).relu()
            return self.l1(y.reshape(-1, 5 * 5 * 16))
    return {"fused": Fused, "composite": Composite}


def step_numbers(which, batch, root=ROOT):
    """(a) and (c) for the models named in `which`, on the package (and its library) under `root`"""
    sys.path.insert(0, root)
    import lightgrad_amd as light
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, HipDevice, lib as L
    lib = L.lib()
    rng = np.random.RandomState(1)
    x = HipTensor.from_numpy(rng.uniform(0, 1, (batch, 1, 28, 28)).astype(np.float32))
    t = HipTensor.from_numpy(np.eye(10, dtype=np.float32)[rng.randint(0, 10, batch)])
    out, graphs, keep = {}, [], []
    for name in which:
        np.random.seed(0)
        model = cnn_models()[name]().map_parameters(lambda p: p.hip())
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
        assert np.isfinite(dict(zip(which, keep))[name][2].item())
    return out


def op_numbers(batch):
    """(b): every case as a captured graph of the forward, and of the forward plus the backward of its nodes"""
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, lib as L
    lib = L.lib()
    rng = np.random.RandomState(2)
    u = lambda *s: HipTensor.from_numpy(rng.uniform(-1, 1, s).astype(np.float32))      # noqa: E731

    def conv_cases(tag, x, w):
        def fused(back):
            y = x.conv2d(w)
            return (y, y.ctx.backward(g)) if back else y

        def composite(back):
            y = x.conv(w, strides=1)
            return (y, y.ctx.backward(g)) if back else y
        g = u(*x.conv2d(w).shape)
        return [(tag + "_conv2d", fused), (tag + "_composite", composite)]

    def pool_cases(tag, x):
        def fused(back):
            y = x.max_pool()
            return (y, y.ctx.backward(g)) if back else y

        def composite(back):
            p = x.pool(kernel=(2, 2))
            y = p.max(axis=0)
            return (y, p.ctx.backward(y.ctx.backward(g))) if back else y
        g = u(*x.max_pool().shape)
        return [(tag + "_max_pool", fused), (tag + "_composite", composite)]
    cases = (conv_cases("c1", u(batch, 1, 28, 28), u(8, 1, 3, 3)) + conv_cases("c2", u(batch, 8, 13, 13), u(16, 8, 3, 3)) +
             pool_cases("pool1", u(batch, 8, 26, 26)) + pool_cases("pool2", u(batch, 16, 11, 11)))
    graphs, kernels, keep = [], {}, []
    for name, fn in cases:
        for back in (False, True):
            fn(back)                                             # eager once: pool, kernels
            graph = HipGraph()
            with graph.capture():
                keep.append(fn(back))
            key = name + ("_fwd_bwd" if back else "_fwd")
            kernels[key] = graph.kernel_count()
            graphs.append((key, graph))
    us = time_graphs(lib, graphs)
    return {k: dict(us[k], kernels=kernels[k]) for k in us}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.parent_child:                                        # this process imports the parent's package and nothing of this tree
        print(json.dumps(step_numbers(["composite"], args.batch, root=args.parent_child)), flush=True)
        return
    result = {"batch": args.batch, "windows": REPS, "replays_per_window": WINDOW}
    if args.parent_tree:                                         # before this process opens the GPU: a fresh child, under a time limit
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", os.path.abspath(args.parent_tree),
                                "--batch", str(args.batch)], stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT)
        if child.returncode != 0:
            sys.exit("the parent library's process ended with status %d - nothing more is started" % child.returncode)
        result["parent_build"] = json.loads(child.stdout.strip().splitlines()[-1])["composite"]
    result["step"] = step_numbers(["composite", "fused"], args.batch)
    result["ops"] = op_numbers(args.batch)
    for name, r in sorted(result["step"].items()) + ([("parent build", result["parent_build"])] if args.parent_tree else []):
        print("step %-13s %3d kernels  %9.1f us (p10 %9.1f, p90 %9.1f)  forward keeps %7.1f MB" % (
            name, r["kernels_per_step"], r["step_us"]["median"], r["step_us"]["p10"], r["step_us"]["p90"], r["forward_in_use_bytes"] / 1e6))
    if not args.parent_tree:
        print("step parent build: not measured (no --parent-tree)")
    for name, r in sorted(result["ops"].items()):
        print("%-28s %2d kernels  %9.1f us (p10 %9.1f, p90 %9.1f)" % (name, r["kernels"], r["median"], r["p10"], r["p90"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
