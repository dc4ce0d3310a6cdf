"""Time the flat-bucket optimizer launches on two buckets - tiny-BERT's parameters and 16 Mi elements in 16 segments:

    python tools/optim_recipe_time.py [--replays 25] [--out profiles/optim_recipe.txt] [--old-only]

    (a) lg_adam_multi_dev_f32                      4 reads + 3 writes = 28 B per element
    (b) lg_adamw_multi_dev_f32, the whole recipe   28 B per element
    (c) lg_grad_norm_clip_f32                       4 B per element
Each launch is captured `PER_GRAPH` times into a hipGraph of its own; a figure is the median over `--replays` replays (after 3
warm-up replays, the three graphs taking turns) of the time between two HIP events around a replay, divided by PER_GRAPH: device
time of one launch including the boundary to the next.  --old-only measures (a) alone and needs nothing newer than that entry
point: with LIGHTGRAD_HIP_LIB pointing at a library built from an earlier commit it gives the old entry point's time before
a change.  Without a GPU this fails; nothing here estimates."""
import argparse
import ctypes
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PER_GRAPH = 20


def tiny_bert_lengths():
    import numpy as np
    spec = importlib.util.spec_from_file_location("bert_example", os.path.join(ROOT, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    model = bert.BertForMaskedLM(**bert.TINY)
    shapes = [tuple(p.shape) for p in model.parameters()]
    return [int(np.prod(s)) for s in shapes], [len(s) >= 2 for s in shapes]


def measure(name, lengths, flags, replays, old_only):
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, HipDevice
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    offsets = tuple(int(o) for o in np.concatenate([[0], np.cumsum(lengths)]))
    n = offsets[-1]
    rng = np.random.RandomState(0)
    p = HipTensor.from_numpy(rng.uniform(-1, 1, n).astype(np.float32), requires_grad=False)
    g = HipTensor.from_numpy(rng.uniform(-1, 1, n).astype(np.float32), requires_grad=False)
    m, v = HipTensor.zeros((n,), requires_grad=False), HipTensor.zeros((n,), requires_grad=False)
    counter = HipTensor._new_step_counter(0, slots=len(lengths) * -(-max(lengths) // 1024))
    launches = {"(a) lg_adam_multi_dev_f32": (lambda: p._fused_adam_multi_dev(g, m, v, offsets, 1e-4, 0.9, 0.999, 1e-8, counter, 1.0, True), 28)}
    if not old_only:
        scratch = HipTensor._new_grad_norm_scratch()
        launches["(b) lg_adamw_multi_dev_f32"] = (lambda: p._fused_adamw_multi_dev(g, m, v, offsets, 1e-4, 0.9, 0.999, 1e-8, counter, 1.0, True,
                                                                                      0.01, flags, scratch[2], 1, 1000, 1000000), 28)
        launches["(c) lg_grad_norm_clip_f32"] = (lambda: g._grad_norm_clip(1.0, 1.0, scratch), 4)
    graphs = {}
    for label, (launch, _) in launches.items():
        launch()                                   # eager once: the code object is loaded
        graphs[label] = HipGraph()
        with graphs[label].capture():
            for _ in range(PER_GRAPH):
                launch()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    L.check(lib.lg_event_create(ctypes.byref(e0)))
    L.check(lib.lg_event_create(ctypes.byref(e1)))
    ms, times = ctypes.c_float(), {label: [] for label in launches}
    for rep in range(3 + replays):
        for label, graph in graphs.items():
            L.check(lib.lg_event_record(e0))
            graph.replay()
            L.check(lib.lg_event_record(e1))
            L.check(lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            if rep >= 3:
                times[label].append(ms.value * 1e3 / PER_GRAPH)
    HipDevice.synchronize()
    lib.lg_event_destroy(e0)
    lib.lg_event_destroy(e1)
    assert np.all(np.isfinite(p.numpy()))
    for graph in graphs.values():
        graph.destroy()
    base = float(np.median(times["(a) lg_adam_multi_dev_f32"]))
    rows = []
    for label, (_, bytes_per_element) in launches.items():
        t = np.sort(np.asarray(times[label]))
        med = float(np.median(t))
        rows.append("%-10s %9d %-28s %9.2f %9.2f %9.2f %7.2f %8.3f" % (name, n, label, med, t[0], t[-1], bytes_per_element * n / (med * 1e-6) / 1e12, med / base))
    if not old_only:
        both = float(np.median(times["(b) lg_adamw_multi_dev_f32"])) + float(np.median(times["(c) lg_grad_norm_clip_f32"]))
        rows.append("%-10s %9d %-28s %9.2f %9s %9s %7.2f %8.3f" % (name, n, "(b) + (c)", both, "", "", 32 * n / (both * 1e-6) / 1e12, both / base))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--old-only", action="store_true")
    args = ap.parse_args()
    assert args.replays >= 20, "medians of at least 20 replays"
    from lightgrad_amd.autograd.hip import lib as L
    if args.old_only:                              # an older library: do not ask it for the newer symbols
        for symbol in ("lg_adamw_multi_dev_f32", "lg_grad_norm_clip_f32"):
            L.PROTOTYPES.pop(symbol, None)
    from lightgrad_amd.autograd.hip import HipDevice
    lines = ["flat-bucket optimizer launches, %s, library %s" % (HipDevice.info()["name"], L.LIB_PATH),
             "us per launch: median / min / max over %d replays of a hipGraph of %d launches" % (args.replays, PER_GRAPH),
             "%-10s %9s %-28s %9s %9s %9s %7s %8s" % ("bucket", "elements", "launch", "median", "min", "max", "TB/s", "vs (a)")]
    lengths, flags = tiny_bert_lengths()
    lines += measure("tiny-BERT", lengths, flags, args.replays, args.old_only)
    lines += measure("16 Mi", [1 << 20] * 16, [True] * 16, args.replays, args.old_only)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
