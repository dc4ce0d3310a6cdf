"""Time the captured tiny-BERT training step in training mode with hidden dropout: the model of bench.py's BERT leg
(examples/bert.py TINY, batch 8, 128 positions, masked-LM loss at every position, gradients in one flat bucket) with
`hidden_dropout_prob = 0.1`, forward + zeroing + backward captured once and replayed:

    python tools/bert_hidden_dropout_time.py [--rounds 3] [--replays 200] [--hidden 0.1] [--attention 0.0] [--nodes] [--out FILE]

Every round builds the model afresh, captures the step and reports the kernels in the graph and the time per replay: a host
clock around `--replays` replays that end in a device synchronise, after 20 warm-up replays.  With --nodes one more line per
tape node follows: the device time between HIP events around the node's forward and backward over 20 eager steps
(HipProfiler), the only per-launch view this tool has.  The tool reads nothing but the public model and tensor API, so the
same file times any commit that has hidden dropout.  Without a GPU this fails; nothing here falls back."""
import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(hidden, attention, replays, nodes):
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, HipDevice
    from lightgrad_amd.autograd.hip.profiler import HipProfiler
    from lightgrad_amd.dist import SingleProcess, DataParallel
    spec = importlib.util.spec_from_file_location("bert_example", os.path.join(ROOT, "examples", "bert.py"))
    bert = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bert)
    np.random.seed(0)
    vocab = bert.TINY["vocab_size"]
    model = bert.BertForMaskedLM(hidden_dropout_prob=hidden, attention_probs_dropout_prob=attention, **bert.TINY).map_parameters(lambda t: t.hip())
    ids = HipTensor.from_numpy(np.random.randint(0, vocab, (8, 128)).astype(np.int32), requires_grad=False)
    labels = HipTensor.from_numpy(np.random.randint(0, vocab, (8 * 128,)).astype(np.int64), requires_grad=False)
    dp = DataParallel(model.parameters(), SingleProcess(), flatten=True)
    light.manual_seed(1)
    HipDevice.synchronize()                                    # the seed is on the device before anything is captured

    def step():
        loss = light.loss.cross_entropy(model(ids).reshape(-1, vocab), labels)
        dp.bucket.fill(0)
        loss.backward()
        return loss

    for _ in range(3):
        step()
    per_node = None
    if nodes:
        with HipProfiler() as prof:
            for _ in range(20):
                step()
        names = sorted(set(prof.device_ms[False]) | set(prof.device_ms[True]))
        per_node = {n: (1e3 * prof.device_ms[False][n] / 20, 1e3 * prof.device_ms[True][n] / 20) for n in names}
    graph = HipGraph()
    with graph.capture():
        loss = step()
    kernels = graph.kernel_count()
    for _ in range(20):
        graph.replay()
    HipDevice.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        graph.replay()
    HipDevice.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / replays
    assert np.isfinite(loss.item())
    graph.destroy()
    return kernels, ms, per_node


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--hidden", type=float, default=0.1)
    ap.add_argument("--attention", type=float, default=0.0)
    ap.add_argument("--nodes", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say("tiny-BERT training step (batch 8, 128 positions), hidden_dropout_prob = %g, attention_probs_dropout_prob = %g, captured graph, "
        "%d rounds of %d replays:" % (args.hidden, args.attention, args.rounds, args.replays))
    per_node = None
    for r in range(args.rounds):
        kernels, ms, per_node = measure(args.hidden, args.attention, args.replays, args.nodes and r == args.rounds - 1)
        say("  round %d: %d kernels per replay, %.4f ms per replay" % (r, kernels, ms))
    if per_node:
        say("  device time per eager step by tape node, us (forward, backward):")
        for n, (f, b) in sorted(per_node.items(), key=lambda kv: -(kv[1][0] + kv[1][1])):
            say("    %-26s %9.2f %9.2f" % (n, f, b))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
