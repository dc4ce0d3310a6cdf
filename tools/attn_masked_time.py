"""Time attention forward + backward, fused against the composite route of the same build, where the fused form used to be
refused: a padded batch (8, 128, 2 heads, d = 64, key-padding mask) and a length that is no multiple of 32 (8, 100, 2, 64).
And the unmasked `attention` at (8, 128, 2, 64) on this build against another build of the library (the parent commit's), in
alternating fresh processes, to show that the unmasked kernels did not move:

    python tools/attn_masked_time.py [--other-lib path/to/the/other/liblghip.so] [--rounds 3] [--out profiles/attention_masked.txt]

Every figure is device time per forward + backward by HIP events around `--iters` steps, both issued eagerly from the tape
(host time included where the host is slower than the device) and replayed from a captured graph (device time alone).
Without a GPU this fails; nothing here falls back."""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(route, b, s, heads, d, masked, iters):
    """{"eager_us", "graph_us"} of one forward + backward of `route` ("fused", "unmasked" or "composite")"""
    import numpy as np
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import HipGraph, HipDevice
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    rng = np.random.RandomState(0)
    width = heads * d
    q, k, v = (HipTensor.from_numpy(rng.uniform(-1, 1, (b, s, width)).astype(np.float32)) for _ in range(3))
    w = HipTensor.from_numpy(rng.uniform(-1, 1, (b, s, width)).astype(np.float32), requires_grad=False)
    mask = None
    if masked:
        m = np.ones((b, s), np.float32)
        for i in range(b):
            m[i, s - 1 - 11 * i:] = 0                                  # padded to different lengths
        mask = HipTensor.from_numpy(m, requires_grad=False)
    scale = math.sqrt(d) ** -1

    def step():
        for t in (q, k, v):
            t.zero_grad()
        if route == "fused":
            out = q.masked_attention(k, v, heads=heads, scale=scale, mask=mask)
        elif route == "unmasked":
            out = q.attention(k, v, heads=heads, scale=scale)
        else:                                                          # examples/bert.py, the composite lines
            q4 = q.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
            k4 = k.reshape(b, s, heads, d).transpose(0, 2, 3, 1)
            v4 = v.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
            scores = (q4 @ k4) / math.sqrt(d)
            if mask is not None:
                scores = scores + ((1.0 - mask.reshape(b, 1, 1, s)) * -10000.0).detach()
            out = (scores.softmax(axis=-1) @ v4).transpose(0, 2, 1, 3).reshape(b, s, width)
        (out * w).backward(allow_fill=True)

    def timed(fn):
        for _ in range(30):
            fn()
        HipDevice.synchronize()
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        L.check(lib.lg_event_create(ctypes.byref(e0)))
        L.check(lib.lg_event_create(ctypes.byref(e1)))
        L.check(lib.lg_event_record(e0))
        for _ in range(iters):
            fn()
        L.check(lib.lg_event_record(e1))
        HipDevice.synchronize()
        ms = ctypes.c_float()
        L.check(lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
        return 1e3 * ms.value / iters

    eager = timed(step)
    graph = HipGraph()
    with graph.capture():
        step()
    replayed = timed(graph.replay)
    graph.destroy()
    assert np.isfinite(q.grad.numpy()).all()
    return {"eager_us": round(eager, 2), "graph_us": round(replayed, 2)}


def worker(args):
    """the unmasked op on whatever library LIGHTGRAD_HIP_LIB names - also one that lacks entry points this tree declares"""
    from lightgrad_amd.autograd.hip import lib as L
    handle = ctypes.CDLL(L.LIB_PATH)
    for table in (L.PROTOTYPES, L.P2P_PROTOTYPES):
        for name in [n for n in table if not hasattr(handle, n)]:
            del table[name]
    print(json.dumps(measure("unmasked", 8, 128, 2, 64, False, args.iters)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", help="another build of liblghip.so (the parent commit's) to time the unmasked op on")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    # the unmasked op first, in fresh processes, before this one opens the GPU; the two builds alternate
    if args.other_lib:
        from lightgrad_amd.autograd.hip import lib as L
        builds = [("other build", os.path.abspath(args.other_lib)), ("this build", L.LIB_PATH)]
        seen = {name: [] for name, _ in builds}
        for _ in range(args.rounds):
            for name, path in builds:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--iters", str(args.iters)], check=True,
                                   env=dict(os.environ, LIGHTGRAD_HIP_LIB=path), stdout=subprocess.PIPE, text=True, timeout=300)
                seen[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
        say("unmasked attention forward + backward, (8, 128, 2 heads, d = 64), %d alternating fresh processes per build, us per step:" % args.rounds)
        for name, _ in builds:
            for key in ("graph_us", "eager_us"):
                xs = [r[key] for r in seen[name]]
                say("  %-12s %-9s %s   min %.2f  max %.2f" % (name, key, "  ".join("%.2f" % x for x in xs), min(xs), max(xs)))
    say("masked / tail attention forward + backward, fused (masked_attention) against the composite tape of this build, us per step:")
    for what, shape, masked in (("padding mask", (8, 128, 2, 64), True), ("length 100, no mask", (8, 100, 2, 64), False)):
        res = {route: [measure(route, *shape, masked, args.iters) for _ in range(args.rounds)] for route in ("fused", "composite")}
        for key in ("graph_us", "eager_us"):
            f, c = [r[key] for r in res["fused"]], [r[key] for r in res["composite"]]
            say("  %-20s %s %-9s fused %s   composite %s   composite / fused %.2f"
                % (what, shape, key, " ".join("%.2f" % x for x in f), " ".join("%.2f" % x for x in c), min(c) / min(f)))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
