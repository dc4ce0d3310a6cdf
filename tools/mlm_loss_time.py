"""Time the masked-LM launches on tiny-BERT's shapes (HIP events, 20 back-to-back calls, best of 5):
  mean       lg_cross_entropy_mean_f32 on (1024, 30522) logits
  ignore0    lg_cross_entropy_ignore_f32, no row ignored          (expected: `mean` + the count launch)
  ignore85   lg_cross_entropy_ignore_f32, 85 % of the rows ignored (expected: clearly below `mean`)
  mask       lg_mlm_mask on (8, 128) int32 ids

    python tools/mlm_loss_time.py            # every case, each in a process of its own under a time limit; stops at the first failure
    python tools/mlm_loss_time.py CASE       # one case in this process
"""
import ctypes
import os
import subprocess
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("mean", "ignore0", "ignore85", "mask")
LIMIT = 120          # seconds per case


def measure(case):
    sys.path.insert(0, ROOT)
    from lightgrad_amd import HipTensor
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    rng = np.random.RandomState(0)
    rows, cols = 1024, 30522

    def event():
        e = ctypes.c_void_p()
        L.check(lib.lg_event_create(ctypes.byref(e)))
        return e

    if case == "mask":
        ids = HipTensor.from_numpy(rng.randint(1000, cols, (8, 128)).astype(np.int32), requires_grad=False)
        masked, labels = HipTensor.empty((8, 128), dtype=np.int32), HipTensor.empty((8, 128), dtype=np.int32)
        base = HipTensor.empty((1,), dtype=np.uint64)
        special = (ctypes.c_int64 * 3)(0, 101, 102)

        def run():
            L.check(lib.lg_mlm_mask(ids.ptr, 4, masked.ptr, labels.ptr, 1024, 0.15, 103, cols, special, 3, -100, base.ptr))
        what = "lg_mlm_mask (8, 128) int32"
    else:
        logits = HipTensor.from_numpy(rng.uniform(-8, 8, (rows, cols)).astype(np.float32))
        host_labels = rng.randint(0, cols, rows).astype(np.int64)
        if case == "ignore85":
            host_labels[rng.permutation(rows)[:int(round(0.85 * rows))]] = -100
        labels = HipTensor.from_numpy(host_labels, requires_grad=False)
        dl, nll, mean = HipTensor.empty((rows, cols)), HipTensor.empty((rows,)), HipTensor.empty(())
        n_valid = HipTensor.empty((1,), dtype=np.int64)
        if case == "mean":
            def run():
                L.check(lib.lg_cross_entropy_mean_f32(logits.ptr, labels.ptr, 8, dl.ptr, nll.ptr, mean.ptr, rows, cols))
            what = "lg_cross_entropy_mean_f32 (1024, 30522)"
        else:
            def run():
                L.check(lib.lg_cross_entropy_ignore_f32(logits.ptr, labels.ptr, 8, dl.ptr, nll.ptr, mean.ptr, n_valid.ptr, rows, cols, -100))
            what = "lg_cross_entropy_ignore_f32 (1024, 30522), %d of 1024 rows ignored" % int((host_labels == -100).sum())

    for _ in range(3):
        run()
    best = 1e9
    for _ in range(5):
        e0, e1 = event(), event()
        L.check(lib.lg_event_record(e0))
        for _ in range(20):
            run()
        L.check(lib.lg_event_record(e1))
        ms = ctypes.c_float()
        L.check(lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
        best = min(best, 1e3 * ms.value / 20)
    print("%-8s %-70s %8.2f us per call" % (case, what, best), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        if sys.argv[1] not in CASES:
            sys.exit("unknown case %r (%s)" % (sys.argv[1], ", ".join(CASES)))
        measure(sys.argv[1])
    else:
        for case in CASES:                                   # this process never opens the GPU: one fresh child per case
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), case], timeout=LIMIT).returncode
            except subprocess.TimeoutExpired:
                sys.exit("%s: no result within %d s - nothing more is started" % (case, LIMIT))
            if rc != 0:
                sys.exit("%s: exit status %d - nothing more is started" % (case, rc))
