"""Benchmark of the north-star path on MI355X (contract: see the task brief / DESIGN.md §Measurement).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]

N > 1 needs no external launcher: this process then only starts N fresh rank processes (lightgrad_amd/launch.py,
one per GPU; it never initialises a GPU itself), passes rank 0's JSON line through and exits non-zero if any rank
fails.  Launching the ranks with `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` works
as well (WORLD_SIZE is then already set and nothing is spawned).

One "step" = one MNIST-MLP training step (784->512->10, bias, batch 1024 PER GPU, loss.mse, AdaBelief lr 1e-3):
forward, backward, gradient all-reduce over RCCL (N > 1, overlapped with the tail of backward), optimizer update.
Inputs are synthetic and resident in HBM before the timed region.  `value` is the whole-job aggregate steps/s
(N ranks x K steps / max-over-ranks wall time): weak scaling.

A plain run sets up, warms up, times the K steps and prints the JSON line (`ms_per_step` = milliseconds of one timed step).
With `--full` the same line also carries BASELINE's second headline, the 4096^2 fp32 matmul forward+backward (`secondary`,
replicas on every rank), the roofline of the dominant kernel (the MFMA SGEMM; HIP events on the library's stream),
the eager-tape rate next to the graph-replay rate, the step with the batch as data, the cost of the exchange (N > 1),
tiny-BERT and the CPU baseline (this repo's CpuTensor backend running the same training loop on this host's cores;
rank 0, N = 1 only).

`--dump-outputs DIR` writes what the last timed step computed on rank 0 - the loss and the updated parameters - as
DIR/<name>.npy (float32).  The inputs are seeded, so two builds can be compared output for output.

`--dry-run` replaces the GPU work by a few CPU steps (CpuTensor + gloo): it exists to test the launcher, the rank
environment and the exchange protocol on machines without GPUs and prints a line marked "dry_run".
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_F32_PEAK_TFLOPS = 157.3        # MI355X_MICROARCH.md: 256 CU x 2.4 GHz x 256 FLOP/clk/CU (dense fp32 matrix)
HBM_PEAK_GBS = 8000.0               # HBM3E spec
MATMUL_N = 4096
MATMUL_FLOP = 3 * 2 * MATMUL_N ** 3  # fwd + dA + dB
MLP_GEMM_FLOP = 3 * 2 * 1024 * (784 * 512 + 512 * 10)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # 2000 timed steps = 0.12 s of GPU time: with 200 (12 ms) the two fences and the first graph launch are 2 % of the
    # measurement (16.4 k vs 16.7 k steps/s; 20 000 steps give what 2000 give)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides the headline: long window, eager tape, dispatch counts, batch as data, exchange "
                         "cost (N > 1), matmul / roofline / HBM / BERT / CPU legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the loss and the parameters after the last timed step (rank 0) as DIR/<name>.npy")
    ap.add_argument("--matmul-iters", type=int, default=20)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-bert", action="store_true", help="skip the tiny-BERT forward+backward timing")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the matmul / roofline / HBM / BERT / CPU legs")
    ap.add_argument("--no-fused-optimizer", action="store_true", help="run the optimizer as ~14 tape ops per parameter")
    ap.add_argument("--update-in-backward", action="store_true",
                    help="also on the legs of a multi-GPU run that train without the exchange (the default at N = 1, see --no-update-in-backward)")
    ap.add_argument("--no-update-in-backward", action="store_true",
                    help="N = 1: launch the optimizer's update as a kernel of its own.  The default lets the backward kernels apply it "
                         "(optim.Adam.fuse_update_into_backward: 3 launches per step instead of 4, same bits; the parameters alternate between "
                         "two buckets, so a recorded graph holds an even number of steps): 49.9 against 51.2 us per step on MI355X "
                         "(profiles/r4/mlp_step_ab_three_products.txt)")
    ap.add_argument("--force-comm", action="store_true",
                    help="exercise the multi-GPU code path (RCCL communicator, forked all-reduce inside the graph) with world_size 1")
    ap.add_argument("--dispatch", choices=["graph", "eager"], default="graph",
                    help="graph: the step's kernels are captured once in hipGraphs and replayed; eager: python tape every step")
    ap.add_argument("--comm-dispatch", choices=["auto", "p2p", "graph", "graph-inline", "eager"], default="auto",
                    help="N > 1, how the gradients are exchanged: p2p = hand-written exchange through peer-mapped device memory INSIDE "
                         "the optimizer launch of the captured step (csrc/p2p.hip: no collective library, no extra launch); graph = RCCL "
                         "all-reduce as a forked branch inside the captured step, overlapped with the input-gradient GEMM; graph-inline = "
                         "RCCL all-reduce inside the captured step on the compute stream; eager = forward+backward replay from a graph, "
                         "RCCL all-reduce and optimizer are host calls; auto = the host-launched RCCL form is timed in full first, then "
                         "a short run of each other form, fastest kept (all ranks agree)")
    ap.add_argument("--watchdog-exit-code", type=int, default=3,
                    help="exit code of a rank whose in-graph exchange did not come back within --exchange-timeout (the JSON line of the "
                         "host-launched form has been printed by then; the device is not to be trusted afterwards)")
    ap.add_argument("--exchange-timeout", type=float, default=180.0,
                    help="N > 1, --comm-dispatch auto: seconds an in-graph form of the exchange may take (calibration or full run) "
                         "before the result of the host-launched form, measured first, is printed and the job ends")
    ap.add_argument("--comm-open-timeout", type=float, default=120.0,
                    help="N > 1: seconds a form of communicator (RCCL, peer windows, host-staged) gets to come up on every rank before "
                         "all ranks drop it and go on with the next one")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="N > 1 on a box with ONE GPU: every rank binds device 0 and the ranks exchange through peer-mapped device "
                         "memory (RCCL refuses a second rank on a device, hipIpc handles are per process) - the multi-rank code of this "
                         "script, of DataParallel and of csrc/p2p.hip runs for real, but N ranks sharing one GPU measure no scaling; "
                         "the metric name says so")
    ap.add_argument("--graph-steps", type=int, default=32,
                    help="training steps recorded per hipGraph (each one complete: forward, backward, exchange, update); a replay "
                         "boundary costs ~8 us of idle GPU, so several steps per graph amortise it (8: 16.74 k, 32: 16.79 k, 50: 16.85 k "
                         "steps/s; 8 at most with rocprofv3 attached, whose queue interceptor faults on large graphs).  1 = one step per replay")
    ap.add_argument("--dry-run", action="store_true", help="CPU stand-in for the GPU work (launcher / protocol test)")
    ap.add_argument("--launch-timeout", type=float, default=None, help="seconds before the self-launcher gives up")
    return ap.parse_args()


def _launcher():
    """lightgrad_amd/launch.py loaded by path: the parent of a multi-rank job imports nothing else of the package"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("lightgrad_launch", os.path.join(ROOT, "lightgrad_amd", "launch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: become the launcher.  No HIP call has happened in this process.
        sys.exit(_launcher().spawn_ranks(args.gpus, [os.path.abspath(__file__)] + sys.argv[1:], timeout=args.launch_timeout))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if args.gpus > 1:
        assert world == args.gpus, "--gpus %d but WORLD_SIZE=%d" % (args.gpus, world)
    else:
        world, rank = 1, 0
    if args.dry_run:
        return dry_rank(args, rank, world)
    return gpu_rank(args, rank, world)


# ---------------------------------------------------------------------------------------------------------- dry run
def dry_rank(args, rank, world):
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd import CpuTensor
    from lightgrad_amd.dist import GlooCommunicator, SingleProcess, DataParallel
    why_not = {}
    if world > 1:
        # the same opening protocol as the GPU ranks (attempt under a timeout, vote through the rendezvous files, next form): here
        # the two device forms cannot work - no GPU in a dry run - so the chain is walked to its last link, the host communicator
        comm, _, comms, why_not = open_job_communicators(args, rank, world, None, dry=True)
    else:
        comm = SingleProcess()

    class MLP(light.nn.Module):
        def __init__(self):
            light.nn.Module.__init__(self)
            self.l1, self.l2 = light.nn.Linear(64, 32), light.nn.Linear(32, 10)

        def forward(self, x):
            return self.l2(self.l1(x).relu())
    np.random.seed(rank)                             # different on purpose: DataParallel broadcasts rank 0's weights
    model = MLP()
    dp = DataParallel(model.parameters(), comm, overlap=True)
    opt = light.optim.AdaBelief(model.parameters(), lr=1e-3, grad_scale=dp.grad_scale)
    rng = np.random.RandomState(1000 + rank)
    x = CpuTensor.from_numpy(rng.uniform(0, 1, (32, 64)).astype(np.float32))
    onehot = CpuTensor.from_numpy(np.eye(10, dtype=np.float32)[rng.randint(0, 10, 32)], requires_grad=False)

    def step():
        loss = light.loss.mse(model(x), onehot)
        opt.zero_grad()
        loss.backward()
        dp.sync_gradients()
        opt.step()
        return loss
    steps = min(args.steps, 20)
    for _ in range(min(args.warmup, 3)):
        step()
    comm.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    comm.barrier()
    mine = time.perf_counter() - t0
    t = CpuTensor.from_numpy(np.asarray([mine], np.float32), requires_grad=False)
    comm.allreduce_max_(t)
    elapsed = float(t.numpy()[0])
    rates = np.zeros(world, np.float32)
    rates[rank] = steps / mine
    rates = CpuTensor.from_numpy(rates, requires_grad=False)
    comm.allreduce_sum_(rates)
    digest = CpuTensor.from_numpy(np.asarray([dp.parameter_digest(), -dp.parameter_digest()], np.float32), requires_grad=False)
    comm.allreduce_max_(digest)
    dmax, dmin = digest.numpy()
    assert abs(dmax + dmin) <= 1e-6 * abs(dmax), "replicas diverged"
    assert np.isfinite(loss.item())
    if rank == 0:
        print(json.dumps({"metric": "DRY_RUN_launcher_and_exchange_check_on_cpu", "dry_run": True, "value": round(world * steps / elapsed, 2),
                          "unit": "steps/s", "n_gpus": world, "steps": steps, "warmup": min(args.warmup, 3),
                          "ms_per_step": round(1e3 * elapsed / steps, 4), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "config": {"workload": "cpu stand-in: mlp_64x32x10 batch 32, CpuTensor + gloo", "parallelism": "dp%d" % world},
                          "ranks": {"world_size": world, "communicator": type(comm).__name__, "communicator_ranks": comm.world_size,
                                    "communicators_not_usable": why_not or None,
                                    "per_rank_steps_per_sec": [round(float(v), 2) for v in rates.numpy()],
                                    "launcher": "lightgrad_amd.launch" if os.environ.get("LIGHTGRAD_LAUNCHED") else "external"}}))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------- GPU ranks
def preflight_report(lib, L, rank, world):
    """what this rank's device sees of the others (pure queries): the SCALE line then explains itself"""
    import ctypes
    n, dev = ctypes.c_int(0), ctypes.c_int(-1)
    lib.lg_device_count(ctypes.byref(n))
    L.check(lib.lg_device(ctypes.byref(dev)))
    names = {0: "hypertransport", 1: "qpi", 2: "pcie", 3: "infiniband", 4: "xgmi"}
    m = min(n.value, max(world, 1))
    access, links, hop_counts = [], [], []
    for a in range(m):                   # hipDeviceCanAccessPeer / hipExtGetLinkTypeAndHopCount for every pair of the job's devices
        row_a, row_l, row_h = [], [], []
        for b in range(m):
            can, kind, hops = ctypes.c_int(0), ctypes.c_int(-1), ctypes.c_int(-1)
            ok = lib.lg_peer_info(a, b, ctypes.byref(can), ctypes.byref(kind), ctypes.byref(hops)) == 0
            row_a.append(int(bool(can.value)) if ok else None)
            row_l.append("self" if a == b else (names.get(kind.value, None if kind.value < 0 else str(kind.value)) if ok else None))
            row_h.append(hops.value if ok and hops.value >= 0 else None)
        access.append(row_a)
        links.append(row_l)
        hop_counts.append(row_h)
    return {"rank": rank, "device": dev.value, "devices_visible": n.value, "enough_devices": n.value >= world,
            "can_access_peer": access, "link_type": links, "hops": hop_counts}


def open_job_communicators(args, rank, world, L, dry=False):
    """-> (bookkeeping communicator, peer-window communicator or None, {name: comm}, {name: why not}).
    dry: no GPU (bench.py --dry-run) - the device forms fail at once and the chain ends at the host communicator over gloo"""
    from lightgrad_amd.dist import open_communicators
    T = args.comm_open_timeout
    simulate = os.environ.get("LG_BENCH_FAIL_RCCL", "")            # tests of the fallback: "init", "init:<rank>", "hang"
    rehearsal = args.rehearse_on_one_gpu and world > 1
    Failure = RuntimeError if dry else L.HipError

    def open_rccl():
        if dry:
            raise Failure("dry run: no GPU, no RCCL")
        from lightgrad_amd.dist import RcclCommunicator
        if simulate.startswith("init") and (":" not in simulate or int(simulate.split(":")[1]) == rank):
            raise L.HipError("simulated RCCL initialisation failure (LG_BENCH_FAIL_RCCL=%s)" % simulate)
        if simulate:                                    # "hang", or a rank whose peer failed: what ncclCommInitRank does then
            time.sleep(10 ** 6)
        return RcclCommunicator(rank, world, rendezvous_timeout=T, selftest_timeout=max(5.0, T / 2))

    def open_peer():
        if dry:
            raise Failure("dry run: no GPU, no peer windows")
        from lightgrad_amd.dist import PeerWindowCommunicator, peer_window_selftest
        return peer_window_selftest(PeerWindowCommunicator(rank, world, rendezvous_timeout=T))

    openers = []
    if not rehearsal or simulate:                       # ranks sharing ONE GPU: RCCL refuses the second rank - not even tried
        openers.append(("rccl", open_rccl))
    if world > 1 or args.comm_dispatch in ("auto", "p2p"):     # world > 1: always - it carries the bookkeeping when RCCL cannot
        openers.append(("peer", open_peer))
    comms, why_not = open_communicators(rank, world, openers, timeout=T)
    if not comms:
        def open_host():
            import datetime
            import torch.distributed as dist
            from lightgrad_amd.dist import HostStagedCommunicator, GlooCommunicator, _c_stdout_to_stderr
            with _c_stdout_to_stderr():              # gloo announces its connections on the C-level stdout
                dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=max(30.0, T)))
                c = GlooCommunicator() if dry else HostStagedCommunicator()
                c.barrier()
            return c
        more, why_more = open_communicators(rank, world, [("host", open_host)], timeout=max(60.0, T) + 120.0)   # first `import torch` on a fresh box: minutes
        comms.update(more)
        why_not.update(why_more)
    comm = comms.get("rccl") or comms.get("peer") or comms.get("host")
    if comm is None:
        raise Failure("no form of the gradient exchange works on this node: %s" % json.dumps(why_not))
    return comm, comms.get("peer"), comms, why_not


def gpu_rank(args, rank, world):
    if not os.path.exists(os.path.join(ROOT, "lightgrad_amd", "liblghip.so")) and rank == 0:
        import subprocess            # the built library normally travels with the tree; compile it if it did not
        subprocess.run(["make", "-C", os.path.join(ROOT, "lightgrad_amd", "csrc"), "-j", "8"], check=True, stdout=sys.stderr)
    import numpy as np
    import lightgrad_amd as light
    from lightgrad_amd import HipTensor, CpuTensor
    from lightgrad_amd.autograd.hip import HipDevice, HipGraph, lib as L
    from lightgrad_amd.dist import SingleProcess, DataParallel

    if args.rehearse_on_one_gpu:
        from lightgrad_amd.dist import shared_gpu_environment
        os.environ.update(shared_gpu_environment(rank, world))      # every rank on the one GPU, each on its own share of the CUs
    lib = L.lib()                                    # binds HIP device LOCAL_RANK; raises without library / GPU
    info = HipDevice.info()
    multi = world > 1 or args.force_comm
    # Three forms of communicator, opened so that no rank is left waiting on one that does not work on this node
    # (dist.open_communicators: every attempt under a timeout, then a vote through the job's rendezvous files):
    #   rccl  RCCL over xGMI            bookkeeping (fences, slowest rank's clock) + the host-launched / in-graph collective forms
    #   peer  peer-mapped device memory the hand-written exchange inside the optimizer launch (csrc/p2p.hip); needs no RCCL, and
    #                                   carries the bookkeeping too when RCCL is not usable - always the case for ranks that
    #                                   share ONE GPU (RCCL refuses a second rank on a device; hipIpc handles are per process)
    #   host  D2H + gloo + H2D          last resort: a job that can still report a number
    # `comm` = the first of them that works everywhere; `why_not` says what happened to the others.
    peer, peer_error, comms, why_not, preflight = None, None, {}, {}, None
    if multi:
        preflight = preflight_report(lib, L, rank, world)
        comm, peer, comms, why_not = open_job_communicators(args, rank, world, L)
        peer_error = why_not.get("peer")
        if peer is None and args.comm_dispatch == "p2p":
            raise L.HipError("--comm-dispatch p2p: %s" % peer_error)
        if rank == 0 and why_not:
            sys.stderr.write("[bench] communicators: using %s; not usable: %s\n" % (type(comm).__name__, json.dumps(why_not)))
    else:
        comm = SingleProcess()
    # rocprofv3 (ROCm 7.2) faults in its HSA queue interceptor when a hipGraph's packet batch crosses the end of the
    # 16384-packet AQL ring (profiles/README.md, r2): keep the number of replayed graph nodes small when it is attached
    under_profiler = "rocprofiler" in os.environ.get("LD_PRELOAD", "") or bool(os.environ.get("ROCP_TOOL_LIBRARIES"))

    def wall_max(seconds):
        """max over ranks (the slowest rank defines the job's time)"""
        if not multi:
            return seconds
        t = HipTensor.from_numpy(np.asarray([seconds], np.float32), requires_grad=False)
        comm.allreduce_max_(t)
        return float(t.numpy()[0])

    def gather(value):
        """[value of rank 0, ..., value of rank world-1] on every rank"""
        v = np.zeros(world, np.float32)
        v[rank] = value
        if not multi:
            return [float(value)]
        t = HipTensor.from_numpy(v, requires_grad=False)
        comm.allreduce_sum_(t)
        return [float(x) for x in t.numpy()]

    def fence():
        comm.barrier()
        HipDevice.synchronize()

    # ------------------------------------------------------------------ MLP training step
    class MLP(light.nn.Module):
        def __init__(self):
            light.nn.Module.__init__(self)
            self.l1 = light.nn.Linear(784, 512)
            self.l2 = light.nn.Linear(512, 10)

        def forward(self, x):
            return self.l2(self.l1(x.reshape(-1, 784)).relu())

    def mlp_leg(comm_dispatch, n_steps=None, n_warmup=None, quick=False, no_exchange=False):
        """build model / optimizer / graphs and time the training step; raises if a capture fails or the replicas diverge.
        quick: a calibration run - only the timed steps, none of the side measurements.
        no_exchange: the same step in the same graph form WITHOUT the gradient exchange (every rank trains alone; the
        difference to the real step is what the exchange costs, `exchange_us_per_step`)"""
        n_steps = args.steps if n_steps is None else n_steps
        n_warmup = args.warmup if n_warmup is None else n_warmup
        np.random.seed(0)                                # identical initial weights on every rank (checked by broadcast)
        model = MLP()
        w0 = {n: p.numpy().copy() for n, p in model.named_parameters()}
        model.map_parameters(lambda p: p.hip())
        use_graph = args.dispatch == "graph" and not args.no_fused_optimizer
        in_optimizer = multi and comm_dispatch == "p2p" and use_graph and not no_exchange     # exchange inside the optimizer launch (csrc/p2p.hip)
        leg_comm = peer if (comm_dispatch == "p2p" or comm is peer) else comm
        if no_exchange:
            leg_comm = SingleProcess()
        streams = multi and leg_comm is comms.get("rccl")            # only RCCL has a communication stream to overlap on
        overlap = streams and not in_optimizer and (comm_dispatch == "graph" or not use_graph)
        dp = DataParallel(model.parameters(), leg_comm, flatten=use_graph, overlap=overlap)
        dp.always_sync = args.force_comm and not no_exchange        # world_size 1: still run the exchange
        opt = light.optim.AdaBelief(model.parameters(), lr=1e-3, fused=not args.no_fused_optimizer, grad_scale=dp.grad_scale,
                                    device_step=use_graph)
        if use_graph:
            dp.attach(opt, exchange_in_optimizer=in_optimizer)        # flat buckets: zero_grad = one flag, update = one launch
        # one GPU (or, with --update-in-backward, a rank training alone): the kernels that make the gradients apply the update themselves -
        # no optimizer launch.  The parameters then alternate between two buckets, so every recorded graph holds an even number of steps.
        wanted = (not multi and not args.no_update_in_backward) or (no_exchange and args.update_in_backward)
        in_backward = (use_graph and wanted and not args.force_comm and n_steps % 2 == 0 and min(args.graph_steps, n_steps) >= 2)
        if in_backward:
            opt.fuse_update_into_backward()
        per_graph = 2 if in_backward else 1                     # steps in the "one step" graph
        rng = np.random.RandomState(1000 + rank)         # every rank draws its own batch
        x_np = rng.uniform(0, 1, (1024, 784)).astype(np.float32)
        x = HipTensor.from_numpy(x_np)                   # requires_grad=True like the reference's loop (mnist.py:52-56): dx is computed
        labels = rng.randint(0, 10, 1024)
        onehot_np = np.zeros((1024, 10), np.float32)
        onehot_np[np.arange(1024), labels] = 1
        onehot = HipTensor.from_numpy(onehot_np)

        def forward_backward():
            loss = light.loss.mse(model(x), onehot)
            opt.zero_grad()
            loss.backward()
            return loss

        def eager_step():
            loss = forward_backward()
            dp.sync_gradients()
            opt.step()
            return loss

        step = eager_step
        comm_in_graph = False
        unroll = 1
        # three eager steps first: they allocate optimizer state, fill the pool, load kernels and teach DataParallel(overlap=True)
        # where the last gradient write is - and their losses are the parity check against the CPU backend on the same problem
        first_losses = [eager_step().item() for _ in range(3)]
        if use_graph:
            n_params = len(opt.parameters)
            g_all = None
            if not multi or comm_dispatch in ("p2p", "graph", "graph-inline") or (no_exchange and comm_dispatch != "eager"):
                # ONE graph for the whole step.  With a communicator the all-reduce is part of it - as a forked branch (started on
                # the communication stream after the last parameter-gradient kernel, joined before the optimizer kernel) or, with
                # graph-inline, as one more node of the chain on the compute stream.
                try:
                    g_all = HipGraph()
                    with g_all.capture():
                        for _ in range(per_graph):
                            graph_loss = eager_step()
                    comm_in_graph = multi and not no_exchange
                except L.HipError:
                    raise                        # multi: gpu_rank repeats the leg with host-launched collectives
                opt.t -= per_graph * n_params        # the capture pass ran the python bookkeeping, not the kernels
            if g_all is not None:
                def step():
                    g_all.replay()
                    opt.on_graph_replay(per_graph)
                    return graph_loss
                # several consecutive steps in ONE graph: the ~8 us the GPU idles between two graph launches (rocprofv3 trace,
                # tools/step_gap.py) is then paid once per `unroll` steps.  Every recorded step is a complete training step
                # on the resident batch; the timed loop below still performs exactly --steps of them.
                unroll = max(1, min(args.graph_steps if not under_profiler else min(args.graph_steps, 8), n_steps))
                while n_steps % unroll or unroll % per_graph:
                    unroll -= 1
                if unroll > 1:
                    g_multi = HipGraph()
                    with g_multi.capture():
                        for _ in range(unroll):
                            multi_loss = eager_step()
                    opt.t -= unroll * n_params
            else:
                # fallback (--comm-dispatch eager): forward+backward replay from a graph; the RCCL all-reduce and the optimizer
                # launch follow as host calls on the same stream
                g_fb = HipGraph()
                with g_fb.capture():
                    graph_loss = forward_backward()

                def step():
                    g_fb.replay()
                    dp.sync_gradients()
                    opt.step()
                    return graph_loss

        for _ in range(-(-n_warmup // per_graph) if (use_graph and g_all is not None) else n_warmup):
            loss = step()
        if unroll > 1:
            g_multi.replay()                             # untimed: first launch of the multi-step graph
            opt.on_graph_replay(unroll)
        fence()
        t0 = time.perf_counter()
        if unroll > 1:
            for _ in range(n_steps // unroll):
                g_multi.replay()
                opt.on_graph_replay(unroll)
            loss = multi_loss
        else:
            for _ in range(n_steps // (per_graph if (use_graph and g_all is not None) else 1)):
                loss = step()
        fence()
        mine = time.perf_counter() - t0
        elapsed = wall_max(mine)
        per_rank = gather(n_steps / mine)
        final_loss = loss.item()
        assert np.isfinite(final_loss), final_loss
        steps_per_s = world * n_steps / elapsed
        digest = dp.parameter_digest()
        if multi and not no_exchange:                    # replicas must still be identical
            d = HipTensor.from_numpy(np.asarray([digest, -digest], np.float32), requires_grad=False)
            comm.allreduce_max_(d)
            dmax, dmin = d.numpy()
            assert abs(dmax + dmin) <= 1e-6 * abs(dmax), "replicas diverged: %r" % ((dmax, -dmin),)
        if quick:
            return dict(steps_per_s=steps_per_s)
        # what the last timed step computed (--dump-outputs), read before any later step moves the parameters
        outputs = None
        if args.dump_outputs and rank == 0:
            outputs = {"loss": np.asarray(final_loss, np.float32)}
            outputs.update((n, np.asarray(p.numpy(), np.float32)) for n, p in model.named_parameters())
        R = dict(steps_per_s=steps_per_s, elapsed=elapsed, per_rank=per_rank, final_loss=final_loss, first_losses=first_losses,
                 in_backward=in_backward, comm_in_graph=comm_in_graph, unroll=unroll, use_graph=use_graph, overlap=dp.overlap, w0=w0, x_np=x_np,
                 onehot_np=onehot_np, outputs=outputs)
        if not args.full:
            return R
        # `value` covers exactly --steps steps; with few steps the two fences and the first launch weigh on it (20 steps = 1.2 ms:
        # -6 %), so the same loop is also timed over >= 0.1 s and reported NEXT to it (`value_long_window`), never as `value`
        long_window = None
        if use_graph and n_steps * (1.0 / steps_per_s * world) < 0.1:
            reps = max(1, int(0.12 * steps_per_s / world / max(1, unroll)))
            fence()
            t0 = time.perf_counter()
            for _ in range(reps):
                if unroll > 1:
                    g_multi.replay()
                    opt.on_graph_replay(unroll)
                else:
                    step()                          # one replayed step (+ the host-launched exchange and update of the "eager" form)
            fence()
            per_rep = unroll if unroll > 1 else (per_graph if g_all is not None else 1)
            long_window = {"steps": reps * per_rep, "steps_per_sec": round(world * reps * per_rep / wall_max(time.perf_counter() - t0), 2)}

        # the python tape every step (no graph): what "drop-in behind the autograd surface" costs without capture
        eager_steps = max(10, min(args.steps, 100))
        for _ in range(5):
            eager_step()
        fence()
        t0 = time.perf_counter()
        for _ in range(eager_steps):
            eager_step()
        fence()
        eager_steps_per_s = world * eager_steps / wall_max(time.perf_counter() - t0)
        # the launch-bound step's honest bound is host dispatch - tape nodes (Function calls) and kernel launches
        # of one eager step, counted by the profiler hooks of the tape and by the pool of a 1-step capture
        from lightgrad_amd.autograd.utils.profiler import Profiler
        with Profiler() as prof:
            eager_step()
        launches_per_step = None
        if use_graph:
            launches_per_step = g_all.kernel_count() // per_graph if g_all is not None else g_fb.kernel_count() + 2      # + host-launched all-reduce and optimizer
        dispatched_ops = int(sum(fc + bc for _, fc, _, bc in prof.table().values()))      # outermost Function calls, forward + backward

        # the same step with the batch marked as data (requires_grad=False): the input gradient, which the reference
        # computes and drops, is then not computed at all.  Reported next to `value`, never as `value`.
        data_input_steps_per_s = None
        if use_graph and not multi:
            x_data = HipTensor.from_numpy(x_np, requires_grad=False)

            def data_step():
                loss = light.loss.mse(model(x_data), onehot)
                opt.zero_grad()
                loss.backward()
                opt.step()
                return loss
            for _ in range(2):
                data_step()
            g_data = HipGraph()
            with g_data.capture():
                for _ in range(per_graph):
                    data_step()
            opt.t -= per_graph * n_params
            for _ in range(-(-args.warmup // per_graph)):
                g_data.replay()
            fence()
            t0 = time.perf_counter()
            for _ in range(max(1, args.steps // per_graph)):
                g_data.replay()
            fence()
            data_input_steps_per_s = max(1, args.steps // per_graph) * per_graph / (time.perf_counter() - t0)
            opt.on_graph_replay((-(-args.warmup // per_graph) + max(1, args.steps // per_graph)) * per_graph)
        R.update(eager_steps_per_s=eager_steps_per_s, dispatched_ops=dispatched_ops, launches_per_step=launches_per_step, long_window=long_window,
                 data_input_steps_per_s=data_input_steps_per_s)
        return R

    def communicator_fallback():
        """None when the bookkeeping runs on the first choice (RCCL between GPUs; peer windows for ranks sharing one GPU)"""
        if not multi or comm is comms.get("rccl") or (args.rehearse_on_one_gpu and "rccl" not in why_not):
            return None
        return "RCCL not usable (%s): fences, clocks and the exchange run through %s" % (why_not.get("rccl", "not attempted"), type(comm).__name__)

    def assemble(R, chosen, calibration, fallback_reason, extra, exchange_cost=None):
        """the one JSON line for a finished leg"""
        exchange_comm = peer if (chosen == "p2p" or comm is peer) else comm
        ranks_info = {"world_size": world, "communicator": type(comm).__name__,
                      "communicator_fallback": communicator_fallback(),
                      "communicators_not_usable": why_not or None,
                      "preflight": preflight,
                      "exchange_communicator": type(exchange_comm).__name__ if multi else None,
                      "peer_window_exchange": None if not multi else ("available" if peer is not None else "not available: %s" % peer_error),
                      "peer_window_memory": peer.memory_kind() if peer is not None else None,
                      # the step with and without its exchange, same graph form, slowest rank's clock (a SCALE line explains its own efficiency)
                      "exchange_us_per_step": exchange_cost,
                      "communicator_ranks": (exchange_comm.ranks_seen() if hasattr(exchange_comm, "ranks_seen") else exchange_comm.world_size) if multi else 1,   # what the library itself reports
                      "per_rank_steps_per_sec": [round(v, 2) for v in R["per_rank"]],
                      "launcher": "lightgrad_amd.launch" if os.environ.get("LIGHTGRAD_LAUNCHED") else
                                  ("torch.distributed.run" if os.environ.get("TORCHELASTIC_RUN_ID") else "none"),
                      "exchange": None if not multi else
                                  {"p2p": "hand-written exchange through peer-mapped device memory inside the optimizer launch of the captured step "
                                          "(push to the chunk owner, sum in rank order, publish; no collective library, no extra launch)",
                                   "graph": "all-reduce forked inside the captured step, overlapped with the input-gradient GEMM",
                                   "graph-inline": "all-reduce inside the captured step on the compute stream (no branch, no overlap)",
                                   "eager": "host-launched all-reduce (%s) after the replayed forward+backward graph" % type(exchange_comm).__name__}.get(chosen, chosen)
                                  if R["use_graph"] else "host-launched all-reduce on the communication stream, overlapped with backward (eager tape)",
                      "exchange_form": chosen if multi else None,
                      "exchange_calibration_steps_per_sec": calibration or None,
                      "in_graph_exchange_fallback": fallback_reason}
        out = {
            "metric": ("REHEARSAL_ranks_share_one_gpu__" if args.rehearse_on_one_gpu else "") +
                      "mnist_mlp_train_steps_per_sec_batch1024_per_gpu", "value": round(R["steps_per_s"], 2), "unit": "steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * R["elapsed"] / args.steps, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "mnist_mlp_784x512x10_bias_batch1024_mse_adabelief_lr1e-3 (fwd+bwd+allreduce+optimizer)",
                       "batch_per_gpu": 1024, "global_batch": 1024 * world, "parallelism": "dp%d" % world,
                       "optimizer_kernel": "tape" if args.no_fused_optimizer else ("applied by the backward kernels (no launch of its own)" if R["in_backward"] else "fused"),
                       "input_requires_grad": True,
                       "dispatch": ("hipGraph replay (python tape captured once; %d consecutive steps per graph)" % R["unroll"]) if R["use_graph"] else "eager python tape",
                       "steps_per_graph": R["unroll"],
                       "device": info["name"], "compute_units": info["compute_units"], "clock_mhz": info["clock_mhz"]},
            "final_loss": round(R["final_loss"], 6),
            "first_losses": [round(v, 7) for v in R["first_losses"]],
            "ranks": ranks_info,
            "mlp_gemm_tflops": round(R["steps_per_s"] * MLP_GEMM_FLOP / 1e12, 3),
        }
        if args.full:
            out.update({
                "value_long_window": R["long_window"],
                "mlp_steps_per_sec_eager": round(R["eager_steps_per_s"], 2),
                # the launch-bound step, per dispatched op - tape dispatches (outermost Function forward / backward calls +
                # the optimizer) of one eager step, the kernel launches they turn into, and the host time per dispatch of the eager tape
                "dispatch": {"tape_dispatches_per_step": R["dispatched_ops"], "launches_per_step": R["launches_per_step"],
                             "us_per_dispatched_op_eager": round(1e6 / R["eager_steps_per_s"] * world / max(1, R["dispatched_ops"]), 2),
                             "us_per_launch_replayed": round(1e6 / R["steps_per_s"] * world / max(1, R["launches_per_step"]), 2) if R["launches_per_step"] else None},
                "mlp_steps_per_sec_batch_as_data": None if R["data_input_steps_per_s"] is None else round(R["data_input_steps_per_s"], 2),
            })
        out.update(extra)
        return out

    def side_measurements(R):
        if args.no_extras or not args.full:
            return {}
        return extras(R["first_losses"], args, rank, world, multi, comm, lib, L, light, HipTensor, CpuTensor, HipDevice, HipGraph, DataParallel,
                      SingleProcess, wall_max, fence, under_profiler, R["w0"], R["x_np"], R["onehot_np"])

    def exchange_cost_of(mode, guard=None):
        """us per step that the exchange costs: the same step in the same graph form with and without it (two short runs of
        equal length, slowest rank's clock)"""
        try:
            quick_steps = 5 * min(args.graph_steps, 8)
            rates = []
            for no_exchange in (True, False):
                run = lambda: mlp_leg(mode, n_steps=quick_steps, n_warmup=min(args.warmup, 10), quick=True, no_exchange=no_exchange)["steps_per_s"]
                rates.append(guard(mode, "exchange cost", run, key="exchange_cost") if guard else run())
            without, with_ = rates
            return {"form": mode, "steps_timed": quick_steps, "with_exchange_us": round(1e6 * world / with_, 2),
                    "without_exchange_us": round(1e6 * world / without, 2), "exchange_us": round(1e6 * world / with_ - 1e6 * world / without, 2)}
        except (L.HipError, AssertionError) as e:
            return {"form": mode, "failed": "%s: %s" % (type(e).__name__, e)}

    calibration, fallback_reason = {}, None
    if multi and args.comm_dispatch == "auto":
        # Where the all-reduce runs is decided by measurement.  FIRST the form that captures nothing of RCCL - forward+backward
        # replayed from a graph, the collective and the optimizer as host calls - is timed in full, and its JSON line is ready.
        # THEN the two in-graph forms get a short calibration run each, under a watchdog: the forked branch inside the captured
        # step is what the hardware invites, but what a branch - or a captured collective - costs in a replayed
        # hipGraph is a property of the runtime, not of this code.  A form that fails drops out; one that does not come back
        # within --exchange-timeout ends the job with the line already in hand; one that beats the host-launched form by more
        # than 2 % is timed in full (same watchdog) and reported if it is still ahead.  Every decision uses the slowest rank's
        # clock, so all ranks decide alike.
        import threading
        state = {"deadline": None, "label": None, "line": None}

        def watchdog():
            while True:
                time.sleep(0.5)
                if state["deadline"] is not None and time.time() > state["deadline"]:
                    sys.stderr.write("[bench] rank %d: %r did not finish within %.0f s - reporting what is in hand\n"
                                     % (rank, state["label"], args.exchange_timeout))
                    if rank == 0:
                        print(state["line"])
                        sys.stdout.flush()
                    sys.stderr.flush()
                    os._exit(args.watchdog_exit_code)   # the stuck collective cannot be recovered in this process: not a success
        threading.Thread(target=watchdog, daemon=True).start()
        # the first leg has no measured line behind it: if even the host-launched form never comes back, the job still ends,
        # with a line that says so (value null) and the watchdog's exit code
        state["line"] = json.dumps({"metric": "mnist_mlp_train_steps_per_sec_batch1024_per_gpu", "value": None, "unit": "steps/s", "n_gpus": world,
                                    "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "scaling": "weak",
                                    "error": "the host-launched form of the exchange did not finish within %.0f s" % (4 * args.exchange_timeout),
                                    "ranks": {"world_size": world, "communicator": type(comm).__name__, "communicators_not_usable": why_not or None,
                                              "preflight": preflight}})
        state["label"], state["deadline"] = "eager (first leg)", time.time() + 4 * args.exchange_timeout
        best, chosen = mlp_leg("eager"), "eager"
        state["deadline"] = None
        extra = side_measurements(best)
        calibration["eager"] = round(best["steps_per_s"], 1)

        def guarded(mode, what, fn, key=None):
            calibration_so_far = dict(calibration)
            calibration_so_far[key or mode] = "no answer within %.0f s (%s)" % (args.exchange_timeout, what)
            state["line"] = json.dumps(assemble(best, chosen, calibration_so_far, "%s: watchdog" % (key or mode), extra))
            state["label"], state["deadline"] = key or mode, time.time() + args.exchange_timeout
            try:
                return fn()
            finally:
                state["deadline"] = None

        # the peer-window form first (the cheapest exchange); in-graph collectives need a device-side communicator, the forked
        # branch RCCL's communication stream.  After ONE failure of a peer-window form the communicator is dead for good
        # (lg_p2p_state: every later launch is refused) - its other forms are not tried.
        candidates = (["p2p"] if peer is not None else []) + (["graph-inline"] if comm is not comms.get("host") else []) \
            + (["graph"] if comm is comms.get("rccl") else [])
        peer_lost = False
        for mode in candidates:
            uses_peer = mode == "p2p" or comm is peer
            if peer_lost and uses_peer:
                calibration[mode] = "not tried: the peer-window communicator failed earlier"
                continue
            try:
                quick_steps = 5 * min(args.graph_steps, 8)
                if os.environ.get("LG_BENCH_SIMULATE_HANG") == mode:          # tests of the watchdog only
                    guarded(mode, "calibration", lambda: time.sleep(10 ** 6))
                rate = guarded(mode, "calibration", lambda: mlp_leg(mode, n_steps=quick_steps, n_warmup=min(args.warmup, 10), quick=True)["steps_per_s"])
                calibration[mode] = round(rate, 1)
            except (L.HipError, AssertionError) as e:
                calibration[mode] = "failed: %s: %s" % (type(e).__name__, e)
                sys.stderr.write("[bench] rank %d: exchange form %r failed in calibration (%s)\n" % (rank, mode, calibration[mode]))
                peer_lost = peer_lost or (uses_peer and peer is not None and peer.failed())
                continue
            if rate > 1.02 * best["steps_per_s"]:
                try:
                    R_mode = guarded(mode, "full run", lambda: mlp_leg(mode))
                    if R_mode["steps_per_s"] > best["steps_per_s"]:
                        best, chosen = R_mode, mode
                except (L.HipError, AssertionError) as e:
                    fallback_reason = "%s: %s: %s" % (mode, type(e).__name__, e)
                    sys.stderr.write("[bench] rank %d: the full run with exchange form %r failed (%s)\n" % (rank, mode, fallback_reason))
                    peer_lost = peer_lost or (uses_peer and peer is not None and peer.failed())
        cost = None
        if args.full and not (peer_lost and (chosen == "p2p" or comm is peer)):
            state["line"] = json.dumps(assemble(best, chosen, calibration, fallback_reason, extra))
            cost = exchange_cost_of(chosen, guarded)
        out = assemble(best, chosen, calibration, fallback_reason, extra, cost)
    else:
        modes = {"graph": ["graph", "eager"], "p2p": ["p2p", "eager"]}.get(args.comm_dispatch, [args.comm_dispatch]) if multi else ["graph"]
        R, chosen = None, None
        for k, mode in enumerate(modes):
            try:
                R = mlp_leg(mode)
                chosen = mode
                break
            except (L.HipError, AssertionError) as e:
                if k == len(modes) - 1:
                    raise
                fallback_reason = "%s: %s: %s" % (mode, type(e).__name__, e)
                sys.stderr.write("[bench] rank %d: the leg with exchange form %r failed (%s); repeating with %r\n"
                                 % (rank, mode, fallback_reason, modes[k + 1]))
        cost = exchange_cost_of(chosen) if world > 1 and args.full else None
        out = assemble(R, chosen, calibration, fallback_reason, side_measurements(R), cost)
        best = R
    if rank == 0 and args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in best["outputs"].items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)
    if rank == 0:
        print(json.dumps(out))
        sys.stdout.flush()
    if multi:
        for c in comms.values():
            try:
                c.close()
            except (L.HipError, TimeoutError) as e:
                sys.stderr.write("[bench] rank %d: closing %s: %s\n" % (rank, type(c).__name__, e))
        if comms.get("host") is not None:
            import torch.distributed as dist
            dist.destroy_process_group()
    import threading
    if any(t.name == "lightgrad-open-communicator" and t.is_alive() for t in threading.enumerate()):
        sys.stderr.flush()               # a communicator attempt was abandoned inside its library: do not run that library's
        os._exit(0)                      # teardown under it - the result has been printed


def extras(first_losses, args, rank, world, multi, comm, lib, L, light, HipTensor, CpuTensor, HipDevice, HipGraph, DataParallel, SingleProcess,
           wall_max, fence, under_profiler, w0, x_np, onehot_np):
    """everything besides the headline: 4096^2 matmul, roofline of the dominant kernel, HBM microbench, tiny-BERT, CPU baseline"""
    import ctypes
    import numpy as np
    # ------------------------------------------------------------------ 4096^2 matmul forward + backward
    np.random.seed(0)
    a = HipTensor.from_numpy(np.random.uniform(-1, 1, (MATMUL_N, MATMUL_N)).astype(np.float32))
    b = HipTensor.from_numpy(np.random.uniform(-1, 1, (MATMUL_N, MATMUL_N)).astype(np.float32))

    def matmul_iter():
        a.zero_grad()
        b.zero_grad()
        y = a @ b
        y.backward(allow_fill=True)

    for _ in range(8):
        matmul_iter()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.matmul_iters):
        matmul_iter()
    fence()
    mm_elapsed = wall_max(time.perf_counter() - t0)
    mm_tflops = world * args.matmul_iters * MATMUL_FLOP / mm_elapsed / 1e12

    # ------------------------------------------------------------------ roofline of the dominant kernel (HIP events)
    def event():
        e = ctypes.c_void_p()
        L.check(lib.lg_event_create(ctypes.byref(e)))
        return e

    def time_launches(fn, n, batches=3):
        """average launch duration over n back-to-back launches (HIP events on the library's stream); the median of
        `batches` such measurements, so that a clock ramp after the light MLP phase does not decide the number"""
        for _ in range(3):
            fn()
        out = []
        for _ in range(batches):
            e0, e1 = event(), event()
            L.check(lib.lg_event_record(e0))
            for _ in range(n):
                fn()
            L.check(lib.lg_event_record(e1))
            ms = ctypes.c_float()
            L.check(lib.lg_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
            lib.lg_event_destroy(e0)
            lib.lg_event_destroy(e1)
            out.append(ms.value / n)
        return sorted(out)[len(out) // 2]

    def time_launches_in_graph(fn, n, batches=3):
        """the same for launches that take less time than the host needs to issue them (the MLP step's products: several C ABI
        calls per launch): n launches recorded in a hipGraph, the replay timed - the kernels back to back as in the training step,
        whatever the box's CPUs are doing"""
        g = HipGraph()
        with g.capture():
            for _ in range(n):
                fn()
        out = time_launches(g.replay, 1, batches) / n
        g.destroy()
        return out

    c = HipTensor.empty((MATMUL_N, MATMUL_N), requires_grad=False)
    n = MATMUL_N
    gemm_ms = {}
    for tag, (ta, tb) in {"NN": (0, 0), "NT": (0, 1), "TN": (1, 0)}.items():
        gemm_ms[tag] = time_launches(lambda: L.check(lib.lg_gemm_f32(ta, tb, n, n, n, a.ptr, n, 0, b.ptr, n, 0, c.ptr, n, 0, 1, 0)), 10)
    gemm_tf = {k: 2 * n ** 3 / (v * 1e-3) / 1e12 for k, v in gemm_ms.items()}
    # HBM bytes per launch of the same kernel from rocprofv3 PMC passes (profiles/rN/pmc_traffic.json; separate runs,
    # corrected as MI355X_MICROARCH.md prescribes) - cannot be collected from inside this process
    traffic = None
    for rnd in ("r4", "r3", "r2", "r1"):
        try:
            with open(os.path.join(ROOT, "profiles", rnd, "pmc_traffic.json")) as f:
                traffic = json.load(f).get("sgemm_mfma_256x256_NN_4096", {}).get("hbm_bytes_per_launch")
            if traffic is not None:
                break
        except (OSError, ValueError):
            pass
    roofline = {"kernel": "sgemm_mfma<256,256,32,4,4> NN 4096^3 (forward GEMM of the matmul workload)", "bound": "mfma",
                "achieved": round(gemm_tf["NN"], 2), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(gemm_tf["NN"] / MFMA_F32_PEAK_TFLOPS, 4), "traffic": traffic,
                "avg_launch_ms": round(gemm_ms["NN"], 4), "algorithmic_flop_per_launch": 2 * n ** 3}
    del c
    # ---- the roofline of the HEADLINE step's own kernels: the two MFMA launches of the MLP step, timed the same
    # way through the C ABI on operands of the step's shapes - the forward product of the first layer (bias epilogue) and the
    # launch that makes the head's dW2 (+ db2), dW1 (+ db1 as row sums), dx and the loss together (lg_gemm_pair_*); the other
    # launch of the backward pass' inputs (the N = 10 head's forward, which also writes the head's input gradients) moves 6 MB
    # and does 20 MFLOP: launch latency, no roofline to speak of
    rs = np.random.RandomState(5 + rank)
    B_, I_, H_ = 1024, 784, 512
    sx = HipTensor.from_numpy(rs.uniform(0, 1, (B_, I_)).astype(np.float32), requires_grad=False)
    sw = HipTensor.from_numpy((rs.uniform(-1, 1, (H_, I_)) / np.sqrt(H_ * I_)).astype(np.float32), requires_grad=False)
    sb = HipTensor.from_numpy(rs.uniform(-1, 1, (H_,)).astype(np.float32), requires_grad=False)
    sg = HipTensor.from_numpy(rs.uniform(-1, 1, (B_, H_)).astype(np.float32), requires_grad=False)
    sy, sdw, sdb, sdx = (HipTensor.empty(shape, requires_grad=False) for shape in ((B_, H_), (H_, I_), (H_,), (B_, I_)))
    O_ = 10
    serr = HipTensor.from_numpy(rs.uniform(-1, 1, (B_, O_)).astype(np.float32), requires_grad=False)
    srl = HipTensor.from_numpy(rs.uniform(0, 1, (B_,)).astype(np.float32), requires_grad=False)
    sdw2, sdb2, sloss = (HipTensor.empty(shape, requires_grad=False) for shape in ((O_, H_), (O_,), ()))

    def step_forward():        # pre = x @ W1^T + b1
        L.check(lib.lg_gemm_bias_f32(0, 1, B_, H_, I_, sx.ptr, I_, 0, sw.ptr, I_, 0, sy.ptr, H_, 0, 1, sb.ptr))

    def step_backward():       # dW2 (+ db2) = err^T @ relu(pre), dW1 (+ db1) = g^T @ x, dx = g @ W1 and the loss in one launch
        L.check(lib.lg_gemm_pair_begin())
        L.check(lib.lg_gemm_fused_f32(1, 0, O_, H_, B_, serr.ptr, O_, sy.ptr, H_, sdw2.ptr, H_, 0, None, sdb2.ptr, 0, 0, 1))
        L.check(lib.lg_gemm_pair_mse_loss(srl.ptr, B_, B_ * O_, sloss.ptr))
        L.check(lib.lg_gemm_rowsum_f32(1, 0, H_, I_, B_, sg.ptr, H_, sx.ptr, I_, sdw.ptr, I_, 0, sdb.ptr, 0))
        L.check(lib.lg_gemm_f32(0, 0, B_, I_, H_, sg.ptr, H_, 0, sw.ptr, I_, 0, sdx.ptr, I_, 0, 1, 0))
        L.check(lib.lg_gemm_pair_end())
    step_forward(), step_backward()
    fwd_us = 1e3 * time_launches_in_graph(step_forward, 20)
    bwd_us = 1e3 * time_launches_in_graph(step_backward, 20)
    fwd_flop, bwd_flop = 2 * B_ * H_ * I_, 2 * 2 * B_ * H_ * I_ + 2 * B_ * H_ * O_
    roofline_step = {
        "kernel": "sgemm_triple_wgrad2_xgrad (dW2 + db2 = err^T @ relu(pre), dW1 + db1 = g^T @ x, dx = g @ W1 and the scalar loss in one launch): the dominant kernel of the MLP step",
        "bound": "mfma", "algorithmic_flop_per_launch": bwd_flop, "avg_launch_us": round(bwd_us, 2),
        "achieved": round(bwd_flop / bwd_us / 1e6, 2), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
        "frac": round(bwd_flop / bwd_us / 1e6 / MFMA_F32_PEAK_TFLOPS, 4),
        "forward_product": {"kernel": "sgemm_mfma 1024x512x784 NT + bias", "algorithmic_flop_per_launch": fwd_flop, "avg_launch_us": round(fwd_us, 2),
                            "achieved": round(fwd_flop / fwd_us / 1e6, 2), "frac": round(fwd_flop / fwd_us / 1e6 / MFMA_F32_PEAK_TFLOPS, 4)},
        "how": "HIP events on the library stream around the replay of a hipGraph of 20 such launches issued through the C ABI (launch boundaries included), median of 3"}
    del sx, sw, sb, sg, sy, sdw, sdb, sdx, serr, srl, sdw2, sdb2, sloss
    # HBM-bound kernels of the path, 16384 x 8192 fp32 (512 MiB per tensor: beyond the 256 MiB Infinity Cache).  The
    # operands hold RANDOM data (a 16 MiB random block repeated; constants switch fewer wires and read high)
    big = (16384, 8192)
    nbig = big[0] * big[1]
    p, q, r = (HipTensor.empty(big, requires_grad=False) for _ in range(3))
    tile_n = 1 << 22
    blk = np.random.RandomState(7 + rank).uniform(-1, 1, 2 * tile_n).astype(np.float32)
    with light.no_grad():
        p.reshape(nbig // tile_n, tile_n)[...] = HipTensor.from_numpy(blk[:tile_n], requires_grad=False)
        q.reshape(nbig // tile_n, tile_n)[...] = HipTensor.from_numpy(blk[tile_n:], requires_grad=False)
    st = L.i64(p.strides)
    sh = L.i64(big)
    hbm = {}

    def ew(op, out, ins):
        args_ = []
        for t in ins + [None] * (4 - len(ins)):
            args_ += [t.ptr if t is not None else None, st if t is not None else None]
        return lambda: L.check(lib.lg_ew(op, 2, sh, out.ptr, st, None, None, *args_, 0.0))
    from lightgrad_amd.autograd.hip import ops as H
    bias_row = HipTensor.from_numpy(np.random.RandomState(3).uniform(-1, 1, (big[1],)).astype(np.float32), requires_grad=False)
    with light.no_grad():
        rowmax = p.max(axis=1, keepdims=True)
    for name, fn, bytes_per_elem in [("add", ew(L.EW_ADD, r, [p, q]), 12), ("mul", ew(L.EW_MUL, r, [p, q]), 12),
                                     ("relu", ew(L.EW_RELU, r, [p]), 8), ("exp", ew(L.EW_EXP, r, [p]), 8),
                                     ("relu_bwd", ew(L.EW_RELU_BWD, r, [p, q]), 12), ("iadd", ew(L.EW_ADD, r, [r, q]), 12),
                                     # backward forms and strided / broadcast operands, through the ops' own entry points
                                     ("exp_bwd  y*g", lambda: H._binary(L.EW_MUL, p, q, out=r), 12),
                                     ("mul_bwd  (g*b, a*g)", lambda: H._ew(L.EW_MUL_BWD, big, [p, q, r], n_out=2), 20),
                                     ("max_bwd  g*(x==max) axis=1", lambda: H._ew(L.EW_MAX_BWD, big, [p, rowmax, rowmax], out=r), 8),
                                     ("add_bias (N,C)+(C,)", lambda: H._binary(L.EW_ADD, p, bias_row, out=r), 8)]:
        ms = time_launches(fn, 5)
        hbm[name] = {"ms": round(ms, 4), "GB/s": round(nbig * bytes_per_elem / (ms * 1e-3) / 1e9, 1)}
    del rowmax
    # transposed operands at 8192^2 (256 MiB per tensor): the strided `dW +=` of the reference's tape and a layout change
    sq = (8192, 8192)
    ta, tb = p.reshape(2, 8192, 8192)[0], q.reshape(2, 8192, 8192)[0]
    tout = r.reshape(2, 8192, 8192)[0]
    for name, fn, nbytes in [("add a + b.T", lambda: H._binary(L.EW_ADD, ta, tb.transpose(1, 0), out=tout), 12 * sq[0] * sq[1]),
                             ("contiguous(b.T)", lambda: tb.transpose(1, 0).contiguous(), 8 * sq[0] * sq[1])]:
        with light.no_grad():
            ms = time_launches(fn, 5)
        hbm[name] = {"ms": round(ms, 4), "GB/s": round(nbytes / (ms * 1e-3) / 1e9, 1), "shape": "8192x8192"}
    del ta, tb, tout
    s_out = HipTensor.empty((), requires_grad=False)
    for name, op in [("sum", L.RED_SUM), ("max", L.RED_MAX)]:
        ms = time_launches(lambda: L.check(lib.lg_reduce(op, 2, sh, p.ptr, st, 3, s_out.ptr)), 5)
        hbm[name] = {"ms": round(ms, 4), "GB/s": round(nbig * 4 / (ms * 1e-3) / 1e9, 1)}
    col_out = HipTensor.empty((big[1],), requires_grad=False)
    ms = time_launches(lambda: L.check(lib.lg_reduce(L.RED_SUM, 2, sh, p.ptr, st, 1, col_out.ptr)), 5)
    hbm["sum_axis0"] = {"ms": round(ms, 4), "GB/s": round(nbig * 4 / (ms * 1e-3) / 1e9, 1)}
    for v in hbm.values():
        v["frac_of_8TBs"] = round(v["GB/s"] / HBM_PEAK_GBS, 3)
    hbm["operands"] = "random U(-1,1), 16 MiB block repeated"
    del p, q, r

    # ------------------------------------------------------------------ tiny-BERT forward + backward (BASELINE config #5)
    bert_ms = bert_graph_ms = bert_launches = None
    bert_replays = 0
    try:
        if args.no_bert:
            raise RuntimeError("skipped (--no-bert)")
        import importlib.util
        spec = importlib.util.spec_from_file_location("bert_example", os.path.join(ROOT, "examples", "bert.py"))
        bert = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bert)
        np.random.seed(0)
        bmodel = bert.BertForMaskedLM(**bert.TINY).map_parameters(lambda t: t.hip())
        ids = HipTensor.from_numpy(np.random.randint(0, bert.TINY["vocab_size"], (8, 128)).astype(np.int32), requires_grad=False)

        mlm_labels = HipTensor.from_numpy(np.random.randint(0, bert.TINY["vocab_size"], (8 * 128,)).astype(np.int64), requires_grad=False)
        # all parameter gradients are views into one flat bucket (the layout the data-parallel path uses): zeroing
        # them is one fill instead of one per parameter
        bdp = DataParallel(bmodel.parameters(), SingleProcess(), flatten=True)

        def bert_iter():
            logits = bmodel(ids)
            loss = light.loss.cross_entropy(logits.reshape(-1, bert.TINY["vocab_size"]), mlm_labels)   # masked-LM loss, every position
            bdp.bucket.fill(0)               # (one fill of the bucket: marking every gradient "zero pending" instead turns into six
            loss.backward()                  #  fills of its own for the parameters whose kernels can only add - 42 -> 48 launches, measured)
        for _ in range(3):
            bert_iter()
        fence()
        batches = []                         # the eager tape is host-bound: best of three batches (shared host CPUs)
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(5):
                bert_iter()
            fence()
            batches.append(time.perf_counter() - t0)
        bert_ms = 1e3 * wall_max(min(batches)) / 5
        bgraph = HipGraph()
        with bgraph.capture():
            bert_iter()
        bert_launches = bgraph.kernel_count()
        # 50 timed replays; only 6 with rocprofv3 attached - its HSA queue interceptor faults once a graph's packet batch
        # crosses the end of the 16384-packet AQL ring (evidence: profiles/README.md r2), un-profiled runs never do
        bert_replays = 6 if under_profiler else 50
        for _ in range(2 if under_profiler else 5):
            bgraph.replay()
        fence()
        t0 = time.perf_counter()
        for _ in range(bert_replays):
            bgraph.replay()
        fence()
        bert_graph_ms = 1e3 * wall_max(time.perf_counter() - t0) / bert_replays
        bgraph.destroy()
        del bmodel
    except Exception as e:            # the BERT row is "next" scope: never let it take the headline numbers down
        bert_ms = "failed: %r" % (e,)

    # ------------------------------------------------------------------ CPU baseline (host cores, rank 0 at N = 1)
    cpu_baseline = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu_baseline = cpu_baseline_leg(light, CpuTensor, w0, x_np, onehot_np, a, b)
        cpu_first = cpu_baseline["first_losses"]
        cpu_baseline["parity_first_losses_max_rel_diff"] = max(abs(g - c) / abs(c) for g, c in zip(first_losses, cpu_first))
        cpu_baseline["parity_first_losses_within_1e-5"] = bool(cpu_baseline["parity_first_losses_max_rel_diff"] < 1e-5)   # north-star tolerance

    return {
        "secondary": {"metric": "matmul4096_fwd_bwd_tflops", "value": round(mm_tflops, 2), "unit": "TFLOP/s",
                      "ms_per_iter": round(1e3 * mm_elapsed / args.matmul_iters, 4), "iters": args.matmul_iters,
                      "flop_per_iter": MATMUL_FLOP, "frac_of_mfma_peak": round(mm_tflops / world / MFMA_F32_PEAK_TFLOPS, 4),
                      "scaling": "replicas", "gemm_kernel_tflops": {k: round(v, 2) for k, v in gemm_tf.items()}},
        "tiny_bert_fwd_bwd": {"ms_per_iter": bert_ms if isinstance(bert_ms, str) else round(bert_ms, 3), "batch": 8, "seq_len": 128,
                              "config": "2 layers, hidden 128, heads 2, intermediate 512, vocab 30522; masked-LM cross-entropy over all 1024 positions",
                              "dispatch": "eager python tape",
                              "ms_per_iter_hipgraph": round(bert_graph_ms, 3) if bert_graph_ms else None,
                              "launches_per_iter": bert_launches,
                              "hipgraph_replays_timed": bert_replays, "profiler_attached": under_profiler},
        "roofline": roofline,
        "roofline_step": roofline_step,
        "roofline_hbm": hbm,
        "cpu_baseline": cpu_baseline,
    }


def cpu_baseline_leg(light, CpuTensor, w0, x_np, onehot_np, a, b):
    """the CPU baseline is this repo's CpuTensor backend (pinned bit for bit to the reference's CPU
    backend by tests/test_cpu_backend.py) running the SAME training loop through the python tape, on this host's cores;
    BLAS on all threads and on one.  The tape-free numpy oracle is timed next to it as a second, friendlier figure."""
    import numpy as np

    class MLP(light.nn.Module):
        def __init__(self):
            light.nn.Module.__init__(self)
            self.l1 = light.nn.Linear(784, 512)
            self.l2 = light.nn.Linear(512, 10)

        def forward(self, x):
            return self.l2(self.l1(x.reshape(-1, 784)).relu())

    def tape_loop(seconds, max_steps):
        model = MLP()
        model.load_parameters(w0)
        opt = light.optim.AdaBelief(model.parameters(), lr=1e-3)
        xc, tc = CpuTensor.from_numpy(x_np), CpuTensor.from_numpy(onehot_np)
        n, t0, first = 0, time.perf_counter(), []
        while time.perf_counter() - t0 < seconds and n < max_steps:
            loss = light.loss.mse(model(xc), tc)
            opt.zero_grad()
            loss.backward()
            opt.step()
            n += 1
            if n <= 3:
                first.append(loss.item())
        assert np.isfinite(loss.item())
        return n, n / (time.perf_counter() - t0), first

    n_all, all_threads, first_losses = tape_loop(8.0, 2000)
    one_thread = n_one = None
    blas = None
    try:
        from threadpoolctl import threadpool_limits, threadpool_info
        blas = [{"library": i.get("internal_api"), "version": i.get("version"), "threads": i.get("num_threads"),
                 "threading_layer": i.get("threading_layer"), "architecture": i.get("architecture")}
                for i in threadpool_info() if i.get("user_api") == "blas"]
        with threadpool_limits(limits=1):
            n_one, one_thread, _ = tape_loop(6.0, 2000)
    except Exception:                # threadpoolctl missing or BLAS not controllable: report the all-threads number only
        pass
    an, bn = CpuTensor.from_numpy(a.numpy()), CpuTensor.from_numpy(b.numpy())
    t0 = time.perf_counter()
    (an @ bn).backward(allow_fill=True)
    cpu_mm = time.perf_counter() - t0
    # the tape-free oracle (no python tape, no per-op dispatch): a second figure, never `value`
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import np_oracle as O                       # the checker, timed here ONLY as a reported CPU figure
    o_opt = O.make_optimizer("adabelief")
    w = {k: v.copy() for k, v in w0.items()}
    t0, n_or = time.perf_counter(), 0
    while time.perf_counter() - t0 < 4.0 and n_or < 1000:
        _, grads, _ = O.mlp_loss_and_grads(w, x_np, onehot_np)
        for name in O.PARAM_ORDER:
            w[name] += o_opt.delta(name, grads[name])
        n_or += 1
    oracle_rate = n_or / (time.perf_counter() - t0)
    best_is_one = one_thread is not None and one_thread > all_threads
    return {"value": round(one_thread if best_is_one else all_threads, 2), "unit": "steps/s",
            "cores": 1 if best_is_one else os.cpu_count(), "kind": "port",
            "what": "lightgrad_amd CpuTensor backend (numpy), same MLP training loop through the python tape",
            "value_all_blas_threads": round(all_threads, 2), "value_one_blas_thread": None if one_thread is None else round(one_thread, 2),
            "host_cpus": os.cpu_count(), "blas": blas,
            "sample": "%d steps in ~8 s on all BLAS threads%s; matmul4096 fwd+bwd x1: %.2f s = %.3f TFLOP/s"
                      % (n_all, "" if n_one is None else ", %d steps in ~6 s on one" % n_one, cpu_mm, MATMUL_FLOP / cpu_mm / 1e12),
            "matmul4096_tflops": round(MATMUL_FLOP / cpu_mm / 1e12, 3),
            "oracle_tape_free_steps_per_sec": round(oracle_rate, 2), "numpy": np.__version__,
            "first_losses": [round(float(v), 7) for v in first_losses]}


if __name__ == "__main__":
    main()
