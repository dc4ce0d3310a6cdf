"""Differential fuzzing of the HIP tape against the CPU backend (tests/tape_fuzz.py): random training programs over the ingredients
the backend's peepholes are made of - lazy relu, the fused head, paired gradient launches, epilogue accumulation, lazily zeroed
gradients, the optimizer in its forms (tape, fused per parameter, flat buckets, update inside the backward kernels, inside a
hipGraph) - every observable value judged by its distance to a float64 run of the same program (tape_fuzz.judge): within 1e-5
(relative Frobenius), or no further than twice the furthest of four float32 CPU runs that sum their products in different orders.
A program on which those four cannot vouch for each other is left out (tape_fuzz.CpuRuns.kept), at most one in ten per test."""
import numpy as np
import pytest
import lightgrad_amd as light
from tape_fuzz import (draw_program, run_program, cpu_runs, judge, merge_worst, worst_lines, within_the_cap, plain_programs,
                       flat_programs, shared_programs)

pytestmark = pytest.mark.gpu


class _Judged(object):
    """one test's programs: run on HIP and judged, or left out by the CPU runs alone; the cap and the printed record at the end"""

    def __init__(self, name):
        self.name, self.drawn, self.ran, self.left_out, self.worst, self.tally = name, 0, 0, [], {}, {}

    def kept(self, seed, prog):
        self.drawn += 1
        if not cpu_runs(prog).kept:
            self.left_out.append(seed)
            return False
        return True

    def judge(self, seed, prog, got):
        runs = cpu_runs(prog)
        merge_worst(self.worst, judge(runs.ref64, runs.variants, got, what="seed %d %r" % (seed, prog), tally=self.tally, known=runs.apart))
        self.ran += 1

    def run(self, hip, seed, prog, prepare=None):
        if self.kept(seed, prog):
            self.judge(seed, prog, run_program(hip, prog, prepare=prepare))

    def close(self):
        print(worst_lines(self.name, self.worst, self.drawn, self.left_out))
        print("%s: %d observables, %d judged at the 1e-5 floor" % (self.name, self.tally.get("observables", 0), self.tally.get("at_floor", 0)))
        assert within_the_cap(self.left_out, self.drawn), (self.name, self.left_out, self.drawn)
        return self.ran


@pytest.mark.parametrize("block", range(8))
def test_random_programs_match_the_cpu_backend(hip, block):
    judged = _Judged("plain/block%d" % block)
    for seed, prog in plain_programs(block * 25, 25):
        judged.run(hip, seed, prog)
    judged.close()


_PEEPHOLES = {"head_ride": ("_HEAD_RIDE",), "head_grad_ahead": ("_HEAD_GRAD_AHEAD",), "grad_group": ("GradGroup",),
              "all_three": ("_HEAD_RIDE", "_HEAD_GRAD_AHEAD", "GradGroup")}


@pytest.mark.parametrize("off", sorted(_PEEPHOLES))
def test_random_programs_with_peepholes_switched_off(hip, off):
    """the programs of the first four blocks with the riding head, the gradients written ahead and the queued weight gradients
    (GradGroup) switched off, one at a time and all together: the plain launches behind each peephole, which the default
    combination never takes, under the same judge"""
    from lightgrad_amd.autograd.hip import ops
    from lightgrad_amd.autograd.hip.tensor import GradGroup
    saved = ops._HEAD_RIDE, ops._HEAD_GRAD_AHEAD, GradGroup.enabled
    judged = _Judged("peepholes_off/" + off)
    try:
        for name in _PEEPHOLES[off]:
            if name == "GradGroup":
                GradGroup.enabled = False
            else:
                setattr(ops, name, False)
        for seed, prog in plain_programs(0, 100):
            judged.run(hip, seed, prog)
    finally:
        ops._HEAD_RIDE, ops._HEAD_GRAD_AHEAD, GradGroup.enabled = saved
    judged.close()


def _flat(in_backward):
    def prepare(model, make_opt):
        from lightgrad_amd.dist import DataParallel, SingleProcess
        dp = DataParallel(model.parameters(), SingleProcess(), flatten=True)
        opt = make_opt(model.parameters())
        dp.attach(opt)
        if in_backward:
            opt.fuse_update_into_backward()
        return opt
    return prepare


@pytest.mark.parametrize("in_backward", [False, True], ids=["flat_buckets", "update_in_backward"])
def test_random_programs_with_flat_bucket_optimizers(hip, in_backward):
    """the same programs with the optimizer over flat buckets (lazy zero_grad, one update launch) and with the update applied by
    the backward kernels - the forms bench.py runs.  Programs that the second form refuses by contract (two backward passes per
    step, no zero_grad before backward) are skipped for it."""
    judged = _Judged("update_in_backward" if in_backward else "flat_buckets")
    for seed, prog in flat_programs(plain_programs(300, 80), in_backward):
        judged.run(hip, seed, prog, prepare=_flat(in_backward))
    assert judged.close() >= 15


def test_random_programs_replayed_from_a_graph(hip):
    """a program's step recorded in a hipGraph after one eager step and replayed: the values of the eager HIP run, bit for bit"""
    from lightgrad_amd.autograd.hip import HipGraph
    from tape_fuzz import Net
    ran = 0
    for seed in range(500, 620):
        prog = draw_program(seed)
        if prog["optimizer"] == "sgd" or any(prog["peek"]) or any(prog["poke_input"]) or prog["second_backward"]:
            continue                                   # host reads / writes inside the step cannot be recorded
        rng = np.random.RandomState(seed)
        x_np = rng.uniform(-1, 1, (prog["batch"], prog["dims"][0])).astype(np.float32)
        t_np = rng.uniform(-1, 1, (prog["batch"], prog["dims"][-1])).astype(np.float32)

        def build():
            np.random.seed(seed)
            model = Net(prog["dims"], prog["biases"], prog["norm"]).map_parameters(lambda p: p.hip())
            cls = light.optim.Adam if prog["optimizer"] == "adam" else light.optim.AdaBelief
            opt = cls(model.parameters(), lr=1e-2, eps=1e-3, fused=True, device_step=True)
            x, t = hip.from_numpy(x_np, requires_grad=prog["x_requires_grad"]), hip.from_numpy(t_np, requires_grad=False)

            def step():
                h = x
                for k, layer in enumerate(model.layers):
                    h = layer(h)
                    if prog["acts"][k] != "none":
                        h = getattr(h, prog["acts"][k])()
                    if prog["norm"][k]:
                        h = model.norms[k](h)
                loss = light.loss.mse(h, t)
                opt.zero_grad()
                loss.backward()
                opt.step()
                return loss
            return model, opt, step
        model_e, _, step_e = build()
        eager = [step_e().item() for _ in range(5)]
        model_g, opt_g, step_g = build()
        losses = [step_g().item()]
        graph = HipGraph()
        with graph.capture():
            loss = step_g()
        opt_g.t -= len(opt_g.parameters)
        for _ in range(4):
            graph.replay()
            opt_g.on_graph_replay()
            losses.append(loss.item())
        np.testing.assert_array_equal(losses, eager, err_msg="seed %d" % seed)
        for (n, p), (_, q) in zip(model_g.named_parameters(), model_e.named_parameters()):
            np.testing.assert_array_equal(p.numpy(), q.numpy(), err_msg="seed %d %s" % (seed, n))
        ran += 1
    assert ran >= 12


# ---- programs that use a parameter twice (tape_fuzz.draw_shared: a square layer applied again, a weight / bias penalty) -------
def test_shared_parameter_programs_match_the_cpu_backend(hip):
    judged = _Judged("shared")
    for seed, prog in shared_programs(700, 60):
        judged.run(hip, seed, prog)
    assert judged.close() >= 25


def test_shared_parameter_programs_with_flat_buckets(hip):
    judged = _Judged("shared/flat_buckets")
    for seed, prog in flat_programs(shared_programs(850, 100)):
        judged.run(hip, seed, prog, prepare=_flat(False))
    assert judged.close() >= 25


def test_shared_parameter_programs_with_the_update_in_backward(hip):
    """accepted and as close to float64 as the CPU backend, or refused with the contract's error - never a silent divergence"""
    from lightgrad_amd.autograd.hip import HipError
    judged, refused = _Judged("shared/update_in_backward"), 0
    for seed, prog in flat_programs(shared_programs(900, 200), in_backward=True):
        made = []

        def prepare(model, make_opt):
            opt = _flat(True)(model, make_opt)
            made.append(opt)
            return opt
        kept = judged.kept(seed, prog)                 # by the CPU runs alone, whatever HIP says to the program
        try:
            got = run_program(hip, prog, prepare=prepare)
        except HipError as e:
            assert "again after its optimizer update was applied" in str(e), "seed %d: %s" % (seed, e)
            made[0]._backward_update.disarm()
            refused += 1
            continue
        if kept:
            judged.judge(seed, prog, got)
    accepted = judged.close()
    assert accepted >= 5 and refused >= 5, (accepted, refused)


def test_shared_parameter_programs_replayed_from_a_graph(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    from tape_fuzz import Net
    ran = 0
    for seed, prog in shared_programs(1100, 150):
        if prog["optimizer"] == "sgd" or any(prog["peek"]) or any(prog["poke_input"]) or prog["second_backward"]:
            continue
        rng = np.random.RandomState(seed)
        x_np = rng.uniform(-1, 1, (prog["batch"], prog["dims"][0])).astype(np.float32)
        t_np = rng.uniform(-1, 1, (prog["batch"], prog["dims"][-1])).astype(np.float32)

        def build():
            np.random.seed(seed)
            model = Net(prog["dims"], prog["biases"], prog["norm"]).map_parameters(lambda p: p.hip())
            cls = light.optim.Adam if prog["optimizer"] == "adam" else light.optim.AdaBelief
            opt = cls(model.parameters(), lr=1e-2, eps=1e-3, fused=True, device_step=True)
            x, t = hip.from_numpy(x_np, requires_grad=prog["x_requires_grad"]), hip.from_numpy(t_np, requires_grad=False)

            def step():
                h = x
                for k, layer in enumerate(model.layers):
                    h = layer(h)
                    if prog["acts"][k] != "none":
                        h = getattr(h, prog["acts"][k])()
                    if prog["reuse"] == k:
                        h = getattr(layer(h), prog["acts"][k] if prog["acts"][k] != "none" else "tanh")()
                    if prog["norm"][k]:
                        h = model.norms[k](h)
                loss = light.loss.mse(h, t)
                if prog["penalty"] is not None:
                    target, k, coef, place = prog["penalty"]
                    p = getattr(model.layers[k], target)
                    loss = (p * p).sum() * coef + loss if place == "before" else loss + (p * p).sum() * coef
                opt.zero_grad()
                loss.backward()
                opt.step()
                return loss
            return model, opt, step
        model_e, _, step_e = build()
        eager = [step_e().item() for _ in range(5)]
        model_g, opt_g, step_g = build()
        losses = [step_g().item()]
        graph = HipGraph()
        with graph.capture():
            loss = step_g()
        opt_g.t -= len(opt_g.parameters)
        for _ in range(4):
            graph.replay()
            opt_g.on_graph_replay()
            losses.append(loss.item())
        np.testing.assert_array_equal(losses, eager, err_msg="seed %d" % seed)
        for (n, p), (_, q) in zip(model_g.named_parameters(), model_e.named_parameters()):
            np.testing.assert_array_equal(p.numpy(), q.numpy(), err_msg="seed %d %s" % (seed, n))
        ran += 1
    assert ran >= 10
