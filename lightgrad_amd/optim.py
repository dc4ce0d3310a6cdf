"""Optimizers written as tensor expressions, backend-agnostic.

Restates the reference's `lightgrad/optim.py`: `step` adds `compute_delta(grad, i)`
to each parameter in place under no_grad (optim.py:10-13); SGD with momentum
(:15-25); Adam (:27-41) and AdaBelief (:43-52).  Note the reference quirk that
is kept on purpose: `self.t` advances once per *parameter*, not once per step
(optim.py:36, :48), so bias correction differs between parameters of one step.

The expression form is the definition and runs on every backend.  Optional
backend hooks (HipTensor implements them) replace it by
kernels that evaluate the SAME expression sequence per element:
  fused=True        one kernel per parameter instead of ~14 elementwise launches
  device_step=True  the step number behind the bias corrections lives in device
                    memory, so the whole training step can be captured in a
                    hipGraph and replayed (autograd/hip/graph.py)
  use_flat_buckets  parameters / gradients / moments live in flat buckets
                    (dist.DataParallel(flatten=True)): zero_grad is one fill and
                    the update of ALL parameters is one launch

Adam / AdaBelief also carry the rest of a BERT recipe, every part off by default:
decoupled weight decay (AdamW), clipping of the gradient by its global L2 norm and
a learning-rate schedule (`WarmupLinear`).  With flat buckets these ride in the
update launch, plus one reduction launch in front of it when clipping is on.
"""
from .autograd import Gradients, AbstractTensor


class Optimizer(object):
    """A tuple of parameters and the rule that turns a gradient into an additive update.

    Subclasses implement `compute_delta(grad, index)`; `step` adds the result to parameter `index` in place (the `+=` of
    the parameter's backend, so views handed out earlier keep seeing the parameter)."""

    def __init__(self, parameters) -> None:
        self.parameters = tuple(parameters)
        strangers = [type(p).__name__ for p in self.parameters if not isinstance(p, AbstractTensor)]
        assert not strangers, "optimizers update tensors, got %s" % strangers
        self._flat_grad = None          # the gradient bucket, once a flat-bucket backend took over (use_flat_buckets)
        self._exchange_outside = False  # dist.DataParallel.attach: the bucket is summed over the ranks after backward, before step

    def zero_grad(self) -> None:
        if self._flat_grad is None:
            for p in self.parameters:
                p.zero_grad()
            return
        # every p.grad is a view into the bucket, written by the first backward kernel that reaches it
        for p in self.parameters:
            p._grad_zero_pending = True

    def compute_delta(self, grad: AbstractTensor, idx: int) -> AbstractTensor:
        raise NotImplementedError("%s does not say how a gradient becomes an update" % type(self).__name__)

    def step(self) -> None:
        with Gradients.no_grad():
            for index, parameter in enumerate(self.parameters):
                parameter += self.compute_delta(parameter.grad, index)


class SGD(Optimizer):
    """gradient descent with (heavy-ball) momentum: the update is -lr * grad plus `momentum` times the previous update"""

    def __init__(self, parameters, lr: float, momentum: float = 0.0):
        Optimizer.__init__(self, parameters)
        self.lr = lr
        self.momentum = momentum
        self.last_update = {}           # parameter index -> the update applied last (missing: none yet)

    def compute_delta(self, grad, i):
        update = -self.lr * grad + self.momentum * self.last_update.get(i, 0)
        self.last_update[i] = update
        return update


class WarmupLinear(object):
    """learning-rate schedule of the BERT recipes: the factor rises linearly over `warmup_steps` steps to 1 and then falls
    linearly to 0 at `total_steps` (and stays there).  `factor(steps_done)` is evaluated in python floats (double); the
    flat-bucket update launch evaluates the same expressions on the device from its step counter (csrc/optim.hip)."""

    def __init__(self, warmup_steps: int, total_steps: int):
        warmup_steps, total_steps = int(warmup_steps), int(total_steps)
        assert 0 <= warmup_steps <= total_steps, "WarmupLinear needs 0 <= warmup_steps <= total_steps, got %d and %d" % (warmup_steps, total_steps)
        self.warmup_steps, self.total_steps = warmup_steps, total_steps

    def factor(self, steps_done: int) -> float:
        if steps_done < self.warmup_steps:
            return (steps_done + 1) / self.warmup_steps
        return max(0.0, (self.total_steps - steps_done) / max(1, self.total_steps - self.warmup_steps))


class Adam(Optimizer):
    """Adam (Kingma & Ba): running means of the gradient (`m`) and of its square (`v`), both bias-corrected by the number of
    updates `t` - which, as in the reference (optim.py:36), counts every PARAMETER's update, not every step.

    The rest of a training recipe, every part off by default (a step then runs exactly as it did without them).  With `s` the
    optimizer steps done before this one (`t // len(parameters)`):
      max_grad_norm  the gradients (after grad_scale) are multiplied by min(1, max_grad_norm / (norm + 1e-6)), norm their
                     global L2 norm - which `grad_norm()` returns afterwards, as it was before clipping
      schedule       an object with `factor(steps_done) -> float` (`WarmupLinear`): the step uses lr * schedule.factor(s)
      weight_decay   decoupled (AdamW): a decaying parameter also moves by -(lr_s * weight_decay) * p.  `decay_mask` holds
                     one bool per parameter; None: a parameter decays iff it has 2 or more dimensions (no decay on biases
                     and LayerNorm parameters)
    The expression form defines them on every backend (it reads the norm back to the host to form the coefficient).  With
    flat buckets they ride in the update launch - the schedule as a function of the DEVICE step counter, so a replayed
    hipGraph follows it - plus one reduction launch in front of it when clipping is on; the only schedule that launch knows
    is `WarmupLinear`.  `fused=True` WITHOUT flat buckets falls back to the expression form when any of them is set."""
    belief = False

    def __init__(self, parameters, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                 fused: bool = False, grad_scale: float = 1.0, device_step: bool = False,
                 weight_decay: float = 0.0, decay_mask=None, max_grad_norm: float = None, schedule=None):
        Optimizer.__init__(self, parameters)
        self.weight_decay, self.max_grad_norm, self.schedule = weight_decay, max_grad_norm, schedule
        if weight_decay == 0:
            self.decay_mask = (False,) * len(self.parameters)            # (the mask is ignored without a decay)
        elif decay_mask is None:
            self.decay_mask = tuple(len(p.shape) >= 2 for p in self.parameters)
        else:
            self.decay_mask = tuple(bool(d) for d in decay_mask)
            assert len(self.decay_mask) == len(self.parameters), \
                "decay_mask holds %d entries for %d parameters" % (len(self.decay_mask), len(self.parameters))
        self._recipe = weight_decay != 0 or max_grad_norm is not None or schedule is not None
        self._grad_norm = None          # 0-d tensor: the global gradient norm of the last step, before clipping
        self._clip_scratch = None       # flat buckets with clipping: (partial sums, ticket, (norm, coef)) of the norm launch
        self.lr, self.eps = lr, eps
        self.b1, self.b2 = beta1, beta2
        count = len(self.parameters)
        self.t, self.m, self.v = 0, [0] * count, [0] * count
        # grad_scale: factor applied to every gradient first (1/world_size in data-parallel training)
        self.fused, self.grad_scale, self.device_step = fused, grad_scale, device_step
        self._step_counter = None
        self._flat = None               # (flat_params, flat_m, flat_v, offsets) once use_flat_buckets() was called
        self._peer_exchange = None
        self._backward_update = None    # fuse_update_into_backward(): the backend object that arms / finishes every step
        self.last_step_launched_update = None

    def second_moment_input(self, grad, m):
        return grad

    def compute_delta(self, grad, i, lr=None):
        self.t += 1
        self.m[i] = self.b1 * self.m[i] + (1 - self.b1) * grad
        self.v[i] = self.b2 * self.v[i] + (1 - self.b2) * self.second_moment_input(grad, self.m[i])**2
        m, v = self.m[i] / (1 - self.b1**self.t), self.v[i] / (1 - self.b2**self.t)
        return -(self.lr if lr is None else lr) * m / (v**0.5 + self.eps)

    def grad_norm(self):
        """the global L2 norm of the gradients of the last step (after grad_scale, BEFORE clipping): a 0-d tensor of the
        parameters' backend.  Needs max_grad_norm."""
        assert self.max_grad_norm is not None, "grad_norm() is computed for clipping: pass max_grad_norm"
        if self._clip_scratch is not None:
            return self._clip_scratch[2][0]
        assert self._grad_norm is not None, "no step taken yet"
        return self._grad_norm

    def _step_recipe_expression(self) -> None:
        """one step with weight decay / clipping / schedule as tensor expressions: the definition, on every backend"""
        steps_done = self.t // len(self.parameters)
        grads = [p.grad if self.grad_scale == 1.0 else p.grad * self.grad_scale for p in self.parameters]
        if self.max_grad_norm is not None:
            total = None
            for g in grads:
                sq = (g * g).sum()
                total = sq if total is None else total + sq
            self._grad_norm = total ** 0.5
            coef = min(1.0, self.max_grad_norm / (float(self._grad_norm.item()) + 1e-6))      # (no tensor-level minimum: host)
            grads = [g * coef for g in grads]
        lr = self.lr if self.schedule is None else self.lr * self.schedule.factor(steps_done)
        for i, (p, g) in enumerate(zip(self.parameters, grads)):
            delta = self.compute_delta(g, i, lr)
            p += (delta + (-(lr * self.weight_decay)) * p) if self.decay_mask[i] else delta

    def use_flat_buckets(self, flat_params, flat_grads, offsets) -> None:
        """called by dist.DataParallel(flatten=True).attach(optimizer): parameter i is
        flat_params[offsets[i]:offsets[i+1]] and its gradient the same slice of flat_grads"""
        assert self.t == 0, "switch to flat buckets before the first step"
        assert self.fused and self.device_step and hasattr(flat_params, "_fused_adam_multi_dev"), \
            "flat buckets need fused=True, device_step=True and a backend with a multi-tensor kernel"
        cls = flat_params.__class__
        self._flat_grad = flat_grads
        self._flat = (flat_params, cls.zeros(flat_params.shape, requires_grad=False),
                      cls.zeros(flat_params.shape, requires_grad=False), tuple(int(o) for o in offsets))
        # the update launch advances the device step number itself: one private copy per workgroup of its grid
        longest = max(b - a for a, b in zip(self._flat[3][:-1], self._flat[3][1:]))
        self._step_counter = flat_params._new_step_counter(0, slots=max(1, len(self.parameters) * -(-longest // 1024)))
        if self._recipe:
            assert hasattr(flat_params, "_fused_adamw_multi_dev"), "the backend's flat-bucket update knows no weight decay / clipping / schedule"
            assert self.schedule is None or type(self.schedule) is WarmupLinear, \
                "the flat-bucket update evaluates the schedule on the device and knows WarmupLinear only"
            if self.max_grad_norm is not None:
                self._clip_scratch = flat_params._new_grad_norm_scratch()        # allocated here, never inside a (capturable) step

    def use_peer_exchange(self, comm) -> None:
        """data parallel with a communicator whose exchange rides in the optimizer launch (dist.PeerWindowCommunicator):
        step() first sums the flat gradient bucket over the ranks, in the same kernel"""
        assert self._flat is not None and hasattr(self._flat[0], "_fused_adam_multi_p2p"), "use_flat_buckets() first"
        assert not self._recipe, \
            "weight_decay / max_grad_norm / schedule are not part of the launch that exchanges the gradients between the ranks " \
            "(clipping needs the whole summed gradient before any update; decay and schedule inside that launch are not built): " \
            "attach(optimizer, exchange_in_optimizer=False) keeps the exchange in sync_gradients()"
        assert self.t == 0, "switch to the exchange inside the optimizer launch before the first step"
        self._peer_exchange = comm
        offsets = self._flat[3]
        chunks = sum(-(-(b - a) // 1024) for a, b in zip(offsets[:-1], offsets[1:]))
        self._step_counter = self._flat[0]._new_step_counter(0, slots=chunks)     # one private copy of the step per exchange workgroup

    def fuse_update_into_backward(self) -> None:
        """let the kernels that PRODUCE the parameter gradients apply this optimizer's update to them (HipTensor: the weight
        gradient GEMM's epilogue, its bias row sums, the skinny-head backward) - `step()` then launches nothing when every
        gradient was produced that way, and one kernel for the rest otherwise.  Same values as the update launch, bit for bit.
        Needs flat buckets; not with a data-parallel exchange of any kind (the update needs the SUMMED gradient: asserted here,
        also for an exchange that DataParallel.attach left to sync_gradients).  A kernel that OVERWRITES a parameter's whole
        gradient applies its update; any later write into that gradient in the same step - a weight shared between layers, a
        penalty on it, a tied table - raises HipError from that write (every writer of the library checks), after which
        `disarm()` of the backend object makes the library usable again.  Gradients that are only ADDED to (or written by
        kernels that carry no update) are updated by `step()` in one launch.  The parameters alternate between two buckets:
        `zero_grad(); backward(); step()` in that order, one backward per step, and an even number of steps inside a captured
        hipGraph, replayed from the bucket it was captured at (lightgrad_amd/autograd/hip/tensor.py: BackwardUpdate)."""
        assert self._flat is not None and hasattr(self._flat[0], "_new_backward_update"), "use_flat_buckets() first (dist.DataParallel(flatten=True).attach)"
        assert self._peer_exchange is None and not self._exchange_outside, \
            "the update cannot ride in the backward kernels when the gradients are exchanged first"
        assert not self._recipe, \
            "weight_decay / max_grad_norm / schedule cannot ride in the backward kernels: clipping needs the WHOLE gradient " \
            "before any parameter moves, and decay and schedule inside the update plans are not built"
        assert self.t % max(1, len(self.parameters)) == 0
        flat_p, flat_m, flat_v, offsets = self._flat
        self._backward_update = flat_p._new_backward_update(self.parameters, self._flat_grad, flat_m, flat_v, offsets, self.lr, self.b1, self.b2,
                                                            self.eps, self.grad_scale, self.belief, steps_done=self.t // max(1, len(self.parameters)))

    def zero_grad(self) -> None:
        Optimizer.zero_grad(self)
        if self._backward_update is not None:
            self._backward_update.arm()

    @Gradients.no_grad()
    def step(self) -> None:
        n_params = len(self.parameters)
        if self._backward_update is not None:
            for p in self.parameters:
                p._materialize_zero_grad()        # parameters no gradient reached since zero_grad
            _, here = self._backward_update.finish()
            self.last_step_launched_update = here > 0
            self.t += n_params
            return
        if self._flat is not None:
            for p in self.parameters:
                p._materialize_zero_grad()        # parameters no gradient reached since zero_grad
            flat_p, flat_m, flat_v, offsets = self._flat
            if self._recipe:
                # (an exchange outside this launch has already summed the bucket: the norm is the same on every rank)
                if self._clip_scratch is not None:
                    self._flat_grad._grad_norm_clip(self.grad_scale, self.max_grad_norm, self._clip_scratch)
                kind, warmup, total = (0, 0, 0) if self.schedule is None else (1, self.schedule.warmup_steps, self.schedule.total_steps)
                flat_p._fused_adamw_multi_dev(self._flat_grad, flat_m, flat_v, offsets, self.lr, self.b1, self.b2, self.eps,
                                              self._step_counter, self.grad_scale, self.belief, self.weight_decay, self.decay_mask,
                                              None if self._clip_scratch is None else self._clip_scratch[2], kind, warmup, total)
                self.t += n_params
                return
            update = flat_p._fused_adam_multi_dev if self._peer_exchange is None else flat_p._fused_adam_multi_p2p
            update(self._flat_grad, flat_m, flat_v, offsets, self.lr, self.b1, self.b2, self.eps,
                                         self._step_counter, self.grad_scale, self.belief)   # advances the device counter too
            self.t += n_params
            return
        if self._recipe:                          # (fused=True has no per-parameter kernel for these: the expression form)
            self._step_recipe_expression()
            return
        for i, p in enumerate(self.parameters):
            kernel = getattr(p, "_fused_adam_step", None) if self.fused else None
            if kernel is None:
                g = p.grad if self.grad_scale == 1.0 else p.grad * self.grad_scale
                p += self.compute_delta(g, i)
                continue
            self.t += 1
            if not isinstance(self.m[i], AbstractTensor):
                self.m[i] = p.__class__.zeros(p.shape, requires_grad=False)
                self.v[i] = p.__class__.zeros(p.shape, requires_grad=False)
            if self.device_step:
                if self._step_counter is None:
                    self._step_counter = p._new_step_counter((self.t - 1) // n_params)
                p._fused_adam_step_dev(p.grad, self.m[i], self.v[i], self.lr, self.b1, self.b2, self.eps,
                                       self._step_counter, n_params, i + 1, self.grad_scale, self.belief)
            else:
                kernel(p.grad, self.m[i], self.v[i], self.lr, self.b1, self.b2, self.eps,
                       (1 - self.b1**self.t) ** -1, (1 - self.b2**self.t) ** -1, self.grad_scale, self.belief)
        if self._step_counter is not None:
            self.parameters[0]._advance_step_counter(self._step_counter)      # these kernels only read the counter: one tiny launch

    def on_graph_replay(self, n: int = 1) -> None:
        """keep the host-side step count in line after `n` replays of a captured step (the schedule needs nothing here: the
        flat-bucket launch evaluates it from the device step counter, which the replays advance)"""
        self.t += n * len(self.parameters)


class AdaBelief(Adam):
    """AdaBelief (arXiv:2010.07468): Adam whose second running mean follows (grad - m)^2, the squared surprise, instead
    of grad^2"""
    belief = True

    def second_moment_input(self, grad, m):
        return grad - m
