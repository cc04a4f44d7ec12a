"""Training-step harness: flat parameter / gradient buffers, fused AdamW, data-parallel gradient all-reduce over
RCCL, checkpoint format and whole-step hipGraph capture.

Mirrors the hot-path-relevant surface of the reference's engine.BaseTrainTester (engine.py:18-230) and
TrainTester.train_one_step (main_keypose.py:207-234, main_trajectory.py:177-204):
  get_optimizer   -> FlatAdamW with the reference's two parameter groups (names containing "bias" -> no decay)
  DDP wrap        -> FlatDataParallel: one flat fp32 gradient buffer, all-reduce(SUM) then 1/world folded into AdamW
  save/load_checkpoint -> {"weight" (module.-prefixed), "optimizer", "iter", "best_loss"}
The reference's CLI, data loaders, tensorboard and evaluation loop are out of scope.
"""
import contextlib
import ctypes
import math
import os

import torch
import torch.distributed as dist

from . import lib as L

NO_DECAY = ["bias", "LayerNorm.weight", "LayerNorm.bias"]       # engine.py:95 (the LayerNorm patterns never match)


def _is_no_decay(name):
    return any(nd in name for nd in NO_DECAY)


def discover_active_parameters(model, run_fwd_bwd):
    """Names of the parameters that receive a gradient in one forward/backward (the reference relies on
    find_unused_parameters=True and AdamW skipping grad=None parameters, engine.py:121-124)."""
    for p in model.parameters():
        p.grad = None
    run_fwd_bwd()
    active = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is not None]
    for p in model.parameters():
        p.grad = None
    return active


class FlatParams:
    """Re-homes the active parameters into ONE flat fp32 buffer and their .grad into one flat gradient buffer.

    Layout: [ no-decay | decay ]; inside each, parameters of `late_prefixes` (the FPN, whose gradients are produced
    last in backward) are placed at the inner edge so that they form one contiguous middle segment:
        [ hot no-decay | late no-decay | late decay | hot decay ]
    which lets the hot-path segments be all-reduced while the FPN backward is still running."""

    def __init__(self, model, active_names=None, late_prefixes=("feature_pyramid",)):
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if active_names is not None:
            keep = set(active_names)
            named = [(n, p) for n, p in named if n in keep]
        is_late = lambda n: any(pre in n for pre in late_prefixes)
        segs = [[], [], [], []]
        for n, p in named:
            nd, late = _is_no_decay(n), is_late(n)
            segs[0 if (nd and not late) else 1 if (nd and late) else 2 if late else 3].append((n, p))
        self.order = [x for s in segs for x in s]
        # torch.optim.AdamW indices of the reference's optimizer (engine.py:89-102): every named parameter, the "bias"
        # group first, each group in named_parameters() order -- used to exchange optimizer state with reference checkpoints
        every = [n for n, _ in model.named_parameters()]
        self.torch_groups = [[n for n in every if _is_no_decay(n)], [n for n in every if not _is_no_decay(n)]]
        self.torch_index = {n: i for i, n in enumerate(self.torch_groups[0] + self.torch_groups[1])}
        sizes = [sum(p.numel() for _, p in s) for s in segs]
        self.n = sum(sizes)
        self.n_nodecay = sizes[0] + sizes[1]
        self.late_range = (sizes[0], sizes[0] + sizes[1] + sizes[2])
        dev = self.order[0][1].device
        self.flat = torch.empty(self.n, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self.slices = {}
        off = 0
        with torch.no_grad():
            for n, p in self.order:
                k = p.numel()
                self.flat[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.flat[off:off + k].view(p.shape)
                p.grad = self.grad[off:off + k].view(p.shape)
                self.slices[n] = (off, off + k)
                off += k

    def rebind_grads(self):
        """Re-attach .grad views (after something set p.grad = None)."""
        for n, p in self.order:
            a, b = self.slices[n]
            p.grad = self.grad[a:b].view(p.shape)

    def zero_grad(self):
        self.grad.zero_()
        for n, p in self.order:
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + self.slices[n][0] * 4:
                self.rebind_grads()
                break


def _check_ema(ema_decay, ema_warmup):
    """The ranges a3d_adamw_ema_step accepts, checked where the keywords enter.  Returns (decay or None, warmup) as floats."""
    if ema_decay is None:
        return None, float(ema_warmup)
    d, w = float(ema_decay), float(ema_warmup)
    if not (math.isfinite(d) and 0.0 <= d < 1.0):
        raise ValueError("ema_decay = %r is outside [0, 1)" % (ema_decay,))
    if not (w == 0.0 or (math.isfinite(w) and w >= 1.0)):
        raise ValueError("ema_warmup = %r must be 0 (constant decay) or a finite value >= 1" % (ema_warmup,))
    return d, w


def _check_max_grad_norm(max_grad_norm):
    """The range a3d_adamw_clip_step accepts for max_norm, checked where the keyword enters.  Returns None (off) or a float;
    +inf is legal: the norm is measured and non-finite steps are skipped, but nothing is ever clipped."""
    if max_grad_norm is None:
        return None
    x = float(max_grad_norm)
    if not (x > 0.0 and ctypes.c_float(x).value > 0.0):      # NaN fails the comparison; the kernel takes an fp32
        raise ValueError("max_grad_norm = %r must be > 0 (None: no clipping)" % (max_grad_norm,))
    return x


def _check_lr_schedule(lr_schedule):
    """The schedules a3d_adamw_sched_step accepts, checked where the keyword enters.  A preset name ("constant", "linear",
    "cosine") or a dict over decay / warmup / total / min_ratio; returns None (off) or the complete dict.  `total` is required
    unless the rate stays constant after the warm-up."""
    if lr_schedule is None:
        return None
    s = {"decay": lr_schedule} if isinstance(lr_schedule, str) else lr_schedule
    if not isinstance(s, dict) or not set(s) <= {"decay", "warmup", "total", "min_ratio"}:
        raise ValueError("lr_schedule = %r: expected a preset name or a dict over decay, warmup, total, min_ratio" % (lr_schedule,))
    decay, warmup, total, ratio = s.get("decay", "constant"), s.get("warmup", 0), s.get("total"), s.get("min_ratio", 0.0)

    def steps(name, x):
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not (0 <= x < 2 ** 24) or x != int(x):
            raise ValueError("lr_schedule: %s = %r must be an integer in [0, 2^24)" % (name, x))
        return int(x)
    if not isinstance(decay, str) or decay not in L.LR_DECAY_KINDS:
        raise ValueError("lr_schedule: decay = %r (expected one of %s)" % (decay, sorted(L.LR_DECAY_KINDS)))
    warmup = steps("warmup", warmup)
    if decay != "constant":
        if total is None:
            raise ValueError("lr_schedule: decay = %r needs total, the step at which the decay ends" % (decay,))
        if steps("total", total) <= warmup:
            raise ValueError("lr_schedule: total = %r must be above warmup = %r" % (total, warmup))
    total = None if total is None else steps("total", total)
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not (0.0 <= ratio <= 1.0):      # NaN fails the comparison
        raise ValueError("lr_schedule: min_ratio = %r is outside [0, 1]" % (ratio,))
    return {"decay": decay, "warmup": warmup, "total": total, "min_ratio": float(ratio)}


class FlatAdamW:
    """torch.optim.AdamW semantics (lr, betas, eps, two weight-decay groups) as one fused kernel over FlatParams.

    With `ema_decay` the same launch also keeps an exponential moving average of the weights (`ema`, a second flat buffer;
    DESIGN 4.21): decay min(ema_decay, (1 + t) / (ema_warmup + t)) at the t-th EMA update, t counted on the device
    (`ema_updates`).  The averages are read by exchanging them with the weights IN PLACE (`swap_ema`, `ema_weights()`): the
    parameters are views of flat.flat and every captured graph addresses that buffer, so nothing is rebound.

    With `max_grad_norm` the step clips the global norm of the (grad_scale-averaged) gradient to that value and skips a step whose
    norm is not finite, both decided on the device inside the same call: `grad_norm`, `clip_scale`, `clipped_steps`,
    `skipped_steps`, `last_step_skipped` are views of the device state.  That state is not part of state_dict() / checkpoints.

    With `lr_schedule` the rate of every step is `lr` times a warm-up + decay factor that the step evaluates on the device from
    its own position, so a captured step graph follows the schedule and a later `optimizer.lr = x`: `current_lr`,
    `lr_factor` and `schedule_step` are views of the device state.  `lr` and the checkpoints keep the base rate; a loaded state
    continues the schedule at its step count."""

    def __init__(self, flat, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4, ema_decay=None, ema_warmup=10,
                 max_grad_norm=None, lr_schedule=None):
        self.flat, self.betas, self.eps, self.weight_decay = flat, betas, eps, weight_decay
        self.ema_decay, self.ema_warmup = _check_ema(ema_decay, ema_warmup)
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)
        self.lr_schedule = _check_lr_schedule(lr_schedule)
        self.lr_state = None
        if self.lr_schedule is not None:
            # {lr_t of the last applied step, position t, f(t) of the last applied step, base rate, 0, 0, 0, 0}
            self.lr_state = torch.zeros(8, device=flat.flat.device, dtype=torch.float32)
            self.lr_state[3] = float(lr)
        self.clip_state = self.clip_ws = None
        if self.max_grad_norm is not None:
            # {e applied, norm, coef, clipped steps, skipped steps, last step skipped, 0, 0} and the norm pass's partials
            self.clip_state = torch.zeros(8, device=flat.flat.device, dtype=torch.float32)
            self.clip_ws = torch.zeros(L.ADAMW_CLIP_WS_DOUBLES, device=flat.flat.device, dtype=torch.float64)
        self.ema = self.ema_state = None
        self.ema_swapped = False                 # True while flat.flat holds the averages and `ema` the raw weights
        if self.ema_decay is not None:
            self.ema = flat.flat.detach().clone()
            self.ema_state = torch.zeros(4, device=flat.flat.device, dtype=torch.float32)       # {w, updates, 0, 0}
        self.exp_avg = torch.zeros_like(flat.flat)
        self.exp_avg_sq = torch.zeros_like(flat.flat)
        self.step_count = torch.zeros(1, device=flat.flat.device, dtype=torch.float32)     # optimizer.step() calls so far
        # per-parameter table of the fused kernel: element offsets of the parameters in buffer order, and per parameter
        # {step (torch's state[p]["step"]), active, lr / bc1, sqrt(bc2)}.  A parameter is updated from the first step in which
        # its gradient segment holds a non-zero element (torch: .grad is not None) and then every step, all elements
        self.seg_off = torch.tensor([flat.slices[n][0] for n, _ in flat.order] + [flat.n], dtype=torch.int64, device=flat.flat.device)
        self.seg_state = torch.zeros((len(flat.order), 4), device=flat.flat.device, dtype=torch.float32)
        self.param_groups = [{"lr": lr, "weight_decay": 0.0}, {"lr": lr, "weight_decay": weight_decay}]

    @property
    def lr(self):
        """The learning rate the fused kernel uses: ONE value for both groups (the reference builds both groups with
        args.lr and resets every group to it on resume, engine.py:89-102,200-201)."""
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value):
        for g in self.param_groups:
            g["lr"] = float(value)
        if self.lr_state is not None:            # the base rate of the device schedule: stream-ordered, reaches every later replay
            self.lr_state[3] = float(value)

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    def step(self, grad_scale=1.0):
        f = self.flat
        if self.ema is not None and self.ema_swapped:
            raise RuntimeError("FlatAdamW.step() while the EMA weights are swapped in: it would train the averages "
                               "(leave ema_weights() / call swap_ema() first)")
        if self.lr_state is not None:
            has_ema, clips, sc = self.ema is not None, self.clip_state is not None, self.lr_schedule
            L.call("a3d_adamw_sched_step", f.flat.data_ptr(), f.grad.data_ptr(), self.exp_avg.data_ptr(),
                   self.exp_avg_sq.data_ptr(), self.ema.data_ptr() if has_ema else None, self.step_count.data_ptr(),
                   self.seg_off.data_ptr(), self.seg_state.data_ptr(), self.ema_state.data_ptr() if has_ema else None,
                   self.clip_state.data_ptr() if clips else None, self.clip_ws.data_ptr() if clips else None,
                   self.lr_state.data_ptr(), len(f.order), f.n, f.n_nodecay, L.LR_DECAY_KINDS[sc["decay"]], float(sc["warmup"]),
                   float(sc["total"] or 0), sc["min_ratio"], self.betas[0], self.betas[1], self.eps, 0.0,
                   float(self.weight_decay), float(grad_scale), self.ema_decay if has_ema else 0.0,
                   self.ema_warmup if has_ema else 0.0, self.max_grad_norm if clips else 0.0, L.stream())
            return
        if self.clip_state is not None:
            has_ema = self.ema is not None
            L.call("a3d_adamw_clip_step", f.flat.data_ptr(), f.grad.data_ptr(), self.exp_avg.data_ptr(),
                   self.exp_avg_sq.data_ptr(), self.ema.data_ptr() if has_ema else None, self.step_count.data_ptr(),
                   self.seg_off.data_ptr(), self.seg_state.data_ptr(), self.ema_state.data_ptr() if has_ema else None,
                   self.clip_state.data_ptr(), self.clip_ws.data_ptr(), len(f.order), f.n, f.n_nodecay, float(self.lr),
                   self.betas[0], self.betas[1], self.eps, 0.0, float(self.weight_decay), float(grad_scale),
                   self.ema_decay if has_ema else 0.0, self.ema_warmup if has_ema else 0.0, self.max_grad_norm, L.stream())
            return
        if self.ema is not None:
            L.call("a3d_adamw_ema_step", f.flat.data_ptr(), f.grad.data_ptr(), self.exp_avg.data_ptr(),
                   self.exp_avg_sq.data_ptr(), self.ema.data_ptr(), self.step_count.data_ptr(), self.seg_off.data_ptr(),
                   self.seg_state.data_ptr(), self.ema_state.data_ptr(), len(f.order), f.n, f.n_nodecay, float(self.lr),
                   self.betas[0], self.betas[1], self.eps, 0.0, float(self.weight_decay), float(grad_scale),
                   self.ema_decay, self.ema_warmup, L.stream())
            return
        L.call("a3d_adamw_step", f.flat.data_ptr(), f.grad.data_ptr(), self.exp_avg.data_ptr(),
               self.exp_avg_sq.data_ptr(), self.step_count.data_ptr(), self.seg_off.data_ptr(), self.seg_state.data_ptr(),
               len(f.order), f.n, f.n_nodecay, float(self.lr),
               self.betas[0], self.betas[1], self.eps, 0.0, float(self.weight_decay), float(grad_scale), L.stream())

    @property
    def param_steps(self):
        """Per-parameter step counts (buffer order): torch.optim.AdamW's state[p]["step"]; 0 = never had a gradient."""
        return self.seg_state[:, 0]

    def reset_state(self):
        """Fresh-optimizer state: zero moments and step counts (parameters re-join with their first gradient)."""
        self.exp_avg.zero_(); self.exp_avg_sq.zero_(); self.step_count.zero_(); self.seg_state.zero_()
        if self.ema is not None:
            self.reset_ema()
        if self.clip_state is not None:
            self.clip_state.zero_()
        if self.lr_state is not None:
            self.lr_state[:3].zero_()            # the schedule starts over; the base rate stays

    # ---- learning-rate schedule (lr_schedule is not None): views of the device state, none of them synchronises
    def _lr_slot(self, what, k):
        if self.lr_state is None:
            raise RuntimeError("%s: this optimizer has no learning-rate schedule (built with lr_schedule=None)" % what)
        return self.lr_state[k]

    @property
    def current_lr(self):
        """The rate the last applied step ran at: fp32(lr * lr_factor) (lr_state[0])."""
        return self._lr_slot("current_lr", 0)

    @property
    def lr_factor(self):
        """The schedule's factor f(t) of the last applied step (lr_state[2])."""
        return self._lr_slot("lr_factor", 2)

    @property
    def schedule_step(self):
        """Scheduled steps applied so far = the position t the next step runs at (lr_state[1]); skipped steps do not count."""
        return self._lr_slot("schedule_step", 1)

    @schedule_step.setter
    def schedule_step(self, value):
        self._lr_slot("schedule_step", 1).fill_(float(value))

    # ---- gradient-norm clipping (max_grad_norm is not None): views of the device state, none of them synchronises
    def _clip_slot(self, what, k):
        if self.clip_state is None:
            raise RuntimeError("%s: this optimizer does not clip (built with max_grad_norm=None)" % what)
        return self.clip_state[k]

    @property
    def grad_norm(self):
        """Global L2 norm of the last step's gradient, grad_scale included, before clipping (clip_state[1])."""
        return self._clip_slot("grad_norm", 1)

    @property
    def clip_scale(self):
        """The factor the last step multiplied every gradient element by: grad_scale * min(1, max_grad_norm / (norm + 1e-6)),
        0 on a skipped step (clip_state[0]) -- what a3d_adamw_step / a3d_adamw_ema_step would take as grad_scale."""
        return self._clip_slot("clip_scale", 0)

    @property
    def clipped_steps(self):
        """Steps whose norm exceeded max_grad_norm so far (clip_state[3])."""
        return self._clip_slot("clipped_steps", 3)

    @property
    def skipped_steps(self):
        """Steps skipped for a non-finite gradient norm so far (clip_state[4])."""
        return self._clip_slot("skipped_steps", 4)

    @property
    def last_step_skipped(self):
        """1.0 if the last step was skipped, else 0.0 (clip_state[5])."""
        return self._clip_slot("last_step_skipped", 5)

    # ---- EMA of the weights (ema_decay is not None)
    def _need_ema(self, what):
        if self.ema is None:
            raise RuntimeError("%s: this optimizer keeps no EMA (built with ema_decay=None)" % what)

    @property
    def ema_updates(self):
        """EMA updates so far: a view of the device counter the kernel advances (ema_state[1])."""
        self._need_ema("ema_updates")
        return self.ema_state[1]

    def reset_ema(self):
        """Restart the average from the current weights; the warm-up starts over."""
        self._need_ema("reset_ema")
        if self.ema_swapped:
            raise RuntimeError("reset_ema() while the EMA weights are swapped in")
        self.ema.copy_(self.flat.flat.detach())
        self.ema_state.zero_()

    def swap_ema(self):
        """Exchange weights and averages in place (stream-ordered, one pass); call again to swap back."""
        self._need_ema("swap_ema")
        L.call("a3d_swap_f32", self.flat.flat.data_ptr(), self.ema.data_ptr(), self.flat.n, L.stream())
        self.ema_swapped = not self.ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """`with optimizer.ema_weights():` the model computes with the averaged weights; without an EMA a no-op."""
        if self.ema is None:
            yield
            return
        self.swap_ema()
        try:
            yield
        finally:
            self.swap_ema()

    def ema_state_dict(self):
        """{parameter name: averaged values} for the parameters of the flat buffer (detached clones, parameter shapes),
        wherever the averages currently live (`ema`, or flat.flat while swapped in)."""
        self._need_ema("ema_state_dict")
        src = self.flat.flat if self.ema_swapped else self.ema
        return {n: src[slice(*self.flat.slices[n])].detach().clone().view(p.shape) for n, p in self.flat.order}

    def state_dict(self):
        """torch.optim.AdamW's state_dict layout for the reference's optimizer (engine.py:89-102: two groups over ALL named
        parameters, int-indexed state with per-parameter `step`), so that the reference's `optimizer.load_state_dict`
        (engine.py:199) accepts a checkpoint written here and vice versa.  Parameters outside the flat buffer (frozen
        backbone, never-used FPN blocks) have no state, exactly like parameters whose .grad stayed None in torch."""
        f = self.flat
        state = {}
        steps = self.param_steps.detach().cpu()
        for (n, p), st in zip(f.order, steps):
            if float(st) <= 0:
                continue               # never received a gradient: torch writes no state for it
            a, b = f.slices[n]
            state[f.torch_index[n]] = {"step": st.clone().reshape(()), "exp_avg": self.exp_avg[a:b].detach().clone().view(p.shape),
                                       "exp_avg_sq": self.exp_avg_sq[a:b].detach().clone().view(p.shape)}
        groups, off = [], 0
        for names, wd in zip(f.torch_groups, (0.0, self.weight_decay)):
            groups.append({"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": wd,
                           "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                           "differentiable": False, "fused": None, "decoupled_weight_decay": True,
                           "params": list(range(off, off + len(names)))})
            off += len(names)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        """Accepts the torch.optim.AdamW layout (a reference checkpoint's "optimizer" entry).  Raises on a layout that does
        not describe this model's parameters (unknown indices, size mismatches, different group sizes).  Parameters WITHOUT
        an entry are legal: torch.optim.AdamW writes no state for parameters whose .grad stayed None (the FPN blocks of maps
        a configuration never reads, find_unused_parameters=True in engine.py:121-124); their moments and step count stay
        zero and, as in torch, they start at step 1 with the first gradient they receive.  Per-parameter step counts are
        kept as stored (they may differ between parameters)."""
        f = self.flat
        if not isinstance(sd, dict) or "state" not in sd or "param_groups" not in sd:
            raise ValueError("optimizer state: expected torch.optim.AdamW's {'state', 'param_groups'} layout")
        sizes = [len(g["params"]) for g in sd["param_groups"]]
        if sizes != [len(g) for g in f.torch_groups]:
            raise ValueError("optimizer state: parameter groups of sizes %s do not match this model's %s "
                             "(reference grouping, engine.py:89-102)" % (sizes, [len(g) for g in f.torch_groups]))
        by_index = {i: n for n, i in f.torch_index.items()}
        seg_of = {n: i for i, (n, _) in enumerate(f.order)}
        steps = torch.zeros(len(f.order), dtype=torch.float32)
        loaded = []
        for idx, st in sd["state"].items():
            n = by_index.get(int(idx))
            if n is None:
                raise ValueError("optimizer state: index %r is not a parameter of this model" % (idx,))
            if n not in f.slices:
                continue                       # state of a parameter that is not trained here (no gradient path)
            a, b = f.slices[n]
            if st["exp_avg"].numel() != b - a:
                raise ValueError("optimizer state of %s has %d elements, the parameter %d" % (n, st["exp_avg"].numel(), b - a))
            loaded.append((a, b, st))
            steps[seg_of[n]] = float(st["step"])
        self.reset_state()
        for a, b, st in loaded:
            self.exp_avg[a:b].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[a:b].copy_(st["exp_avg_sq"].reshape(-1))
        self.seg_state[:, 0].copy_(steps)
        self.step_count.fill_(float(steps.max()) if len(loaded) else 0.0)
        if self.lr_state is not None:            # the schedule continues where the loaded run stood: no persisted state of its own
            self.schedule_step = float(steps.max()) if len(loaded) else 0.0
        self.lr = sd["param_groups"][0].get("lr", self.lr)


def get_optimizer(model, lr=1e-4, active_names=None, ema_decay=None, ema_warmup=10, max_grad_norm=None, lr_schedule=None):
    """engine.py:89-102 on the flat buffers.  Returns (FlatParams, FlatAdamW).  With active_names=None every trainable
    parameter is placed in the buffer; parameters that never receive a gradient are left untouched by the fused AdamW kernel
    (as torch.optim.AdamW skips parameters whose .grad is None -- no weight decay on unused FPN blocks).  ema_decay / ema_warmup:
    FlatAdamW's EMA of the weights (off by default).  max_grad_norm: FlatAdamW's global gradient-norm clipping + non-finite step
    skip (off by default).  lr_schedule: FlatAdamW's device-resident warm-up + decay of the rate (off by default)."""
    _check_ema(ema_decay, ema_warmup)                # before the parameters are re-homed
    _check_max_grad_norm(max_grad_norm)
    _check_lr_schedule(lr_schedule)
    flat = FlatParams(model, active_names)
    return flat, FlatAdamW(flat, lr=lr, ema_decay=ema_decay, ema_warmup=ema_warmup, max_grad_norm=max_grad_norm,
                           lr_schedule=lr_schedule)


DP_ONESHOT = os.environ.get("A3D_DP_ONESHOT", "0") == "1"


class FlatDataParallel:
    """Data parallelism over one flat gradient buffer (replaces DistributedDataParallel, engine.py:121-124).

    broadcast_parameters(): rank 0 -> all (DDP's initial broadcast).
    sync_gradients(): all-reduce(SUM); the 1/world_size averaging is returned as the grad_scale for FlatAdamW.step.
    With `overlap=True` the hot-path segments [hot no-decay] and [hot decay] of the buffer are reduced on a side stream as
    soon as `hot_path_done()` is called -- by the split backward of `fwd_bwd_keypose` / `fwd_bwd_trajectory`, the moment
    the gradients of the FPN's output tokens exist and before the FPN / convolution backward is enqueued -- while that
    backward runs on the main stream; the FPN segment follows in sync_gradients().  `arm(False)` disables the early
    reduction for the non-final micro-batches of a gradient-accumulation window.
    Works with backend "nccl" (= RCCL on ROCm) and with "gloo" (device or CPU buffers; tests)."""

    def __init__(self, flat, process_group=None, overlap=True, model=None):
        self.flat = flat
        self.model = model
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # A3D_DP_ONESHOT=1: ONE all-reduce of the whole flat buffer after the backward instead of the three overlapped messages
        # (hot no-decay | hot decay early on the side stream, FPN segment late) -- the A/B switch for the first multi-GPU run
        self.overlap = overlap and flat.flat.is_cuda and not DP_ONESHOT
        self._pending = []
        self._side = torch.cuda.Stream() if self.overlap else None
        self._early_done = False
        self._begun = False
        self._armed = True

    def broadcast_parameters(self, src=0):
        """rank `src`'s state to every rank, as DistributedDataParallel does at construction: the flat (trainable) buffer
        and, when the model was given, every other state_dict entry -- the frozen backbone's weights and its BatchNorm
        statistics.  (Per-rank generator states -- ghost sampler, dropout -- are non-persistent buffers and stay per rank.)"""
        if self.world == 1:
            return
        dist.broadcast(self.flat.flat, src=src, group=self.pg)
        if self.model is not None:
            flat_ptrs = {p.data_ptr() for _, p in self.flat.order}
            for name, t in self.model.state_dict().items():
                if t.data_ptr() in flat_ptrs:
                    continue
                if t.is_contiguous():
                    dist.broadcast(t, src=src, group=self.pg)
                else:                                   # channels-last convolution weights of the bf16 backbone
                    c = t.contiguous()
                    dist.broadcast(c, src=src, group=self.pg)
                    t.copy_(c)

    def _segments(self):
        a, b = self.flat.late_range
        return [(0, a), (b, self.flat.n)], (a, b)

    def arm(self, on=True):
        self._armed = bool(on)

    def hot_path_done(self):
        """Call when every hot-path gradient has been produced (FPN backward not yet enqueued)."""
        if self.world == 1 or not self.overlap or not self._armed or self._early_done:
            return
        hot, _ = self._segments()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._side.wait_event(ev)
        with torch.cuda.stream(self._side):
            for a, b in hot:
                if b > a:
                    self._pending.append(dist.all_reduce(self.flat.grad[a:b], op=dist.ReduceOp.SUM, group=self.pg,
                                                         async_op=True))
        self._early_done = True

    def begin_sync(self):
        """Enqueue the all-reduce of everything that has not been reduced yet WITHOUT waiting for it: on the side stream
        (device buffers with overlap) so that whatever the caller runs next on the main stream -- the other model's step of a
        joint iteration (JointStep) -- hides it.  finish_sync() joins.  Without a side stream this is the plain blocking
        all-reduce."""
        if self.world == 1 or self._begun:
            return
        hot, late = self._segments()
        todo = [late] if self._early_done else [(0, self.flat.n)]
        if self._side is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self._side.wait_event(ev)
            with torch.cuda.stream(self._side):
                for a, b in todo:
                    if b > a:
                        self._pending.append(dist.all_reduce(self.flat.grad[a:b], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
        else:
            for a, b in todo:
                if b > a:
                    dist.all_reduce(self.flat.grad[a:b], op=dist.ReduceOp.SUM, group=self.pg)
        self._begun = True

    def finish_sync(self):
        """Join the reductions started by hot_path_done() / begin_sync().  Returns the grad_scale (1 / world)."""
        if self.world == 1:
            return 1.0
        for w in self._pending:
            w.wait()
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)
        self._pending, self._early_done, self._begun = [], False, False
        return 1.0 / self.world

    def sync_gradients(self):
        """Returns the grad_scale (1/world) to pass to the optimizer."""
        if self.world == 1:
            return 1.0
        self.begin_sync()
        return self.finish_sync()


# ------------------------------------------------------------------------------------------------ the step, split at the tokens
def _split_backward(tokens, run_hot, on_hot_done):
    """Backward in two stages around the FPN's output tokens: the hot path runs on detached leaves, its backward fills
    every hot-path parameter gradient and the token gradients; `on_hot_done()` (the early all-reduce) is called; then the
    token gradients are pushed through the FPN (MIOpen convolution backward).  Same gradients as one backward() call."""
    from . import ops
    from .ops import TokenMap
    uniq, leaves = {}, []
    for t in tokens:
        tm = TokenMap.of(t)                  # tokens + the FPN output bias owed to gathered rows (Act3D.compute_visual_tokens)
        if id(tm.tokens) not in uniq:
            uniq[id(tm.tokens)] = (tm.tokens, tm.leaf())
        leaf = uniq[id(tm.tokens)][1]
        leaves.append(leaf if isinstance(t, TokenMap) else leaf.tokens)      # plain tensors in, plain leaves out
    loss = run_hot(leaves)
    loss.backward()
    ops.flush_reduce_queue()                 # the hot path's deferred gradient reductions (its end-of-backward callback ran them;
                                             # this is the boundary the early all-reduce relies on)
    if on_hot_done is not None:
        on_hot_done()
    pairs = [(t, l.tokens.grad) for t, l in uniq.values() if t.requires_grad and l.tokens.grad is not None]
    if pairs:
        torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
    return loss.detach()


def fwd_bwd_keypose(model, criterion, sample, use_gt_sampling=True, on_hot_done=None):
    """forward + loss + backward of main_keypose.py:207-224 with the backward split at the FPN tokens"""
    maps = sample.get("backbone_maps")               # prefetched by the previous step (GraphedStep(prefetch=...)); else computed here
    tokens = model.compute_visual_tokens(sample["rgbs"]) if maps is None else model.compute_visual_tokens(sample["rgbs"], maps=maps)

    def hot(leaves):
        out = model(sample["rgbs"], sample["pcds"], sample["instr"], sample["curr_gripper"],
                    gt_action=sample["action"] if use_gt_sampling else None, visual_features=leaves)
        return sum(criterion.compute_loss(out, sample).values())

    return _split_backward(tokens, hot, on_hot_done)


def fwd_bwd_trajectory(model, criterion, sample, on_hot_done=None):
    """forward + loss + backward of main_trajectory.py:177-195 with the backward split at the FPN tokens"""
    maps = sample.get("backbone_maps")               # prefetched by the previous step (GraphedStep(prefetch=...)); else computed here
    head = model.prediction_head
    tokens = head.encode_images(sample["rgbs"], None) if maps is None else head.encode_images(sample["rgbs"], None, maps=maps)
    multi = isinstance(tokens, (list, tuple))                  # one token tensor per scale for a multi-scale head

    # additive test hooks: a batch may carry the DDPM noise / timesteps to use instead of the device draws
    kw = {k: sample[k] for k in ("noise", "timesteps") if k in sample}

    def hot(leaves):
        return criterion.compute_loss(model(sample["trajectory"], sample["trajectory_mask"], sample["rgbs"], sample["pcds"],
                                            sample["instr"], sample["curr_gripper"], sample["action"],
                                            visual_tokens=list(leaves) if multi else leaves[0], **kw))

    return _split_backward(list(tokens) if multi else [tokens], hot, on_hot_done)


class EagerStep:
    """The training-step protocol, written once: launch() is everything up to the point where the gradient reductions must have
    finished -- zero_grad at the start of an accumulation window, arm the early reduction (only the window's final micro-batch may
    start reducing its gradients early), `fwd_bwd(sample, on_hot_done)` with the backward split at the FPN tokens, and on the final
    micro-batch begin_sync() (started, not awaited); finish() joins the reductions and takes the optimizer step with 1/world.
    Whatever the caller enqueues between the two -- the other model's launch() in a JointStep -- hides the reductions.
    GraphedStep is the same pair on captured graphs."""

    def __init__(self, fwd_bwd, optimizer, ddp=None, accumulate=1):
        self.fwd_bwd, self.optimizer, self.ddp, self.accumulate = fwd_bwd, optimizer, ddp, max(1, int(accumulate))
        self.loss, self._last = None, True

    def launch(self, sample, step_id=0):
        if step_id % self.accumulate == 0:
            self.optimizer.zero_grad()
        self._last = step_id % self.accumulate == self.accumulate - 1
        if self.ddp is not None:
            self.ddp.arm(self._last)
        self.loss = self.fwd_bwd(sample, None if self.ddp is None else self.ddp.hot_path_done)
        if self.ddp is not None and self._last:
            self.ddp.begin_sync()

    def finish(self):
        if self._last:
            scale = self.ddp.finish_sync() if self.ddp is not None else 1.0
            self.optimizer.step(grad_scale=scale) if isinstance(self.optimizer, FlatAdamW) else self.optimizer.step()
        return self.loss

    def __call__(self, sample, step_id=0):
        self.launch(sample, step_id)
        return self.finish()


def train_one_step(model, criterion, optimizer, step_id, sample, ddp=None, accumulate_grad_batches=1,
                   use_ground_truth_position_for_sampling_train=True):
    """TrainTester.train_one_step for the keypose model (main_keypose.py:207-234): zero_grad, forward, loss, backward,
    (all-reduce, overlapped with the FPN backward), optimizer step.  Returns the detached total loss."""
    return EagerStep(lambda s, cb: fwd_bwd_keypose(model, criterion, s, use_ground_truth_position_for_sampling_train, cb),
                     optimizer, ddp, accumulate_grad_batches)(sample, step_id)


def train_one_step_trajectory(model, criterion, optimizer, step_id, sample, ddp=None, accumulate_grad_batches=1):
    """TrainTester.train_one_step for the trajectory model (main_trajectory.py:177-204)."""
    return EagerStep(lambda s, cb: fwd_bwd_trajectory(model, criterion, s, cb), optimizer, ddp, accumulate_grad_batches)(sample, step_id)


class JointStep:
    """One joint iteration of BASELINE.json configs[3]: an Act3D keypose training step AND a trajectory-diffusion training
    step -- two models, two optimizers, as the reference trains them (main_keypose.py:207-234, main_trajectory.py:177-204),
    each data-parallel over the same ranks (engine.py:121-124).  `kp_step` / `tr_step` are any two launch() / finish() pairs:
    EagerStep (JointStep.eager) or GraphedStep.

    Order of one iteration:  keypose launch (forward + backward, hot segments reduced early, begin_sync() of its FPN segment on
    the side stream) -> trajectory launch ON THE MAIN STREAM, which hides the keypose reductions -> both finish (join, AdamW).
    The result is the same as running the two train_one_step functions one after the other (tests/test_joint_gpu.py)."""

    def __init__(self, kp_step, tr_step):
        self.kp, self.tr = kp_step, tr_step

    @classmethod
    def eager(cls, kp_model, kp_criterion, kp_optimizer, tr_model, tr_criterion, tr_optimizer, kp_ddp=None, tr_ddp=None,
              use_ground_truth_position_for_sampling_train=True):
        use_gt = use_ground_truth_position_for_sampling_train
        return cls(EagerStep(lambda s, cb: fwd_bwd_keypose(kp_model, kp_criterion, s, use_gt, cb), kp_optimizer, kp_ddp),
                   EagerStep(lambda s, cb: fwd_bwd_trajectory(tr_model, tr_criterion, s, cb), tr_optimizer, tr_ddp))

    def __call__(self, kp_sample=None, tr_sample=None):
        self.kp.launch(kp_sample)
        self.tr.launch(tr_sample)
        return self.kp.finish(), self.tr.finish()


GraphedJointStep = JointStep          # JointStep over two GraphedSteps: the same four lines


def save_checkpoint(path, model, optimizer, step_id, best_loss=None):
    """engine.py:214-230 format: {"weight" (DDP's "module." prefix), "optimizer" (torch.optim.AdamW layout), "iter",
    "best_loss"} -- loadable by the reference's load_checkpoint (engine.py:195-212).  An optimizer that keeps an EMA adds a
    fifth key the reference's loader never reads: "ema": {"weight" (same prefix, the flat buffer's parameters), "decay",
    "warmup", "updates"}."""
    ema = getattr(optimizer, "ema", None)
    if ema is not None and optimizer.ema_swapped:
        raise RuntimeError("save_checkpoint while the EMA weights are swapped in: \"weight\" would hold the averages")
    weight = {"module." + k: v.detach().clone() for k, v in model.state_dict().items()}
    d = {"weight": weight, "optimizer": optimizer.state_dict(), "iter": step_id + 1, "best_loss": best_loss}
    if ema is not None:
        d["ema"] = {"weight": {"module." + k: v.cpu() for k, v in optimizer.ema_state_dict().items()},
                    "decay": optimizer.ema_decay, "warmup": optimizer.ema_warmup, "updates": int(optimizer.ema_updates.item())}
    torch.save(d, path)


def _ema_entries(path, d):
    if "ema" not in d:
        raise RuntimeError("checkpoint %s holds no \"ema\" entry (it was written without ema_decay)" % path)
    return {(k[7:] if k.startswith("module.") else k): v for k, v in d["ema"]["weight"].items()}


def load_checkpoint(path, model, optimizer=None, strict=True, weights="raw"):
    """engine.py:195-212 (+ online_evaluation/eval1.py:138-152 prefix stripping).  Returns (start_iter, best_loss).
    strict (the reference's load_state_dict default): missing / unexpected weight keys raise.  Parameters keep their
    storage (the flat buffer views): values are copied in place.
    weights="ema" (deployment / evaluation, no optimizer): the trained parameters are then overwritten with the checkpoint's
    averages.  An optimizer that keeps an EMA resumes it from the file's "ema" entry, or restarts it from the loaded weights when
    the file has none."""
    if weights not in ("raw", "ema"):
        raise ValueError("load_checkpoint: weights=%r (expected \"raw\" or \"ema\")" % (weights,))
    if weights == "ema" and optimizer is not None:
        raise ValueError("load_checkpoint: weights=\"ema\" with an optimizer -- a resumed run starts from the raw weights")
    d = torch.load(path, map_location="cpu", weights_only=False)
    weight = {(k[7:] if k.startswith("module.") else k): v for k, v in d["weight"].items()}
    res = model.load_state_dict(weight, strict=False)
    if strict and (res.missing_keys or res.unexpected_keys):
        raise RuntimeError("checkpoint %s does not match the model: missing %s, unexpected %s" %
                           (path, res.missing_keys[:5], res.unexpected_keys[:5]))
    if weights == "ema":
        params = dict(model.named_parameters())
        with torch.no_grad():
            for n, v in _ema_entries(path, d).items():
                if n not in params or params[n].numel() != v.numel():
                    raise RuntimeError("checkpoint %s: EMA entry %s does not match a parameter of the model" % (path, n))
                params[n].copy_(v.view(params[n].shape))
    if optimizer is not None:
        if "optimizer" not in d:
            raise RuntimeError("checkpoint %s holds no optimizer state" % path)
        optimizer.load_state_dict(d["optimizer"])
        if getattr(optimizer, "ema", None) is not None:
            if "ema" in d:
                entries, f = _ema_entries(path, d), optimizer.flat
                bad = [n for n in set(entries) | set(f.slices)
                       if n not in entries or n not in f.slices or entries[n].numel() != f.slices[n][1] - f.slices[n][0]]
                if bad:
                    raise RuntimeError("checkpoint %s: EMA entries do not match the optimizer's parameters: %s" % (path, sorted(bad)[:5]))
                for n, v in entries.items():
                    optimizer.ema[slice(*f.slices[n])].copy_(v.reshape(-1))
                optimizer.ema_state.zero_()
                optimizer.ema_state[1] = float(d["ema"]["updates"])
            else:
                optimizer.reset_ema()
                print("checkpoint %s holds no EMA: the average restarts from the loaded weights" % path)
    return d.get("iter", 0), d.get("best_loss", None)


# A/B switch (measured, round 6: both lose -- "main" 23.0 ms, default 18.9 ms per keypose step): "main" captures the prefetching step on
# a high-priority stream, "side" gives the prefetch stream the high priority instead
PREFETCH_HIPRIO = os.environ.get("A3D_PREFETCH_HIPRIO", "0")
# BatchNorm-apply workgroups of the prefetched backbone (a3d_bn_grid_cap; 0: leave the library default)
PREFETCH_BN_GRID = int(os.environ.get("A3D_PREFETCH_BN_GRID", "256"))
# A3D_PREFETCH_CHECK=1: every launch verifies that its images are the ones the previous launch announced (one host sync per step)
PREFETCH_CHECK = os.environ.get("A3D_PREFETCH_CHECK", "0") == "1"
# (forking the backbone after the FPN forward instead of at the start of the step measured the same, 18.86 vs 18.91 ms,
# profiles/r06_prefetch_ab.json: the knob was removed)


class GraphedStep:
    """Captures one full training step into hipGraphs and replays it.

    Every kernel of the hot path is enqueued on the caller's stream with static shapes and no host sync, the ghost
    sampler, the dropout generator and the AdamW step counter live on the device, so the step is capturable as is.
    Inputs are copied into static buffers before each replay.
      world == 1 : ONE graph  [zero_grad + forward + loss + backward + AdamW].
      world  > 1 : `step_fwd_bwd(inputs, on_hot_done)` must split its backward at the FPN tokens (fwd_bwd_keypose /
                   fwd_bwd_trajectory).  Three graphs around the two collectives:
                   [zero_grad + forward + hot-path backward] -> all-reduce(hot segments) on a side stream, concurrent with
                   [FPN backward] -> all-reduce(FPN segment) -> [AdamW with 1/world].
    The collectives themselves are issued eagerly between the replays (RCCL calls are not captured).

    prefetch (round 6; `model.backbone_maps`, a callable (rgbs, out=None) -> {name: map}): the FROZEN backbone of the NEXT batch runs
    on a side stream inside step k's graph, next to step k's FPN + hot path + backward + AdamW, which read the maps step k - 1
    left for them (`inputs["backbone_maps"]`, engine.fwd_bwd_keypose).  The backbone has no gradient and its weights never change,
    so the result of every step is the one of the sequential order (act3d.py:363-366 runs under no_grad in the reference too); what
    changes is that its ~9 ms of HBM-bound kernels fill the chip while the hot path's launch- and issue-bound kernels run.  Two map
    sets and two graph sets alternate (step k reads set k % 2 and writes set (k + 1) % 2).  Contract: launch(inputs, next_rgbs)
    -- `next_rgbs` are the images of the batch the NEXT launch will pass (None: the same static images again, a fixed synthetic
    batch); the first launch primes its own maps eagerly."""

    def __init__(self, step_fwd_bwd, optimizer, static_inputs, ddp=None, warmup=3, prefetch=None):
        self.static_inputs = static_inputs
        self.optimizer = optimizer
        self.ddp = ddp
        self.world = ddp.world if ddp is not None else 1
        self.prefetch = prefetch
        self.parity, self._primed, self._last = 0, False, 0
        split = self.world > 1
        # one calling convention from here on, (inputs, cb): a world == 1 step function takes the inputs alone
        self._step = step_fwd_bwd if split else (lambda inputs, cb: step_fwd_bwd(inputs))
        self._graph_kw = {}
        inputs = [dict(static_inputs)]
        if prefetch is not None:
            self.next_rgbs = static_inputs["rgbs"].clone()
            with torch.no_grad():
                m0 = prefetch(static_inputs["rgbs"])
            self.maps = [m0, {k: torch.empty_like(v) for k, v in m0.items()}]
            self._pf_stream = torch.cuda.Stream(priority=-1) if PREFETCH_HIPRIO == "side" else torch.cuda.Stream()
            if PREFETCH_HIPRIO in ("1", "main"):     # capture stream above the prefetch stream: the hot path's short kernels dispatch first
                self._graph_kw["stream"] = torch.cuda.Stream(priority=-1)
            inputs = [dict(static_inputs, backbone_maps=m) for m in self.maps]
        self._warm_up(inputs[0], warmup)
        self.g_fb, self.g_late, self.loss, self.g_opt = [], [], [], None
        pool = None                                  # shared by every graph of this step
        for p_, inp in enumerate(inputs):
            pool = (self._capture_split if split else self._capture_single)(p_, inp, pool)
        if split:
            self.g_opt = torch.cuda.CUDAGraph()
            with self._capturing(self.g_opt, pool):
                optimizer.step(grad_scale=1.0 / self.world)

    def _warm_up(self, inputs, steps):
        """`steps` eager steps on a side stream, so that every lazily created workspace / MIOpen plan exists before the capture"""
        eager = EagerStep(self._step, self.optimizer, self.ddp)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(steps):
                eager(inputs)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()

    def _capturing(self, graph, pool):
        return torch.cuda.graph(graph, pool=pool, **self._graph_kw)

    def _fork_prefetch(self, p_):
        """the next batch's backbone on the side stream (joined by _join_prefetch()); no-op without prefetch"""
        if self.prefetch is None:
            return
        self._pf_stream.wait_stream(torch.cuda.current_stream())
        # the overlapped backbone's BatchNorm-apply passes with one workgroup per CU: the hot path's kernels find free wave slots
        # (18.87 -> 18.45 ms per keypose step; grids are baked into the captured graph, so only this capture sees the setting)
        lib = L.load()
        prev = lib.a3d_bn_grid_cap(PREFETCH_BN_GRID) if PREFETCH_BN_GRID > 0 else 0
        try:
            with torch.cuda.stream(self._pf_stream), torch.no_grad():
                self.prefetch(self.next_rgbs, out=self.maps[1 - p_])
        finally:
            if PREFETCH_BN_GRID > 0:
                lib.a3d_bn_grid_cap(prev)

    def _join_prefetch(self):
        if self.prefetch is not None:
            torch.cuda.current_stream().wait_stream(self._pf_stream)

    def _capture_single(self, p_, inputs, pool):
        """world == 1: ONE graph [prefetch fork + zero_grad + forward + loss + backward + AdamW + prefetch join].  Returns the pool."""
        g = torch.cuda.CUDAGraph()
        self.g_fb.append(g)
        with self._capturing(g, pool):
            self._fork_prefetch(p_)
            self.optimizer.zero_grad()
            self.loss.append(self._step(inputs, None))
            self.optimizer.step(grad_scale=1.0)
            self._join_prefetch()
        return g.pool()

    def _capture_split(self, p_, inputs, pool):
        """world > 1: the capture of the first graph ends inside the step function's callback (hot path done, prefetch joined: the
        prefetched backbone overlaps the forward + hot-path backward), the second one starts there.  Returns the pool."""
        g, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        self.g_fb.append(g)
        self.g_late.append(g2)
        with contextlib.ExitStack() as capture:
            capture.enter_context(self._capturing(g, pool))
            # unwound before the first capture ends -- at the split point, or by a step function that raises before reaching it: no
            # capture is left open and the side stream is not left unjoined
            capture.callback(self._join_prefetch)

            def switch_graphs():
                capture.close()
                capture.enter_context(self._capturing(g2, g.pool() if pool is None else pool))

            self._fork_prefetch(p_)
            self.optimizer.zero_grad()
            self.loss.append(self._step(inputs, switch_graphs))
        return g.pool()

    def launch(self, inputs=None, next_rgbs=None):
        """Enqueue the step up to (not including) the point where the gradient reductions must have finished: input copies,
        forward + backward replay(s) and, under DP, the all-reduces (started, not awaited).  finish() completes the step.
        next_rgbs (prefetch only): the images of the batch the next launch will pass; None: the static images again."""
        if inputs is not None:
            for k, v in inputs.items():
                if torch.is_tensor(v) and k in self.static_inputs and v.data_ptr() != self.static_inputs[k].data_ptr():
                    self.static_inputs[k].copy_(v, non_blocking=True)
        p_ = 0
        if self.prefetch is not None:
            p_ = self.parity
            if self._primed and PREFETCH_CHECK and not torch.equal(self.static_inputs["rgbs"], self.next_rgbs):
                # (a host synchronisation per step: a debugging aid, off by default)
                raise RuntimeError("GraphedStep(prefetch): this launch's images are not the next_rgbs the previous launch was given -- "
                                   "the maps prefetched for it belong to another batch")
            if not self._primed:                 # the first launch computes its own maps (nobody prefetched them)
                with torch.no_grad():
                    self.prefetch(self.static_inputs["rgbs"], out=self.maps[p_])
                self._primed = True
            src = next_rgbs if next_rgbs is not None else self.static_inputs["rgbs"]
            if src.data_ptr() != self.next_rgbs.data_ptr():
                self.next_rgbs.copy_(src, non_blocking=True)
            self.parity ^= 1
        self._last = p_
        self.g_fb[p_].replay()
        if self.world > 1:
            self.ddp.arm(True)
            self.ddp.hot_path_done()           # hot segments on the side stream (whole buffer later if overlap is off) ...
            self.g_late[p_].replay()           # ... while the FPN backward runs
            self.ddp.begin_sync()

    def finish(self):
        if self.world > 1:
            self.ddp.finish_sync()
            self.g_opt.replay()
        return self.loss[self._last]

    def __call__(self, inputs=None, next_rgbs=None):
        self.launch(inputs, next_rgbs)
        return self.finish()
