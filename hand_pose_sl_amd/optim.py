"""`Adam`: the optimizer of the reference's training loop (`torch.optim.Adam(model.parameters(), lr=args.lr)`,
steps/traintest.py:48, stepped at :121) on libb2h's own kernel.

    optimizer = hand_pose_sl_amd.Adam(model.parameters(), lr=args.lr)
    ...
    optimizer.zero_grad(); loss.backward(); optimizer.step()

`step()` updates every parameter, exp_avg and exp_avg_sq with one b2h_adam_step call (kernel_adam.h: one launch per 80
tensors, each element read and written once) on the current stream of the parameters' device, where torch's default
Adam makes about nine elementwise passes.  The arithmetic is torch's `_single_tensor_adam` with amsgrad = False and
maximize = False (include/b2h.h lists it line by line); results agree with torch.optim.Adam to rounding, not bit for bit.

The step count is a one-element int64 tensor on the device that the kernel reads and a stream-ordered `add_(1)`
advances, and the learning rate a one-element float tensor, so `step()` can be captured into a graph together with the
forward, the loss and the backward, and every replay advances the bias correction.  Warm up before capturing: the
first `step()` allocates the state and the two words.  To change the learning rate between replays call
`set_lr(x)`, or edit `param_groups` and call `sync_hyper()`; an eager `step()` reads `param_groups[0]["lr"]` itself.
betas, eps and weight_decay are read at every eager `step()` and are constants of a captured one.

`state_dict()` / `load_state_dict()` have torch.optim.Adam's structure and keys (per parameter `step`, `exp_avg`,
`exp_avg_sq`), so the reference's `--resume` (`last_optim.pth`, traintest.py:56-73) works across a switch between the
two classes in either direction.  `state_dict()` synchronises to read the step word.

Between `loss.backward()` and the update, opt-in and on the device (b2h_step_prepare, kernel_step_control.h), so that a
captured step has them on every replay:

    optimizer = hand_pose_sl_amd.Adam(model.parameters(), lr=args.lr, max_grad_norm=1.0, skip_nonfinite=True,
                                      warmup_steps=1000, schedule="linear")

`max_grad_norm` is `torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)` in front of the update: the gradients are
scaled by `min(1, max_grad_norm / (norm + 1e-6))`, the norm taken over all of them in fp64 of exact products (it neither
overflows nor underflows, where torch's fp32 norm overflows near 1.8e19).  The scaling happens inside the update's
kernel: `p.grad` is left UNSCALED.  `skip_nonfinite` leaves parameters, moments and the step count alone when that norm
is inf or NaN, and counts the skip (`skipped_steps()`); without it a NaN gradient makes every weight NaN, as with torch.
`warmup_steps=W` multiplies the learning rate by `t / W` for the first W updates (t counts from 1) and then, with
`schedule="linear"`, leaves it alone, or with `"inv_sqrt"` decays it by `sqrt(W / t)`; `_lr_word`, `set_lr()` and
`param_groups` stay the BASE rate, `current_lr()` reads the rate of the last step.  `grad_norm` is the one-element device
tensor holding the norm of the last step before clipping (None until a step ran with clipping or the guard on).  The four
options are attributes of the optimizer, not state: they are in neither `defaults`, `param_groups` nor `state_dict()`
(the schedule needs no state beyond the step count), they may be changed between eager steps, and they are constants of
a captured one.

Not supported (use torch.optim.Adam): amsgrad, maximize, param groups with different hyper-parameters, parameters that
are not contiguous fp32 tensors on one GPU, sparse gradients.  There is no CPU path.
"""
import ctypes

import torch

from . import _lib

_FALLBACK = "; use torch.optim.Adam for this"


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 max_grad_norm=None, skip_nonfinite=False, warmup_steps=0, schedule="linear"):
        if amsgrad or maximize:
            raise ValueError("hand_pose_sl_amd.Adam has no amsgrad and no maximize" + _FALLBACK)
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, skip_nonfinite
        self.warmup_steps, self.schedule = warmup_steps, schedule
        self._control()
        # the keys of torch.optim.Adam's defaults, so that the param_groups of a state_dict interchange
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._check_groups()
        self._steps = 0          # updates made so far, as of the last host-side knowledge (the device word is the truth)
        self._step_word = None   # one-element int64 tensor on the parameters' device
        self._lr_word = None     # one-element float32 tensor there
        self._lr_seen = None     # the value last written to _lr_word
        self._ctl = None         # the words and the workspace of b2h_step_prepare, once a step needed them

    # ---- checks ----------------------------------------------------------------------------------------------------
    def _hyper(self):
        g = self.param_groups[0]
        return float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])

    def _check_groups(self):
        first = self._hyper()
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize") or g.get("decoupled_weight_decay") or g.get("differentiable"):
                raise ValueError("hand_pose_sl_amd.Adam has no amsgrad, maximize, decoupled weight decay or differentiable "
                                 "mode" + _FALLBACK)
            if (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"])) != first:
                raise ValueError("hand_pose_sl_amd.Adam takes one set of hyper-parameters for all param groups" + _FALLBACK)
            for p in g["params"]:
                if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                    raise ValueError("hand_pose_sl_amd.Adam updates contiguous fp32 parameters only" + _FALLBACK)
        lr, b1, b2, eps, wd = first
        if not (lr >= 0 and 0 <= b1 < 1 and 0 <= b2 < 1 and eps >= 0 and wd >= 0):
            raise ValueError(f"invalid Adam hyper-parameters lr={lr}, betas=({b1}, {b2}), eps={eps}, weight_decay={wd}")

    def _control(self):
        """(max_norm, guard, schedule, warmup) as b2h_step_prepare takes them, or None with every option off."""
        clip, warm, sched = self.max_grad_norm, self.warmup_steps, self.schedule
        if clip is not None and not float(clip) > 0:
            raise ValueError(f"max_grad_norm must be > 0, not {clip}: pass None for no clipping")
        if int(warm) != warm or warm < 0:
            raise ValueError(f"warmup_steps must be an integer >= 0, not {warm}: pass 0 for no warmup")
        if sched not in ("linear", "inv_sqrt"):
            raise ValueError(f"unknown schedule {sched!r}: \"linear\" (warm up, then the base rate) or \"inv_sqrt\" "
                             "(warm up, then decay by sqrt(warmup_steps / step))")
        if clip is None and not self.skip_nonfinite and not warm:
            return None
        return (0.0 if clip is None else float(clip), int(bool(self.skip_nonfinite)),
                _lib.SCHEDULES[sched] if warm else _lib.SCHEDULES["none"], int(warm))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if len(self.param_groups) > 1:
            self._check_groups()

    # ---- the two device words --------------------------------------------------------------------------------------
    def _words_on(self, dev):
        if self._step_word is None or self._step_word.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("hand_pose_sl_amd.Adam: take one eager step() (a warm-up) before capturing")
            self._step_word = torch.full((1,), self._steps, dtype=torch.int64, device=dev)
            self._lr_word = torch.empty(1, dtype=torch.float32, device=dev)
            self._lr_seen = None
        return self._step_word, self._lr_word

    def _control_on(self, dev, sizes, n):
        """The words b2h_step_prepare stores and its workspace, for these gradient sizes, on `dev`."""
        need = int(_lib.load().b2h_step_prepare_bytes(sizes, n))
        c = self._ctl
        if c is None or c["skipped"].device != dev or c["need"] < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("hand_pose_sl_amd.Adam: take one eager step() (a warm-up) with these options before "
                                   "capturing")
            f = dict(dtype=torch.float32, device=dev)
            self._ctl = c = dict(need=need, norm=torch.zeros(1, **f), scale=torch.ones(1, **f), lr=torch.zeros(1, **f),
                                 apply=torch.ones(1, dtype=torch.int64, device=dev),
                                 skipped=torch.zeros(1, dtype=torch.int64, device=dev) if c is None else c["skipped"].to(dev),
                                 workspace=torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev))
        return c

    def sync_hyper(self):
        """Mirror `param_groups[0]["lr"]` into the device word a captured step reads (a stream-ordered fill on the
        current stream; nothing happens when it has not changed).  Returns self."""
        self._check_groups()
        lr = self._hyper()[0]
        if self._lr_word is not None and lr != self._lr_seen:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("hand_pose_sl_amd.Adam: the learning rate changed since the last step; call sync_hyper() "
                                   "before capturing, not inside the capture")
            self._lr_word.fill_(lr)
            self._lr_seen = lr
        return self

    def set_lr(self, lr):
        """Set the learning rate of every param group and of the device word; returns self."""
        for g in self.param_groups:
            g["lr"] = lr
        return self.sync_hyper()

    # ---- step ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        control = self._control()        # the options are attributes: checked at every step, before any GPU work
        active = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not active:
            return loss
        dev = active[0].device
        if dev.type != "cuda":
            raise RuntimeError("hand_pose_sl_amd.Adam runs on an MI355X only (there is no CPU path)" + _FALLBACK)
        had_state = len(self.state)
        for p in active:
            g = p.grad
            if g.is_sparse:
                raise RuntimeError("hand_pose_sl_amd.Adam does not take sparse gradients" + _FALLBACK)
            if p.device != dev or g.device != dev or g.dtype != torch.float32 or not g.is_contiguous() or not p.is_contiguous():
                raise RuntimeError("hand_pose_sl_amd.Adam needs contiguous fp32 parameters and gradients on one GPU" + _FALLBACK)
            if len(self.state[p]) == 0:
                if had_state or self._steps:
                    raise RuntimeError("hand_pose_sl_amd.Adam: a parameter without a gradient at the first step got one "
                                       "later; the native optimizer holds one step count for all" + _FALLBACK)
                st = self.state[p]
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if len(active) != sum(1 for st in self.state.values() if len(st)):
            raise RuntimeError("hand_pose_sl_amd.Adam: a parameter that had a gradient at the first step has none now; the "
                               "native optimizer holds one step count for all" + _FALLBACK)
        self._check_groups()
        lib = _lib.load()
        n = len(active)
        vps, i64s = ctypes.c_void_p * n, ctypes.c_int64 * n
        states = [self.state[p] for p in active]
        with _lib.on_device(dev):
            step_word, lr_word = self._words_on(dev)
            self.sync_hyper()
            lr, b1, b2, eps, wd = self._hyper()
            st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            grads, sizes = vps(*[p.grad.data_ptr() for p in active]), i64s(*[p.numel() for p in active])
            tensors = (vps(*[p.data_ptr() for p in active]), grads, vps(*[s["exp_avg"].data_ptr() for s in states]),
                       vps(*[s["exp_avg_sq"].data_ptr() for s in states]), sizes, n)
            step_ptr = ctypes.c_void_p(step_word.data_ptr())
            if control is None:
                _lib.check(lib.b2h_adam_step(*tensors, lr, ctypes.c_void_p(lr_word.data_ptr()), b1, b2, eps, wd, 1, step_ptr, st))
                step_word.add_(1)
            else:
                max_norm, guard, schedule, warmup = control
                c = self._control_on(dev, sizes, n)
                ptr = {k: ctypes.c_void_p(c[k].data_ptr()) for k in ("norm", "scale", "apply", "skipped", "lr", "workspace")}
                _lib.check(lib.b2h_step_prepare(grads, sizes, n, max_norm, guard, lr, ctypes.c_void_p(lr_word.data_ptr()), schedule,
                                                max(warmup, 1), 1, step_ptr, ptr["norm"], ptr["scale"], ptr["apply"],
                                                ptr["skipped"], ptr["lr"], ptr["workspace"], 8 * c["workspace"].numel(), st))
                _lib.check(lib.b2h_adam_step_guarded(*tensors, lr, ptr["lr"], b1, b2, eps, wd, 1, step_ptr, ptr["scale"],
                                                     ptr["apply"], st))
                step_word.add_(c["apply"])       # a skipped update leaves the step count alone
        self._steps += 1
        # the kernel wrote through raw pointers: tell autograd and the models' packed-weights key (_native._packed_key)
        torch.autograd.graph.increment_version(active)
        return loss

    # ---- state_dict ------------------------------------------------------------------------------------------------
    def steps_done(self):
        """The number of updates made so far, read from the device word (synchronises)."""
        if self._step_word is not None:
            self._steps = int(self._step_word.item())
        return self._steps

    def skipped_steps(self):
        """The number of updates `skip_nonfinite` left out so far, read from the device word (synchronises)."""
        return 0 if self._ctl is None else int(self._ctl["skipped"].item())

    def current_lr(self):
        """The learning rate of the last step, warmup included, read from the device word (synchronises); the base rate
        before the first step and with every option off."""
        if self._ctl is None or self._control() is None or not self._steps:
            return self._hyper()[0]
        return float(self._ctl["lr"].item())

    @property
    def grad_norm(self):
        """The one-element device tensor that holds the gradients' 2-norm of the last step, before clipping; None with
        neither `max_grad_norm` nor `skip_nonfinite`, and before the first step."""
        if self._ctl is None or (self.max_grad_norm is None and not self.skip_nonfinite):
            return None
        return self._ctl["norm"]

    def state_dict(self):
        k = float(self.steps_done())
        for st in self.state.values():
            if len(st):
                st["step"] = torch.tensor(k, dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._check_groups()
        steps = set()
        for p, st in self.state.items():
            if not len(st):
                continue
            if "max_exp_avg_sq" in st:
                raise ValueError("hand_pose_sl_amd.Adam cannot continue an amsgrad state" + _FALLBACK)
            steps.add(int(float(st["step"])))
            st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
            for key in ("exp_avg", "exp_avg_sq"):
                st[key] = st[key].to(device=p.device, dtype=torch.float32).contiguous()
        if len(steps) > 1:
            raise ValueError("hand_pose_sl_amd.Adam holds one step count for all parameters; this state has "
                             f"{sorted(steps)}" + _FALLBACK)
        self._steps = steps.pop() if steps else 0
        if self._step_word is not None:
            self._step_word.fill_(self._steps)
        self._lr_seen = None
