"""nn.Module surface of the reference's PDE layers, running on libpdecnn_hip.so.

Every class keeps the reference's constructor signature (positional order), parameter
names / shapes / initial values (they are state_dict keys, optimizer-group selectors and
regulariser selectors — SURVEY.md §8b), plain attributes and helper methods, so a reference
``state_dict`` loads unchanged and the reference's training / plotting code can keep reaching
into ``model.diff.alpha_base`` etc.  ``forward`` returns a new tensor and never mutates its
input.  There is no CPU path: calling a layer on CPU tensors raises.

    reference class                               here
    mnist_test.DiffusionLayer                     MnistDiffusionLayer
    fashion_mnist.DiffusionLayer                  FashionDiffusionLayer
    SVHN.DiffusionLayer                           SvhnDiffusionLayer
    cifar10.EnhancedDiffusionLayer                EnhancedDiffusionLayer
    cifar_2version.LearnableDiffusionLayer        LearnableDiffusionLayer
    tiny_imagenet.ImprovedDiffusionLayer          ImprovedDiffusionLayer
    emotion_recognition.PDELayer                  PDELayer

``compat/<script>.py`` re-exports each one under the reference's own class name.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import functional as F_
from . import _lib as L

__all__ = ["MnistDiffusionLayer", "FashionDiffusionLayer", "SvhnDiffusionLayer", "EnhancedDiffusionLayer",
           "LearnableDiffusionLayer", "ImprovedDiffusionLayer", "PDELayer"]


def _plane(size):
    """(H, W) of a layer's ``size``: an int is the reference's square ``size x size``, a pair is a rectangle of H rows
    and W columns (the reference's sweeps are shape-generic, mnist_test.py:45,72,105; only its constructors fix the
    square)."""
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError(f"size must be an int or a pair (H, W), got {size!r}")
        return int(size[0]), int(size[1])
    return size, size


def _size_attr(size):
    """What ``layer.size`` keeps: the int as given, or the pair as a tuple."""
    return tuple(_plane(size)) if isinstance(size, (tuple, list)) else size


class _AdiBase(nn.Module):
    """Shared machinery of the implicit (Thomas) layers.  ``size`` is an int (a square, every kernel family) or a pair
    (H, W) with H != W (the any-size kernels behind pde_adi_rect_*, both sides in [2, 128])."""
    _split = "strang"
    _smooth3 = False
    _clamp_max = None

    def _schedule(self):
        """Per-step sweep lists; cached per (dt, dx, dy, steps) — the attributes may be changed from outside."""
        dy = getattr(self, "dy", self.dx)
        key = (self.dt, self.dx, dy, self.num_steps, self._split)
        cache = self.__dict__.setdefault("_schedule_cache", {})
        steps = cache.get(key)
        if steps is None:
            cache.clear()
            steps = cache[key] = F_.Schedule(F_.adi_schedule(self.dt, self.dx, dy, self.num_steps, self._split))
        return steps

    def get_alpha_beta_at_time(self, t):
        """clamp(base + slope*t) — mnist_test.py:33-42 / cifar10.py:53-63 (host-side helper)."""
        alpha_t = self.alpha_base + self.alpha_time_coeff * t
        beta_t = self.beta_base + self.beta_time_coeff * t
        if self._clamp_max is None:
            return torch.clamp(alpha_t, min=self.stability_eps), torch.clamp(beta_t, min=self.stability_eps)
        return (torch.clamp(alpha_t, min=self.stability_eps, max=self._clamp_max),
                torch.clamp(beta_t, min=self.stability_eps, max=self._clamp_max))

    #: How the backward's checkpoints are chosen (functional.plan_checkpoints).
    #: "auto" (default): from THIS call's coefficients.  Their per-sweep maxima leave the device right
    #: behind the forward's factorisation kernel (pinned copy + event recorded inside pde_adi_forward, before
    #: the sweep launch), so the backward's wait for them is over long before it is reached; exact after
    #: load_state_dict, a change of dt/dx/dy, or any optimiser step.
    #: "lagged": from the coefficients of the previous call in grad mode (never waits; half the error budget
    #: to cover one optimiser step of drift).  The cache is dropped by load_state_dict and by a change of
    #: dt/dx/dy/num_steps, but a LARGE in-place jump of the parameters between two calls is not seen: use it
    #: only in loops whose parameters move by optimiser steps.
    #: An int is an explicit bit mask.
    checkpoint_policy = "auto"

    def _load_from_state_dict(self, *args, **kwargs):
        self.__dict__.pop("_kmax_cache", None)              # a lagged plan made for the old parameters is void
        return super()._load_from_state_dict(*args, **kwargs)

    def _lagged_plan(self, key, u, args, kw, flat, plan):
        """(mask, cache, key): the plan from the previous call's coefficients; the first call (or the first after
        the cache was dropped) computes them synchronously."""
        dy = getattr(self, "dy", self.dx)
        key = key + (self.dt, self.dx, dy, self.num_steps, u.device)
        cache = self.__dict__.setdefault("_kmax_cache", {})
        old = cache.get(key)
        if old is None:
            for k in [k for k in cache if k[-5:] != key[-5:]]:      # plans made for another dt/dx/dy/num_steps/device
                del cache[k]
            km = F_.kappa_max_async(u, *args, flat, **kw)
            km.event.synchronize()
            old = (km, plan(km.host.tolist()))
        elif old[0].event.query():
            old = (old[0], plan(old[0].host.tolist()))
        return old, cache, key

    def _uses_operator(self):
        """Whether the layer runs a channel operator between its steps (then checkpoint masks are step-local)."""
        return False

    def _step_groups(self, steps):
        per = max(1, L.PDE_MAX_SWEEPS // len(steps[0]))
        return [steps[i:i + per] for i in range(0, len(steps), per)]

    def freeze_checkpoint_plan(self, example=None):
        """Pin the checkpoint plan to explicit masks made from the CURRENT parameters alone — one small kernel and one
        synchronous wait per group of steps, no forward pass of the layer (nothing else in the model runs, no BatchNorm
        statistics move, no random numbers are drawn); the conservative budget of the lagged policy.  A call with explicit
        masks issues launches only — no wait for the coefficient maxima, no host copy — which is what hipGraph capture needs
        (``graphs.py``).  The masks stay valid while the coefficients do not grow by more than the budget's margin (a factor
        2 in error amplification); call again after large parameter changes.  ``example`` is accepted for compatibility and
        ignored.  Returns the mask (an int) or, for schedules that run as several launch groups, one mask per group."""
        ab = self.alpha_base
        Cc = 1 if ab.dim() == 2 else ab.shape[0]
        like = torch.empty((1, Cc, ab.shape[-2], ab.shape[-1]), dtype=torch.float32, device=ab.device)
        args = (self.alpha_base, self.beta_base, self.alpha_time_coeff, self.beta_time_coeff)
        kw = dict(smooth3=self._smooth3, clamp_max=self._clamp_max, eps=self.stability_eps)
        masks = []
        with torch.no_grad():
            for grp in self._step_groups(self._schedule()):
                sps = len(grp[0])
                km = F_.kappa_max_async(like, *args, [s for st in grp for s in st], **kw)
                km.event.synchronize()
                v = km.host.tolist()
                if self._uses_operator():
                    bits = 0
                    for k in range(len(grp)):
                        bits |= F_.plan_checkpoints(v[k * sps:(k + 1) * sps], F_.CKPT_AMAX / 2)
                else:
                    bits = F_.plan_checkpoints(v, F_.CKPT_AMAX / 2)
                masks.append(int(bits))
        self.__dict__.pop("_kmax_cache", None)
        self.checkpoint_policy = masks[0] if len(masks) == 1 else tuple(masks)
        return self.checkpoint_policy

    def _policy_of_group(self, gi, num_sweeps=None):
        """The checkpoint policy of launch group ``gi``: a frozen plan is one mask per group; a single mask given for a
        schedule of several groups keeps the bits the group's own schedule has (a plain group of S sweeps: bits 0..S-2)."""
        ck = self.checkpoint_policy
        if isinstance(ck, (tuple, list)):
            ck = ck[gi]
        if isinstance(ck, int) and not isinstance(ck, bool) and num_sweeps is not None:
            ck &= (1 << max(num_sweeps - 1, 0)) - 1
        return ck

    def _diffuse(self, u, sweeps, gi=0):
        args = (self.alpha_base, self.beta_base, self.alpha_time_coeff, self.beta_time_coeff)
        kw = dict(smooth3=self._smooth3, clamp_max=self._clamp_max, eps=self.stability_eps)
        ck = self._policy_of_group(gi, len(sweeps))
        if not (torch.is_grad_enabled() and (u.requires_grad or any(p.requires_grad for p in args))):
            ck = 0
        if ck != "lagged":
            return F_.adi_diffuse(u, *args, sweeps, checkpoints=ck, **kw)
        old, cache, key = self._lagged_plan(("plain", len(sweeps), sweeps[0].t), u, args, kw, sweeps,
                                            lambda km: F_.plan_checkpoints(km, F_.CKPT_AMAX / 2))
        sink = []
        y = F_.adi_diffuse(u, *args, sweeps, checkpoints=old[1], kmax_sink=sink, **kw)
        cache[key] = (sink[0], old[1]) if sink else old
        return y

    def _run(self, u, steps, M=None, mode=None, skip_weight=None):
        """All steps of the layer.  One launch sequence holds at most PDE_MAX_SWEEPS sweeps: longer schedules
        (num_steps > 32 Strang steps) are cut into groups of whole steps, chained through autograd."""
        # a rectangle on either side must match exactly; a square input on a square layer of another size is left to the
        # calls below, which refuse it as they always have (existing behaviour, empty batches included, stays as it is)
        hw, phw = tuple(u.shape[-2:]), tuple(self.alpha_base.shape[-2:])
        if u.dim() == 4 and hw != phw and (hw[0] != hw[1] or phw[0] != phw[1]):
            raise L.PdeError(f"input plane {hw[0]}x{hw[1]} does not match the layer's {phw[0]}x{phw[1]} coefficients")
        # one route for the whole layer: its calls (sweeps, operator, skip blend) each see only some of the parameters
        u = F_.route_input(u, self.alpha_base, self.beta_base, self.alpha_time_coeff, self.beta_time_coeff, M, skip_weight)
        per = max(1, L.PDE_MAX_SWEEPS // len(steps[0]))
        if len(steps) <= per:
            if M is None:
                return self._diffuse(u, steps.flat if isinstance(steps, F_.Schedule) else [s for st in steps for s in st])
            return self._diffuse_mixed(u, steps, M, mode, skip_weight)
        u0 = u
        for gi, grp in enumerate(self._step_groups(steps)):
            u = (self._diffuse(u, [s for st in grp for s in st], gi) if M is None
                 else self._diffuse_mixed(u, grp, M, mode, gi=gi))
        return u if skip_weight is None else F_.skip_blend(u0, u, skip_weight)

    # ---- the trajectory: the states after chosen time steps --------------------------------------------------------
    #: layers whose forward takes (B,1,H,W) only (mnist, fashion)
    _single_channel = False

    def _operator(self):
        """(M, mode) of the channel operator between the steps, or (None, None)."""
        return None, None

    def _diffuse_states(self, u, sweeps, emit, gi=0):
        """``_diffuse`` returning the states after the sweeps in ``emit`` too (functional.adi_diffuse_states): the same
        checkpoint policies, one sweep launch per pass."""
        args = (self.alpha_base, self.beta_base, self.alpha_time_coeff, self.beta_time_coeff)
        kw = dict(smooth3=self._smooth3, clamp_max=self._clamp_max, eps=self.stability_eps)
        ck = self._policy_of_group(gi, len(sweeps))
        if not (torch.is_grad_enabled() and (u.requires_grad or any(p.requires_grad for p in args))):
            ck = 0
        if ck != "lagged":
            return F_.adi_diffuse_states(u, *args, sweeps, emit, checkpoints=ck, **kw)
        old, cache, key = self._lagged_plan(("plain", len(sweeps), sweeps[0].t), u, args, kw, sweeps,
                                            lambda km: F_.plan_checkpoints(km, F_.CKPT_AMAX / 2))
        sink = []
        y = F_.adi_diffuse_states(u, *args, sweeps, emit, checkpoints=old[1], kmax_sink=sink, **kw)
        cache[key] = (sink[0], old[1]) if sink else old
        return y

    def trajectory(self, u, steps=None):
        """The diffusion trajectory: a tensor (K', B, C, H, W) whose slice ``i`` is the state after time step
        ``steps[i]`` — what the reference's time loop holds at the end of that iteration: after the step's sweeps, for
        SVHN after the coupling that follows them, for a "pre" mixing layer what the next step's mixing would read; never
        the SVHN skip blend (``skip_weight`` is not used and gets no gradient).  It equals the output of the same layer
        built with ``num_steps=steps[i]``.

        ``steps``: None (every step) or a strictly increasing sequence of 1-based step numbers in 1..num_steps; the
        schedule is cut after ``max(steps)``.  Inputs are routed as in ``forward`` (fp32, bf16, ``model.half()``,
        float64; squares and rectangles; ``checkpoint_policy``; launch groups beyond 32 steps); with 16-bit tensors a
        returned state is the fp32 state rounded once while the time loop goes on unrounded, so ``trajectory(u)[-1]`` is
        bit for bit ``forward(u)`` of a layer without skip blend.  Differentiable in ``u``, the four coefficient
        tensors and the channel operator.

        A layer without a channel operator returns all states out of the launches ``forward`` makes (one sweep launch
        per pass and launch group).  So does a layer with an operator wherever ``forward`` runs on the one-launch C <= 4
        kernels (``small_channel_kernels`` and functional.adi_small_supported: C <= 4, N in {16, 28, 32}, Strang or Lie
        steps, fp32 / bf16 / fp16 tensors): functional.adi_diffuse_small_states, one launch per pass and launch group,
        every checkpoint policy as in ``forward``.  There, with 16-bit tensors, the time loop goes on from the rounded
        sweep output of every step, as the training forward of such a layer does, in grad mode and under ``no_grad``
        alike, so the two return the same tensor.  Every other layer with an operator (C > 4, other N, rectangles,
        float64, ``small_channel_kernels = False``) runs step by step (functional.adi_diffuse_mixed_per_step): the wide
        kernels do not emit states; "lagged" plans there as "auto"."""
        K = int(self.num_steps)
        sel = F_.check_steps(steps, K)
        if self._single_channel and (u.dim() != 4 or u.shape[1] != 1):
            raise ValueError("expected (B,1,%d,%d), got %s" % (*_plane(self.size), tuple(u.shape)))
        sched = self._schedule()
        if sel[-1] < K:                                        # the first k steps of a schedule are the schedule of k steps
            sched = F_.Schedule(sched[:sel[-1]])
        M, mode = self._operator()
        hw, phw = tuple(u.shape[-2:]), tuple(self.alpha_base.shape[-2:])
        if u.dim() == 4 and hw != phw and (hw[0] != hw[1] or phw[0] != phw[1]):
            raise L.PdeError(f"input plane {hw[0]}x{hw[1]} does not match the layer's {phw[0]}x{phw[1]} coefficients")
        u = F_.route_input(u, self.alpha_base, self.beta_base, self.alpha_time_coeff, self.beta_time_coeff, M)
        sps = len(sched[0])
        per = max(1, L.PDE_MAX_SWEEPS // sps)
        if M is not None:
            args = (self.alpha_base, self.beta_base, self.alpha_time_coeff, self.beta_time_coeff)
            kw = dict(smooth3=self._smooth3, clamp_max=self._clamp_max, eps=self.stability_eps)
            live = (M,) + args
            grad = torch.is_grad_enabled() and (u.requires_grad or any(p.requires_grad for p in live))
            groups = self._step_groups(sched)
            if self.small_channel_kernels and all(F_.adi_small_supported(u, grp, **kw) for grp in groups):
                pieces = []
                for gi, grp in enumerate(groups):
                    first = gi * per                           # steps first+1 .. first+len(grp) are this group's
                    mine = [k - first for k in sel if first < k <= first + len(grp)]
                    out = self._diffuse_small_states(u, grp, M, mode, [k - 1 for k in mine], gi, grad)
                    u = out[-1]
                    if len(groups) == 1 and len(mine) == out.shape[0]:
                        return out                             # one group, its last step wanted: the launch's own tensor
                    pieces.append(out if mine and mine[-1] == len(grp) else out[:-1])
                return torch.cat(pieces)
            states = []
            for gi, grp in enumerate(groups):
                ck = self._policy_of_group(gi) if grad else 0
                u = F_.adi_diffuse_mixed_per_step(u, *args, M, grp, mode, checkpoints="auto" if ck == "lagged" else ck,
                                                  states=states, **kw)
            return torch.stack([states[k - 1] for k in sel])
        pieces = []
        for gi, grp in enumerate(self._step_groups(sched)):
            first = gi * per                                   # steps first+1 .. first+len(grp) are this group's
            mine = [k - first for k in sel if first < k <= first + len(grp)]
            out = self._diffuse_states(u, [s for st in grp for s in st], [k * sps - 1 for k in mine], gi)
            u = out[-1]
            if len(grp) == len(sched) and len(mine) == out.shape[0]:
                return out                                     # one group, its last step wanted: the launch's own tensor
            pieces.append(out if mine and mine[-1] == len(grp) else out[:-1])
        return torch.cat(pieces)

    #: False forces the per-step launch path (pde_adi_mixed_*) where the single-launch C <= 4 kernels would apply
    small_channel_kernels = True

    def _diffuse_small_states(self, u, steps, M, mode, emit, gi, grad):
        """One launch group of ``trajectory`` on the one-launch C <= 4 kernels (functional.adi_diffuse_small_states): the
        states after the 0-based steps in ``emit`` and after the last one; checkpoints as in ``_diffuse_mixed``."""
        args = (self.alpha_base, self.beta_base, self.alpha_time_coeff, self.beta_time_coeff)
        kw = dict(smooth3=self._smooth3, clamp_max=self._clamp_max, eps=self.stability_eps)
        ck = self._policy_of_group(gi) if grad else 0
        if ck != "lagged":
            return F_.adi_diffuse_small_states(u, *args, M, steps, mode, emit, checkpoints=ck, **kw)
        sps = len(steps[0])

        def plan(km):
            bits = 0
            for k in range(len(steps)):
                bits |= F_.plan_checkpoints(km[k * sps:(k + 1) * sps], F_.CKPT_AMAX / 2)
            return bits
        old, cache, key = self._lagged_plan(("mixed", len(steps), sps, steps[0][0].t), u, args, kw,
                                            [s for st in steps for s in st], plan)
        sink = []
        y = F_.adi_diffuse_small_states(u, *args, M, steps, mode, emit, checkpoints=old[1], kmax_sink=sink, **kw)
        cache[key] = (sink[0], old[1]) if sink else old
        return y

    def _diffuse_mixed(self, u, steps, M, mode, skip_weight=None, gi=0):
        """All steps of a layer with a channel operator between them; checkpoints as in ``_diffuse`` (one step-local
        mask for every step).  C <= 4 (the reference's own models): the whole time loop — and for SVHN the skip
        blend — in one launch per pass (functional.adi_diffuse_small); otherwise one mixing and one sweep launch per
        step (functional.adi_diffuse_mixed) and the skip blend as its own pass."""
        args = (self.alpha_base, self.beta_base, self.alpha_time_coeff, self.beta_time_coeff)
        kw = dict(smooth3=self._smooth3, clamp_max=self._clamp_max, eps=self.stability_eps)
        small = self.small_channel_kernels and F_.adi_small_supported(u, steps, **kw)
        u_in = u

        def run(ck, sink=None):
            if small:
                return F_.adi_diffuse_small(u, *args, M, steps, mode, skip_weight, checkpoints=ck, kmax_sink=sink, **kw)
            y = F_.adi_diffuse_mixed(u, *args, M, steps, mode, checkpoints=ck, kmax_sink=sink, **kw)
            return y if skip_weight is None else F_.skip_blend(u_in, y, skip_weight)          # SVHN.py:73-74

        ck = self._policy_of_group(gi)
        live = (M, skip_weight) + args
        if not (torch.is_grad_enabled() and (u.requires_grad or any(p is not None and p.requires_grad for p in live))):
            ck = 0
        if ck != "lagged":
            return run(ck)
        sps = len(steps[0])

        def plan(km):
            bits = 0
            for k in range(len(steps)):
                bits |= F_.plan_checkpoints(km[k * sps:(k + 1) * sps], F_.CKPT_AMAX / 2)
            return bits
        old, cache, key = self._lagged_plan(("mixed", len(steps), sps, steps[0][0].t), u, args, kw,
                                            [s for st in steps for s in st], plan)
        sink = []
        y = run(old[1], sink)
        cache[key] = (sink[0], old[1]) if sink else old
        return y


class MnistDiffusionLayer(_AdiBase):
    """mnist_test.py:11-219.  (B,1,size,size) -> same — or (B,1,H,W) with ``size=(H, W)``; Strang split, smoothed
    coefficients."""
    _smooth3 = True
    _single_channel = True

    def __init__(self, size=28, dt=0.001, dx=1.0, dy=1.0, num_steps=10):
        super().__init__()
        self.size, self.dt, self.dx, self.dy, self.num_steps = _size_attr(size), dt, dx, dy, num_steps
        hw = _plane(size)
        self.alpha_base = nn.Parameter(torch.ones(*hw) * 2.0)
        self.beta_base = nn.Parameter(torch.ones(*hw) * 2.0)
        self.alpha_time_coeff = nn.Parameter(torch.zeros(*hw))
        self.beta_time_coeff = nn.Parameter(torch.zeros(*hw))
        self.stability_eps = 1e-6
        print(f"Initialized DiffusionLayer with dx={dx}, dy={dy}")

    def forward(self, u):
        if u.dim() != 4 or u.shape[1] != 1:
            raise ValueError("expected (B,1,%d,%d), got %s" % (*_plane(self.size), tuple(u.shape)))
        return self._run(u, self._schedule())

    def get_numerical_stability_info(self):
        """mnist_test.py:200-219."""
        with torch.no_grad():
            alpha_max = torch.max(self.alpha_base + torch.abs(self.alpha_time_coeff) * self.dt * self.num_steps)
            beta_max = torch.max(self.beta_base + torch.abs(self.beta_time_coeff) * self.dt * self.num_steps)
            cfl_x = alpha_max * self.dt / (self.dx ** 2)
            cfl_y = beta_max * self.dt / (self.dy ** 2)
            return {"cfl_x": cfl_x.item(), "cfl_y": cfl_y.item(), "dx": self.dx, "dy": self.dy, "dt": self.dt,
                    "stable_x": cfl_x.item() < 0.5, "stable_y": cfl_y.item() < 0.5}


class FashionDiffusionLayer(_AdiBase):
    """fashion_mnist.py:18-196: the mnist layer with dy == dx, dt=0.3, 4 steps, base 1.8."""
    _smooth3 = True
    _single_channel = True

    def __init__(self, size=28, dt=0.3, dx=1.0, num_steps=4):
        super().__init__()
        self.size, self.dt, self.dx, self.num_steps = _size_attr(size), dt, dx, num_steps
        hw = _plane(size)
        self.alpha_base = nn.Parameter(torch.ones(*hw) * 1.8)
        self.beta_base = nn.Parameter(torch.ones(*hw) * 1.8)
        self.alpha_time_coeff = nn.Parameter(torch.zeros(*hw))
        self.beta_time_coeff = nn.Parameter(torch.zeros(*hw))
        self.stability_eps = 1e-6

    def forward(self, u):
        if u.dim() != 4 or u.shape[1] != 1:
            raise ValueError("expected (B,1,%d,%d), got %s" % (*_plane(self.size), tuple(u.shape)))
        return self._run(u, self._schedule())


class SvhnDiffusionLayer(_AdiBase):
    """SVHN.py:12-230: per-channel smoothed Strang steps, channel coupling after every step
    (SVHN.py:71), learnable sigmoid skip blend with the input (SVHN.py:74)."""
    _smooth3 = True

    def __init__(self, size=32, channels=3, dt=0.01, dx=1.0, num_steps=10):
        super().__init__()
        self.size, self.channels, self.dt, self.dx, self.num_steps = _size_attr(size), channels, dt, dx, num_steps
        hw = _plane(size)
        self.alpha_base = nn.Parameter(torch.ones(channels, *hw) * 0.1)
        self.beta_base = nn.Parameter(torch.ones(channels, *hw) * 0.1)
        self.alpha_time_coeff = nn.Parameter(torch.randn(channels, *hw) * 0.001)
        self.beta_time_coeff = nn.Parameter(torch.randn(channels, *hw) * 0.001)
        self.channel_coupling = nn.Parameter(torch.eye(channels) * 0.01)
        self.stability_eps = 1e-6
        self.skip_weight = nn.Parameter(torch.tensor(0.9))

    def _uses_operator(self):
        return True

    def _operator(self):
        return self.channel_coupling, "post"

    def forward(self, u):
        # SVHN.py:55-76: sweeps, coupling after every step, then sigmoid(w) u0 + (1 - sigmoid(w)) u
        return self._run(u, self._schedule(), self.channel_coupling, "post", self.skip_weight)


class EnhancedDiffusionLayer(_AdiBase):
    """cifar10.py:24-211: coefficients clamped to [eps,10], no smoothing, channel mixing before
    every Strang step (cifar10.py:91).

    ``channel_mixing_enabled=False`` (keyword only, not in the reference) skips the C x C
    mixing product; the whole time loop then runs as ONE fused kernel launch.  It equals the
    reference layer with ``channel_mixing`` set to the identity."""
    _clamp_max = 10.0

    def __init__(self, size=32, channels=3, dt=0.001, dx=1.0, dy=1.0, num_steps=10, *, channel_mixing_enabled=True):
        super().__init__()
        self.size, self.channels, self.dt, self.dx, self.dy, self.num_steps = _size_attr(size), channels, dt, dx, dy, num_steps
        hw = _plane(size)
        self.alpha_base = nn.Parameter(torch.ones(channels, *hw) * 1.0)
        self.beta_base = nn.Parameter(torch.ones(channels, *hw) * 1.0)
        self.alpha_time_coeff = nn.Parameter(torch.zeros(channels, *hw) * 0.1)
        self.beta_time_coeff = nn.Parameter(torch.zeros(channels, *hw) * 0.1)
        self.channel_mixing = nn.Parameter(torch.eye(channels) + torch.randn(channels, channels) * 0.01)
        self.stability_eps = 1e-6
        self.channel_mixing_enabled = channel_mixing_enabled
        self._banner()

    def _banner(self):
        h, w = _plane(self.size)
        print(f"Alpha/Beta-Focused DiffusionLayer: {h}x{w}x{self.channels}")
        print(f"  Spatial: dx={self.dx}, dy={self.dy}")
        print(f"  Temporal: dt={self.dt}, steps={self.num_steps}")
        print(f"  Learnable parameters: α matrices ({self.channels}x{h}x{w}), "
              f"β matrices ({self.channels}x{h}x{w})")

    def _uses_operator(self):
        return bool(self.channel_mixing_enabled)

    def _operator(self):
        return (self.channel_mixing, "pre") if self.channel_mixing_enabled else (None, None)

    def forward(self, u):
        steps = self._schedule()
        if not self.channel_mixing_enabled:
            return self._run(u, steps)
        return self._run(u, steps, self.channel_mixing, "pre")


class LearnableDiffusionLayer(EnhancedDiffusionLayer):
    """cifar_2version.py:20-187: as EnhancedDiffusionLayer with the Lie split x(dt/2), y(dt/2)."""
    _split = "lie"

    def _banner(self):
        h, w = _plane(self.size)
        print(f"Learnable Diffusion Layer: {h}x{w}x{self.channels}")
        print(f"  Learnable α coefficients: {self.channels}x{h}x{w}")
        print(f"  Learnable β coefficients: {self.channels}x{h}x{w}")
        print(f"  Temporal: dt={self.dt}, steps={self.num_steps}")


class ImprovedDiffusionLayer(nn.Module):
    """tiny_imagenet.py:14-72 (the live part): per-channel scaled explicit 5-point step with a
    0.1 relaxation.  ``beta_base`` exists but is unused, as in the reference (its grad is None).
    The reference's training script reads ``model.diff.spatial_modulation`` (tiny_imagenet.py:614),
    an attribute its own class never defines; it is not defined here either."""

    def __init__(self, size=64, channels=3, dt=0.01, num_steps=1, use_implicit=False):
        super().__init__()
        self.size, self.channels, self.dt, self.num_steps, self.use_implicit = size, channels, dt, num_steps, use_implicit
        self.alpha_base = nn.Parameter(torch.ones(channels) * 0.05)
        self.beta_base = nn.Parameter(torch.ones(channels) * 0.05)
        self.channel_scaling = nn.Parameter(torch.ones(channels))
        self.stability_eps = 1e-6
        self.max_coeff = 0.15

    #: the relaxation of tiny_imagenet.py:49
    _relax = 0.1

    def forward(self, u):
        # all num_steps steps in one call (64x64 / 32x32 / 16x16 planes: one launch, the plane stays in registers)
        return F_.explicit5_step(u, self.alpha_base, self.channel_scaling, self.dt, self.stability_eps,
                                 self.max_coeff, self._relax, self.num_steps)


class PDELayer(nn.Module):
    """emotion_recognition.py:56-97: reflect-pad once, Nt explicit Jacobi updates with separable
    coefficients alpha(y) (rows) and beta(x) (columns) made from six scalars."""

    def __init__(self, Nx=48, Ny=48, Lx=1.0, Ly=1.0, T=0.01, dt=0.001):
        super().__init__()
        self.Nx, self.Ny, self.Lx, self.Ly = Nx, Ny, Lx, Ly
        self.T, self.dt = T, dt
        self.dx = Lx / Nx
        self.dy = Ly / Ny
        self.Nt = int(T / dt)
        self.alpha_w1 = nn.Parameter(torch.tensor(0.1))
        self.alpha_w2 = nn.Parameter(torch.tensor(0.1))
        self.alpha_w3 = nn.Parameter(torch.tensor(0.1))
        self.beta_w1 = nn.Parameter(torch.tensor(0.3))
        self.beta_w2 = nn.Parameter(torch.tensor(0.2))
        self.beta_w3 = nn.Parameter(torch.tensor(0.2))
        self.register_buffer("x", torch.linspace(0, Lx, Nx))
        self.register_buffer("y", torch.linspace(0, Ly, Ny))

    def alpha(self, y_val):
        return 0.5 * self.dt * (self.alpha_w1 + self.alpha_w2 * torch.sin(2 * torch.pi * y_val)
                                + self.alpha_w3 * torch.sin(4 * torch.pi * y_val)) / self.dx ** 2

    def beta(self, x_val):
        return self.dt * (self.beta_w1 + self.beta_w2 * torch.cos(2 * torch.pi * x_val)
                          + self.beta_w3 * torch.cos(4 * torch.pi * x_val)) / self.dy ** 2

    def forward(self, u0):
        if u0.dim() != 4 or u0.shape[1] != 1:
            raise ValueError(f"expected (B,1,H,W), got {tuple(u0.shape)}")
        # coefficient vectors: alpha varies along dim 1 (rows), beta along dim 2 (columns)
        out = F_.jacobi_diffuse(u0.squeeze(1), self.alpha(self.y), self.beta(self.x), self.Nt)
        return out.unsqueeze(1)


def layer_trajectory(layer, u, steps=None):
    """The trajectory of any PDE layer's time loop: a tensor whose slice ``i`` is the state after time step ``steps[i]``,
    out of the launches ``layer(u)`` makes, differentiable in ``u`` and the layer's parameters.

    ``steps``: None (every step) or a strictly increasing sequence of whole 1-based step numbers within the layer's own
    time loop (``1..num_steps``; ``1..Nt`` for ``PDELayer``), ValueError otherwise; the loop ends after ``max(steps)``.

    * an implicit layer (every class with a ``trajectory`` method): ``layer.trajectory(u, steps)``, (K', B, C, H, W);
    * ``ImprovedDiffusionLayer``: (K', B, C, H, W) from functional.explicit5_states with the layer's dt, eps, max_coeff
      and relaxation — one launch per pass for 64x64, 32x32 and 16x16 planes, one per step otherwise;
    * ``PDELayer``: (K', B, 1, H, W) from functional.jacobi_diffuse_states; an input that is not (B,1,H,W) is refused as
      ``forward`` refuses it.  The plane is reflect-padded once and the ring keeps the input's values, so this is not what
      chained one-step layers give.

    For the two explicit layers at most 128 steps per call; slice ``i`` is bit for bit the output of the same layer with
    ``num_steps`` / ``Nt`` = ``steps[i]``, so ``layer_trajectory(layer, u)[-1]`` is ``layer(u)``; inputs are routed as in
    ``forward`` (fp32, bf16 where it takes it, ``model.half()``, float64).  The two explicit classes themselves carry no
    ``trajectory`` method; this function is their layer-level entry, and the classes of ``compat/`` are the same classes."""
    if isinstance(layer, ImprovedDiffusionLayer):
        sel = F_.check_steps(steps, int(layer.num_steps))
        return F_.explicit5_states(u, layer.alpha_base, layer.channel_scaling, layer.dt, layer.stability_eps,
                                   layer.max_coeff, layer._relax, sel)
    if isinstance(layer, PDELayer):
        sel = F_.check_steps(steps, layer.Nt)
        if u.dim() != 4 or u.shape[1] != 1:
            raise ValueError(f"expected (B,1,H,W), got {tuple(u.shape)}")
        out = F_.jacobi_diffuse_states(u.squeeze(1), layer.alpha(layer.y), layer.beta(layer.x), sel)
        return out.unsqueeze(2)
    if isinstance(layer, _AdiBase):
        return layer.trajectory(u, steps)
    raise TypeError(f"{type(layer).__name__} has no time loop to return the trajectory of")


def layer_jvp(layer, u, du=None, dparams=None):
    """Forward-mode derivative of an implicit layer: ``(y, ydot)`` with ``y = layer(u)`` and ``ydot`` its directional
    derivative along the input tangent ``du`` and the parameter tangents ``dparams`` — a mapping from names of
    ``layer.named_parameters()`` to tensors of the parameters' shapes; a missing name (and ``du`` None) is a zero tangent.

    The layer's own ``forward`` runs once under ``torch.autograd.forward_ad.dual_level()`` (``torch.func.functional_call``
    with dual parameters), so the routing is ``forward``'s: fp32, bf16, ``model.half()``, float64, squares and rectangles,
    launch groups beyond 32 steps.  The sweeps go through functional.adi_diffuse — with a coefficient tangent one
    tangent-linear launch per group of sweeps (pde_adi_tangent_fused on square planes of N = 8 .. 32 that are not float64,
    pde_adi*_tangent on the any-size kernels elsewhere), with ``du`` alone the layer's usual forward at ``du`` —
    and a channel operator or skip blend through functional.channel_mix / functional.skip_blend, step by step.  No autograd
    graph is built.  Every implicit class (Mnist, Fashion, Svhn, Enhanced, Learnable); ``ImprovedDiffusionLayer`` and
    ``PDELayer`` are served by ``explicit_layer_jvp``: TypeError here."""
    if not isinstance(layer, _AdiBase):
        hint = "explicit_layer_jvp serves this class" if isinstance(layer, (ImprovedDiffusionLayer, PDELayer)) else \
            "the implicit diffusion layers have one"
        raise TypeError(f"{type(layer).__name__} has no forward-mode derivative here ({hint})")
    return _layer_jvp(layer, u, du, dparams)


def explicit_layer_jvp(layer, u, du=None, dparams=None):
    """``layer_jvp`` for the two explicit layers: ``(y, ydot)`` with ``y = layer(u)`` and ``ydot`` its directional derivative
    along ``du`` and the parameter tangents ``dparams`` (names of ``layer.named_parameters()``; a missing name, and ``du``
    None, is a zero tangent; an unknown name is a KeyError, a wrong shape a ValueError).

    The layer's own ``forward`` runs once under ``torch.autograd.forward_ad.dual_level()``, so the routing is
    ``forward``'s (fp32, bf16 where it takes it, ``model.half()``, float64).  With a parameter tangent the time loop is one
    tangent-linear call (pde_explicit5_tangent / pde_jacobi_io_tangent and their float64 forms: the primal and the tangent
    state advanced together), with ``du`` alone the layer's usual forward at ``du``.  No autograd graph is built.

    * ``ImprovedDiffusionLayer``: ``alpha_base`` and ``channel_scaling``; ``beta_base`` is unused by the layer, so a tangent
      on it contributes exactly zero.
    * ``PDELayer``: its six scalars reach ``a_row`` / ``b_col`` through torch's own forward AD of ``alpha()`` / ``beta()``.

    Any other class: TypeError (``layer_jvp`` serves the implicit ones)."""
    if not isinstance(layer, (ImprovedDiffusionLayer, PDELayer)):
        raise TypeError(f"{type(layer).__name__} is not an explicit PDE layer (layer_jvp serves the implicit ones)")
    return _layer_jvp(layer, u, du, dparams)


def _layer_jvp(layer, u, du, dparams):
    """The body ``layer_jvp`` and ``explicit_layer_jvp`` share: ``functional_call`` with dual parameters under a dual level."""
    import torch.autograd.forward_ad as fwad
    named = dict(layer.named_parameters())
    dparams = dict(dparams or {})
    unknown = sorted(set(dparams) - set(named))
    if unknown:
        raise KeyError(f"no such parameters: {unknown} (the layer has {sorted(named)})")
    with fwad.dual_level():
        params = {}
        for name, p in named.items():
            t = dparams.get(name)
            if t is None:
                params[name] = p.detach()
                continue
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"tangent of {name}: shape {tuple(t.shape)}, expected {tuple(p.shape)}")
            params[name] = fwad.make_dual(p.detach(), t.detach().to(device=p.device, dtype=p.dtype))
        x = u.detach()
        if du is not None:
            if du.shape != u.shape:
                raise ValueError(f"du of shape {tuple(du.shape)} does not match u {tuple(u.shape)}")
            x = fwad.make_dual(x, du.detach().to(device=u.device, dtype=u.dtype))
        out = torch.func.functional_call(layer, params, (x,))
        y, ydot = fwad.unpack_dual(out)
        y = y.detach()
        ydot = torch.zeros_like(y) if ydot is None else ydot.detach()
    return y, ydot
