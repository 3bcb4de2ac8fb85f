"""torch.optim.Adam with a one-launch step on the HIP path.

The reference builds two ``torch.optim.Adam`` (GAN_models/wind_field_GAN_3D.py:151-162) and calls ``.step()`` once per
iteration (:460, :566).  torch's fused multi-tensor implementation packs tensor pointers into kernel arguments, so the
generator's 297 tensors take 8 launches of ~78 workgroups (0.39 ms of a 93 ms step at 0.97 GB of traffic); here the
pointers live in a DEVICE table (``wsr_adam_multi``, one workgroup per 32 768-element chunk) and the whole parameter list
is one launch.  Same hyper-parameters, same ``state`` layout (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter) and
therefore the same ``state_dict`` and checkpoints as ``torch.optim.Adam(fused=True)``, which it falls back to whenever
the fast path does not apply (CPU tensors, a missing gradient, amsgrad / maximize / capturable / differentiable).

Gradient-norm clipping (``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_`` over each param group, applied INSIDE
``step()``, i.e. after the step pre-hooks - under data parallelism the one that waits for the gradient averaging) is
two launches on the fast path: ``wsr_grad_sqnorm_multi`` over the table, then ``wsr_adam_multi_clip``, which takes the
coefficient on the device, writes the clipped gradients back and updates.  ``track_grad_norm`` measures without
clipping.  Either way ``last_grad_norm`` holds the pre-clip norm as a 0-d device tensor (no host sync).

Moving average of the weights (``ema_decay``): one shadow tensor per parameter (``ema_shadows``, group order),
``e <- d * e + (1 - d) * p`` on the parameters each step has just produced; ``d`` = 0 makes the shadows follow the
weights.  On the fast path the update rides in the Adam launch (``wsr_adam_multi_ema`` / ``wsr_adam_multi_clip_ema``:
the shadow pointers in a device array parallel to the job table), so it costs no launch of its own; behind every torch
fallback it is two ``_foreach`` ops in the same formula.  The shadows are NOT optimizer state: ``state_dict()`` keeps
the layout of ``torch.optim.Adam(fused=True)``, their owner saves them.
"""
import math
from typing import Dict, List, Optional, Tuple

import torch

from .. import hip_ops


@torch.no_grad()
def ema_update_(shadows: List[torch.Tensor], params: List[torch.Tensor], decay: float) -> None:
    """``e <- decay * e + (1 - decay) * p`` with torch ops (the kernels' formula up to rounding); ``decay`` = 0 copies"""
    params = [p.detach() for p in params]
    if decay == 0.0:
        torch._foreach_copy_(shadows, params)
    else:
        torch._foreach_mul_(shadows, decay)
        torch._foreach_add_(shadows, params, alpha=1.0 - decay)


class TableAdam(torch.optim.Adam):
    def __init__(self, params, max_grad_norm: Optional[float] = None, track_grad_norm: bool = False,
                 ema_decay: Optional[float] = None, ema_shadows: Optional[List[torch.Tensor]] = None, **kw):
        kw.setdefault("fused", True)
        super().__init__(params, **kw)
        self.ema_decay = ema_decay                   # None: no moving average
        self._ema: Optional[List[torch.Tensor]] = None  # the shadows, one per parameter in group order
        self._ema_tables: Dict[int, torch.Tensor] = {}  # per param group: one shadow pointer per job of its table
        self.max_grad_norm = max_grad_norm           # None: no clipping
        self.track_grad_norm = track_grad_norm       # measure the norm even when not clipping
        self.last_grad_norm: Optional[torch.Tensor] = None  # pre-clip norm of the last measured step (one per group)
        self._partials: Dict[int, torch.Tensor] = {}  # per param group: one float per job of its table
        self._tables: Dict[int, torch.Tensor] = {}   # per param group: device table of (param, grad, state) chunks
        self._sig: Dict[int, tuple] = {}             # ... and the (param, grad) pointers it was built from
        self._host_step: List[int] = [-1] * len(self.param_groups)  # -1: not yet read from the state
        self._steps_dirty = False
        if ema_shadows is not None:
            self.ema_shadows = ema_shadows

    @property
    def max_grad_norm(self) -> Optional[float]:
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, v: Optional[float]) -> None:
        if v is not None:
            v = float(v)
            if not (v > 0 and math.isfinite(v)):
                raise ValueError(f"max_grad_norm must be > 0 and finite, not {v}")
        self._max_grad_norm = v

    @property
    def ema_decay(self) -> Optional[float]:
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, d: Optional[float]) -> None:
        if d is not None:
            d = float(d)
            if not 0.0 <= d < 1.0:  # (NaN fails both)
                raise ValueError(f"ema_decay must be in [0, 1), not {d}")
        self._ema_decay = d

    def _all_params(self) -> List[torch.Tensor]:
        return [p for g in self.param_groups for p in g["params"]]

    @property
    def ema_shadows(self) -> List[torch.Tensor]:
        """one tensor per parameter, group order; clones of the parameters when nobody handed them in"""
        if self._ema is None:
            self._ema = [p.detach().clone(memory_format=torch.contiguous_format) for p in self._all_params()]
        return self._ema

    @ema_shadows.setter
    def ema_shadows(self, shadows: List[torch.Tensor]) -> None:
        shadows, params = list(shadows), self._all_params()
        if len(shadows) != len(params):
            raise ValueError(f"ema_shadows: {len(shadows)} tensors for {len(params)} parameters")
        for e, p in zip(shadows, params):
            if e.shape != p.shape or e.dtype != p.dtype or e.device != p.device or e.requires_grad:
                raise ValueError("ema_shadows: each shadow wants its parameter's shape, dtype and device, no grad")
        self._ema = shadows
        self._ema_tables.clear()
        self._sig.clear()

    def _ema_fallback(self) -> None:
        """behind a step that torch took"""
        ema_update_(self.ema_shadows, self._all_params(), self._ema_decay)

    def _measures(self) -> bool:
        return self._max_grad_norm is not None or self.track_grad_norm

    def _set_norms(self, norms: List[torch.Tensor]) -> None:
        self.last_grad_norm = norms[0] if len(norms) == 1 else torch.stack(norms)

    def _clip_fallback(self) -> None:
        """torch's own clip (or, tracking only, its norm) over each group, in front of torch's step"""
        norms = []
        for group in self.param_groups:
            params = [p for p in group["params"] if p.grad is not None]
            if self._max_grad_norm is not None:
                norms.append(torch.nn.utils.clip_grad_norm_(params, self._max_grad_norm))
            else:
                norms.append(torch.nn.utils.get_total_norm([p.grad for p in params]))
        self._set_norms(norms)

    # ---- state bookkeeping ----------------------------------------------------------------------------------
    def _init_state(self, p: torch.Tensor) -> dict:
        st = self.state[p]
        if len(st) == 0:  # as torch.optim.Adam._init_group does for fused=True
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _sync_steps(self) -> None:
        """write the host step counts into the per-parameter ``step`` tensors (before anything reads the state)"""
        if not self._steps_dirty:
            return
        for gi, group in enumerate(self.param_groups):
            steps = [self.state[p]["step"] for p in group["params"] if "step" in self.state.get(p, {})]
            if steps and self._host_step[gi] >= 0:
                torch._foreach_zero_(steps)
                torch._foreach_add_(steps, float(self._host_step[gi]))
        self._steps_dirty = False

    def _fast_ok(self, group: dict) -> bool:
        if group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable") \
                or group.get("decoupled_weight_decay"):  # (the kernel implements Adam's L2 form of weight decay only)
            return False
        if not isinstance(group["lr"], float) and not isinstance(group["lr"], int):
            return False
        for p in group["params"]:
            g = p.grad
            if g is None or g.is_sparse or not p.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 \
                    or not p.is_contiguous() or not g.is_contiguous() or g.device != p.device:
                return False
        return len(group["params"]) > 0

    # ---- torch.optim.Optimizer interface ----------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        # (host cost matters at the small presets, where ~1 600 launches per 30 ms step leave the host no slack: one pass
        # over the pointers decides whether last step's table still describes this one - then nothing else is looked at)
        # ... the pointers AND what _fast_ok decides from the group's options: a learning rate that became a tensor, a
        # flag switched on after construction must not ride on a table built before
        sigs = [(type(g["lr"]) in (float, int), bool(g.get("amsgrad") or g.get("maximize") or g.get("capturable")
                                                      or g.get("differentiable") or g.get("decoupled_weight_decay")))
                + tuple((p.data_ptr(), p.grad.data_ptr()) if p.grad is not None else None for p in g["params"])
                for g in self.param_groups]
        ema = self._ema_decay is not None
        if ema:  # (a shadow that was re-allocated, or swapped with its parameter, must not ride on an old table)
            it = iter(self.ema_shadows)
            sigs = [sig + tuple(next(it).data_ptr() for _ in g["params"]) for sig, g in zip(sigs, self.param_groups)]
        hit = closure is None and all(self._sig.get(gi) == sig for gi, sig in enumerate(sigs))
        fast = hit or (closure is None and all(self._fast_ok(g) for g in self.param_groups))
        if fast:
            for gi, group in enumerate(self.param_groups):
                if self._host_step[gi] < 0:  # first fast step (or after a fallback / load_state_dict): one read of the state
                    steps = torch.stack([self._init_state(p)["step"].float() for p in group["params"]])
                    lo, hi = (float(v) for v in torch.stack([steps.min(), steps.max()]).tolist())
                    if lo != hi:  # parameters of one group at different step counts: only torch's per-tensor form is right
                        fast = False
                        break
                    self._host_step[gi] = int(round(hi))
        if not fast:
            self._sync_steps()
            if self._measures():
                if closure is not None:  # (the gradients a closure computes exist only inside torch's step)
                    raise ValueError("TableAdam: gradient-norm clipping does not take a closure")
                self._clip_fallback()
            out = super().step(closure)
            if ema:
                self._ema_fallback()
            self._host_step = [-1] * len(self.param_groups)
            self._sig.clear()
            return out
        norms: List[torch.Tensor] = []
        first = 0  # index of the group's first parameter in ema_shadows
        for gi, group in enumerate(self.param_groups):
            self._host_step[gi] += 1
            if self._sig.get(gi) != sigs[gi]:
                quads: List[Tuple[torch.Tensor, ...]] = []
                for p in group["params"]:
                    st = self._init_state(p)
                    quads.append((p, p.grad, st["exp_avg"], st["exp_avg_sq"]))
                self._tables[gi] = hip_ops.adam_job_table(quads)
                self._ema_tables.pop(gi, None)
                if ema:
                    shadows = self.ema_shadows[first:first + len(quads)]
                    if any(not e.is_cuda or not e.is_contiguous() for e in shadows):
                        raise ValueError("TableAdam: the EMA shadows of device parameters must be contiguous device tensors")
                    self._ema_tables[gi] = hip_ops.ema_ptr_table(quads, shadows)
                self._partials.pop(gi, None)
                self._sig[gi] = sigs[gi]
            first += len(group["params"])
            table = self._tables[gi]
            b1, b2 = group["betas"]
            if not self._measures():
                if ema:
                    hip_ops.adam_multi_ema(table, self._ema_tables[gi], float(group["lr"]), b1, b2, group["eps"],
                                           group["weight_decay"], self._host_step[gi], self._ema_decay)
                else:
                    hip_ops.adam_multi(table, float(group["lr"]), b1, b2, group["eps"], group["weight_decay"],
                                       self._host_step[gi])
                continue
            if gi not in self._partials:
                self._partials[gi] = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
            partials = self._partials[gi]
            norm = torch.empty((), dtype=torch.float32, device=table.device)
            hip_ops.grad_sqnorm_multi(table, partials)
            bound = self._max_grad_norm if self._max_grad_norm is not None else math.inf
            if ema:
                hip_ops.adam_multi_clip_ema(table, self._ema_tables[gi], partials, bound, float(group["lr"]), b1, b2,
                                            group["eps"], group["weight_decay"], self._host_step[gi], self._ema_decay,
                                            total_norm=norm)
            else:
                hip_ops.adam_multi_clip(table, partials, bound, float(group["lr"]), b1, b2, group["eps"],
                                        group["weight_decay"], self._host_step[gi], total_norm=norm)
            norms.append(norm)
        if norms:
            self._set_norms(norms)
        self._steps_dirty = True
        return None

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables.clear()
        self._ema_tables.clear()
        self._partials.clear()
        self._sig.clear()
        self._host_step = [-1] * len(self.param_groups)
        self._steps_dirty = False

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_host_step"):
            self._host_step.append(-1)
        if getattr(self, "_ema", None) is not None:  # shadows of the new group's parameters: clones, as on first use
            self._ema += [p.detach().clone(memory_format=torch.contiguous_format) for p in self.param_groups[-1]["params"]]
