"""Fused AdamW and Adam over flat parameter arenas.  FusedAdamW replaces torch.optim.AdamW (the
reference's optimizer: configs/optimizer/adamw.yaml, built in
VisionLanguageModule.configure_optimizers :130-184 from the parameter groups of
_configure_optimizer_parameters :186-243); FusedAdam, at the end of this file, is the same
machinery for torch.optim.Adam (configs/optimizer/adam.yaml), whose step differs in the weight
decay alone.

Same parameter-group semantics as torch.optim.AdamW: per-group lr, parameters
whose .grad is None are skipped entirely (the unused TinyBERT pooler, as in the
reference), decoupled weight decay (torch default 0.01), bias correction with
the parameter's step count.  Each group is updated by one `vlp_adamw` launch per
contiguous arena span of parameters that have gradients.

State: the first/second moments live in two flat fp32 buffers per arena (same
offsets as the parameters), and `self.state[p]` holds {"step", "exp_avg",
"exp_avg_sq"} with the moments as views of those buffers -- torch.optim.AdamW's
layout, so `state_dict()` / `load_state_dict()` round-trip (and a torch AdamW
state dict loads here) while the update stays one launch per span.

Gradient clipping (`set_gradient_clipping`, Lightning's gradient_clip_val /
gradient_clip_algorithm) is fused into the step and never reads the device back.
"norm" is torch.nn.utils.clip_grad_norm_ over every parameter that has a gradient,
across all groups: one `vlp_grad_sumsq` per span into one fp64 partials buffer,
one `vlp_clip_coef`, then `vlp_adamw_clip` per span scales the gradient by the
device-side coefficient, writes it back and updates.  "value" is clip_grad_value_:
`vlp_adamw_clip` clamps instead, with no norm pass.  Off (the default), the step
launches `vlp_adamw` only.

Gradient accumulation (Lightning's accumulate_grad_batches): the towers' backward overwrites
the gradient arenas, so `accumulate(w, first)` folds the micro-batch just run into an
accumulator the size of each arena (`vlp_grad_accum`, one pass; the buffer is allocated by the
first call and never cleared: `first` does not read it) and drops the .grad views, and the next
`step()` takes what is pending: with fresh gradients in the arenas it steps on acc + w*g
(`vlp_grad_accum_sumsq` for the norm, `vlp_adamw_clip_accum` for the update: the last
micro-batch's sum is never stored), with none (every micro-batch folded, as under data
parallelism, where `reduce_accumulated()` all-reduces the accumulators once per step) on the
accumulator alone, through the kernels of the plain step.  Both clip modes act on the
accumulated gradient.  Without `accumulate()` nothing changes and no buffer exists.
"""
from __future__ import annotations

import torch

from . import ops


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 arenas=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        # map parameter -> (arena, offset, numel)
        self._loc = {}
        for a in arenas or []:
            mod = a
            for owner, attr, full in mod._param_slots:
                p = owner._parameters[attr]
                o, n, _ = mod.arena.layout[full]
                self._loc[id(p)] = (mod.arena, o, n)
        for g in self.param_groups:
            for p in g["params"]:
                if id(p) not in self._loc:
                    raise ValueError("FusedAdamW: every parameter must live in a ParamArena")
        self._flat = {}        # id(arena) -> (m, v) flat fp32 buffers
        self._span_cache = {}
        self._steps = {}       # id(p) -> step count (mirrored into state[p]["step"] by state_dict())
        self._clip = None      # None | ("norm", max_norm) | ("value", clip_value)
        self._clip_bufs = None  # (fp64 partials, fp32 {norm, coef}) on the arenas' device
        self._copied = []      # (p.grad, arena view) pairs _spans copied in this step
        self.last_grad_norm = None   # device scalar: the global norm before clipping ("norm" only)
        self._acc = {}         # id(arena) -> gradient accumulator (fp32, the arena's size), made by accumulate()
        self._pending = None   # (signature, per-group spans) of the micro-batches folded since the last step
        self._src = None       # gradient of the running step: None = arena.grad | ("sum", w) | ("acc",)

    def set_gradient_clipping(self, val, algorithm="norm"):
        """Clip in every later step(): "norm" to a global L2 norm of `val`
        (clip_grad_norm_), "value" each element to [-val, val] (clip_grad_value_).
        None or val <= 0 turns clipping off."""
        if algorithm not in ("norm", "value"):
            raise ValueError(f"FusedAdamW: gradient clip algorithm must be 'norm' or 'value', got {algorithm!r}")
        self._clip = None if val is None or val <= 0 else (algorithm, float(val))
        self.last_grad_norm = None

    def _clip_buffers(self, device, nparts):
        b = self._clip_bufs
        if b is None or b[0].device != device or b[0].numel() < nparts:
            out = b[1] if b is not None and b[1].device == device else torch.zeros(2, dtype=torch.float32, device=device)
            b = (torch.empty(max(nparts, 1), dtype=torch.float64, device=device), out)
            self._clip_bufs = b
        return b

    def _moments(self, arena):
        b = self._flat.get(id(arena))
        if b is None or b[0].numel() != arena.numel or b[0].device != arena.data.device:
            b = (torch.zeros(arena.numel, dtype=torch.float32, device=arena.data.device),
                 torch.zeros(arena.numel, dtype=torch.float32, device=arena.data.device))
            self._flat[id(arena)] = b
        return b

    def _bind(self, p):
        """state[p] with moment views into the flat buffers (created at step 0)."""
        arena, o, n = self._loc[id(p)]
        m, v = self._moments(arena)
        st = self.state[p]
        mv, vv = m[o:o + n].view_as(p), v[o:o + n].view_as(p)
        if "exp_avg" in st and st["exp_avg"].data_ptr() != mv.data_ptr():
            mv.copy_(st["exp_avg"])       # loaded from a state dict: move into the flat buffer
            vv.copy_(st["exp_avg_sq"])
        st["exp_avg"], st["exp_avg_sq"] = mv, vv
        self._steps.setdefault(id(p), int(st["step"].item()) if "step" in st else 0)
        return st

    def _spans(self, group):
        """Contiguous (arena, off, len, [params]) spans of params with gradients."""
        items = []
        for p in group["params"]:
            if p.grad is None:
                continue
            arena, o, n = self._loc[id(p)]
            g = arena.grad[o:o + n].view_as(p)
            if p.grad.data_ptr() != g.data_ptr():
                g.copy_(p.grad)  # gradients not produced in place (e.g. accumulated by autograd)
                if self._clip is not None:
                    self._copied.append((p.grad, g))   # step() copies the clipped gradient back
            items.append((arena, o, n, p))
        sig = tuple(t[1] for t in items) + tuple(id(t[0]) for t in items)
        cached = self._span_cache.get(sig)
        if cached is not None:
            return cached
        items.sort(key=lambda t: (id(t[0]), t[1]))
        spans = []
        for arena, o, n, p in items:
            if spans and spans[-1][0] is arena and self._gap_free(arena, spans[-1][1] + spans[-1][2], o):
                a, so, sn, ps = spans[-1]
                spans[-1] = (a, so, o + n - so, ps + [p])
            else:
                spans.append((arena, o, n, [p]))
        self._span_cache[sig] = spans
        return spans

    @staticmethod
    def _gap_free(arena, end, start):
        """True if [end, start) holds only alignment padding (zeros with zero
        gradient, which AdamW leaves at zero), i.e. no other parameter."""
        if start < end:
            return False
        return not any(end <= o < start for o, _, _ in arena.layout.values())

    def _accumulator(self, arena):
        b = self._acc.get(id(arena))
        if b is None or b.numel() != arena.numel or b.device != arena.data.device:
            b = torch.empty(arena.numel, dtype=torch.float32, device=arena.data.device)
            self._acc[id(arena)] = b
        return b

    @staticmethod
    def _signature(work):
        return tuple((id(arena), o, n) for spans in work for arena, o, n, _ in spans)

    @torch.no_grad()
    def accumulate(self, w=1.0, first=None):
        """Fold the gradients of the backward just run into the accumulators: acc = w * g if
        `first` (the accumulators' old contents are not read), else acc += w * g.  first=None:
        whether anything is pending.  The .grad views are dropped, so the next backward writes
        the arenas afresh; `step()` then uses what is pending."""
        if first is None:
            first = self._pending is None
        copied, self._copied = self._copied, []
        work = [self._spans(group) for group in self.param_groups]
        self._copied = copied
        sig = self._signature(work)
        if not sig:
            raise RuntimeError("FusedAdamW.accumulate: no parameter has a gradient")
        if first:
            self._pending = (sig, work)
        elif self._pending is None:
            raise RuntimeError("FusedAdamW.accumulate: first=False with nothing accumulated")
        elif self._pending[0] != sig:
            raise RuntimeError("FusedAdamW.accumulate: the parameters with gradients changed between micro-batches")
        for spans in work:
            for arena, o, n, _ in spans:
                ops.grad_accum(self._accumulator(arena)[o:o + n], arena.grad[o:o + n], w, first)
        for group in self.param_groups:
            for p in group["params"]:
                p.grad = None

    def reduce_accumulated(self):
        """Data parallelism: SUM all-reduce of the pending accumulators, once per optimizer step
        (one collective per span), for modules whose backward was told not to reduce each
        micro-batch.  Every micro-batch must have been folded by accumulate()."""
        from . import dist as vdist
        if self._pending is None:
            raise RuntimeError("FusedAdamW.reduce_accumulated: nothing accumulated")
        for spans in self._pending[1]:
            for arena, o, n, _ in spans:
                vdist.all_reduce_sum_(self._accumulator(arena)[o:o + n])

    @torch.no_grad()
    def step(self, closure=None, w=1.0):
        """`w`: the weight of the fresh gradients when micro-batches are pending (acc + w * g)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # every group's spans first: the norm covers all of them before any update
        self._copied = []
        spans_of = [self._spans(group) for group in self.param_groups]
        self._src = None
        if self._pending is not None:
            sig, folded = self._pending
            self._pending = None
            if not self._signature(spans_of):
                spans_of, self._src = folded, ("acc",)     # every micro-batch was folded
            elif self._signature(spans_of) == sig:
                self._src = ("sum", float(w))
                self._copied = []                            # neither kernel writes g back
            else:
                raise RuntimeError("FusedAdamW.step: the parameters with gradients differ from the accumulated ones")
        work = list(zip(self.param_groups, spans_of))
        if self._clip is not None and self._clip[0] == "norm":
            self._launch_norm([s for _, spans in work for s in spans])
        for group, spans in work:
            for arena, o, n, ps in spans:
                steps = set()
                for p in ps:
                    if id(p) not in self._steps:
                        self._bind(p)
                    self._steps[id(p)] += 1
                    steps.add(self._steps[id(p)])
                if len(steps) != 1:
                    # parameters of one span disagree on their step count (a parameter
                    # that had no gradient in earlier steps): update them one by one
                    for p in ps:
                        _, po, pn = self._loc[id(p)]
                        self._launch(arena, po, pn, group, self._steps[id(p)])
                    continue
                self._launch(arena, o, n, group, steps.pop())
        for grad, g in self._copied:   # p.grad outside the arena: leave it clipped as well
            grad.copy_(g)
        self._copied = []
        self._src = None
        return loss

    def _launch_norm(self, spans):
        """Global gradient norm and clip coefficient of the step, on the device."""
        if not spans:
            self.last_grad_norm = None
            return
        total = sum(ops.grad_sumsq_nparts(n) for _, _, n, _ in spans)
        partials, out = self._clip_buffers(spans[0][0].grad.device, total)
        off = 0
        for arena, o, n, _ in spans:
            if self._src is None:
                off += ops.grad_sumsq(arena.grad[o:o + n], partials, off)
            elif self._src[0] == "acc":
                off += ops.grad_sumsq(self._accumulator(arena)[o:o + n], partials, off)
            else:
                off += ops.grad_accum_sumsq(self._accumulator(arena)[o:o + n], arena.grad[o:o + n], self._src[1],
                                            partials, off)
        ops.clip_coef(off, partials, self._clip[1], out)
        self.last_grad_norm = out[0]

    def _launch(self, arena, o, n, group, step, op=None):
        """One span's step.  op: the entry point that takes every case (FusedAdam's); None: AdamW's
        entry point for this case."""
        b1, b2 = group["betas"]
        m, v = self._moments(arena)
        grad = self._accumulator(arena) if self._src == ("acc",) else arena.grad
        kw = {} if self._clip is None else (dict(coef=self._clip_bufs[1][1:]) if self._clip[0] == "norm"
                                            else dict(clip_value=self._clip[1]))
        if self._src is not None and self._src[0] == "sum":
            kw.update(acc=self._accumulator(arena)[o:o + n], w=self._src[1])
        if op is None:
            op = ops.adamw_clip_accum if "acc" in kw else ops.adamw_clip if kw else ops.adamw
        op(arena.data[o:o + n], grad[o:o + n], m[o:o + n], v[o:o + n],
           group["lr"], b1, b2, group["eps"], group["weight_decay"], step, **kw)

    def state_dict(self):
        for group in self.param_groups:
            for p in group["params"]:
                if id(p) in self._steps:
                    self.state[p]["step"] = torch.tensor(float(self._steps[id(p)]))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps = {}
        for group in self.param_groups:
            for p in group["params"]:
                if p in self.state and "exp_avg" in self.state[p]:
                    self.state[p]["step"] = torch.as_tensor(self.state[p]["step"], dtype=torch.float32).cpu()
                    self._bind(p)

    def zero_grad(self, set_to_none: bool = True):
        self._pending = None   # accumulated micro-batches are gradients too
        for group in self.param_groups:
            for p in group["params"]:
                p.grad = None


class FusedAdam(FusedAdamW):
    """torch.optim.Adam (configs/optimizer/adam.yaml, the reference's `optimizer: adam`
    experiments) over the same arenas: FusedAdamW with the weight decay as an L2 term of the
    gradient (torch's grad.add(param, alpha=weight_decay), after any clipping) in place of the
    decay of the parameter, and torch.optim.Adam's defaults (weight_decay 0).  Every case of the
    step -- plain, clipped by norm or value, on fresh gradients, on acc + w*g or on the
    accumulator alone -- is one `vlp_adam_step` launch per span; spans, step counts, the norm
    pass, accumulate(), reduce_accumulated(), zero_grad() and the moment buffers are
    FusedAdamW's.  The clipped gradient that is written back to g is the one torch leaves in
    p.grad: without the L2 term.

    The parameter groups carry torch.optim.Adam's remaining keys at their defaults, so a
    state_dict() loads into torch.optim.Adam and one of torch's loads here.  amsgrad and
    maximize have no kernel and raise ValueError."""

    _TORCH_KEYS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False,
                       fused=None)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 maximize=False, arenas=None):
        if amsgrad or maximize:
            raise ValueError("FusedAdam: amsgrad / maximize are not implemented on the device (use torch.optim.Adam)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, arenas=arenas)
        for k, v in self._TORCH_KEYS.items():
            self.defaults.setdefault(k, v)
            for group in self.param_groups:
                group.setdefault(k, v)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if any(g.get("amsgrad") or g.get("maximize") for g in self.param_groups):
            raise ValueError("FusedAdam: the loaded state asks for amsgrad / maximize")

    def _launch(self, arena, o, n, group, step):
        super()._launch(arena, o, n, group, step, op=ops.adam_step)
