"""Fused optimizer tail for the HIP training path.

``FusedAdamW`` is a drop-in for ``torch.optim.AdamW`` (same constructor arguments, param groups, state keys
``step`` / ``exp_avg`` / ``exp_avg_sq``, so optimizer checkpoints are interchangeable) whose ``step`` runs the whole
tail of the reference's train step (train.py:285-299) --

    nn.utils.clip_grad_norm_(params, max_norm)   ->   optimizer.step()

-- as two multi-tensor HBM-bound kernels (csrc/optim.hip): a deterministic squared-norm reduction over all gradients
and one AdamW pass that applies the clip coefficient on the fly (gradients themselves are left untouched).

``ModelEma`` / ``accumulate`` are the third part of that row: the reference's model EMA (train_util.py:70-84, called on
every micro-batch from train.py:304-316) as one multi-tensor launch per pack instead of two torch launches per tensor,
and -- ``FusedAdamW.step(ema=(model_ema, decay))`` -- inside the AdamW pass itself.
"""
import ctypes

import torch

from . import ops


def pair_by_name(model1, model2, ema_bn=False):
    """The (name, target, source) pairs of the reference's ``accumulate(model1, model2)``: ``model1``'s parameters in its own
    order, each with the parameter of the SAME NAME of ``model2`` (KeyError when it has none, like the reference's
    ``par2[k]``); with ``ema_bn`` also the buffers whose name contains ``running_mean`` / ``running_var``.  Entries are
    (name, getter of the live target tensor, getter of the live source tensor): ``module.to()`` replaces buffer objects."""
    par1, par2 = dict(model1.named_parameters()), dict(model2.named_parameters())
    pairs = []
    for k in par1.keys():
        pairs.append((k, par1[k], par2[k]))
    if ema_bn:
        buf1, buf2 = dict(model1.named_buffers()), dict(model2.named_buffers())
        for k in buf1.keys():
            if "running_mean" in k or "running_var" in k:
                buf2[k]                                      # (KeyError like the reference's ``buf2[k]``)
                pairs.append((k, _buffer_ref(model1, k), _buffer_ref(model2, k)))
    for k, t, s in pairs:
        t, s = _live(t), _live(s)
        if t.shape != s.shape:
            raise ops.VtxError(f"vtx: EMA pair '{k}': shapes {tuple(t.shape)} and {tuple(s.shape)} differ")
    return pairs


class _buffer_ref:
    """A module buffer by owner and key: ``module.to()`` / ``.float()`` replace the tensor object in ``_buffers``."""

    def __init__(self, model, name):
        owner, _, self.key = name.rpartition(".")
        self.owner = model.get_submodule(owner) if owner else model

    def __call__(self):
        return self.owner._buffers[self.key]


def _live(ref):
    return ref() if isinstance(ref, _buffer_ref) else ref


class ModelEma:
    """The pairing of ``accumulate(model_ema, model, decay, ema_bn)`` done once, with the address arrays of its launches held
    and revalidated against the live ``data_ptr()`` of every tensor before each use (``p.data = ...``, ``.to()``,
    a ``load_state_dict`` that replaces storage), the way ``FusedAdamW._launch_plan`` does.

    ``update(decay)`` moves every target: target = target * decay + source * (1 - decay), the weights as the reference
    forms them (``ops.ema_weights``).  ``FusedAdamW.step(ema=(this, decay))`` moves the targets of the stepped parameters
    inside the AdamW pass and the rest through one ``update`` over what is left."""

    def __init__(self, model_ema, model, ema_bn=False):
        self._init(pair_by_name(model_ema, model, ema_bn))
        self.model_ema, self.model, self.ema_bn = model_ema, model, ema_bn

    @classmethod
    def from_pairs(cls, targets, sources):
        """Positional pairing (DINO: ``zip(student.parameters(), teacher.parameters())``, train_dino.py:258-263)."""
        targets, sources = list(targets), list(sources)
        if len(targets) != len(sources):
            raise ValueError("vtx: ModelEma.from_pairs needs as many sources as targets")
        for i, (t, s) in enumerate(zip(targets, sources)):
            if t.shape != s.shape:
                raise ops.VtxError(f"vtx: EMA pair {i}: shapes {tuple(t.shape)} and {tuple(s.shape)} differ")
        me = cls.__new__(cls)
        me._init([(str(i), t, s) for i, (t, s) in enumerate(zip(targets, sources))])
        me.model_ema = me.model = None
        me.ema_bn = False
        return me

    def _init(self, pairs):
        self.names = [k for k, _, _ in pairs]
        self._tgt = [t for _, t, _ in pairs]
        self._src = [s for _, _, s in pairs]
        # pair index of a source PARAMETER object (held above, so the ids stay unique): how FusedAdamW finds a target
        self.index_of = {id(s): j for j, s in enumerate(self._src) if not isinstance(s, _buffer_ref)}
        self._pl = None

    @staticmethod
    def decay_at(ema, t):
        """The reference's decay at global micro-batch ``t`` (train.py:314)."""
        return min(ema, (1 + t) / (10 + t))

    def __len__(self):
        return len(self.names)

    def tensors(self):
        """(live target tensors, live source tensors), validated: dense contiguous fp32 on the GPU, equal shapes."""
        return self._plan()[1:3]

    def _plan(self):
        ts, ss = [_live(t) for t in self._tgt], [_live(s) for s in self._src]
        key = tuple(t.data_ptr() for t in ts + ss)
        pl = self._pl
        if pl is None or pl[0] != key:
            for k, t, s in zip(self.names, ts, ss):
                if t.shape != s.shape:
                    raise ops.VtxError(f"vtx: EMA pair '{k}': shapes {tuple(t.shape)} and {tuple(s.shape)} differ")
                if t.dtype != torch.float32 or s.dtype != torch.float32:
                    raise ops.VtxError(f"vtx: EMA pair '{k}': fp32 tensors only (got {t.dtype} / {s.dtype})")
            ops._dev(*ts, *ss)
            n = len(ts)
            numel = (ctypes.c_int64 * n)(*[t.numel() for t in ts])
            static = (ops._ptr_array(ts), ops._ptr_array(ss), numel, n, sum(t.numel() for t in ts))
            pl = self._pl = (key, ts, ss, static)
        else:
            pl = self._pl = (key, ts, ss, pl[3])        # (hold the live tensor objects: a replaced buffer is a new object)
        return pl

    @torch.no_grad()
    def update(self, decay):
        """One standalone pass over ALL pairs."""
        ops.ema_update2(None, None, decay, static=self._plan()[3])


def accumulate(model1, model2, decay=0.99999, ema_bn=False):
    """Drop-in for the reference's ``train_util.accumulate``: model1 = model1 * decay + model2 * (1 - decay) over the
    parameters paired by name (and the BatchNorm running statistics with ``ema_bn``), one launch per pack of pairs.
    Non-fp32, non-contiguous or CPU tensors raise: there is no fallback."""
    ModelEma(model1, model2, ema_bn).update(decay)


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if lr < 0 or eps < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1 or weight_decay < 0:
            raise ValueError("FusedAdamW: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._recs = None           # static per-parameter records (see _records)
        self._plans = {}
        self._checked = set()       # plans validated in the current step
        self._ema_plans = {}        # idx -> EMA target addresses of that launch (see _ema_plan)

    # ---- host-side bookkeeping.  A step touches ~330 parameters; looking at each one's state dict, validating four
    # tensors per parameter, building four address arrays and bumping 330 CPU step tensors cost ~2.4 ms of host time per
    # step (tools/probe/host_profile.py).  Everything that does not change from step to step is recorded once:
    # (parameter, state, group) triples in group order, the address arrays of params / exp_avg / exp_avg_sq per launch,
    # and ALL ``state["step"]`` tensors as 0-dim views of ONE CPU tensor, so that a step is one ``add_`` (the state
    # layout stays torch.optim.AdamW's: ``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter, checkpoints interchangeable).
    def _records(self):
        key = tuple(id(p) for g in self.param_groups for p in g["params"])
        if self._recs is not None and self._recs[0] == key and all(st["step"] is v for (_, st, _), v in zip(self._recs[1], self._recs[3])):
            return self._recs
        recs = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                    raise ops.VtxError("FusedAdamW: dense contiguous fp32 parameters on the GPU only")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                recs.append((p, st, group))
        flat = torch.tensor([float(st["step"]) for _, st, _ in recs], dtype=torch.float32)
        views = []
        for i, (_, st, _) in enumerate(recs):
            st["step"] = flat[i]                       # 0-dim view: float(st["step"]) / state_dict() see the live count
            views.append(st["step"])
        self._recs = (key, recs, flat, views, [int(v) for v in flat.tolist()])
        self._plans = {}
        return self._recs

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._recs = None

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._recs = None

    def _launch_plan(self, idx, recs):
        """Address arrays of one multi-tensor launch over the parameters ``idx`` (a tuple), built once and VALIDATED once
        per step against the live storage addresses of every parameter and moment tensor: ``p.data = ...``, ``module.to()``
        / ``.float()`` after construction or a replaced ``exp_avg_sq`` change an address without changing any Python
        object identity (and ``id()`` values are reused after garbage collection) -- the kernel would read and write freed
        memory.  The plan also holds references to the moment tensors it addresses.  ~0.1 ms per step for 330 tensors."""
        pl = self._plans.get(idx)
        if pl is not None and idx not in self._checked:
            ps = [recs[i][0] for i in idx]
            ms = [recs[i][1]["exp_avg"] for i in idx]
            vs = [recs[i][1]["exp_avg_sq"] for i in idx]
            if pl[6] != tuple(t.data_ptr() for t in ps + ms + vs):
                pl = None                                # some storage moved: rebuild the address arrays
            else:
                self._checked.add(idx)
        if pl is None:
            import ctypes
            ps = [recs[i][0] for i in idx]
            ms = [recs[i][1]["exp_avg"] for i in idx]
            vs = [recs[i][1]["exp_avg_sq"] for i in idx]
            ops._dev(*ps, *ms, *vs)
            for p, m, v in zip(ps, ms, vs):
                if m.shape != p.shape or v.shape != p.shape or m.dtype != torch.float32 or v.dtype != torch.float32:
                    raise ops.VtxError("FusedAdamW: exp_avg / exp_avg_sq must be fp32 tensors of the parameter's shape")
            chunk = ops._lib.load().vtx_opt_chunk()
            numel = (ctypes.c_int64 * len(idx))(*[p.numel() for p in ps])
            pl = self._plans[idx] = (ops._ptr_array(ps), ops._ptr_array(ms), ops._ptr_array(vs), numel,
                                     sum(p.numel() for p in ps), sum((p.numel() + chunk - 1) // chunk for p in ps),
                                     tuple(t.data_ptr() for t in ps + ms + vs), (ms, vs))
            self._checked.add(idx)
        return pl

    def _ema_plan(self, idx, recs, me, targets):
        """EMA side of the launch over ``idx``: the target address array (NULL where a parameter has none), keyed like the
        launch plan and validated against the ModelEma, the live target addresses and the launch plan it extends."""
        base = self._launch_plan(idx, recs)
        es = [targets.get(id(recs[i][0])) for i in idx]
        ptrs = tuple(0 if e is None else e[1].data_ptr() for e in es)
        pl = self._ema_plans.get(idx)
        if pl is None or pl[0] is not me or pl[1] != ptrs or pl[2] is not base:
            for i, e in zip(idx, es):
                if e is not None and e[1].shape != recs[i][0].shape:
                    raise ops.VtxError("FusedAdamW: an EMA target must have its parameter's shape")
            ea = (ctypes.c_void_p * len(idx))(*[p or None for p in ptrs])
            pl = self._ema_plans[idx] = (me, ptrs, base, ea, sum(e[1].numel() for e in es if e is not None),
                                         [e[0] for e in es if e is not None])
        return base, pl

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=0.0, ema=None):
        """One AdamW update of every parameter that has a gradient.  ``max_grad_norm > 0`` additionally applies
        ``clip_grad_norm_(all these parameters, max_grad_norm)`` semantics inside the update; returns the total gradient
        norm (device scalar tensor) in that case, else None.

        ``ema`` = (ModelEma, decay): every pair of the ModelEma moves exactly once in this call -- the targets of the
        parameters stepped here inside the AdamW pass (from the new value), all others (no gradient this step, not in this
        optimizer, ``ema_bn`` buffers) through one standalone launch afterwards."""
        me = decay = targets = None
        fused = set()
        if ema is not None:
            me, decay = ema
            if not isinstance(me, ModelEma):
                raise TypeError("FusedAdamW.step: ema must be (vtx.optim.ModelEma, decay)")
            decay = float(decay)
            ts, ss = me.tensors()
            targets = {i: (j, ts[j]) for i, j in me.index_of.items()}
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _, recs, flat, _, counts = self._records()
        self._checked = set()
        live, gs = [], []
        for i, (p, _, _) in enumerate(recs):
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or g.is_sparse or not g.is_cuda:
                raise ops.VtxError("FusedAdamW: dense fp32 gradients on the GPU only")
            live.append(i)
            gs.append(g if g.is_contiguous() else g.contiguous())
        if not live:
            if me is not None:
                me.update(decay)
            return loss
        live = tuple(live)
        norm = None
        if max_grad_norm and max_grad_norm > 0:              # over ALL gradients, whatever their step counts
            pl = self._launch_plan(live, recs)
            norm = ops.grad_sqnorm(gs, static=(pl[3], pl[5]))
        # torch.optim.AdamW keeps a step count PER PARAMETER (a parameter that gets its first gradient late -- DINO's
        # last layer is frozen during epoch 0, train_dino.py:250 -- starts at step 1 then): one multi-tensor launch per
        # distinct (betas, eps, step) -- a single one in the steady state
        by_key = {}
        for j, i in enumerate(live):
            g = recs[i][2]
            by_key.setdefault((g["betas"], g["eps"], counts[i]), []).append(j)
        for (betas, eps, t0), js in by_key.items():
            idx = live if len(js) == len(live) else tuple(live[j] for j in js)
            if me is not None:
                pl, epl = self._ema_plan(idx, recs, me, targets)
                if epl[5]:
                    ops.adamw_ema_step(None, gs if len(js) == len(live) else [gs[j] for j in js], None, None,
                                       [float(recs[i][2]["lr"]) for i in idx],
                                       [float(recs[i][2]["weight_decay"]) for i in idx], norm,
                                       float(max_grad_norm or 0.0), betas[0], betas[1], eps, t0 + 1, None, decay,
                                       static=pl[:5] + (epl[3], epl[4]))
                    fused.update(epl[5])
                    continue
            pl = self._launch_plan(idx, recs)
            ops.adamw_step(None, gs if len(js) == len(live) else [gs[j] for j in js], None, None,
                           [float(recs[i][2]["lr"]) for i in idx], [float(recs[i][2]["weight_decay"]) for i in idx], norm,
                           float(max_grad_norm or 0.0), betas[0], betas[1], eps, t0 + 1, static=pl[:5])
        if len(live) == len(recs):
            flat.add_(1.0)                                   # every state["step"] is a view of this one tensor
        else:
            flat[list(live)] += 1.0
        for i in live:
            counts[i] += 1
        if me is not None and len(fused) < len(me):
            rest = [j for j in range(len(me)) if j not in fused]      # exactly once: whatever the AdamW pass did not move
            ops.ema_update2([ts[j] for j in rest], [ss[j] for j in rest], decay)
        return norm[1] if norm is not None else loss
