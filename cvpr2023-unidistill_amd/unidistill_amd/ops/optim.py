"""ClipAdamW: gradient-norm clipping + decoupled-weight-decay AdamW in two hand-written launches (csrc/optim.hip).

What ``clip_grad_norm_(foreach=True)`` followed by ``torch.optim.AdamW(fused=True)`` does in 16 launches per step, with one
capability on top: with ``skip_nonfinite`` a step whose total gradient norm is inf / nan leaves every parameter, both
moments and the step count untouched and counts itself in ``skipped`` -- decided on the device, without a host sync.

The parameter set is cut into chunks of ``chunk_elems()`` elements (``build_chunk_table``), one workgroup each.  The device
holds a table of chunk records and four rows of per-tensor pointers (parameter, exp_avg, exp_avg_sq, gradient).  The first
three rows are static and re-validated by comparing ``data_ptr()`` every step; gradient pointers change every step under
``zero_grad(set_to_none=True)`` and travel through a ring of pinned host slots (one async copy, a slot is reused only after
the event recorded behind its copy has completed).  When they do not change (DDP bucket views, static graph buffers)
nothing is uploaded.  ``p.grad`` is only read: it is NOT clipped in place.

One step count serves the whole set (``state_dict`` repeats it per parameter in AdamW's layout), so a parameter whose
gradient is ``None`` in some steps is skipped in those but shares the others' bias correction afterwards.

``ema_decay`` adds an exponential moving average of the weights to the same two launches: the update kernel lerps a fifth
stream towards each parameter's new value while that value is still in a register.  The weight of the lerp is formed on the
device from the count of APPLIED steps, so a step the guard skips leaves the average alone and does not advance the warm-up
ramp -- something an average kept by the host (``AveragedModel``, ``_foreach_lerp_``) cannot know without a sync per step.
``swap_ema()`` / ``ema_weights()`` exchange parameters and average in place, in one launch, to evaluate with the average.
"""
import contextlib

import numpy as np
import torch

from .. import _lib

# indices into the device state block: UD_OPTIM_ST_* of include/unidistill_hip.h
ST_LR, ST_STEP, ST_STEP_IN, ST_NORM, ST_COEF, ST_SKIPPED, ST_FINITE, STATE_DOUBLES = 0, 1, 2, 3, 4, 5, 6, 8
CHUNK_DTYPE = np.dtype([("offset", "<i8"), ("tensor", "<i4"), ("length", "<i4")])   # UdOptimChunk
RING_SLOTS = 8


def chunk_elems():
    """The kernels' compile-time chunk size in elements."""
    return int(_lib.load().ud_optim_chunk_elems())


def build_chunk_table(numels, chunk):
    """Chunk records for tensors of ``numels`` elements: every element of every tensor in exactly one chunk, no chunk across
    two tensors, a tensor's chunks in order with only the last one short.  Empty tensors get none.
    -> structured array (offset, tensor, length)."""
    numels = np.asarray(list(numels), dtype=np.int64)
    if chunk <= 0 or chunk > 2 ** 31 - 1:
        raise ValueError(f"chunk size {chunk}")
    if numels.size and numels.min() < 0:
        raise ValueError("negative element count")
    if numels.size > 2 ** 31 - 1:
        raise ValueError("too many tensors")
    per = (numels + chunk - 1) // chunk
    total = int(per.sum())
    if total > 2 ** 31 - 1:
        raise ValueError("too many chunks for one launch")
    table = np.zeros(total, dtype=CHUNK_DTYPE)
    tensor = np.repeat(np.arange(numels.size, dtype=np.int64), per)
    first = np.cumsum(per) - per                                   # index of each tensor's first chunk
    offset = (np.arange(total, dtype=np.int64) - first[tensor]) * chunk
    table["tensor"] = tensor
    table["offset"] = offset
    table["length"] = np.minimum(numels[tensor] - offset, chunk)
    return table


def _same_layout(g, p):
    """Same element order in memory: equal sizes and equal strides on every axis longer than 1."""
    return g.shape == p.shape and all(n == 1 or a == b for n, a, b in zip(p.shape, g.stride(), p.stride()))


class ClipAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` semantics with ``clip_grad_norm_(params, max_norm)`` folded in.  One parameter group, fp32
    parameters and gradients on one GPU.  ``max_norm=None`` disables clipping (the norm is still computed for the guard).
    ``last_norm`` / ``last_coef`` / ``skipped`` are device tensors; ``step()`` never synchronises with the device.

    ``ema_decay`` in (0, 1) keeps ``ema = lerp(ema, p, 1 - d)`` after every applied step, started from the parameters as they
    are at construction; ``d = ema_decay``, or with ``ema_ramp`` (> 0, in steps) ``d = ema_decay * (1 - exp(-n / ema_ramp))``
    with n the number of applied steps.  A parameter without a gradient is not stepped, but its average still moves towards
    it (as in ``torch.optim.swa_utils.AveragedModel``).  The average is not part of ``state_dict()``, which stays loadable
    by ``torch.optim.AdamW``: see ``ema_state_dict()``.  With ``ema_decay=None`` nothing of this exists."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None,
                 skip_nonfinite=True, ema_decay=None, ema_ramp=None):
        if not 0.0 <= lr:
            raise ValueError(f"invalid learning rate {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas {betas}")
        if not 0.0 <= eps:
            raise ValueError(f"invalid eps {eps}")
        if max_norm is not None and not max_norm > 0.0:
            raise ValueError(f"invalid max_norm {max_norm}")
        if ema_decay is None and ema_ramp is not None:
            raise ValueError("ema_ramp needs ema_decay")
        if ema_decay is not None and not 0.0 < ema_decay < 1.0:
            raise ValueError(f"invalid ema_decay {ema_decay}: must lie in (0, 1)")
        if ema_ramp is not None and not ema_ramp > 0.0:
            raise ValueError(f"invalid ema_ramp {ema_ramp}: must be > 0")
        # the torch.optim.AdamW keys ride along so that a checkpoint of this optimizer loads into AdamW(fused=True) as it is
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=True, decoupled_weight_decay=True,
                        max_norm=max_norm, skip_nonfinite=bool(skip_nonfinite))
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("ClipAdamW takes one parameter group")
        self._params = list(self.param_groups[0]["params"])
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_ramp = None if ema_ramp is None else float(ema_ramp)
        self.ema_swapped = False       # host flag: parameters and average currently stand in each other's place
        self.table_builds = 0          # chunk table + static pointer rows written to the device
        self.grad_uploads = 0          # gradient pointer rows sent through the pinned ring
        self._dev = None
        self._flat = None              # both moments (and the EMA): [2 or 3, padded element count], viewed per parameter
        self._static_ptrs = None
        self._grad_ptrs = None
        self._lr_on_device = None
        self._build()

    # ---- set-up ---------------------------------------------------------------------------------------------------------
    def _check_params(self):
        dev = self._params[0].device
        for p in self._params:
            if not p.is_cuda:
                raise RuntimeError(f"ClipAdamW runs on the GPU only (no CPU fallback); got a parameter on {p.device}")
            if p.device != dev:
                raise RuntimeError("ClipAdamW: all parameters must live on one device")
            if p.dtype != torch.float32:
                raise RuntimeError(f"ClipAdamW: parameters must be fp32 (they stay fp32 under autocast); got {p.dtype}")
            if p.is_sparse or not torch._prims_common.is_non_overlapping_and_dense(p):
                raise RuntimeError(f"ClipAdamW: parameter of shape {tuple(p.shape)} / strides {p.stride()} is not dense")
        return dev

    def _build(self):
        """(Re)build everything that depends on where the parameters live: chunk table, moments' views, static pointers."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClipAdamW: the device table would be rebuilt during graph capture "
                               "(take one eager step with the static buffers first)")
        dev = self._check_params()
        params = self._params
        T = len(params)
        first = self._dev is None
        ema = self.ema_decay is not None
        if first:
            numels = [p.numel() for p in params]
            self._chunk = chunk_elems()
            table = build_chunk_table(numels, self._chunk)
            self._n_chunks = len(table)
            self._table_host = table
            # each tensor's moments start on a 16-byte boundary of the flat allocation
            starts, cur = [], 0
            for n in numels:
                starts.append(cur)
                cur += (n + 3) // 4 * 4
            self._starts, self._flat_elems = starts, max(cur, 4)
            self._state = torch.zeros(STATE_DOUBLES, dtype=torch.float64, device=dev)
            self._flat = torch.zeros(3 if ema else 2, self._flat_elems, dtype=torch.float32, device=dev)
            self._ring = torch.zeros(RING_SLOTS, T, dtype=torch.int64).pin_memory()
            self._ring_np = self._ring.numpy()
            self._ring_events = [None] * RING_SLOTS
            self._ring_next = 0
        elif dev != self._dev:                  # module.to(other device): the moments and the counters follow
            self._state = self._state.to(dev)
            self._flat = self._flat.to(dev)
        self._dev = dev
        self._chunks_dev = torch.from_numpy(self._table_host.view(np.uint8).copy()).to(dev)
        self._partial = torch.zeros(max(self._n_chunks, 1), dtype=torch.float64, device=dev)
        self._exp_avg = [self._flat[0, s:s + p.numel()].as_strided(p.shape, p.stride(), s)
                         for p, s in zip(params, self._starts)]
        self._exp_avg_sq = [self._flat[1, s:s + p.numel()].as_strided(p.shape, p.stride(), self._flat_elems + s)
                            for p, s in zip(params, self._starts)]
        self._strides = [p.stride() for p in params]
        ptrs = np.zeros((5 if ema else 4, T), dtype=np.int64)   # rows: parameter, exp_avg, exp_avg_sq, gradient(, EMA)
        ptrs[0] = [p.data_ptr() for p in params]
        ptrs[1] = [m.data_ptr() for m in self._exp_avg]
        ptrs[2] = [v.data_ptr() for v in self._exp_avg_sq]
        if ema:
            self._ema = [self._flat[2, s:s + p.numel()].as_strided(p.shape, p.stride(), 2 * self._flat_elems + s)
                         for p, s in zip(params, self._starts)]
            ptrs[4] = [e.data_ptr() for e in self._ema]
            if first:
                self.reset_ema()
        self._static_ptrs = ptrs[0].tolist()
        self._ptrs_dev = torch.from_numpy(ptrs).to(dev)
        self._grad_ptrs = [0] * T
        self._lr_on_device = None
        self.last_norm = self._state[ST_NORM]
        self.last_coef = self._state[ST_COEF]
        self.skipped = self._state[ST_SKIPPED]
        self.steps_done = self._state[ST_STEP]
        self.table_builds += 1

    def _gradient_pointers(self):
        ptrs = []
        for p, st in zip(self._params, self._strides):
            g = p.grad
            if g is None:
                ptrs.append(0)
                continue
            if g.dtype != torch.float32 or g.device != p.device or g.is_sparse:
                raise RuntimeError(f"ClipAdamW: gradients must be dense fp32 on the parameter's device; got {g.dtype} "
                                   f"on {g.device} for a parameter of shape {tuple(p.shape)}")
            if g.stride() != st and not _same_layout(g, p):
                raise RuntimeError(f"ClipAdamW: gradient strides {g.stride()} do not follow the parameter's {p.stride()} "
                                   f"(shape {tuple(p.shape)})")
            ptrs.append(g.data_ptr())
        return ptrs

    def _upload_gradient_pointers(self, ptrs):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClipAdamW: gradient pointers changed during graph capture (keep the gradients in static "
                               "buffers and take one eager step with them first)")
        slot = self._ring_next
        self._ring_next = (slot + 1) % RING_SLOTS
        ev = self._ring_events[slot]
        if ev is not None and not ev.query():
            ev.synchronize()           # the copy out of this slot, RING_SLOTS steps ago, has not run yet: do not overwrite it
        self._ring_np[slot, :] = ptrs
        self._ptrs_dev[3].copy_(self._ring[slot], non_blocking=True)
        if ev is None:
            ev = self._ring_events[slot] = torch.cuda.Event()
        ev.record()
        self._grad_ptrs = ptrs
        self.grad_uploads += 1

    def _revalidate(self):
        if [p.data_ptr() for p in self._params] != self._static_ptrs or self._params[0].device != self._dev:
            self._build()              # .to() / a reload moved the parameters

    # ---- the step -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        if self.ema_swapped:
            raise RuntimeError("ClipAdamW: step() while the EMA is swapped in would train the average; swap_ema() back first")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise RuntimeError("ClipAdamW: amsgrad / maximize are not implemented")
        self._revalidate()
        with torch.cuda.device(self._dev):
            ptrs = self._gradient_pointers()
            if ptrs != self._grad_ptrs:
                self._upload_gradient_pointers(ptrs)
            lr = float(group["lr"])
            if lr != self._lr_on_device:
                self._state[ST_LR].fill_(lr)
                self._lr_on_device = lr
            if self._n_chunks:
                stream = _lib.stream_of(self._state)
                pd = self._ptrs_dev
                row = pd.stride(0) * 8
                base = pd.data_ptr()
                _lib.ud.ud_optim_sqnorm(self._chunks_dev.data_ptr(), self._n_chunks, base + 3 * row, self._partial.data_ptr(),
                                        self._state.data_ptr(), stream)
                max_norm = group.get("max_norm")
                b1, b2 = group["betas"]
                max_norm = float("inf") if max_norm is None else float(max_norm)
                skip = 1 if group.get("skip_nonfinite", True) else 0
                if self.ema_decay is None:
                    _lib.ud.ud_optim_clip_adamw(self._chunks_dev.data_ptr(), self._n_chunks, base, base + row, base + 2 * row,
                                                base + 3 * row, self._partial.data_ptr(), self._state.data_ptr(), float(b1),
                                                float(b2), float(group["eps"]), float(group["weight_decay"]), max_norm, skip,
                                                stream)
                else:
                    _lib.ud.ud_optim_clip_adamw_ema(self._chunks_dev.data_ptr(), self._n_chunks, base, base + row,
                                                    base + 2 * row, base + 4 * row, base + 3 * row, self._partial.data_ptr(),
                                                    self._state.data_ptr(), float(b1), float(b2), float(group["eps"]),
                                                    float(group["weight_decay"]), max_norm, skip, self.ema_decay,
                                                    0.0 if self.ema_ramp is None else self.ema_ramp, stream)
        return loss

    # ---- the weight average ---------------------------------------------------------------------------------------------
    def _need_ema(self):
        if self.ema_decay is None:
            raise RuntimeError("ClipAdamW: no EMA is kept (construct with ema_decay=...)")

    def ema_params(self):
        """The average, one view per parameter in registration order, shaped and strided like it.  (While ``ema_swapped``
        these hold the training weights.)"""
        self._need_ema()
        self._revalidate()
        return list(self._ema)

    @torch.no_grad()
    def reset_ema(self):
        """Restart the average from the parameters' present values."""
        self._need_ema()
        if self.ema_swapped:
            raise RuntimeError("ClipAdamW: reset_ema() while the EMA is swapped in")
        for e, p in zip(self._ema, self._params):
            e.copy_(p)

    @torch.no_grad()
    def swap_ema(self):
        """Exchange parameters and average in place, bit for bit, in one launch; flips ``ema_swapped``.  The exchange goes
        through raw pointers: no version counter moves, so whoever caches something derived from the weights must drop it
        (``Trainer.ema_weights`` does)."""
        self._need_ema()
        self._revalidate()
        with torch.cuda.device(self._dev):
            if self._n_chunks:
                pd = self._ptrs_dev
                _lib.ud.ud_optim_swap(self._chunks_dev.data_ptr(), self._n_chunks, pd.data_ptr(),
                                      pd.data_ptr() + 4 * pd.stride(0) * 8, _lib.stream_of(self._state))
        self.ema_swapped = not self.ema_swapped

    @contextlib.contextmanager
    def ema_weights(self):
        """``with opt.ema_weights():`` the parameters hold the average; they are swapped back on the way out, always."""
        self.swap_ema()
        try:
            yield
        finally:
            self.swap_ema()

    def ema_state_dict(self):
        """The average for a checkpoint (copies, in registration order).  Kept apart from ``state_dict()``, which has to stay
        loadable by ``torch.optim.AdamW``; the ramp's position is the optimizer's step count and travels there."""
        self._need_ema()
        if self.ema_swapped:
            raise RuntimeError("ClipAdamW: ema_state_dict() while the EMA is swapped in")
        self._revalidate()
        return {"decay": self.ema_decay, "ramp": self.ema_ramp, "params": [e.detach().clone() for e in self._ema]}

    @torch.no_grad()
    def load_ema_state_dict(self, state):
        """Values only: decay and ramp stay the constructor's."""
        self._need_ema()
        if self.ema_swapped:
            raise RuntimeError("ClipAdamW: load_ema_state_dict() while the EMA is swapped in")
        self._revalidate()
        values = state["params"]
        if len(values) != len(self._ema):
            raise ValueError(f"EMA checkpoint holds {len(values)} tensors, the optimizer {len(self._ema)}")
        for i, (e, x) in enumerate(zip(self._ema, values)):
            if tuple(x.shape) != tuple(e.shape):
                raise ValueError(f"EMA checkpoint tensor {i} has shape {tuple(x.shape)}, the parameter {tuple(e.shape)}")
        for e, x in zip(self._ema, values):
            e.copy_(x)

    # ---- checkpoints in torch.optim.AdamW's layout ----------------------------------------------------------------------
    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)     # a torch.optim.AdamW checkpoint knows nothing of max_norm / skip_nonfinite

    def state_dict(self):
        """``exp_avg`` / ``exp_avg_sq`` (the live moments, as with torch) and ``step`` (an fp32 device scalar) per parameter."""
        if self.ema_swapped:
            raise RuntimeError("ClipAdamW: state_dict() while the EMA is swapped in")
        step = self._state[ST_STEP].to(torch.float32)
        for i, p in enumerate(self._params):
            self.state[p] = {"step": step.clone(), "exp_avg": self._exp_avg[i], "exp_avg_sq": self._exp_avg_sq[i]}
        try:
            return super().state_dict()
        finally:
            self.state.clear()

    def load_state_dict(self, state_dict):
        if self.ema_swapped:
            raise RuntimeError("ClipAdamW: load_state_dict() while the EMA is swapped in")
        super().load_state_dict(state_dict)
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize"):
            raise RuntimeError("ClipAdamW: cannot load an amsgrad / maximize checkpoint")
        self._params = list(group["params"])
        if [p.data_ptr() for p in self._params] != self._static_ptrs:
            self._build()
        steps = []
        with torch.no_grad():
            for i, p in enumerate(self._params):
                st = self.state.get(p) or {}
                if not st:                     # torch keeps no state for a parameter that never had a gradient
                    self._exp_avg[i].zero_()
                    self._exp_avg_sq[i].zero_()
                    continue
                self._exp_avg[i].copy_(st["exp_avg"])
                self._exp_avg_sq[i].copy_(st["exp_avg_sq"])
                steps.append(torch.as_tensor(st["step"]).to(device=self._dev, dtype=torch.float64).reshape(()))
            if steps:
                steps = torch.stack(steps)
                if bool((steps != steps[0]).any()):    # (loading may wait for the device; step() never does)
                    raise RuntimeError("ClipAdamW keeps one step count for the whole set; the checkpoint has "
                                       f"{sorted(set(steps.tolist()))}")
                self._state[ST_STEP].copy_(steps[0])
            else:
                self._state[ST_STEP].zero_()
        self.state.clear()
        self._lr_on_device = None
