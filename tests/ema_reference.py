"""float64 numpy restatement of the weight EMA that ``unidistill_amd.ops.optim.ClipAdamW(ema_decay=...)`` keeps: the yardstick
of tests/test_optim_ema_cpu.py and tests/test_optim_ema_gpu.py.

After every APPLIED step n = 1, 2, ... (a step the non-finite-gradient guard skips is not one and does not advance n)

    e <- e + w_n * (p - e),    w_n = 1 - d_n,    d_n = decay                             (constant mode)
                                                 d_n = decay * (1 - exp(-n / ramp))      (ramp mode)

for every tensor, also one without a gradient in that step (its p is simply unchanged).  The average starts at the initial
parameters.  Arrays are flat or shaped float64; the arithmetic is elementwise, so any consistent element order will do."""
import math

import numpy as np

from optim_reference import ClipAdamWReference


class EmaReference:
    def __init__(self, params, decay, ramp=None):
        self.e = [np.array(p, dtype=np.float64) for p in params]
        self.decay, self.ramp = float(decay), None if ramp is None else float(ramp)
        self.n = 0                                  # applied steps so far

    def weight(self, n):
        """w_n of the n-th applied step (n >= 1)."""
        d = self.decay if self.ramp is None else self.decay * (1.0 - math.exp(-n / self.ramp))
        return 1.0 - d

    def update(self, params, applied=True):
        """params: every tensor's value after the step.  applied=False: the step was skipped, nothing moves."""
        if not applied:
            return
        self.n += 1
        w = self.weight(self.n)
        for i, p in enumerate(params):
            self.e[i] = self.e[i] + w * (np.asarray(p, dtype=np.float64) - self.e[i])


class ClipAdamWEmaReference(ClipAdamWReference):
    """``ClipAdamWReference`` with the average riding along: ``ema.e`` after every ``step``."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, skip_nonfinite=True,
                 ema_decay=0.999, ema_ramp=None):
        super().__init__(params, lr, betas, eps, weight_decay, max_norm, skip_nonfinite)
        self.ema = EmaReference(self.p, ema_decay, ema_ramp)

    def step(self, grads):
        before = self.step_count
        super().step(grads)
        self.ema.update(self.p, applied=self.step_count > before)
