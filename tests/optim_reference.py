"""float64 numpy restatement of ``clip_grad_norm_`` + decoupled-weight-decay AdamW over a list of tensors, with the
skip rule of ``unidistill_amd.ops.optim.ClipAdamW``: the yardstick of tests/test_optim_cpu.py and tests/test_optim_gpu.py.

Arrays are flat or shaped float64; the arithmetic is elementwise, so any consistent element order will do."""
import numpy as np


class ClipAdamWReference:
    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, skip_nonfinite=True):
        self.p = [np.array(p, dtype=np.float64) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), betas, float(eps), float(weight_decay)
        self.max_norm, self.skip_nonfinite = max_norm, skip_nonfinite
        self.step_count = 0
        self.skipped = 0
        self.total_norm = None
        self.coef = None

    def step(self, grads):
        """grads: one array (or None: parameter skipped, nothing to the norm) per parameter."""
        grads = [None if g is None else np.asarray(g, dtype=np.float64) for g in grads]
        with np.errstate(all="ignore"):
            self.total_norm = float(np.sqrt(sum(float((g * g).sum()) for g in grads if g is not None)))
            coef = 1.0 if self.max_norm is None else self.max_norm / (self.total_norm + 1e-6)
            self.coef = coef if np.isnan(coef) else min(1.0, coef)
            if self.skip_nonfinite and not np.isfinite(self.total_norm):
                self.skipped += 1
                return
            self.step_count += 1
            b1, b2 = self.betas
            bc1 = 1.0 - b1 ** self.step_count
            bc2 = 1.0 - b2 ** self.step_count
            for i, g in enumerate(grads):
                if g is None:
                    continue
                g = g * self.coef
                self.p[i] = self.p[i] * (1.0 - self.lr * self.weight_decay)
                self.m[i] = self.m[i] + (1.0 - b1) * (g - self.m[i])
                self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
                self.p[i] = self.p[i] - self.lr / bc1 * self.m[i] / (np.sqrt(self.v[i]) / np.sqrt(bc2) + self.eps)
