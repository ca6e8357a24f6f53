"""TF-1.14 Adam as every trainer here applies it (training/adam.py + ApplyAdam): the beta powers are fp32 variables,
alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power) is evaluated in fp32, and the powers are multiplied AFTER the update.
Every parity statement of the project rests on this expression rounding as TF's does; it is stated here and nowhere else."""
from __future__ import annotations

import numpy as np

from . import capi          # the device library itself loads on the first call, not on import

f = np.float32


class AdamClock:
    """the host side of one tf.train.AdamOptimizer, for steps whose update runs inside a kernel of their own (IRGAN, CFGAN):
    ``alpha()`` for the step about to run, ``advance()`` once it is enqueued"""

    def __init__(self, lr: float, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8):
        self.lr, self.b1, self.b2, self.eps = f(lr), f(b1), f(b2), f(eps)
        self.b1p, self.b2p = self.b1, self.b2

    def alpha(self) -> float:
        return float(f(self.lr * np.sqrt(f(1) - self.b2p, dtype=f) / (f(1) - self.b1p)))

    def advance(self):
        self.b1p = f(self.b1p * self.b1); self.b2p = f(self.b2p * self.b2)


class Adam(AdamClock):
    """one variable's slots and the dense update (qrec_adam_step) over its first ``n`` elements (default: all of ``theta``;
    the row-partitioned trainers leave the pad rows of their block out)"""

    def __init__(self, theta, lr: float, n: int | None = None):
        super().__init__(lr)
        self.theta = theta
        self.m = capi.DeviceBuffer.zeros(theta.shape, np.float32); self.v = capi.DeviceBuffer.zeros(theta.shape, np.float32)
        self.n = int(np.prod(theta.shape)) if n is None else int(n)
        self.last = None

    def step(self, grad, grad_scale=1.0, stream=None, grad_l2=0.0):
        capi.adam_step(self.theta, self.m, self.v, grad, self.n, grad_scale, self.alpha(), float(self.b1), float(self.b2),
                       float(self.eps), stream, grad_l2=grad_l2)
        self.advance()
        self.last = (grad, grad_scale, grad_l2)

    def applied_gradient(self, before=None):
        """Host copy of what the last ``step`` handed to Adam, BEFORE the update (the gradient buffer survives until the next
        step): grad_scale * grad + grad_l2 * theta, theta the variable when the step started (``before``, padded like the
        buffer; needed only when grad_l2 != 0: the kernel forms that term from theta itself).  Parity tests compare this with
        the gradients the reference's ``minimize`` applied (tests/golden/tf_*.npz: grad<k>_<var>), before Adam's normalisation
        amplifies noise."""
        buf, scale, l2 = self.last
        g = buf.numpy().astype(np.float32) * np.float32(scale)
        if l2:
            if before is None:
                raise ValueError("this gradient has a full-table L2 part: pass the variable's value at the start of the step")
            g = g + np.float32(l2) * np.asarray(before, np.float32)
        return g
