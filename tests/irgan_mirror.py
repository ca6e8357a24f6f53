"""IRGAN (model/ranking/IRGAN.py) in float64 numpy: every formula of the reference's loop, one function each, and ``Mirror``, the
whole training loop over them.  The CPU tests hold it to the reference's recorded run (tests/golden/tf_irgan_*.npz); the GPU tests
hold the kernels of csrc/irgan.hip to it.  ``dtype=np.float32`` evaluates the distribution functions as the reference's host code
does (float32 arithmetic), for the band checks of the draw tests."""
import numpy as np

TEMPERATURE = 0.2          # IRGAN.py:88
SAMPLE_LAMBDA = 0.2        # IRGAN.py:143
NEG_PER_POS, GEN_PER_POS, GEN_PASSES = 2, 3, 5


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def logits(P, Q, b, u, dtype=np.float64):
    return (Q.astype(dtype) @ P[u].astype(dtype) + b.astype(dtype)).astype(dtype)


def negative_weights(z, pos, T=TEMPERATURE, shift=True):
    """get_data: w = exp(z / T), 0 at the positives (IRGAN.py:88-91).  ``shift`` subtracts the row maximum first (the device does):
    prob = w / sum(w) is the same either way"""
    zt = z / z.dtype.type(T)
    w = np.exp(zt - zt.max() if shift else zt)
    w[np.asarray(pos)] = 0
    return w


def mixture(z, pos, lam=SAMPLE_LAMBDA):
    """the generator's sampling distribution (IRGAN.py:148-153): p = softmax(z), pn = (1 - lam) p, plus lam / |pos| at the positives"""
    e = np.exp(z - z.max())
    p = e / e.sum()
    pn = z.dtype.type(1 - lam) * p
    pn[np.asarray(pos)] += z.dtype.type(lam * 1.0 / len(pos))
    return p, pn


def cdf(w):
    """np.random.choice's CDF: float64 cumsum, normalised by its last element"""
    c = np.cumsum(w.astype(np.float64))
    return c / c[-1]


def draw(w, x):
    """np.random.choice(n, size, p=w / sum(w)) given its uniforms ``x`` (= np.random.random_sample(size))"""
    return np.searchsorted(cdf(w), x, side="right")


def reward(Pd, Qd, bd, u, samples, p, pn):
    """IRGAN.py:160-162"""
    s = np.asarray(samples)
    return 2 * (sigmoid(Qd[s] @ Pd[u] + bd[s]) - 0.5) * p[s] / pn[s]


def generator_gradients(P, Q, b, u, samples, rew, lam):
    """loss and gradients of gan_loss (IRGAN.py:36-39) for one user: dict(loss, g [n_items], gP (row u), gQ, gb)"""
    s = np.asarray(samples); K = s.size; ni = Q.shape[0]
    z = Q @ P[u] + b
    e = np.exp(z - z.max()); p = e / e.sum()
    c = np.zeros(ni); np.add.at(c, s, rew)
    n = np.bincount(s, minlength=ni).astype(np.float64)
    R = rew.sum()
    g = -(c - R * p) / K
    loss = -np.mean(np.log(p[s]) * rew) + lam * 0.5 * ((P[u] ** 2).sum() + (Q[s] ** 2).sum() + (b[s] ** 2).sum())
    return dict(loss=loss, g=g, n=n, gP=g @ Q + lam * P[u], gQ=np.outer(g, P[u]) + lam * n[:, None] * Q, gb=g + lam * n * b)


def discriminator_gradients(P, Q, b, u, i, y, lam, per_slot_regulariser=True):
    """pre_loss is a [B] VECTOR (IRGAN.py:66-68: the bce vector plus the scalar regulariser), minimize differentiates its sum: the
    regulariser enters B times, once per occurrence of a row.  ``per_slot_regulariser=False`` is the scalar-loss reading (lambda
    instead of B lambda), kept so that a test can show the fixture refuses it.  Returns dict(loss (the sum), dz, gP, gQ, gb)."""
    u = np.asarray(u); i = np.asarray(i); y = np.asarray(y, np.float64); B = u.size
    x = (P[u] * Q[i]).sum(1) + b[i]
    dz = sigmoid(x) - y
    bl = (B if per_slot_regulariser else 1) * lam
    gP = np.zeros_like(P); gQ = np.zeros_like(Q); gb = np.zeros_like(b)
    np.add.at(gP, u, dz[:, None] * Q[i] + bl * P[u])
    np.add.at(gQ, i, dz[:, None] * P[u] + bl * Q[i])
    np.add.at(gb, i, dz + bl * b[i])
    bce = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
    loss = bce.sum() + bl * 0.5 * ((P[u] ** 2).sum() + (Q[i] ** 2).sum() + (b[i] ** 2).sum())
    return dict(loss=loss, dz=dz, gP=gP, gQ=gQ, gb=gb)


class Adam:
    """tf.train.AdamOptimizer over a list of dense variables (one pair of beta powers)"""

    def __init__(self, variables, lr, b1=0.9, b2=0.999, eps=1e-8):
        self.vars = variables
        self.m = [np.zeros_like(v) for v in variables]; self.v = [np.zeros_like(v) for v in variables]
        self.lr, self.b1, self.b2, self.eps, self.b1p, self.b2p = lr, b1, b2, eps, b1, b2

    def step(self, grads):
        alpha = self.lr * np.sqrt(1 - self.b2p) / (1 - self.b1p)
        for x, m, v, g in zip(self.vars, self.m, self.v, grads):
            m += (g - m) * (1 - self.b1)
            v += (g * g - v) * (1 - self.b2)
            x -= m * alpha / (np.sqrt(v) + self.eps)
        self.b1p *= self.b1; self.b2p *= self.b2


def get_data_rows(order, pos, negatives):
    """the rows get_data returns (IRGAN.py:93-100): per user of ``order`` its positives with label 1, then its negatives with label 0"""
    us, it, lab = [], [], []
    for u, neg in zip(order, negatives):
        us += [u] * (len(pos[u]) + len(neg)); it += list(pos[u]) + list(neg); lab += [1.0] * len(pos[u]) + [0.0] * len(neg)
    return np.array(us, np.int32), np.array(it, np.int32), np.array(lab, np.float32)


def discriminator_batches(rows, train_size, batch_size):
    """IRGAN.py:127-133: only the FIRST ``train_size`` rows are consumed, in batches of ``batch_size``; the last holds the rest"""
    u, i, y = rows
    return [(u[a:min(a + batch_size, train_size)], i[a:min(a + batch_size, train_size)], y[a:min(a + batch_size, train_size)])
            for a in range(0, train_size, batch_size)]


class Mirror:
    """the six variables and the two optimizers; ``pos``: user id -> rated item ids in the reference's order"""

    def __init__(self, init, lr, lam, per_slot_regulariser=True):
        self.p = {k: np.array(v, np.float64) for k, v in init.items()}
        self.lam, self.per_slot = lam, per_slot_regulariser
        self.g_opt = Adam([self.p[k] for k in ("g_P", "g_Q", "g_b")], lr)
        self.d_opt = Adam([self.p[k] for k in ("d_P", "d_Q", "d_b")], lr)

    def negatives_weights(self, u, pos):
        return negative_weights(logits(self.p["g_P"], self.p["g_Q"], self.p["g_b"], u), pos)

    def discriminator_step(self, u, i, y):
        r = discriminator_gradients(self.p["d_P"], self.p["d_Q"], self.p["d_b"], u, i, y, self.lam, self.per_slot)
        self.d_opt.step([r["gP"], r["gQ"], r["gb"]])
        return r

    def generator_step(self, u, pos, samples):
        p = self.p
        pr, pn = mixture(logits(p["g_P"], p["g_Q"], p["g_b"], u), pos)
        rew = reward(p["d_P"], p["d_Q"], p["d_b"], u, samples, pr, pn)
        r = generator_gradients(p["g_P"], p["g_Q"], p["g_b"], u, samples, rew, self.lam)
        gP = np.zeros_like(p["g_P"]); gP[u] = r["gP"]
        r.update(reward=rew, p=pr, pn=pn, gP_full=gP)
        self.g_opt.step([gP, r["gQ"], r["gb"]])
        return r

    def snapshot(self):
        return {k: v.copy() for k, v in self.p.items()}
