"""APR in numpy, written from the equations of include/qrec_hip.h (the APR section): the perturbation update, the step on two
objectives, TF-1.14 Adam and the whole two-phase run.  Evaluated in float64 (the comparison point of the kernels) or in float32
with the class-ordered sums of csrc/ordered.hip (np.add.at walks its index array in order: a row's slots in ascending slot
order, one lookup at a time, the lookups' sums added afterwards).

Tables here are joint: E = [U; V] ([n_users + n_items, d]), D the perturbations in the same layout; item row = n_users + item."""
import numpy as np

LN2 = float(np.log(2.0))


def softplus(z):
    return np.maximum(z, 0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid_neg(x):
    """sigma(-x) = 1 / (1 + e^x), without overflow warnings"""
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(x))


def _rows(E, D, nu, u, i, j, dt):
    E = np.asarray(E, dt)
    u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
    p, qi, qj = E[u], E[nu + i], E[nu + j]
    if D is None:
        return p, qi, qj, p, None
    D = np.asarray(D, dt)
    pa = p + D[u]
    da = (qi + D[nu + i]) - (qj + D[nu + j])
    return p, qi, qj, pa, da


def perturb(E, D, nu, u, v, n, reg_adv, eps, dt=np.float64):
    """the perturbations after one update on the feeds (u, v, n): eps * l2_normalize(Gamma) at the batch's rows, zero elsewhere"""
    dt = np.dtype(dt).type
    u, v, n = (np.asarray(a, np.int64) for a in (u, v, n))
    _, _, _, pa, da = _rows(E, D, nu, u, v, n, dt)
    c = -dt(reg_adv) * sigmoid_neg((pa * da).sum(1, dtype=dt)).astype(dt)
    w = c[:, None] * pa
    G = np.zeros(np.shape(E), dt)
    Gv, Gn = np.zeros_like(G), np.zeros_like(G)
    np.add.at(G, u, c[:, None] * da)
    np.add.at(Gv, nu + v, w)
    np.add.at(Gn, nu + n, -w)
    G = G + (Gv + Gn)
    ss = (G * G).sum(1, keepdims=True, dtype=dt)
    return ((G * (dt(1) / np.sqrt(np.maximum(ss, dt(1e-12))))) * dt(eps) + dt(0)).astype(dt)


def step(E, D, nu, u, i, j, reg, reg_adv, dt=np.float64):
    """(losses [3] = sum softplus(-x), reg (l2_loss(p_u) + l2_loss(q_i)), reg_adv sum softplus(-x'); dE) -- D None or reg_adv 0: no
    perturbed term"""
    dt = np.dtype(dt).type
    u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
    adv = D is not None and reg_adv != 0
    p, qi, qj, pa, da = _rows(E, D if adv else None, nu, u, i, j, dt)
    x = (p * (qi - qj)).sum(1, dtype=dt)
    g = -sigmoid_neg(x).astype(dt)
    losses = [float(softplus(-x).sum(dtype=np.float64)), float(0.5 * reg * ((p * p).sum(dtype=np.float64) + (qi * qi).sum(dtype=np.float64))), 0.0]
    du = g[:, None] * (qi - qj) + dt(reg) * p
    di = g[:, None] * p + dt(reg) * qi
    dj = -(g[:, None] * p)
    if adv:
        xa = (pa * da).sum(1, dtype=dt)
        c = -dt(reg_adv) * sigmoid_neg(xa).astype(dt)
        losses[2] = float(reg_adv * softplus(-xa).sum(dtype=np.float64))
        w = c[:, None] * pa
        du = du + c[:, None] * da; di = di + w; dj = dj - w
    dE = np.zeros(np.shape(E), dt)
    Gi, Gj = np.zeros_like(dE), np.zeros_like(dE)
    np.add.at(dE, u, du)
    np.add.at(Gi, nu + i, di)
    np.add.at(Gj, nu + j, dj)
    return np.array(losses, np.float64), dE + (Gi + Gj)


class Adam:
    """training/adam.py + ApplyAdam in the float type ``dt`` on one dense variable: the beta powers are kept in that type and advance
    after the update"""

    def __init__(self, lr, dt=np.float64):
        self.dt = dt = np.dtype(dt).type
        self.lr, self.b1, self.b2, self.eps = dt(lr), dt(0.9), dt(0.999), dt(1e-8)
        self.b1p, self.b2p = self.b1, self.b2
        self.m = self.v = None

    def step(self, theta, g):
        dt = self.dt
        alpha = dt(self.lr * np.sqrt(dt(1) - self.b2p, dtype=dt) / (dt(1) - self.b1p))
        g = np.asarray(g, dt)
        if self.m is None:
            self.m, self.v = np.zeros_like(g), np.zeros_like(g)
        self.m += (g - self.m) * (dt(1) - self.b1)
        self.v += (g * g - self.v) * (dt(1) - self.b2)
        out = np.asarray(theta, dt) - (self.m * alpha) / (np.sqrt(self.v) + self.eps)
        self.b1p, self.b2p = dt(self.b1p * self.b1), dt(self.b2p * self.b2)
        return out


def perturb_feeds(mode, u, i, j):
    """what the perturbation update is fed as (u, v, n): the reference file feeds the negatives twice (APR.py:116-117)"""
    if mode == "reference":
        return u, j, j
    if mode == "paper":
        return u, i, j
    raise ValueError(mode)


def train(E0, nu, batches, n_pretrain, lr, reg, reg_adv, eps, mode, dt=np.float64):
    """the whole run over ``batches`` = [(u, i, j), ...]: the first ``n_pretrain`` are pretraining steps, every later one is a
    perturbation update followed by the adversarial step, ONE Adam across both (APR.py:67-70).  Returns a dict: E, D, losses
    (total_loss in pretraining, loss_adv after), the first gradient of each phase with the table it started from, D after the
    first and after the last update."""
    dt = np.dtype(dt).type
    E, D = np.asarray(E0, dt).copy(), np.zeros(np.shape(E0), dt)
    opt = Adam(lr, dt)
    out = dict(losses=[], grad0=None, grad1=None, pre1=None, D_first=None, D_all_zero=True)
    for k, (u, i, j) in enumerate(batches):
        if k < n_pretrain:
            L, g = step(E, None, nu, u, i, j, reg, 0.0, dt)
            if out["grad0"] is None:
                out["grad0"] = g
        else:
            D = perturb(E, D, nu, *perturb_feeds(mode, u, i, j), reg_adv, eps, dt)
            out["D_all_zero"] = out["D_all_zero"] and not D.any()
            if out["D_first"] is None:
                out["D_first"] = D.copy()
            L, g = step(E, D, nu, u, i, j, reg, reg_adv, dt)
            if out["grad1"] is None:
                out["grad1"], out["pre1"] = g, E.copy()
        out["losses"].append(float(L.sum()))
        E = opt.step(E, g)
    out.update(E=E, D=D, losses=np.array(out["losses"], np.float64))
    return out
