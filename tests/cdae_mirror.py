"""CDAE (model/ranking/CDAE.py:51-105) restated in numpy, in any float type: the training step in the DENSE form the reference writes
(four batch x n_items arrays, two dense products) and in the SPARSE form the device kernels evaluate (kept inputs and live loss
positions only), TF-1.14 Adam, the scores of predictForRanking, and the draw loop of next_batch in plain Python.

Parameters are a dict in the reference's shapes: W_enc [n_items, nh], W_dec [nh, n_items], b_enc [nh], b_dec [n_items], V [n_users, nh].
Gradients are what ``minimize`` applies: the reg * theta terms are in (V's per occurrence of a user in the batch)."""
import numpy as np

VARS = ("W_enc", "W_dec", "b_enc", "b_dec", "V")
CLAMP = 1e-6


def sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def cast(p, dt):
    return {k: np.asarray(v, dt) for k, v in p.items()}


def _reg(p, users, reg, dt):
    l2 = lambda a: (a * a).sum(dtype=dt) / dt(2)
    Vu = p["V"][users]
    return dt(reg) * (l2(p["W_enc"]) + l2(p["W_dec"]) + l2(p["b_enc"]) + l2(p["b_dec"])) + dt(reg) * l2(Vu)


def dense_step(p, users, X, positive, negative, mask, reg, dt=np.float64):
    """(loss, grads) exactly as CDAE.py:71-82 composes them.  An unsampled position whose output is exactly 1.0 gives
    0 * log(0) = NaN here, as in the reference; the sparse form never visits it."""
    p = cast(p, dt); X, positive, negative, mask = (np.asarray(a, dt) for a in (X, positive, negative, mask))
    users = np.asarray(users); B, n = X.shape
    x = mask * X
    h = sig(x @ p["W_enc"] + p["b_enc"] + p["V"][users])
    y = sig(h @ p["W_dec"] + p["b_dec"])
    ym = y * mask
    passed = ym >= dt(CLAMP)
    yc = np.where(passed, ym, dt(CLAMP))
    yp, yn = positive * mask, negative * mask
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = -yp * np.log(yc) - yn * np.log(dt(1) - yc)
        loss = terms.mean(dtype=dt) + _reg(p, users, reg, dt)
        dyc = (-yp / yc + yn / (dt(1) - yc)) / dt(B * n)
    ds = dyc * passed * mask * y * (dt(1) - y)
    dh = ds @ p["W_dec"].T
    dz = dh * h * (dt(1) - h)
    gV = np.zeros_like(p["V"]); np.add.at(gV, users, dz + dt(reg) * p["V"][users])
    grads = dict(W_enc=x.T @ dz + dt(reg) * p["W_enc"], W_dec=h.T @ ds + dt(reg) * p["W_dec"], b_enc=dz.sum(0) + dt(reg) * p["b_enc"],
                 b_dec=ds.sum(0) + dt(reg) * p["b_dec"], V=gV)
    return loss, grads


def sparse_parts(p, L, reg, dt=np.float64):
    """the sparse evaluation over the lists ``L`` (qrec_amd.autoencoder.BatchLists, host): everything the kernels produce --
    h, the logits, g per live slot, dz, the loss and the gradients"""
    p = cast(p, dt); B, n = L.B, L.n_items
    users = np.asarray(L.users)
    Wd = np.ascontiguousarray(p["W_dec"].T)                                  # item-major
    in_row = np.repeat(np.arange(B), np.diff(L.in_ptr)); lv_row = np.repeat(np.arange(B), np.diff(L.lv_ptr))
    z = np.zeros((B, p["b_enc"].size), dt)
    np.add.at(z, in_row, np.asarray(L.in_val, dt)[:, None] * p["W_enc"][L.in_item])
    h = sig(z + p["b_enc"] + p["V"][users])
    s = (h[lv_row] * Wd[L.lv_item]).sum(1) + p["b_dec"][L.lv_item]
    y = sig(s)
    passed = y >= dt(CLAMP)
    yc = np.where(passed, y, dt(CLAMP))
    pos = np.asarray(L.lv_label) != 0
    with np.errstate(divide="ignore"):
        terms = np.where(pos, -np.log(yc), -np.log(dt(1) - yc))
    g = np.where(pos, -(dt(1) - y), y) * passed / dt(B * n)
    loss = terms.sum(dtype=dt) / dt(B * n) + _reg(p, users, reg, dt)
    dh = np.zeros_like(h); np.add.at(dh, lv_row, g[:, None] * Wd[L.lv_item])
    dz = dh * h * (dt(1) - h)
    gWd = np.zeros_like(Wd); np.add.at(gWd, L.lv_item, g[:, None] * h[lv_row])
    gbd = np.zeros_like(p["b_dec"]); np.add.at(gbd, L.lv_item, g)
    gWe = np.zeros_like(p["W_enc"]); np.add.at(gWe, L.in_item, np.asarray(L.in_val, dt)[:, None] * dz[in_row])
    gV = np.zeros_like(p["V"]); np.add.at(gV, users, dz + dt(reg) * p["V"][users])
    raw = dict(W_enc=gWe, W_dec=gWd.T, b_enc=dz.sum(0), b_dec=gbd, V=gV)              # without reg * theta of the four weights
    grads = dict(raw, **{k: raw[k] + dt(reg) * p[k] for k in VARS[:4]})
    return dict(h=h, logits=s, g=g, dz=dz, loss=loss, grads=grads, raw=raw)


def sparse_step(p, L, reg, dt=np.float64):
    r = sparse_parts(p, L, reg, dt)
    return r["loss"], r["grads"]


class Adam:
    """training/adam.py + ApplyAdam in the float type ``dt``: the beta powers are kept in that type and advance after the update"""

    def __init__(self, lr, dt=np.float64):
        self.dt = dt
        self.lr, self.b1, self.b2, self.eps = dt(lr), dt(0.9), dt(0.999), dt(1e-8)
        self.b1p, self.b2p = self.b1, self.b2
        self.m, self.v = {}, {}

    def step(self, p, grads):
        dt = self.dt
        alpha = dt(self.lr * np.sqrt(dt(1) - self.b2p, dtype=dt) / (dt(1) - self.b1p))
        out = {}
        for k in VARS:
            g = np.asarray(grads[k], dt)
            m = self.m.setdefault(k, np.zeros_like(g)); v = self.v.setdefault(k, np.zeros_like(g))
            m += (g - m) * (dt(1) - self.b1)
            v += (g * g - v) * (dt(1) - self.b2)
            out[k] = np.asarray(p[k], dt) - (m * alpha) / (np.sqrt(v) + self.eps)
        self.b1p, self.b2p = dt(self.b1p * self.b1), dt(self.b2p * self.b2)
        return out


def train(p, batches, lr, reg, dt=np.float64, step=sparse_step):
    """``batches``: per step what ``step`` takes after the parameters (a BatchLists for sparse_step).  Returns (parameters, losses,
    first-step gradients)."""
    p = cast(p, dt); opt = Adam(lr, dt); losses, first = [], None
    for b in batches:
        loss, g = step(p, b, reg, dt)
        first = g if first is None else first
        losses.append(float(loss))
        p = opt.step(p, g)
    return p, np.array(losses), first


def hidden(p, users, R, dt=np.float64):
    """the encoder of predictForRanking: all-ones mask over the users' dense rating rows ``R`` [len(users), n_items]"""
    p = cast(p, dt)
    return sig(np.asarray(R, dt) @ p["W_enc"] + p["b_enc"] + p["V"][np.asarray(users)])


def scores(p, users, R, dt=np.float64):
    """sigmoid(h W_dec + b_dec) (CDAE.py:100-105), before the rated items are set to 0"""
    p = cast(p, dt)
    return sig(hidden(p, users, R, dt) @ p["W_dec"] + p["b_dec"])


def draw_batch(rnd, n_users, n_items, rated, batch, per_rated=5):
    """next_batch's draws (CDAE.py:26-41) in plain Python on the generator ``rnd`` (the ``random`` module or a random.Random):
    ids stand for names, ``rated[u]`` is the set of the user's train item ids.  Returns (users, one set of negatives per row)."""
    user_list, item_list = list(range(n_users)), list(range(n_items))
    users, negatives = [], []
    for _ in range(batch):
        user = rnd.choice(user_list)
        users.append(user)
        neg = set()
        for _ in range(per_rated * len(rated[user])):
            ng = rnd.choice(item_list)
            while ng in rated[user]:
                ng = rnd.choice(item_list)
            neg.add(ng)
        negatives.append(neg)
    return users, negatives
