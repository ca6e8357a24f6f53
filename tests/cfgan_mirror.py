"""CFGAN (model/ranking/CFGAN.py:46-127) restated in numpy, in any float type: the losses and gradients in the DENSE form the reference
writes (batch x n_items arrays, C @ G_W1) and in the SPARSE form the device kernels evaluate (rated entries and mask positions only),
TF-1.14 Adam with one optimizer per network, the epoch (one D step, three G steps on one batch), the scores of predictForRanking,
and the draw loop of next_batch in plain Python.

Parameters are a dict: G_W1 [n_items, n_items], G_b1 [n_items], D_W1 [2 n_items] (the reference's [2 n_items, 1] column, flat),
D_b1 [1].  The lists are qrec_amd.autoencoder.BatchLists with everything kept: "in" = the rated entries of the batch rows, "live" =
the mask positions, ``lv_label`` = 1 where the position is in N_zr as well."""
import numpy as np

VARS = ("G_W1", "G_b1", "D_W1", "D_b1")
G_VARS, D_VARS = VARS[:2], VARS[2:]
EPS = 10e-5          # CFGAN.py:106-107


def sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def cast(p, dt):
    """the parameters in the float type ``dt``, D_W1 flat whichever of its two shapes came in"""
    return {k: np.asarray(v, dt).reshape(-1) if k == "D_W1" else np.asarray(v, dt) for k, v in p.items()}


def dense_parts(p, C, mask, N_zr, alpha, dt=np.float64):
    """both losses and the gradients of both, as CFGAN.py:84-107 composes them"""
    p = cast(p, dt); C, mask, N_zr = (np.asarray(a, dt) for a in (C, mask, N_zr))
    B, ni = C.shape
    Dw, Db = p["D_W1"], p["D_b1"][0]
    r = sig(C @ p["G_W1"] + p["G_b1"])
    fake = r * mask
    Dr = sig(np.concatenate([C, C], 1) @ Dw + Db)
    Df = sig(np.concatenate([fake, C], 1) @ Dw + Db)
    d_loss = -(np.log(Dr + dt(EPS)) + np.log(dt(1) - Df + dt(EPS))).mean(dtype=dt)
    g_loss = np.log(dt(1) - Df + dt(EPS)).mean(dtype=dt) + dt(alpha) * ((N_zr * fake) ** 2).sum(dtype=dt) / dt(2)
    a_r = -Dr * (dt(1) - Dr) / (Dr + dt(EPS)) / dt(B)
    a_f = Df * (dt(1) - Df) / (dt(1) - Df + dt(EPS)) / dt(B)
    gDw = np.concatenate([C, C], 1).T @ a_r + np.concatenate([fake, C], 1).T @ a_f
    dfake = -a_f[:, None] * Dw[None, :ni] + dt(alpha) * N_zr * fake
    delta = dfake * mask * r * (dt(1) - r)
    grads = dict(G_W1=C.T @ delta, G_b1=delta.sum(0), D_W1=gDw, D_b1=np.array([a_r.sum() + a_f.sum()], dt))
    return dict(d_loss=d_loss, g_loss=g_loss, grads=grads, r=r, D_real=Dr, D_fake=Df)


def sparse_parts(p, L, alpha, dt=np.float64):
    """the same over the lists ``L``: everything the kernels produce -- r and delta per live slot, the row quantities, losses, gradients"""
    p = cast(p, dt); B, ni = L.B, L.n_items
    W, b, Dw, Db = p["G_W1"], p["G_b1"], p["D_W1"], p["D_b1"][0]
    in_row = np.repeat(np.arange(B), np.diff(L.in_ptr)); lv_row = np.repeat(np.arange(B), np.diff(L.lv_ptr))
    in_item, lv_item = np.asarray(L.in_item), np.asarray(L.lv_item)
    val, flag = np.asarray(L.in_val, dt), np.asarray(L.lv_label, dt)
    r = np.zeros(lv_item.size, dt)
    for n in range(B):
        e, s = slice(L.in_ptr[n], L.in_ptr[n + 1]), slice(L.lv_ptr[n], L.lv_ptr[n + 1])
        r[s] = sig(val[e] @ W[np.ix_(in_item[e], lv_item[s])] + b[lv_item[s]])
    rows = lambda w, row: np.bincount(row, weights=w, minlength=B).astype(dt) if w.size else np.zeros(B, dt)
    c_hi = rows(val * Dw[ni + in_item], in_row)
    logit_r = rows(val * Dw[in_item], in_row) + c_hi + Db
    logit_f = rows(r * Dw[lv_item], lv_row) + c_hi + Db
    Dr, Df = sig(logit_r), sig(logit_f)
    d_loss = -(np.log(Dr + dt(EPS)) + np.log(dt(1) - Df + dt(EPS))).mean(dtype=dt)
    g_loss = np.log(dt(1) - Df + dt(EPS)).mean(dtype=dt) + dt(alpha) * ((flag * r) ** 2).sum(dtype=dt) / dt(2)
    a_r = -Dr * (dt(1) - Dr) / (Dr + dt(EPS)) / dt(B)
    a_f = Df * (dt(1) - Df) / (dt(1) - Df + dt(EPS)) / dt(B)
    delta = (-a_f[lv_row] * Dw[lv_item] + dt(alpha) * flag * r) * r * (dt(1) - r)
    gW = np.zeros((ni, ni), dt)
    for n in range(B):                # a row's rated items and its mask positions are each distinct
        e, s = slice(L.in_ptr[n], L.in_ptr[n + 1]), slice(L.lv_ptr[n], L.lv_ptr[n + 1])
        gW[np.ix_(in_item[e], lv_item[s])] += np.outer(val[e], delta[s])
    gb = np.zeros(ni, dt); np.add.at(gb, lv_item, delta)
    gDw = np.zeros(2 * ni, dt)
    np.add.at(gDw, in_item, a_r[in_row] * val); np.add.at(gDw, lv_item, a_f[lv_row] * r)
    np.add.at(gDw, ni + in_item, (a_r + a_f)[in_row] * val)
    grads = dict(G_W1=gW, G_b1=gb, D_W1=gDw, D_b1=np.array([a_r.sum() + a_f.sum()], dt))
    return dict(d_loss=d_loss, g_loss=g_loss, grads=grads, r=r, delta=delta, D_real=Dr, D_fake=Df, a_r=a_r, a_f=a_f,
                logit_real=logit_r, logit_fake=logit_f)


class Adam:
    """training/adam.py + ApplyAdam in the float type ``dt`` over the variables ``keys``: the beta powers are kept in that type and
    advance after the update"""

    def __init__(self, lr, keys, dt=np.float64):
        self.dt, self.keys = dt, keys
        self.lr, self.b1, self.b2, self.eps = dt(lr), dt(0.9), dt(0.999), dt(1e-8)
        self.b1p, self.b2p = self.b1, self.b2
        self.m, self.v = {}, {}

    def step(self, p, grads):
        dt = self.dt
        alpha = dt(self.lr * np.sqrt(dt(1) - self.b2p, dtype=dt) / (dt(1) - self.b1p))
        out = dict(p)
        for k in self.keys:
            g = np.asarray(grads[k], dt)
            m = self.m.setdefault(k, np.zeros_like(g)); v = self.v.setdefault(k, np.zeros_like(g))
            m += (g - m) * (dt(1) - self.b1)
            v += (g * g - v) * (dt(1) - self.b2)
            out[k] = np.asarray(p[k], dt) - (m * alpha) / (np.sqrt(v) + self.eps)
        self.b1p, self.b2p = dt(self.b1p * self.b1), dt(self.b2p * self.b2)
        return out


def train(p, batches, lr, alpha, dt=np.float64, parts=sparse_parts):
    """one epoch per entry of ``batches`` (what ``parts`` takes between the parameters and alpha, as a tuple): a D step, then three
    G steps on the same batch.  Returns (parameters, d_losses [E], g_losses [E, 3], first D-step gradients, first G-step gradients)."""
    p = cast(p, dt)
    opt_d, opt_g = Adam(lr, D_VARS, dt), Adam(lr, G_VARS, dt)
    d_losses, g_losses, first_d, first_g = [], [], None, None
    for batch in batches:
        batch = batch if isinstance(batch, tuple) else (batch,)
        out = parts(p, *batch, alpha, dt)
        first_d = out["grads"] if first_d is None else first_d
        d_losses.append(float(out["d_loss"]))
        p = opt_d.step(p, out["grads"])
        row = []
        for _ in range(3):
            out = parts(p, *batch, alpha, dt)
            first_g = out["grads"] if first_g is None else first_g
            row.append(float(out["g_loss"]))
            p = opt_g.step(p, out["grads"])
        g_losses.append(row)
    return p, np.array(d_losses), np.array(g_losses), first_d, first_g


def scores(p, C, dt=np.float64):
    """r_hat of the users' whole rows (CFGAN.py:129-134), before the rated items are set to 0"""
    p = cast(p, dt)
    return sig(np.asarray(C, dt) @ p["G_W1"] + p["G_b1"])


def draw_batch(rnd, n_users, n_items, rated, batch, n_zr, n_pm):
    """next_batch's draws (CFGAN.py:18-44) in plain Python on the generator ``rnd`` (the ``random`` module or a random.Random): ids
    stand for names, ``rated[u]`` is the set of the user's train item ids, ``n_zr`` / ``n_pm`` the draws per row.  Returns
    (users, one set of N_zr negatives per row, one set of mask negatives per row)."""
    user_list, item_list = list(range(n_users)), list(range(n_items))
    users, zr, pm = [], [], []
    for _ in range(batch):
        user = rnd.choice(user_list)
        users.append(user)
        sets = []
        for count in (n_zr, n_pm):
            neg = set()
            for _ in range(count):
                ng = rnd.choice(item_list)
                while ng in rated[user]:
                    ng = rnd.choice(item_list)
                neg.add(ng)
            sets.append(neg)
        zr.append(sets[0]); pm.append(sets[1])
    return users, zr, pm
