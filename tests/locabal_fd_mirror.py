"""numpy host mirror of the two rating models that carry a dense d x d matrix H (model/rating/{LOCABAL,SocialFD}.py),
restated from their contract: both trainModel loops, LOCABAL's derived data (PageRank ranks -> W, the
cosine list S) and a whole run against a fixture.

The reference's aliasing is part of the semantics.  SocialFD holds x = P[u], y = Q[i] as VIEWS (the Q[i] update and the
trailing P[u] += lr*(err*x - regU*x) see the new rows; in its social pass x moves as the followee loop updates P[u]);
LOCABAL takes copies and applies the weighted update AND THEN the plain one.

Every product of a pass goes through an ``ops`` object, so the same loops run with numpy's ``dot`` (:class:`NumpyOps`, the
reference to the letter), with strictly sequential sums in the reference's association (:class:`SeqOps`: another
legitimate fp64 reading of the same lines) or with a kernel's association (tests/test_locabal_fd_cpu.py)."""
from __future__ import annotations

import math
import random

import numpy as np

from social_mirror import Graph, conf_value, fold, opt, sha


# ---- products ------------------------------------------------------------------------------------------------------------------
class NumpyOps:
    """the reference's own expressions"""

    def dot(self, a, b):
        return a.dot(b)

    def quad(self, v, H):                       # SocialFD.py:38,81,98
        return v.dot(H).dot(H.T).dot(v.T)

    def sq(self, v):                            # (x - y).T.dot(x - y): 1-D arrays, a scalar
        return v.T.dot(v)

    def metric_times(self, H, v):               # SocialFD.py:44-46: W = H.H^T + (H.H^T)^T, then W . column
        W = H.dot(H.T) + H.dot(H.T).T
        return W.dot(np.array([v]).T).T[0]

    def social_times(self, H, w):               # SocialFD.py:82,84: R = H.H^T + H^T.H
        R = H.dot(H.T) + H.T.dot(H)
        return R.dot(np.array([w]).T).T[0]

    def bilinear(self, p, H, q):                # LOCABAL.py:74
        return np.dot(np.dot(p, H), q)

    def Hv(self, H, v):
        return H.dot(v)

    def vH(self, v, H):
        return v.T.dot(H)


def seq_dot(a, b):
    return float(np.cumsum(a * b)[-1])         # add.accumulate: one term after the other


def seq_vH(v, H):
    acc = np.zeros(H.shape[1])
    for i in range(H.shape[0]):
        acc += v[i] * H[i]
    return acc


def seq_Hv(H, v):
    acc = np.zeros(H.shape[0])
    for j in range(H.shape[1]):
        acc += H[:, j] * v[j]
    return acc


def seq_matmul(A, B):
    acc = np.zeros((A.shape[0], B.shape[1]))
    for k in range(A.shape[1]):
        acc += A[:, k:k + 1] * B[k:k + 1, :]
    return acc


class SeqOps(NumpyOps):
    """the reference's association, every sum strictly in index order"""

    def dot(self, a, b):
        return seq_dot(a, b)

    def quad(self, v, H):
        return seq_dot(seq_vH(seq_vH(v, H), H.T), v)

    def sq(self, v):
        return seq_dot(v, v)

    def metric_times(self, H, v):
        M = seq_matmul(H, H.T)
        return seq_Hv(M + M.T, v)

    def social_times(self, H, w):
        return seq_Hv(seq_matmul(H, H.T) + seq_matmul(H.T, H), w)

    def bilinear(self, p, H, q):
        return seq_dot(seq_vH(p, H), q)

    def Hv(self, H, v):
        return seq_Hv(H, v)

    def vH(self, v, H):
        return seq_vH(v, H)


# ---- LOCABAL's derived data ---------------------------------------------------------------------------------------------------
def pagerank_ranks(pairs, alpha=0.85, tol=1e-6, max_iter=100):
    """{node: 1-based rank} of nx.pagerank(DiGraph of ``pairs``) sorted by value, descending and stable (LOCABAL.py:26-31).
    Nodes in order of first appearance, unit weights (a repeated edge is one edge), rows normalised, uniform start and
    teleport vectors, the dangling nodes' mass spread uniformly, L1 change < N*tol ends the iteration."""
    nodes, index = [], {}
    for a, b in pairs:
        for x in (a, b):
            if x not in index:
                index[x] = len(nodes); nodes.append(x)
    n = len(nodes)
    if n == 0:
        return {}
    out = [dict() for _ in range(n)]
    for a, b in pairs:
        out[index[a]][index[b]] = 1.0
    src = np.array([i for i in range(n) for _ in out[i]], dtype=np.int64)
    dst = np.array([j for i in range(n) for j in out[i]], dtype=np.int64)
    deg = np.array([len(o) for o in out], dtype=np.float64)
    inv = np.zeros(n); inv[deg != 0] = 1.0 / deg[deg != 0]
    w = inv[src]
    order = np.argsort(dst, kind="stable")          # per target: sources ascending, the order of a column walk
    src, dst, w = src[order], dst[order], w[order]
    dangling = np.where(deg == 0)[0]
    x = np.repeat(1.0 / n, n); p = x.copy()
    for _ in range(max_iter):
        last = x
        flow = np.zeros(n)
        np.add.at(flow, dst, last[src] * w)
        x = alpha * (flow + sum(last[dangling]) * p) + (1 - alpha) * p
        if np.absolute(x - last).sum() < n * tol:
            break
    else:
        raise RuntimeError("pagerank: no convergence")
    by_value = sorted(range(n), key=lambda k: float(x[k]), reverse=True)
    rank = {k: r + 1 for r, k in enumerate(by_value)}
    return {nodes[k]: rank[k] for k in range(n)}


def cosine_sp(x1: dict, x2: dict) -> float:
    total = d1 = d2 = 0
    try:
        for k in x1:
            if k in x2:
                total += x1[k] * x2[k]
                d1 += x1[k] ** 2
                d2 += x2[k] ** 2
        return total / (math.sqrt(d1) * math.sqrt(d2))
    except ZeroDivisionError:
        return 0


def locabal_derived(g: Graph, rated: dict):
    """(ranks {user: rank}, W {user: weight}, S as a walk [(u, k, sim)]) from the pruned relation list (LOCABAL.py:26-44)"""
    ranks = pagerank_ranks([(a, b) for a, b, _ in g.relation])
    W = {u: 1 / (1 + math.log(r)) for u, r in ranks.items()}
    S = {}
    for a, b, _ in g.relation:
        S.setdefault(a, {})[b] = cosine_sp(rated.get(a, {}), rated.get(b, {}))
    return ranks, W, [(a, b, S[a][b]) for a in S for b in S[a]]


# ---- LOCABAL -------------------------------------------------------------------------------------------------------------------
def rating_locabal(P, Q, W, rows, lr, regU, regI, ops=NumpyOps(), count=None):
    """LOCABAL.py:50-67; W: {user: weight} or an array with 0 for a user outside it"""
    loss = 0.0
    for u, i, r in rows:
        e = r - ops.dot(P[u], Q[i])
        w = W.get(u) if isinstance(W, dict) else (W[u] if W[u] != 0 else None)
        loss += w * e ** 2 if w is not None else e ** 2
        p, q = P[u].copy(), Q[i].copy()
        if w is not None:
            P[u] += lr * (w * e * q - regU * p)
            Q[i] += lr * (w * e * p - regI * q)
        P[u] += lr * (e * q - regU * p)
        Q[i] += lr * (e * p - regI * q)
        if count is not None:
            count["weighted" if w is not None else "unweighted"] += 1
    return loss


def social_locabal(P, H, edges, lr, alpha, regS, slots, ops=NumpyOps(), count=None):
    """LOCABAL.py:68-80 over edges (u, k, sim); H is updated in place, one loss slot per edge"""
    d = H.shape[0]
    last = None
    for t, (u, k, sim) in enumerate(edges):
        p, q = P[u].copy(), P[k].copy()
        e = sim - ops.bilinear(p, H, q)
        slots[t] = alpha * e ** 2
        H += lr * alpha * e * (p.reshape(d, 1).dot(q.reshape(1, d)))
        H -= lr * regS * H
        P[u] += lr * alpha * e * ops.Hv(H, q)
        P[k] += lr * alpha * e * ops.vH(p, H)
        if count is not None:
            count["self_loop"] += u == k
            count["same_user_again"] += u == last
        last = u


# ---- SocialFD ------------------------------------------------------------------------------------------------------------------
def predict_fd(P, Q, Bu, Bi, H, mean, u, i, ops=NumpyOps()):
    x, y = P[u], Q[i]
    return Bi[i] + Bu[u] + mean - ops.quad(x - y, H)


def rating_socialfd(P, Q, Bu, Bi, H, rows, lr, regU, regI, eta, alpha, mean, ops=NumpyOps(), count=None):
    """SocialFD.py:28-72; x, y are views"""
    loss = 0.0
    for u, i, r in rows:
        e = r - predict_fd(P, Q, Bu, Bi, H, mean, u, i, ops)
        loss += e ** 2
        bu, bi = Bu[u], Bi[i]
        x, y = P[u], Q[i]
        dist = ops.quad(x - y, H)
        dd = H.dot(ops.sq(x - y))                                   # H times a scalar
        if r > 0.7:
            loss += eta * alpha * dist
            H -= lr * ((e + eta * alpha) * dd)
            P[u] -= lr * ((e + eta * alpha) * ops.metric_times(H, x - y))
            Q[i] += lr * ((e + eta * alpha) * ops.metric_times(H, x - y))
            band = "high"
        elif r <= 0.5:
            loss += eta * alpha * abs(1 - min(dist, 1))
            if dist < 1:
                H += lr * ((eta * alpha - e) * dd)
                P[u] += lr * ((-e + eta * alpha) * ops.metric_times(H, x - y))
                Q[i] += lr * ((e - eta * alpha) * ops.metric_times(H, x - y))
                band = "low_near"
            else:
                H -= lr * e * dd
                P[u] += lr * (-e * ops.metric_times(H, x - y))
                Q[i] += lr * (e * ops.metric_times(H, x - y))
                band = "low_far"
        else:
            H -= lr * (e * dd)
            P[u] += lr * ((-e) * ops.metric_times(H, x - y) - regU * x)
            Q[i] += lr * (e * ops.metric_times(H, x - y) - regI * y)
            band = "mid"
        Bu[u] += lr * (e - regU * bu)
        Bi[i] += lr * (e - regI * bi)
        P[u] += lr * (e * x - regU * x)
        Q[i] += lr * (e * y - regI * y)
        if count is not None:
            count[band] += 1
    return loss


def fd_steps(g: Graph, n_users):
    """the walk of SocialFD.py:74-80: every training user in id (data.user) order with its followees in dict order"""
    return [(u, list(g.fe(u))) for u in range(n_users)]


def social_socialfd(P, H, steps, lr, eta, beta, slots, ops=NumpyOps(), count=None):
    """SocialFD.py:74-86; one loss slot per followee edge in walk order"""
    t = 0
    for u, fol in steps:
        x = P[u]
        for f in fol:
            slots[t] = ops.quad(x - P[f], H)
            ds = H.dot(ops.sq(x - P[f]))
            delta = ops.social_times(H, x - P[f])
            P[u] -= lr * eta * beta * delta
            H -= lr * eta * beta * ds
            t += 1
            if count is not None:
                count["self_loop"] += u == f


# ---- a whole run against a fixture ---------------------------------------------------------------------------------------------
def run(model, meta, z, ops=NumpyOps()):
    """the whole recorded run on the host; returns dict(P, Q, H, Bu?, Bi?, losses, orders_ok, init_ok, ...)"""
    conf = meta["conf"]
    seed, d = meta["seed"], int(conf_value(conf, "num.factors"))
    U, I = meta["n_users"], meta["n_items"]
    reg = conf_value(conf, "reg.lambda")
    regU, regI, regS = opt(reg, "-u"), opt(reg, "-i"), opt(reg, "-s")
    own = conf_value(conf, model)
    alpha = opt(own, "-alpha")
    random.seed(seed); np.random.seed(seed)
    P = np.random.rand(U, d) / 3
    Q = np.random.rand(I, d) / 3
    out = {}
    if model == "SocialFD":
        eta, beta = opt(own, "-eta"), opt(own, "-beta")
        Bu = np.random.rand(U) / 5
        Bi = np.random.rand(I) / 5
        H = np.random.rand(d, d) / 5
        P /= 10
        Q /= 10
    else:
        H = np.random.rand(d, d)
    init = dict(P0=P, Q0=Q, H0=H, **({"Bu0": Bu, "Bi0": Bi} if model == "SocialFD" else {}))
    init_ok = all(sha(v) == meta["init_sha256"][k] for k, v in init.items())
    out["H0"] = H.copy()
    g = Graph(z["raw_follower"].tolist(), z["raw_followee"].tolist(), z["raw_weight"].tolist())
    rows = list(zip(z["order0_u"].tolist(), z["order0_i"].tolist(), z["order0_r"].tolist()))
    mean = meta["globalMean"]
    if model == "LOCABAL":
        rated = {}
        for u, i, r in rows:                    # data.trainSet_u keeps the rows' FILE order per user; order0 is the file order
            rated.setdefault(u, {})[i] = r
        ranks, W, edges = locabal_derived(g, rated)
        out.update(ranks=ranks, W=W, edges=edges)
    else:
        steps = fd_steps(g, U)
        n_slots = sum(len(f) for _, f in steps)
    losses, orders_ok = [], True
    for ep in meta["epochs"]:
        lr = ep["lr_used"]
        if model == "LOCABAL":
            loss = rating_locabal(P, Q, W, rows, lr, regU, regI, ops)
            slots = np.zeros(len(edges))
            social_locabal(P, H, edges, lr, alpha, regS, slots, ops)
            loss = fold(loss, slots)
            loss += regU * (P * P).sum() + regI * (Q * Q).sum() + regS * (H * H).sum()
        else:
            loss = rating_socialfd(P, Q, Bu, Bi, H, rows, lr, regU, regI, eta, alpha, mean, ops)
            slots = np.zeros(n_slots)
            social_socialfd(P, H, steps, lr, eta, beta, slots, ops)
            loss = fold(loss, slots)
            loss += regU * Bu.dot(Bu) + regI * Bi.dot(Bi)
        losses.append(loss)
        random.shuffle(rows)
        orders_ok = orders_ok and sha(np.array([(u, i) for u, i, _ in rows], dtype=np.int32)) == ep["order_sha256"]
        if model == "SocialFD" and ep["converged"]:
            break
    out.update(P=P, Q=Q, H=H, losses=losses, orders_ok=orders_ok, init_ok=init_ok, graph=g, rows=rows, mean=mean)
    if model == "SocialFD":
        out["Bu"], out["Bi"] = Bu, Bi
    return out
