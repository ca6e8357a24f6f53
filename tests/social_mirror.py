"""numpy host mirror of the social-trust rating models (model/rating/{SoRec,SoReg,SocialMF,RSTE,SREE}.py), restated from
their contract: the rating passes, and the social passes as one function per STEP, so that a test can
run them sequentially or level by level in any order inside a level.  Loss terms go to slots in walk order and are added
onto the running loss one by one (:func:`fold`)."""
from __future__ import annotations

import hashlib
import math
import random

import numpy as np


# ---- the social graph as the reference prunes it ------------------------------------------------------------------------------
class Graph:
    """followees / followers dicts (insertion order), social.user order and the relation list, over codes: a code >= 0 is a
    training user's id, a code < 0 a name the training data does not know (pruned as base/socialRecommender.py does)"""

    def __init__(self, follower, followee, weight):
        self.users = []                     # social.user: first appearance, unknown names included
        seen = set()
        self.followees, self.followers = {}, {}
        for a, b, w in zip(follower, followee, weight):
            for x in (a, b):
                if x not in seen:
                    seen.add(x); self.users.append(x)
            if a >= 0 and b >= 0:
                self.followees.setdefault(a, {})[b] = w
                self.followers.setdefault(b, {})[a] = w
        self.relation = [(a, b, w) for a, b, w in zip(follower, followee, weight) if a >= 0 and b >= 0]

    def fe(self, u):
        return self.followees.get(u, {})

    def fr(self, u):
        return self.followers.get(u, {})

    def step_users(self):
        return [u for u in self.users if u >= 0]


def pearson_sp(x1: dict, x2: dict) -> float:
    total = d1 = d2 = 0
    hit = False
    try:
        m1 = sum(x1.values()) / len(x1)
        m2 = sum(x2.values()) / len(x2)
        for k in x1:
            if k in x2:
                total += (x1[k] - m1) * (x2[k] - m2)
                d1 += (x1[k] - m1) ** 2
                d2 += (x2[k] - m2) ** 2
                hit = True
        return total / (math.sqrt(d1) * math.sqrt(d2))
    except ZeroDivisionError:
        return 1 if hit else 0


def soreg_sim(g: Graph, rated: dict, n_users: int):
    """Sim[u][f] in data.user (id) order, each pair set once for both directions with weight(u, f) of the direction met first"""
    sim = {}
    for u in range(n_users):
        for f in g.fe(u):
            if f not in sim.get(u, {}):
                s = (pearson_sp(rated.get(u, {}), rated.get(f, {})) + g.fe(u).get(f, 0)) / 2.0
                sim.setdefault(u, {})[f] = s
                sim.setdefault(f, {})[u] = s
    return sim


# ---- rating passes ----------------------------------------------------------------------------------------------------------
def rating_pmf(P, Q, rows, lr, regU, regI, copies=False):
    loss = 0.0
    for u, i, r in rows:
        e = r - P[u].dot(Q[i])
        loss += e ** 2
        p, q = (P[u].copy(), Q[i].copy()) if copies else (P[u], Q[i])
        P[u] += lr * (e * q - regU * p)
        Q[i] += lr * (e * p - regI * q)
    return loss


def rating_ee(P, Q, Bu, Bi, rows, lr, regU, regI, regB, mean):
    loss = 0.0
    for u, i, r in rows:
        df = P[u] - Q[i]
        e = r - (mean + Bi[i] + Bu[u] - df.dot(df))
        loss += e ** 2
        loss += regU * (P[u] - Q[i]).dot(P[u] - Q[i])
        bu, bi = Bu[u], Bi[i]
        P[u] -= lr * (e + regU) * (P[u] - Q[i])
        Q[i] += lr * (e + regI) * (P[u] - Q[i])
        Bu[u] += lr * (e - regB * bu)
        Bi[i] += lr * (e - regB * bi)
    return loss


def rste_predict(P, Q, g: Graph, u, i, alpha):
    fol = g.fe(u)
    w = np.array([fol[f] for f in fol])
    den = w.sum()
    if den != 0:
        idx = np.array(list(fol))
        return alpha * P[u].dot(Q[i]) + (1 - alpha) * (0 + w.dot(P[idx].dot(Q[i]))) / den
    return P[u].dot(Q[i])


def rating_rste(P, Q, g: Graph, rows, lr, alpha, regU, regI):
    loss = 0.0
    for u, i, r in rows:
        e = r - rste_predict(P, Q, g, u, i, alpha)
        loss += e ** 2
        p, q = P[u], Q[i]
        P[u] += lr * (alpha * e * q - regU * p)
        Q[i] += lr * (alpha * e * p - regI * q)
    return loss


# ---- social passes, one step at a time -----------------------------------------------------------------------------------------
class UserPass:
    """SocialMF / SoReg / SREE: step k = k-th training user of social.user.  ``slots``: one per step (SocialMF) or one per
    followee edge in walk order (SoReg, SREE)."""

    def __init__(self, kind, g: Graph, sim=None):
        self.kind, self.g, self.sim = kind, g, sim
        self.users = g.step_users()
        self.edge0 = np.zeros(len(self.users) + 1, dtype=np.int64)
        np.cumsum([len(g.fe(u)) for u in self.users], out=self.edge0[1:])
        self.n_slots = len(self.users) if kind == "SocialMF" else int(self.edge0[-1])

    def reads_writes(self, k):
        u = self.users[k]
        reads = list(self.g.fe(u)) + (list(self.g.fr(u)) if self.kind == "SoReg" else [])
        return reads, [u]

    def step(self, P, k, lr, coef, slots):
        u = self.users[k]
        fol = self.g.fe(u)
        if self.kind == "SocialMF":
            fp, den = 0, 0
            for f in fol:
                fp += fol[f] * P[f]
                den += fol[f]
            rl = P[u] - fp / den if den != 0 else np.zeros(P.shape[1])
            slots[k] = coef * rl.dot(rl)
            P[u] -= lr * coef * rl
        elif self.kind == "SoReg":
            s1, simsum, s2 = 0, 0, 0
            for j, f in enumerate(fol):
                s = self.sim[u][f]
                s1 += s * (P[u] - P[f])
                simsum += s * ((P[u] - P[f]).dot(P[u] - P[f]))
                slots[self.edge0[k] + j] = simsum
            for gg in self.g.fr(u):
                s2 += self.sim[u][gg] * (P[u] - P[gg])
            P[u] += lr * (-coef * (s1 + s2))
        else:
            for j, v in enumerate(fol):
                p, z = P[u], P[v]
                P[u] -= lr * coef * fol[v] * (p - z)
                slots[self.edge0[k] + j] = coef * fol[v] * (p - z).dot(p - z)

    @property
    def n_steps(self):
        return len(self.users)


class RelationPass:
    """SoRec: step k = k-th kept relation (u, v, t); P[u] and Z[v] are read and written"""

    def __init__(self, g: Graph, n_users):
        self.rel = g.relation
        self.n_users = n_users
        self.weight = []
        for u, v, _ in self.rel:
            vm, up = len(g.fr(v)), len(g.fe(u))
            try:
                self.weight.append(math.sqrt(vm / (up + vm + 0.0)))
            except ZeroDivisionError:
                self.weight.append(1)
        self.n_slots = len(self.rel)

    def reads_writes(self, k):
        u, v, _ = self.rel[k]
        return [], [u, self.n_users + v]

    def step(self, P, Z, k, lr, regS, regZ, slots):
        u, v, t = self.rel[k]
        e = self.weight[k] * t - P[u].dot(Z[v])
        slots[k] = regS * (e ** 2)
        p, z = P[u], Z[v]
        P[u] += lr * (regS * e * z)
        Z[v] += lr * (regS * e * p - regZ * z)

    @property
    def n_steps(self):
        return len(self.rel)


def fold(loss, slots):
    for s in slots:
        loss += s
    return loss


# ---- a whole run against a fixture -------------------------------------------------------------------------------------------
def conf_value(conf_text, key):
    for line in conf_text.strip().splitlines():
        k, v = line.split("=", 1)
        if k == key:
            return v
    raise KeyError(key)


def opt(value, flag):
    parts = value.split()
    return float(parts[parts.index(flag) + 1])


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(model, meta, z, schedule=None):
    """the whole recorded run on the host; returns dict(P, Q, Z?, Bu?, Bi?, losses, orders_ok, init_ok, py_state).
    ``schedule(pass_) -> list of step lists``: run the social pass level by level in the given orders (default: sequential)"""
    conf = meta["conf"]
    seed, d = meta["seed"], int(conf_value(conf, "num.factors"))
    U, I = meta["n_users"], meta["n_items"]
    reg = conf_value(conf, "reg.lambda")
    regU, regI, regB, regS = opt(reg, "-u"), opt(reg, "-i"), opt(reg, "-b"), opt(reg, "-s")
    random.seed(seed); np.random.seed(seed)
    P = np.random.rand(U, d) / 3
    Q = np.random.rand(I, d) / 3
    out = {}
    init_ok = sha(P) == meta["init_sha256"]["P0"] and sha(Q) == meta["init_sha256"]["Q0"]
    if model == "SoRec":
        Z = np.random.rand(U, d) / 10
    if model == "SREE":
        Bu = np.random.rand(U) / 10; Bi = np.random.rand(I) / 10
        init_ok = init_ok and sha(Bu) == meta["init_sha256"]["Bu0"] and sha(Bi) == meta["init_sha256"]["Bi0"]
    g = Graph(z["raw_follower"].tolist(), z["raw_followee"].tolist(), z["raw_weight"].tolist())
    rows = list(zip(z["order0_u"].tolist(), z["order0_i"].tolist(), z["order0_r"].tolist()))
    mean = meta["globalMean"]                # data.globalMean as the reference's data model computes it
    if model in ("SoReg", "SocialMF", "SREE"):
        sim = None
        if model == "SoReg":
            rated = {}
            for u, i, r in rows:
                rated.setdefault(u, {})[i] = r
            # data.trainSet_u keeps the rows' FILE order per user; order0 is the file order
            sim = soreg_sim(g, rated, U)
        sp = UserPass(model, g, sim)
    elif model == "SoRec":
        sp = RelationPass(g, U)
    own = {"SoRec": "-z", "SoReg": "-alpha", "RSTE": "-alpha", "SREE": "-alpha"}
    coef = opt(conf_value(conf, model), own[model]) if model in own else None
    losses, orders_ok = [], True
    levels = schedule(sp) if (schedule and model != "RSTE") else None
    for ep in meta["epochs"]:
        lr = ep["lr_used"]
        if model == "RSTE":
            loss = rating_rste(P, Q, g, rows, lr, coef, regU, regI)
        elif model == "SREE":
            loss = rating_ee(P, Q, Bu, Bi, rows, lr, regU, regI, regB, mean)
            loss += regB * (Bu * Bu).sum() + regB * (Bi * Bi).sum()
        else:
            loss = rating_pmf(P, Q, rows, lr, regU, regI, copies=model == "SocialMF")
        if model != "RSTE":
            slots = np.zeros(sp.n_slots)
            steps = levels if levels is not None else [[k] for k in range(sp.n_steps)]
            for level in steps:
                for k in level:
                    if model == "SoRec":
                        sp.step(P, Z, k, lr, regS, coef, slots)
                    else:
                        sp.step(P, k, lr, regS if model == "SocialMF" else coef, slots)
            loss = fold(loss, slots)
        if model == "SoRec":
            loss += regU * (P * P).sum() + regI * (Q * Q).sum() + coef * (Z * Z).sum()
        elif model in ("SoReg", "SocialMF", "RSTE"):
            loss += regU * (P * P).sum() + regI * (Q * Q).sum()
        losses.append(loss)
        random.shuffle(rows)
        orders_ok = orders_ok and sha(np.array([(u, i) for u, i, _ in rows], dtype=np.int32)) == ep["order_sha256"]
    out.update(P=P, Q=Q, losses=losses, orders_ok=orders_ok, init_ok=init_ok, graph=g, rows=rows, mean=mean)
    if model == "SoRec":
        out["Z"] = Z
    if model == "SREE":
        out["Bu"], out["Bi"] = Bu, Bi
    if model == "SoReg":
        out["sim"] = sim
    if model != "RSTE":
        out["pass"] = sp
    return out
