"""Host side of the social-trust rating models (model/rating/{SoRec,SoReg,SocialMF,RSTE,SREE,LOCABAL,SocialFD}.py): the walk
orders of their social passes as index arrays, and the level schedule the device runs the first five by (LOCABAL and
SocialFD carry a d x d matrix every step rewrites: nothing to schedule, their passes run step by step).

The orders are fixed for a whole run -- ``social.user`` (first appearance in the relation file) for the per-user passes,
the pruned ``social.relation`` list for SoRec -- so the schedule is built once per model instance.  A step reads and
writes table rows; :func:`level_schedule` puts every step one level after the last earlier step it conflicts with
(read-after-write, write-after-read, write-after-write), so the steps of one level touch disjoint written rows and may
run in any order; a schedule of width 1 (:func:`sequential_schedule`) is the reference's walk itself."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class Schedule:
    order: np.ndarray        # int32 [n_steps]: step indices, level by level, ascending inside a level
    level_ptr: np.ndarray    # int32 [n_levels + 1]: level L = order[level_ptr[L]:level_ptr[L + 1]]

    @property
    def n_levels(self) -> int:
        return self.level_ptr.size - 1

    @property
    def max_width(self) -> int:
        return int(np.diff(self.level_ptr).max()) if self.level_ptr.size > 1 else 0


def sequential_schedule(n_steps: int) -> Schedule:
    """width 1: every step its own level, in walk order"""
    return Schedule(np.arange(n_steps, dtype=np.int32), np.arange(n_steps + 1, dtype=np.int32))


def level_schedule(n_rows: int, read_ptr, read_rows, write_ptr, write_rows) -> Schedule:
    """ASAP levels of a walk whose step k reads rows read_rows[read_ptr[k]:read_ptr[k+1]] and writes
    write_rows[write_ptr[k]:write_ptr[k+1]] (a row a step both reads and writes is listed as written; it may also be
    listed as read).  level(k) = 1 + the latest level of an earlier step that writes a row k reads or writes, or reads a
    row k writes."""
    n = len(read_ptr) - 1
    last_w = [-1] * n_rows           # latest level that wrote the row
    last_r = [-1] * n_rows           # latest level that read it
    rp, rr = np.asarray(read_ptr).tolist(), np.asarray(read_rows).tolist()
    wp, wr = np.asarray(write_ptr).tolist(), np.asarray(write_rows).tolist()
    level = [0] * n
    for k in range(n):
        reads, writes = rr[rp[k]:rp[k + 1]], wr[wp[k]:wp[k + 1]]
        lv = 0
        for r in reads:
            if last_w[r] >= lv:
                lv = last_w[r] + 1
        for r in writes:
            m = last_w[r] if last_w[r] > last_r[r] else last_r[r]
            if m >= lv:
                lv = m + 1
        level[k] = lv
        for r in reads:
            if last_r[r] < lv:
                last_r[r] = lv
        for r in writes:
            last_w[r] = lv
    lv = np.asarray(level, dtype=np.int64)
    order = np.argsort(lv, kind="stable").astype(np.int32)
    counts = np.bincount(lv, minlength=int(lv.max()) + 1 if n else 0)
    ptr = np.zeros(counts.size + 1, dtype=np.int32)
    np.cumsum(counts, out=ptr[1:])
    return Schedule(order, ptr)


@dataclass
class UserSteps:
    """The per-user pass of SocialMF / SoReg / SREE: step k is training user ``user[k]`` (social.user order); its
    followees ``fe_ids[fe_ptr[k]:fe_ptr[k+1]]`` in dict order with weights ``fe_w`` (SoReg: Sim[u][f]); SoReg also walks
    its followers ``fr_*`` (weights Sim[u][g])."""
    user: np.ndarray
    fe_ptr: np.ndarray
    fe_ids: np.ndarray
    fe_w: np.ndarray
    fr_ptr: np.ndarray | None = None
    fr_ids: np.ndarray | None = None
    fr_w: np.ndarray | None = None

    @property
    def n_steps(self) -> int:
        return int(self.user.size)

    def schedule(self, n_users: int) -> Schedule:
        """reads: the followees (and followers); writes: the user's own row"""
        n = self.n_steps
        if self.fr_ptr is None:
            read_ptr, reads = self.fe_ptr, self.fe_ids
        else:
            cnt = np.diff(self.fe_ptr) + np.diff(self.fr_ptr)
            read_ptr = np.zeros(n + 1, dtype=np.int64); np.cumsum(cnt, out=read_ptr[1:])
            reads = np.empty(int(read_ptr[-1]), dtype=np.int32)
            for k in range(n):
                a, b = self.fe_ptr[k], self.fe_ptr[k + 1]
                reads[read_ptr[k]:read_ptr[k] + b - a] = self.fe_ids[a:b]
                reads[read_ptr[k] + b - a:read_ptr[k + 1]] = self.fr_ids[self.fr_ptr[k]:self.fr_ptr[k + 1]]
        return level_schedule(n_users, read_ptr, reads, np.arange(n + 1, dtype=np.int64), self.user)


@dataclass
class Relations:
    """SoRec's relation pass: relation k = (follower u[k], followee v[k], trust t[k]) in list order, with the weight
    sqrt(|followers(v)| / (|followees(u)| + |followers(v)|)) of SoRec.py:45-50."""
    u: np.ndarray
    v: np.ndarray
    t: np.ndarray
    w: np.ndarray

    @property
    def n(self) -> int:
        return int(self.u.size)

    def schedule(self, n_users: int) -> Schedule:
        """step k reads and writes P[u[k]] (row u) and Z[v[k]] (row n_users + v)"""
        rows = np.empty(2 * self.n, dtype=np.int64)
        rows[0::2] = self.u; rows[1::2] = n_users + self.v.astype(np.int64)
        no_reads = np.zeros(self.n + 1, dtype=np.int64)
        return level_schedule(2 * n_users, no_reads, rows[:0], np.arange(0, 2 * self.n + 1, 2, dtype=np.int64), rows)


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    ids = np.fromiter((i for x in lists for i, _ in x), dtype=np.int32, count=int(ptr[-1]))
    w = np.fromiter((float(v) for x in lists for _, v in x), dtype=np.float64, count=int(ptr[-1]))
    return ptr, ids, w


def user_steps(rec, weight=None, followers: bool = False) -> UserSteps:
    """The per-user walk of a SocialRecommender ``rec``: users of ``social.user`` that train, their (pruned) followees in
    dict order; ``weight(user, other)`` (default: the followee dict's weight) gives each edge's weight."""
    data, social = rec.data, rec.social
    users, fe, fr = [], [], []
    for name in social.user:
        if not data.containsUser(name):
            continue
        users.append(data.user[name])
        fol = social.getFollowees(name)
        fe.append([(data.user[f], fol[f] if weight is None else weight(name, f)) for f in fol if data.containsUser(f)])
        if followers:
            fr.append([(data.user[g], weight(name, g)) for g in social.getFollowers(name) if data.containsUser(g)])
    out = UserSteps(np.asarray(users, dtype=np.int32), *_csr(fe))
    if followers:
        out.fr_ptr, out.fr_ids, out.fr_w = _csr(fr)
    return out


def sorec_relations(rec) -> Relations:
    import math
    data, social = rec.data, rec.social
    u, v, t, w = [], [], [], []
    for a, b, tuv in social.relation:
        if not (data.containsUser(a) and data.containsUser(b)):
            continue
        vminus = len(social.getFollowers(b))
        uplus = len(social.getFollowees(a))
        try:
            weight = math.sqrt(vminus / (uplus + vminus + 0.0))
        except ZeroDivisionError:
            weight = 1
        u.append(data.user[a]); v.append(data.user[b]); t.append(float(tuv)); w.append(float(weight))
    return Relations(np.asarray(u, dtype=np.int32), np.asarray(v, dtype=np.int32), np.asarray(t, dtype=np.float64),
                     np.asarray(w, dtype=np.float64))


def socialfd_steps(rec) -> UserSteps:
    """SocialFD's walk (SocialFD.py:74-80): :func:`user_steps` over ``data.user`` (id) order instead of ``social.user``;
    a user without followees is a step with no edges"""
    data, social = rec.data, rec.social
    users, fe = [], []
    for name, k in data.user.items():
        users.append(k)
        fol = social.getFollowees(name)
        fe.append([(data.user[f], fol[f]) for f in fol if data.containsUser(f)])
    return UserSteps(np.asarray(users, dtype=np.int32), *_csr(fe))


def pagerank_ranks(relation_pairs) -> dict:
    """{node: 1-based rank} by descending PageRank, as ``nx.pagerank(G, alpha=0.85)`` of the DiGraph of the pairs followed by a
    stable descending sort gives it (LOCABAL.py:26-31): nodes in order of first appearance, unit edge weights with parallel
    edges collapsed, the adjacency matrix row-normalised, uniform start and teleport vectors, the dangling nodes' mass
    spread uniformly, at most 100 iterations, stopped by an L1 change below N * 1e-6; ties keep node order."""
    import scipy.sparse as sp
    index = {}
    for a, b in relation_pairs:
        for x in (a, b):
            if x not in index:
                index[x] = len(index)
    n = len(index)
    if n == 0:
        return {}
    rows = np.fromiter((index[a] for a, _ in relation_pairs), dtype=np.int64)
    cols = np.fromiter((index[b] for _, b in relation_pairs), dtype=np.int64)
    A = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))       # duplicates are summed ...
    A.data[:] = 1.0                                                           # ... and collapse to one unit edge
    S = np.asarray(A.sum(axis=1)).ravel()
    S[S != 0] = 1.0 / S[S != 0]
    A = sp.diags(S).tocsr() @ A
    x = np.repeat(1.0 / n, n)
    p = x.copy()
    dangling = np.where(S == 0)[0]
    for _ in range(100):
        last = x
        x = 0.85 * (A.T @ last + sum(last[dangling]) * p) + (1 - 0.85) * p
        if np.absolute(x - last).sum() < n * 1e-6:
            break
    else:
        raise RuntimeError("pagerank_ranks: the power iteration did not converge within 100 iterations")
    nodes = list(index)
    by_value = sorted(range(n), key=lambda k: float(x[k]), reverse=True)
    rank = {k: r + 1 for r, k in enumerate(by_value)}
    return {nodes[k]: rank[k] for k in range(n)}


@dataclass
class Edges:
    """LOCABAL's social pass: edge t = (user u[t], friend k[t], cosine sim[t]) in the walk order of its S dict"""
    u: np.ndarray
    k: np.ndarray
    sim: np.ndarray

    @property
    def n(self) -> int:
        return int(self.u.size)


def locabal_weights(rec) -> np.ndarray:
    """W of LOCABAL.py:26-34 as an array over user ids: 1 / (1 + log(rank)) for a user of the pruned relation list, 0 for
    every other user (a real weight is positive)"""
    import math
    ranks = pagerank_ranks([(r[0], r[1]) for r in rec.social.relation])
    w = np.zeros(len(rec.data.user), dtype=np.float64)
    for name, rank in ranks.items():
        w[rec.data.user[name]] = 1 / (1 + math.log(rank))
    return w


def locabal_edges(rec, sim=None) -> Edges:
    """S of LOCABAL.py:35-44 as its walk (:68-69): the outer dict's insertion order, then the inner dict's; a repeated
    relation overwrites its value in place.  ``sim(relation line)``: the edge's value (default: cosine_sp of the two
    users' rating dicts)"""
    from .util.qmath import cosine_sp
    data = rec.data
    if sim is None:
        sim = lambda line: cosine_sp(data.trainSet_u[line[0]], data.trainSet_u[line[1]])
    S = {}
    for line in rec.social.relation:
        u1, u2 = line[0], line[1]
        if data.containsUser(u1) and data.containsUser(u2):
            S.setdefault(u1, {})[u2] = sim(line)
    walk = [(data.user[a], data.user[b], float(S[a][b])) for a in S for b in S[a]]
    return Edges(np.asarray([a for a, _, _ in walk], dtype=np.int32), np.asarray([b for _, b, _ in walk], dtype=np.int32),
                 np.asarray([s for _, _, s in walk], dtype=np.float64))


def followee_csr_by_user(rec):
    """RSTE: every training user's (id order) followees in dict order, their weights, and the weight sum as RSTE.py:47-54
    forms it (``np.array(weights).sum()``)"""
    data, social = rec.data, rec.social
    lists, den = [None] * len(data.user), np.zeros(len(data.user), dtype=np.float64)
    for name, k in data.user.items():
        fol = social.getFollowees(name)
        row = [(data.user[f], fol[f]) for f in fol if data.containsUser(f)]
        lists[k] = row
        den[k] = float(np.array([x for _, x in row]).sum())
    ptr, ids, w = _csr(lists)
    return ptr, ids, w, den


def synthetic_graph_steps(kind: str, n_users: int, follower, followee, weight):
    """The walk of model ``kind`` for a relation list over user ids 0 .. n_users-1 that all train (benchmarks and tests);
    SoReg's Sim and LOCABAL's cosine of an edge are taken to be its trust weight.  LOCABAL: (Edges, the weight array W)."""
    from types import SimpleNamespace

    from .data.social import Social
    social = Social(None, [[int(a), int(b), float(w)] for a, b, w in zip(follower, followee, weight)])
    data = SimpleNamespace(user={k: k for k in range(n_users)}, containsUser=lambda u: 0 <= u < n_users)
    rec = SimpleNamespace(data=data, social=social)
    if kind == "SoRec":
        return sorec_relations(rec)
    if kind == "SocialFD":
        return socialfd_steps(rec)
    if kind == "LOCABAL":
        return locabal_edges(rec, sim=lambda line: float(line[2])), locabal_weights(rec)
    if kind == "RSTE":
        return followee_csr_by_user(rec)
    if kind == "SoReg":
        return user_steps(rec, weight=lambda u, v: social.weight(u, v) or social.weight(v, u), followers=True)
    return user_steps(rec)
