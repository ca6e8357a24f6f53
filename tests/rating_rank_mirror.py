"""numpy mirror of the device ranking forms (csrc/rank_forms.hip, ranking.FormRanker): predictForRanking of SVD, SVDPlusPlus, EE,
SREE, RSTE and SocialFD written in the EXPANDED form the device computes -- one inner product of an effective user row with an
item row, the squared distance as (|y|^2 - 2 y.x) + |x|^2 --, the error scale S of every score, the rule that says which users'
ids must agree position by position, and the recorded FilmTrust runs as inputs.

Error bound (everywhere): |s_a - s_b| <= RTOL * S with
  dot forms       S = sum_k |q_k e_k| + |Bi| + |Bu| + |mu|      (e = the effective user row)
  distance forms  S = |x|^2 + |y|^2 + |Bi| + |Bu| + |mu|        (x, y = the rows, H-projected for METRIC)
A d <= 128 sum in fp64 carries about 1.4e-14 S of rounding; RTOL = 1e-12 leaves about 70x for another summation order.
Ids: a user whose N + 1 best post-mask scores are pairwise further apart than 2 RTOL S (S = the larger of the two neighbours'; two
masked neighbours are exact zeros everywhere and do not count) must have the same ids in the same positions; the other users' scores are compared as sorted multisets.  At most NEAR_TIE_CAP of
the users of one fixture or case may be such users."""
from __future__ import annotations

import functools
import json
import math
import os

import numpy as np

from helpers import GOLDEN

RTOL = 1e-12
NEAR_TIE_CAP = 0.02
FORMS = ("DOT", "BIASED", "SVDPP", "EUCLID", "METRIC", "RSTE")
DISTANCE = ("EUCLID", "METRIC")
# class -> (form, sign): EE and SREE rank by the distance ITSELF (a plus, unlike their predictForRating), SocialFD subtracts it
CLASSES = {"SVD": ("BIASED", 1.0), "SVDPlusPlus": ("SVDPP", 1.0), "EE": ("EUCLID", 1.0), "SREE": ("EUCLID", 1.0), "RSTE": ("RSTE", 1.0),
           "SocialFD": ("METRIC", -1.0)}


def find_k_largest(K, candidates):
    from qrec_amd.util.qmath import find_k_largest as f
    return f(K, candidates)


def user_row(form, u, P, *, Y=None, y_rated=None, H=None, followees=None, alpha=0.0, **_):
    """the effective user operand of the form, summed in the order the reference adds"""
    e = P[u].copy()
    if form == "SVDPP":
        ptr, items = y_rated
        row = items[ptr[u]:ptr[u + 1]]
        if row.size:
            acc = np.zeros(P.shape[1])
            for j in row.tolist():
                acc = acc + Y[j]
            e = e + acc / row.size
    elif form == "RSTE":
        ptr, ids, w, den = followees
        if den[u] != 0:
            acc = np.zeros(P.shape[1])
            for t in range(int(ptr[u]), int(ptr[u + 1])):
                acc = acc + w[t] * P[ids[t]]
            e = alpha * e + ((1.0 - alpha) * acc) / den[u]
    elif form == "METRIC":
        e = e.dot(H)
    return e


def item_rows(form, Q, H=None):
    return Q.dot(H) if form == "METRIC" else Q


def scores_and_scale(form, u, P, Q, *, mu=0.0, sign=1.0, Bu=None, Bi=None, item_op=None, **kw):
    """(scores [n_items], S [n_items]) of user u over all items, before masking"""
    e = user_row(form, u, P, **kw)
    V = item_rows(form, Q, kw.get("H")) if item_op is None else item_op
    dot = V.dot(e)
    if form in ("DOT", "RSTE"):
        return dot, np.abs(V).dot(np.abs(e))
    bias_scale = np.abs(Bi) + abs(Bu[u]) + abs(mu)
    if form in ("BIASED", "SVDPP"):
        return ((dot + mu) + Bi) + Bu[u], np.abs(V).dot(np.abs(e)) + bias_scale
    nq, np_ = (V * V).sum(axis=1), float(e.dot(e))
    dist = (nq - 2.0 * dot) + np_
    return ((sign * dist + Bi) + Bu[u]) + mu, nq + np_ + bias_scale


def topk(scores, N):
    """find_k_largest(N, scores): by its definition when ties or a short catalogue make the heap's history matter, else the N
    largest in descending order (the same list: every one of them enters the heap and stays, the stable sort has nothing to break)"""
    n = scores.size
    if n > N + 1:
        part = np.argpartition(-scores, N)[:N + 1]
        best = part[np.argsort(-scores[part], kind="stable")]
        vals = scores[best]
        if np.all(vals[:-1] > vals[1:]):
            return best[:N].astype(np.int64), vals[:N].copy()
    ids, sc = find_k_largest(N, scores.tolist())
    return np.array(ids, dtype=np.int64), np.array(sc, dtype=np.float64)


def rank_user(form, u, P, Q, rated_row, N, **kw):
    """(ids [min(N, I)], scores, near_tie, S of the listed ids, S_max) after the rated items were set to 0"""
    s, S = scores_and_scale(form, u, P, Q, **kw)
    s = s.copy(); S = S.copy()
    s[rated_row] = 0.0; S[rated_row] = 0.0          # a masked score is an exact zero on every side
    ids, sc = topk(s, N)
    order = np.argsort(-s, kind="stable")[:N + 1]
    v, w = s[order], S[order]
    # two neighbours that are both masked are exact zeros on the device, in the mirror and in the reference alike: no near tie, the
    # heap breaks that tie the same way everywhere (holding such users to their ids asks more, not less)
    pair_S = np.maximum(w[:-1], w[1:])
    near = bool(np.any((v[:-1] - v[1:] <= 2 * RTOL * pair_S) & (pair_S > 0))) if order.size > 1 else False
    return ids, sc, near, S[ids], float(S.max()) if S.size else 0.0


def rank_users(form, users, P, Q, rated, N, **kw):
    """rank_user for many users; ``rated`` = (indptr, items) over all users.  Lists are padded to N with id -1 / score 0."""
    ptr, items = rated
    item_op = item_rows(form, Q, kw.get("H"))
    n = len(users)
    ids = np.full((n, N), -1, np.int64); sc = np.zeros((n, N)); near = np.zeros(n, bool); S = np.zeros((n, N)); smax = np.zeros(n)
    for k, u in enumerate(np.asarray(users).tolist()):
        i, s, t, w, m = rank_user(form, u, P, Q, items[ptr[u]:ptr[u + 1]], N, item_op=item_op, **kw)
        ids[k, :i.size] = i; sc[k, :i.size] = s; near[k] = t; S[k, :i.size] = w; smax[k] = m
    return dict(ids=ids, scores=sc, near=near, S=S, S_max=smax)


def compare_lists(what, got_ids, got_sc, want, cut=None):
    """the two rules: ids position by position and scores within RTOL * S for the users without a near tie, sorted score multisets
    within RTOL * S_max for the others, who may be at most NEAR_TIE_CAP of the case.  Returns the worst |diff| / S seen."""
    N = got_ids.shape[1] if cut is None else cut
    ids, sc, near, S, smax = (want[k] for k in ("ids", "scores", "near", "S", "S_max"))
    assert near.mean() <= NEAR_TIE_CAP, f"{what}: {int(near.sum())} of {near.size} users have a near tie among their N + 1 best"
    worst = 0.0
    clear = ~near
    bad = np.flatnonzero(clear & np.any(got_ids[:, :N] != ids[:, :N], axis=1))
    assert bad.size == 0, f"{what}: ids differ for users {bad[:5].tolist()}: {got_ids[bad[:2], :N].tolist()} vs {ids[bad[:2], :N].tolist()}"
    diff = np.abs(got_sc[:, :N] - sc[:, :N])
    ratio = np.where(S[:, :N] > 0, diff / np.where(S[:, :N] > 0, S[:, :N], 1.0), np.where(diff == 0, 0.0, np.inf))
    if clear.any():
        worst = float(ratio[clear].max())
    for k in np.flatnonzero(near).tolist():
        d = np.abs(np.sort(got_sc[k, :N]) - np.sort(sc[k, :N])).max()
        worst = max(worst, float(d / smax[k]) if smax[k] > 0 else (0.0 if d == 0 else math.inf))
    assert worst <= RTOL, f"{what}: |score - mirror| / S = {worst:.3e} above {RTOL:.0e}"
    return worst


def hits_and_dcg(ids, test_rows, cut):
    """Measure.hits / the DCG sum of Measure.NDCG per user for the first ``cut`` ids; test_rows[k] = the set of user k's test item ids"""
    hits = np.zeros(len(test_rows), np.int64); dcg = np.zeros(len(test_rows))
    for k, truth in enumerate(test_rows):
        h, x = 0, 0.0
        for pos, i in enumerate(ids[k, :cut].tolist()):
            if i < 0:
                break
            if i in truth:
                h += 1; x += 1.0 / math.log(pos + 2)
        hits[k] = h; dcg[k] = x
    return hits, dcg


# ---- the recorded FilmTrust runs (tests/golden/gen_golden_rating_rank.py) ---------------------------------------------------------
def meta():
    return json.load(open(os.path.join(GOLDEN, "golden_rating_rank_meta.json")))


def followee_den(ptr, w):
    """the weight sum as RSTE.py:47-54 forms it and social.followee_csr_by_user keeps it (np.array(weights).sum())"""
    return np.array([float(np.array(w[ptr[u]:ptr[u + 1]].tolist()).sum()) for u in range(ptr.size - 1)])


@functools.lru_cache(maxsize=None)
def recorded(model):
    """a recorded run as the mirror's and the ranker's arguments.  Treat the arrays as read-only: the tests share them."""
    m = meta()[model]
    assert m["ranking_path_unmodified"], model
    z = np.load(os.path.join(GOLDEN, f"rating_rank_{model.lower()}_filmtrust.npz"))
    form, sign = CLASSES[model]
    kw = dict(mu=m["globalMean"], sign=sign)
    for name in ("Bu", "Bi", "Y", "H"):
        if name in z.files:
            kw[name] = z[name]
    rated = (z["rated_indptr"], z["rated_items"].astype(np.int32))
    if form == "SVDPP":
        kw["y_rated"] = rated
    if form == "RSTE":
        ptr, w = z["fe_indptr"], z["fe_w"]
        kw["followees"] = (ptr, z["fe_ids"], w, followee_den(ptr, w)); kw["alpha"] = m["alpha"]
    users = z["rec_users"]
    tests = {}
    for u, i in zip(z["test_uid"].tolist(), z["test_iid"].tolist()):      # testSet_u: first appearance of a user, a SET of items per user
        tests.setdefault(u, set()).add(i)
    assert [max(u, -1) for u in tests] == users.tolist()
    warm = np.flatnonzero(users >= 0)
    return dict(model=model, form=form, P=z["P"], Q=z["Q"], rated=rated, kw=kw, users=users, warm=warm, test_rows=list(tests.values()),
                rec_ids=z["rec_ids"], rec_scores=z["rec_scores"], measure=m["measure"], top=[int(x) for x in m["topN"].split(",")], z=z, meta=m)


@functools.lru_cache(maxsize=None)
def recorded_mirror(model):
    """the mirror's lists of the recorded run's warm test users, N = the recorded list length; computed once, shared, read-only"""
    c = recorded(model)
    return rank_users(c["form"], c["users"][c["warm"]], c["P"], c["Q"], c["rated"], c["rec_ids"].shape[1], **c["kw"])


def ranker(case):
    """ranking.FormRanker.from_host over a case of :func:`recorded` or one built the same way"""
    from qrec_amd.interactions import CSR
    from qrec_amd.ranking import FormRanker
    kw = dict(case["kw"])
    if "y_rated" in kw:
        kw["y_rated"] = CSR(np.asarray(kw["y_rated"][0], np.int64), np.asarray(kw["y_rated"][1], np.int32))
    rated = case["rated"]
    rated = None if rated is None else CSR(np.asarray(rated[0], np.int64), np.asarray(rated[1], np.int32))
    return FormRanker.from_host(case["form"], case["P"], case["Q"], rated, **kw)


# ---- synthetic problems ------------------------------------------------------------------------------------------------------------
def synthetic(form, d, n_users, n_items, seed=0, integer=False):
    """tables in [0, 1/3), biases and H in [0, 1/5) -- or small integers (every score then exact, ties plentiful, negative scores and
    masked zeros inside the lists).  User 0 has an EMPTY rated row (SVD++: w = 0) and no followee, user 1 follows users whose
    weights are all zero (den == 0), user 2 follows user 3 twice."""
    rng = np.random.default_rng(7919 * d + 31 * n_items + n_users + seed)
    if integer:
        P = rng.integers(-2, 3, (n_users, d)).astype(np.float64); Q = rng.integers(-2, 3, (n_items, d)).astype(np.float64)
    else:
        P = rng.random((n_users, d)) / 3; Q = rng.random((n_items, d)) / 3
    kw = dict(mu=0.0, sign=1.0)
    if form in ("BIASED", "SVDPP", "EUCLID", "METRIC"):
        kw["mu"] = 2.0 if integer else float(rng.random() * 2 + 1.5)
        kw["Bu"] = rng.integers(-2, 3, n_users).astype(np.float64) if integer else rng.random(n_users) / 5
        kw["Bi"] = rng.integers(-2, 3, n_items).astype(np.float64) if integer else rng.random(n_items) / 5
    if form == "METRIC":
        kw["H"] = rng.integers(-1, 2, (d, d)).astype(np.float64) if integer else rng.random((d, d)) / 5
        kw["sign"] = -1.0
    lens = rng.integers(1, min(12, n_items) + 1, n_users); lens[0] = 0
    ptr = np.zeros(n_users + 1, np.int64); ptr[1:] = np.cumsum(lens)
    items = np.concatenate([rng.choice(n_items, int(k), replace=False) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    rated = (ptr, items)
    if form == "SVDPP":
        kw["Y"] = rng.integers(-1, 2, (n_items, d)) * 4.0 if integer else rng.random((n_items, d)) / 3
        if integer:      # row lengths that divide exactly: 1, 2 or 4 items
            lens = rng.choice([1, 2, 4], n_users); lens[0] = 0
            ptr = np.zeros(n_users + 1, np.int64); ptr[1:] = np.cumsum(lens)
            items = np.concatenate([rng.choice(n_items, int(k), replace=False) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
            rated = (ptr, items)
        kw["y_rated"] = rated
    if form == "RSTE":
        flens = rng.integers(1, 6, n_users); flens[0] = 0
        if n_users > 2:
            flens[2] = 2
        fptr = np.zeros(n_users + 1, np.int64); fptr[1:] = np.cumsum(flens)
        ids = rng.integers(0, n_users, int(fptr[-1])).astype(np.int32)
        w = (rng.choice([1.0, 2.0, 4.0], int(fptr[-1])) if integer else rng.integers(1, 11, int(fptr[-1])) / 10.0)
        if n_users > 1:
            w[fptr[1]:fptr[2]] = 0.0
        if n_users > 3:
            ids[fptr[2]:fptr[3]] = 3
            if integer:
                w[fptr[2]:fptr[3]] = 2.0
        den = followee_den(fptr, w)
        if integer:      # den a power of two and alpha = 1/2: the blend stays exact
            for u in range(n_users):
                k = int(fptr[u + 1] - fptr[u])
                if k and den[u] != 0:
                    w[fptr[u]:fptr[u + 1]] = 0.0; w[fptr[u]] = 2.0
            den = followee_den(fptr, w)
        kw["followees"] = (fptr, ids, w, den); kw["alpha"] = 0.5 if integer else 0.4
    return dict(form=form, P=P, Q=Q, rated=rated, kw=kw)
