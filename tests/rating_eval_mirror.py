"""numpy host mirror of the rating models' evaluation: the six prediction forms of engine.RatingEvaluator, each the
expression its class's ``predictForRating`` evaluates, the boundary rule of ``checkRatingBoundary`` as the device states
it, and the two error sums.  The device is held to this file; this file is held to the recorded reference runs
(tests/test_rating_eval_cpu.py)."""
from __future__ import annotations

import math

import numpy as np

FORMS = ("DOT", "BIASED", "SVDPP", "EUCLID", "METRIC", "RSTE")


# ---- checkRatingBoundary ---------------------------------------------------------------------------------------------------------
def boundary(x: float, lo: float, hi: float) -> float:
    """hi above hi, lo below lo, else round(x, 3) by the device's rule: y = x * 1000 rounded, e = the product's exact
    residual (an fma), k = floor(y); up when y - k > 1/2, or == 1/2 and (e > 0, or e == 0 and k odd); k / 1000."""
    if x > hi:
        return hi
    if x < lo:
        return lo
    y = x * 1000.0
    e = _fma_residual(x, 1000.0, y)
    k = math.floor(y)
    f = y - k
    up = f > 0.5 or (f == 0.5 and (e > 0 or (e == 0 and k % 2 == 1)))
    return (k + 1 if up else k) / 1000.0


def _fma_residual(a: float, b: float, y: float) -> float:
    """a * b - y exactly, for y = fl(a * b) (Dekker's product: the halves multiply without rounding)"""
    def split(v):
        c = 134217729.0 * v          # 2^27 + 1
        hi = c - (c - v)
        return hi, v - hi
    ah, al = split(a); bh, bl = split(b)
    return ((ah * bh - y) + ah * bl + al * bh) + al * bl


def boundary_array(x, lo, hi):
    return np.array([boundary(float(v), lo, hi) for v in np.asarray(x).tolist()], dtype=np.float64)


def boundary_cases(seed: int = 0):
    """the case set the rule is held to: 300,000 uniform draws in [-1, 6]; for every k in [-1000, 6000] the doubles nearest
    (k + 1/2) / 1000 and k / 1000 with both neighbours of each; values above and below any rating scale in use"""
    rng = np.random.default_rng(seed)
    k = np.arange(-1000, 6001, dtype=np.float64)
    centres = np.concatenate([(k + 0.5) / 1000.0, k / 1000.0])
    near = np.concatenate([centres, np.nextafter(centres, np.inf), np.nextafter(centres, -np.inf)])
    return np.concatenate([rng.uniform(-1.0, 6.0, 300000), near, np.array([-3.0, -0.75, 6.5, 9.25, 1e6, -1e6])])


# ---- the forms ---------------------------------------------------------------------------------------------------------------
def implicit(Y, rated_ptr, rated_items, u):
    """SVDPlusPlus._implicit: ((Y[j0] + Y[j1]) + ...) / count in userRated order, None without rated items"""
    items = rated_items[rated_ptr[u]:rated_ptr[u + 1]]
    if len(items) == 0:
        return None
    total = 0
    for j in items:
        total = total + Y[j]
    return total / len(items)


def predict(form, u, i, P, Q, *, global_mean, user_means=None, item_means=None, Bu=None, Bi=None, Y=None, rated=None, H=None,
            followees=None, alpha=0.0):
    """predictForRating of pair (u, i), ids with -1 = unknown to the training set; ``rated`` = (indptr, items),
    ``followees`` = (ptr, ids, w, den)"""
    ku, ki = u >= 0, i >= 0
    if not (ku and ki):
        if form == "DOT":
            return user_means[u] if ku else item_means[i] if ki else global_mean
        return global_mean
    if form == "DOT":
        return P[u].dot(Q[i])
    if form == "BIASED":
        return P[u].dot(Q[i]) + global_mean + Bi[i] + Bu[u]
    if form == "SVDPP":
        pred = 0
        imp = implicit(Y, rated[0], rated[1], u)
        if imp is not None:
            pred += imp.dot(Q[i])
        pred += P[u].dot(Q[i]) + global_mean + Bi[i] + Bu[u]
        return pred
    if form == "EUCLID":
        diff = P[u] - Q[i]
        return global_mean + Bi[i] + Bu[u] - diff.dot(diff)
    if form == "METRIC":
        diff = P[u] - Q[i]
        return Bi[i] + Bu[u] + global_mean - diff.dot(H).dot(H.T).dot(diff.T)
    if form == "RSTE":
        ptr, ids, w, den = followees
        if den[u] != 0:
            idx, ww = ids[ptr[u]:ptr[u + 1]], w[ptr[u]:ptr[u + 1]]
            fpred = 0 + ww.dot(P[idx].dot(Q[i]))
            return alpha * P[u].dot(Q[i]) + (1 - alpha) * fpred / den[u]
        return P[u].dot(Q[i])
    raise ValueError(form)


def raw_predictions(form, uid, iid, P, Q, **kw):
    return np.array([float(predict(form, int(u), int(i), P, Q, **kw)) for u, i in zip(uid, iid)], dtype=np.float64)


def predictions(form, uid, iid, P, Q, scale, **kw):
    return boundary_array(raw_predictions(form, uid, iid, P, Q, **kw), float(scale[0]), float(scale[-1]))


def error_sums(rating, pred):
    """(sum |r - p|, sum (r - p)(r - p)), each a plain left-to-right sum"""
    s_abs = s_sq = 0.0
    for r, p in zip(np.asarray(rating).tolist(), np.asarray(pred).tolist()):
        e = r - p
        s_abs += abs(e)
        s_sq += e * e
    return s_abs, s_sq


def measure(rating, pred):
    n = len(pred)
    if n == 0:
        return ["MAE:0\n", "RMSE:0\n"]
    s_abs, s_sq = error_sums(rating, pred)
    return ["MAE:" + str(s_abs / n) + "\n", "RMSE:" + str(math.sqrt(s_sq / n)) + "\n"]


# ---- what a recorded run's evaluation reads, from its training rows ------------------------------------------------------------------
def means_from_rows(u, i, r, n_users, n_items):
    """(userMeans[n_users], itemMeans[n_items], globalMean, rScale) as data/rating.py forms them from the training rows in
    file order: a repeated (user, item) keeps its first position and its last rating; a mean is sum(values) / len in dict
    order, the global mean the mean of the user means in id order"""
    by_u = [dict() for _ in range(n_users)]; by_i = [dict() for _ in range(n_items)]
    for a, b, x in zip(np.asarray(u).tolist(), np.asarray(i).tolist(), np.asarray(r).tolist()):
        by_u[a][b] = x
        by_i[b][a] = x
    um = np.array([sum(row.values()) / len(row) if row else 0.0 for row in by_u])
    im = np.array([sum(col.values()) / len(col) if col else 0.0 for col in by_i])
    total = sum(um.tolist())
    rated_ptr = np.zeros(n_users + 1, np.int64)
    rated_ptr[1:] = np.cumsum([len(row) for row in by_u])
    rated_items = np.array([b for row in by_u for b in row], dtype=np.int32)
    return dict(user_means=um, item_means=im, global_mean=0 if total == 0 else total / n_users,
                scale=sorted(set(np.asarray(r).tolist())), rated=(rated_ptr, rated_items))


def followee_csr(follower, followee, weight, n_users):
    """(ptr, ids, w, den) over user ids as social.followee_csr_by_user builds them, from a relation list over codes
    (>= 0 a training user's id, < 0 a name the training data does not know; both ends must train to count)"""
    rows = [dict() for _ in range(n_users)]
    for a, b, w in zip(np.asarray(follower).tolist(), np.asarray(followee).tolist(), np.asarray(weight).tolist()):
        if a >= 0 and b >= 0:
            rows[a][b] = w
    ptr = np.zeros(n_users + 1, np.int64)
    ptr[1:] = np.cumsum([len(row) for row in rows])
    ids = np.array([b for row in rows for b in row], dtype=np.int32)
    w = np.array([x for row in rows for x in row.values()], dtype=np.float64)
    den = np.array([float(np.array(list(row.values())).sum()) for row in rows], dtype=np.float64)
    return ptr, ids, w, den
