"""Inputs the rating-evaluation tests share: the recorded FilmTrust runs as evaluator arguments, the rule for pairs at a
rounding boundary, and synthetic problems drawn as tests/test_gpu_social.py draws them."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import rating_eval_mirror as M
from helpers import GOLDEN

# model -> (npz, meta file, meta key, form); the eleven recorded rating runs that carry test_pred (SREE's run ranks)
RECORDED = {
    "BasicMF": ("basicmf_filmtrust", "golden_meta.json", "basicmf_filmtrust", "DOT"),
    "PMF": ("pmf_filmtrust", "golden_meta.json", "pmf_filmtrust", "DOT"),
    "SVD": ("svd_filmtrust", "golden_meta.json", "svd_filmtrust", "BIASED"),
    "SVDPlusPlus": ("svdpp_filmtrust", "golden_meta.json", "svdpp_filmtrust", "SVDPP"),
    "EE": ("ee_filmtrust", "golden_meta.json", "ee_filmtrust", "EUCLID"),
    "SoRec": ("social_sorec_filmtrust", "golden_social_meta.json", "SoRec", "DOT"),
    "SoReg": ("social_soreg_filmtrust", "golden_social_meta.json", "SoReg", "DOT"),
    "SocialMF": ("social_socialmf_filmtrust", "golden_social_meta.json", "SocialMF", "DOT"),
    "RSTE": ("social_rste_filmtrust", "golden_social_meta.json", "RSTE", "RSTE"),
    "LOCABAL": ("social_locabal_filmtrust", "golden_locabal_fd_meta.json", "LOCABAL", "DOT"),
    "SocialFD": ("social_socialfd_filmtrust", "golden_locabal_fd_meta.json", "SocialFD", "METRIC"),
}
BOUNDARY_WINDOW = 1e-9      # a pair whose unrounded value lies this close to (k + 1/2) / 1000 may round either way
BOUNDARY_CAP = 1            # ... and a recorded run may hold at most this many of them


def _final(z, key):
    """the run's last recorded table: `key` itself (social runs) or the highest-numbered `key<k>`"""
    if key in z.files:
        return z[key]
    ks = [int(f[len(key):]) for f in z.files if f.startswith(key) and f[len(key):].isdigit()]
    return z[key + str(max(ks))] if ks else None


@functools.lru_cache(maxsize=None)
def recorded(model):
    """(form, uid, iid, rating, test_pred, P, Q, kwargs of the mirror's predict incl. scale) of a recorded run; a form's
    missing array raises KeyError naming it"""
    npz, meta_file, key, form = RECORDED[model]
    meta = json.load(open(os.path.join(GOLDEN, meta_file)))[key]
    z = np.load(os.path.join(GOLDEN, npz + ".npz"))
    P, Q = _final(z, "P"), _final(z, "Q")
    if "order0" in z.files:
        tu, ti, tr = z["order0"][:, 0], z["order0"][:, 1], z["rating0"]
    else:
        tu, ti, tr = z["order0_u"], z["order0_i"], z["order0_r"]
    m = M.means_from_rows(tu, ti, tr, P.shape[0], Q.shape[0])
    assert m["global_mean"] == meta["globalMean"]
    kw = dict(global_mean=m["global_mean"], user_means=m["user_means"], item_means=m["item_means"])
    need = {"BIASED": ("Bu", "Bi"), "SVDPP": ("Bu", "Bi", "Y"), "EUCLID": ("Bu", "Bi"), "METRIC": ("Bu", "Bi", "H")}.get(form, ())
    for name in need:
        a = _final(z, name)
        if a is None:
            raise KeyError(f"{npz}.npz lacks {name}, which form {form} needs")
        kw[name] = a
    if form == "SVDPP":
        kw["rated"] = m["rated"]
    if form == "RSTE":
        conf = dict(line.split("=", 1) for line in meta["conf"].strip().splitlines())
        parts = conf["RSTE"].split()
        kw["alpha"] = float(parts[parts.index("-alpha") + 1])
        kw["followees"] = M.followee_csr(z["raw_follower"], z["raw_followee"], z["raw_weight"], P.shape[0])
    # the social recordings give every unknown name a negative code of its own; the evaluator knows one: -1
    uid, iid = np.maximum(z["test_uid"], -1).astype(np.int32), np.maximum(z["test_iid"], -1).astype(np.int32)
    return dict(form=form, uid=uid, iid=iid, rating=z["test_rating"], want=z["test_pred"], P=P, Q=Q, scale=m["scale"], kw=kw)


def near_boundary(raw):
    """True where the unrounded value lies within BOUNDARY_WINDOW of a rounding boundary (k + 1/2) / 1000"""
    y = np.asarray(raw) * 1000.0
    return np.abs((y - np.floor(y)) - 0.5) < BOUNDARY_WINDOW * 1000.0


def assert_equals_recorded(model, got, raw, want):
    """got == want exactly, but for at most BOUNDARY_CAP pairs, each at a rounding boundary"""
    off = np.flatnonzero(got != want)
    assert off.size <= BOUNDARY_CAP, f"{model}: {off.size} predictions differ from the recorded run: pairs {off[:8].tolist()}"
    assert near_boundary(raw[off]).all(), f"{model}: pair {off.tolist()} differs away from a rounding boundary: " \
                                          f"raw {raw[off].tolist()} got {got[off].tolist()} want {want[off].tolist()}"


# ---- synthetic problems --------------------------------------------------------------------------------------------------------
def synthetic(form, d, n, seed=0, n_users=67, n_items=45):
    """tables in [0, 1/3), H and biases in [0, 1/5); n pairs that hold a cold user, a cold item, both cold and a repeated
    user (where n allows); user 0 follows nobody (den == 0) and rates one item, user 1 follows one user, user 2 rates 300
    items (with repeats of the 45: userRated order only needs a list)"""
    rng = np.random.default_rng(1000 * d + n + seed)
    P = rng.random((n_users, d)) / 3; Q = rng.random((n_items, d)) / 3
    uid = rng.integers(0, n_users, n).astype(np.int32); iid = rng.integers(0, n_items, n).astype(np.int32)
    special = [(-1, 3), (4, -1), (-1, -1), (0, 1), (1, 2), (2, 3), (2, 4), (5, 5), (5, 6)]
    if n >= 7 * len(special):
        for k, (u, i) in enumerate(special):          # spread over the list, user 2 and user 5 repeating
            uid[7 * k], iid[7 * k] = u, i
    else:
        for k, (u, i) in enumerate(special[3:3 + n]):
            uid[k], iid[k] = u, i
    rating = rng.integers(1, 9, n) / 2.0
    kw = dict(global_mean=float(rng.random() * 2 + 1.5), user_means=rng.random(n_users) * 4 + 0.5, item_means=rng.random(n_items) * 4 + 0.5)
    if form in ("BIASED", "SVDPP", "EUCLID", "METRIC"):
        kw["Bu"] = rng.random(n_users) / 5; kw["Bi"] = rng.random(n_items) / 5
    if form == "METRIC":
        kw["H"] = rng.random((d, d)) / 5
    if form == "SVDPP":
        kw["Y"] = rng.random((n_items, d)) / 3
        lens = rng.integers(1, 12, n_users); lens[0] = 1; lens[2] = 300
        ptr = np.zeros(n_users + 1, np.int64); ptr[1:] = np.cumsum(lens)
        kw["rated"] = (ptr, rng.integers(0, n_items, int(ptr[-1])).astype(np.int32))
    if form == "RSTE":
        lens = rng.integers(0, 6, n_users); lens[0] = 0; lens[1] = 1
        ptr = np.zeros(n_users + 1, np.int64); ptr[1:] = np.cumsum(lens)
        ids = rng.integers(0, n_users, int(ptr[-1])).astype(np.int32)
        w = rng.integers(1, 11, int(ptr[-1])) / 10.0
        den = np.array([float(w[ptr[u]:ptr[u + 1]].sum()) for u in range(n_users)])
        kw["followees"] = (ptr, ids, w, den); kw["alpha"] = 0.4
    return dict(form=form, uid=uid, iid=iid, rating=rating, P=P, Q=Q, scale=(0.5, 4.0), kw=kw)


def evaluator(case):
    """engine.RatingEvaluator.from_host over a case of :func:`recorded` or :func:`synthetic`"""
    from qrec_amd.engine import RatingEvaluator
    from qrec_amd.interactions import CSR
    kw = dict(case["kw"])
    um, im, gm = kw.pop("user_means"), kw.pop("item_means"), kw.pop("global_mean")
    if "rated" in kw:
        kw["rated"] = CSR(np.asarray(kw["rated"][0], np.int64), np.asarray(kw["rated"][1], np.int32))
    return RatingEvaluator.from_host(case["form"], case["P"], case["Q"], case["uid"], case["iid"], case["rating"], case["scale"], um, im, gm, **kw)
