"""UserKNN, ItemKNN and SlopeOne without a GPU: the models are provided, the item-major CSR is ``trainSet_i``, and a host
mirror of the contract the kernels implement -- written with numpy and plain Python, not taken from the
reference -- reproduces the unmodified reference's runs (tests/golden/gen_golden_knn.py) bit for bit."""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN

K = 20
PCC, COS, EUCLIDEAN, SLOPEONE = 0, 1, 2, 3
MEASURE = {"pcc": PCC, "cos": COS, "euclidean": EUCLIDEAN}


def load_knn(name):
    meta = json.load(open(os.path.join(GOLDEN, "golden_knn_meta.json")))[name]
    return meta, np.load(os.path.join(GOLDEN, f"knn_{name}.npz"))


# ---- the data model, by dict semantics ------------------------------------------------------------------------------------
class Side:
    """one side of the training data: ``rows[c]`` = {key: value} in dict order (a duplicated pair keeps its last value at its
    first position), ``cols[key]`` = (candidates ascending, values), the rows' means"""

    def __init__(self, cand, key, val, n_cands, n_keys):
        self.rows = [dict() for _ in range(n_cands)]
        for c, k, v in zip(cand.tolist(), key.tolist(), val.tolist()):
            self.rows[c][k] = v
        self.n, self.n_keys = n_cands, n_keys
        self.means = np.array([sum(r.values()) / len(r) for r in self.rows], dtype=np.float64)
        by_key = [[] for _ in range(n_keys)]
        for c, r in enumerate(self.rows):
            for k, v in r.items():
                by_key[k].append((c, v))
        self.cols = [(np.array([c for c, _ in lst], dtype=np.int64), np.array([v for _, v in lst], dtype=np.float64))
                     for lst in by_key]


def sides(z):
    u, i, r = z["train_uid"], z["train_iid"], z["train_r"]
    nu, ni = int(u.max()) + 1, int(i.max()) + 1
    return Side(u, i, r, nu, ni), Side(i, u, r, ni, nu)


def pow2(x):
    """elementwise ``v ** 2`` as Python floats compute it (numpy's power would square exactly)"""
    return np.array([v ** 2 for v in x.tolist()], dtype=np.float64)


# ---- the contract ----------------------------------------------------------------------------------------------------------
def sweep(measure, qrows, qmeans, side):
    """S[t][c] = similarity(qrows[t] (x1), side.rows[c] (x2)) summed over x1's keys in order; SlopeOne: (diffAverage, freq)"""
    n = side.n
    S = np.zeros((len(qrows), n))
    F = np.zeros((len(qrows), n), dtype=np.int64)
    for t, row in enumerate(qrows):
        A, B, C, N = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
        m1 = qmeans[t]
        for k, a in row.items():
            c, b = side.cols[k]
            if measure == PCC:
                da, db = a - m1, b - side.means[c]
                A[c] = A[c] + da * db
                B[c] = B[c] + da ** 2                  # Python's ** on floats: the C library's pow, not always da * da
                C[c] = C[c] + pow2(db)
            elif measure == COS:
                A[c] = A[c] + a * b
                B[c] = B[c] + a ** 2
                C[c] = C[c] + pow2(b)
            elif measure == EUCLIDEAN:
                A[c] = A[c] + (a ** 2 - pow2(b))
            else:
                A[c] = A[c] + (a - b)
            N[c] += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            if measure in (PCC, COS):
                den = np.sqrt(B) * np.sqrt(C)
                S[t] = np.where(den == 0, np.where(N > 0, 1.0, 0.0) if measure == PCC else 0.0, A / den)
            elif measure == EUCLIDEAN:
                S[t] = np.where(A == 0, 0.0, 1.0 / A)
            else:
                S[t] = np.where(N == 0, 0.0, A / N)
        F[t] = N
    return (S, F) if measure == SLOPEONE else S


def sequence(S, query_ids, t):
    """query t's candidate sequence: (ids, values) -- the earlier queries (x1 = the earlier one), then the other candidates"""
    q = query_ids[t]
    if q < 0:
        return np.arange(S.shape[1]), S[t].copy()
    earlier = query_ids[:t]
    ids1 = np.where(earlier >= 0, earlier, -1 - np.arange(t))
    vals1 = S[:t, q]
    skip = np.zeros(S.shape[1], dtype=bool)
    skip[earlier[earlier >= 0]] = True
    skip[q] = True
    rest = np.flatnonzero(~skip)
    return np.concatenate([ids1, rest]), np.concatenate([vals1, S[t, rest]])


def top_k(ids, vals, k):
    """the first k of the stable sort by value, descending (-0.0 == 0.0)"""
    order = np.lexsort((np.arange(vals.size), -(vals + 0.0)))[:k]
    return ids[order], vals[order]


def knn_predict(side_name, u, i, top, user_side, item_side, global_mean, k=K):
    """UserKNN / ItemKNN's predictForRating over a neighbour list [(id, sim)] (ids: training ids, < 0 test-only)"""
    total, denom = 0, 0
    urow = user_side.rows[u] if u >= 0 else {}
    for c, s in top[:k]:
        if c < 0:
            continue
        if side_name == "user":
            r = user_side.rows[c].get(i) if i >= 0 else None
            mean = user_side.means[c]
        else:
            r = urow.get(c)
            mean = item_side.means[c]
        if r is not None:
            total += s * (r - mean)
            denom += s
    own, means = (u, user_side.means) if side_name == "user" else (i, item_side.means)
    if total == 0:
        return means[own] if own >= 0 else global_mean
    return means[own] + total / float(denom)


def slopeone_predict(u, i_t, dev, freq, user_side, item_side, i, global_mean):
    if u >= 0:
        total, fs = 0, 0
        for j, r in user_side.rows[u].items():
            total += (r + dev[i_t, j]) * freq[i_t, j]
            fs += freq[i_t, j]
        return float(total) / fs if fs else user_side.means[u]
    return item_side.means[i] if i >= 0 else global_mean


def bounded(p, lo, hi):
    p = float(p)
    return hi if p > hi else (lo if p < lo else round(p, 3))


def query_names(z, side_name):
    """testSet_u / testSet_i order: (names, training ids or -1)"""
    key = "test_uname" if side_name == "user" else "test_iname"
    ids = z["test_uid"] if side_name == "user" else z["test_iid"]
    seen = {}
    for n, c in zip(z[key].tolist(), ids.tolist()):
        seen.setdefault(n, c)
    return list(seen), np.array(list(seen.values()), dtype=np.int64)


def mirror_knn(z, side_name, sim, sample=None):
    """(ids, sims, counts) of the sampled queries and every test row's prediction"""
    us, its = sides(z)
    side = us if side_name == "user" else its
    names, qids = query_names(z, side_name)
    qrows = [side.rows[c] if c >= 0 else {} for c in qids.tolist()]
    qmeans = np.array([side.means[c] if c >= 0 else 0.0 for c in qids.tolist()])
    S = sweep(MEASURE.get(sim, COS), qrows, qmeans, side)
    sample = range(len(names)) if sample is None else sample
    nb = {}
    for t in sample:
        nb[t] = top_k(*sequence(S, qids, t), K)
    return names, qids, S, nb, us, its


def global_mean(us):
    return float(sum(us.means.tolist()) / len(us.means))


# ---- tests -----------------------------------------------------------------------------------------------------------------
def test_models_are_provided():
    from qrec_amd.QRec import resolve_model
    from qrec_amd.model.rating.ItemKNN import ItemKNN
    from qrec_amd.model.rating.SlopeOne import SlopeOne
    from qrec_amd.model.rating.UserKNN import UserKNN
    assert resolve_model("UserKNN") is UserKNN
    assert resolve_model("ItemKNN") is ItemKNN
    assert resolve_model("SlopeOne") is SlopeOne


def test_item_major_csr_is_trainset_i():
    from qrec_amd.data.rating import Rating
    from qrec_amd.data.rows import RatingRows
    from qrec_amd.util.config import ModelConf
    conf = ModelConf.from_dict({"evaluation.setup": "-testSet x", "ratings.setup": "-columns 0 1 2"})
    rows = [["a", "x", 1.0], ["b", "x", 2.0], ["a", "y", 3.0], ["c", "y", 4.0], ["a", "x", 5.0], ["b", "z", 1.5], ["c", "x", 2.5],
            ["b", "x", 0.5]]
    test = [["a", "z", 1.0]]
    names_u, names_i = ["a", "b", "c"], ["x", "y", "z"]
    compact = RatingRows([names_u.index(r[0]) for r in rows], [names_i.index(r[1]) for r in rows], [r[2] for r in rows], names_u, names_i)
    tcompact = RatingRows([0], [2], [1.0], names_u, names_i)
    for d in (Rating(conf, [r[:] for r in rows], [r[:] for r in test]), Rating(conf, compact, tcompact)):
        csr = d.item_rated_csr()
        for i, iid in d.item.items():
            col = d.trainSet_i[i]
            sl = slice(csr.indptr[iid], csr.indptr[iid + 1])
            assert [d.id2user[u] for u in csr.indices[sl].tolist()] == list(col)
            assert csr.values[sl].tolist() == list(col.values())
        assert d.trainSet_i["x"] == {"a": 5.0, "b": 0.5, "c": 2.5}
        assert list(d.trainSet_i["x"]) == ["a", "b", "c"]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize("model,sim", [("UserKNN", "pcc"), ("UserKNN", "cos"), ("UserKNN", "euclidean"),
                                       ("ItemKNN", "pcc"), ("ItemKNN", "cos"), ("ItemKNN", "euclidean")])
def test_mirror_reproduces_filmtrust_knn(model, sim):
    meta, z = load_knn("filmtrust")
    tag = f"{model}_{sim}"
    side_name = "user" if model == "UserKNN" else "item"
    names, qids, S, nb, us, its = mirror_knn(z, side_name, sim)
    cnt = z[tag + "_nb_count"]
    for t in range(len(names)):
        ids, vals = nb[t]
        assert ids.size == cnt[t]
        assert np.array_equal(ids, z[tag + "_nb_ids"][t, :cnt[t]]), (tag, t)
        assert same_bits(vals, z[tag + "_nb_sims"][t, :cnt[t]]), (tag, t)
    check_predictions(z, meta[tag], tag, side_name, names, nb, us, its)


def check_predictions(z, meta, tag, side_name, names, nb, us, its):
    from qrec_amd.util.measure import Measure
    tpos = {n: k for k, n in enumerate(names)}
    gm = global_mean(us)
    assert gm == meta["globalMean"]
    preds = []
    key = "test_uname" if side_name == "user" else "test_iname"
    for n, u, i in zip(z[key].tolist(), z["test_uid"].tolist(), z["test_iid"].tolist()):
        ids, vals = nb[tpos[n]]
        preds.append(knn_predict(side_name, u, i, list(zip(ids.tolist(), vals.tolist())), us, its, gm))
    assert same_bits(preds, z[tag + "_pred"])
    lo, hi = float(z["train_r"].min()), float(z["train_r"].max())
    bd = [bounded(p, lo, hi) for p in preds]
    assert same_bits(bd, z[tag + "_pred_bounded"])
    rows = [[a, b, c, p] for a, b, c, p in zip(z["test_uname"].tolist(), z["test_iname"].tolist(), z["test_r"].tolist(), bd)]
    assert Measure.ratingMeasure(rows) == meta["measure"]


def test_mirror_reproduces_filmtrust_slopeone():
    meta, z = load_knn("filmtrust")
    us, its = sides(z)
    names, qids = query_names(z, "item")
    dev, freq = sweep(SLOPEONE, [its.rows[c] if c >= 0 else {} for c in qids.tolist()], np.zeros(len(names)), its)
    tpos = {n: k for k, n in enumerate(names)}
    gm = global_mean(us)
    preds = [slopeone_predict(u, tpos[n], dev, freq, us, its, i, gm)
             for n, u, i in zip(z["test_iname"].tolist(), z["test_uid"].tolist(), z["test_iid"].tolist())]
    assert same_bits(preds, z["SlopeOne_pred"])
    lo, hi = float(z["train_r"].min()), float(z["train_r"].max())
    assert same_bits([bounded(p, lo, hi) for p in preds], z["SlopeOne_pred_bounded"])
    assert meta["SlopeOne"]["printed"][1:1 + len(names)] == ["item " + n + " finished." for n in names]


def test_mirror_reproduces_lastfm_sample():
    meta, z = load_knn("lastfm")
    names, qids, S, nb, us, its = mirror_knn(z, "user", "pcc", sample=[])
    rng = np.random.default_rng(0)
    sample = sorted(set(rng.choice(len(names), 48, replace=False).tolist()) | {0, len(names) - 1})
    cnt = z["UserKNN_pcc_nb_count"]
    for t in sample:
        ids, vals = top_k(*sequence(S, qids, t), K)
        assert np.array_equal(ids, z["UserKNN_pcc_nb_ids"][t, :cnt[t]]), t
        assert same_bits(vals, z["UserKNN_pcc_nb_sims"][t, :cnt[t]]), t
    # the predictions of the sampled users' test rows, from the recorded neighbours
    tpos = {n: k for k, n in enumerate(names)}
    gm = global_mean(us)
    keep = set(sample)
    got, want = [], []
    for k, (n, u, i) in enumerate(zip(z["test_uname"].tolist(), z["test_uid"].tolist(), z["test_iid"].tolist())):
        t = tpos[n]
        if t in keep:
            top = list(zip(z["UserKNN_pcc_nb_ids"][t, :cnt[t]].tolist(), z["UserKNN_pcc_nb_sims"][t, :cnt[t]].tolist()))
            got.append(knn_predict("user", u, i, top, us, its, gm)); want.append(z["UserKNN_pcc_pred"][k])
    assert len(got) > 100 and same_bits(got, want)
