"""GPU tests of the co-rating kernels (knn.hip) and the drop-in UserKNN, ItemKNN and SlopeOne classes: the sweep and the
top-K against the host mirror of tests/test_knn_cpu.py bit for bit, the K limit, the classes end to end against the
unmodified reference's runs (tests/golden/gen_golden_knn.py), and the Yelp2018 shape on samples."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from qrec_amd import capi
from qrec_amd.engine import CoRatingKnn, SlopeOneSolver
from qrec_amd.interactions import CSR

from helpers import ROOT, conf_from_text
from test_knn_cpu import COS, EUCLIDEAN, K, PCC, SLOPEONE, Side, knn_predict, load_knn, same_bits, sequence, sweep, top_k

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_knn import yelp_problem  # noqa: E402

pytestmark = pytest.mark.gpu
TILE = capi.KNN_TILE


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    assert capi.device_info()["arch"].startswith("gfx950")
    yield


def side_csr(side):
    """the Side's rows as the engine's CSR (dict order)"""
    indptr = np.zeros(side.n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in side.rows], out=indptr[1:])
    keys = np.array([k for r in side.rows for k in r], dtype=np.int32)
    vals = np.array([v for r in side.rows for v in r.values()], dtype=np.float64)
    return CSR(indptr, keys, vals)


def synthetic(rng, n_cands, n_keys, per_row, scale=5.0, special=True):
    """candidate rows: random keys / half-star values, plus the edge cases of the contract"""
    cand, key, val = [], [], []
    for c in range(n_cands):
        k = rng.choice(n_keys, size=min(n_keys, 1 + rng.integers(0, per_row)), replace=False)
        v = np.round(rng.random(k.size) * scale * 2) / 2 + 0.5
        cand += [c] * k.size; key += k.tolist(); val += v.tolist()
    if special and n_cands >= 4:
        # constant rows (pcc zero denominator), a single-overlap pair, a duplicate pair (dict keeps the last value), big ratings
        cand += [0, 0, 0, 1, 1, 2, 3, 3, 3]
        key += [0, 1, 2, 0, 1, 5, 7, 8, 0]
        val += [3.0, 3.0, 3.0, 2.0, 4.0, 1e6, 999999.5, 0.5, 7.0]
    return np.array(cand), np.array(key), np.array(val)


def run_case(measure, cand, key, val, n_cands, n_keys, query_ids, k):
    side = Side(cand, key, val, n_cands, n_keys)
    rows = side_csr(side)
    knn = CoRatingKnn(measure, rows, n_keys, side.means, query_ids, k)
    knn.run()
    S = knn.similarities()
    qrows = [side.rows[c] if c >= 0 else {} for c in query_ids.tolist()]
    qmeans = np.array([side.means[c] if c >= 0 else 0.0 for c in query_ids.tolist()])
    Sh = sweep(measure, qrows, qmeans, side)
    assert same_bits(S, Sh), f"sweep measure {measure} n_cands {n_cands}"
    ids, vals, counts = knn.neighbours()
    for t in range(query_ids.size):
        hi, hv = top_k(*sequence(Sh, query_ids, t), k)
        assert counts[t] == hi.size
        assert np.array_equal(ids[t, :counts[t]], hi) and same_bits(vals[t, :counts[t]], hv), (measure, n_cands, t)
    return knn, side


@pytest.mark.parametrize("n_cands", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
@pytest.mark.parametrize("measure", [PCC, COS, EUCLIDEAN])
def test_sweep_and_topk_match_mirror(measure, n_cands):
    rng = np.random.default_rng(n_cands * 7 + measure)
    n_keys = 60
    cand, key, val = synthetic(rng, n_cands, n_keys, 12, special=n_cands >= 4)
    nq = min(n_cands, 40)
    q = rng.permutation(n_cands)[:nq].astype(np.int64)
    q = np.concatenate([q[:nq // 2], [-1, -1], q[nq // 2:]])      # test-only queries inside the order
    for k in sorted({1, 20, capi.KNN_MAX_K}):
        run_case(measure, cand, key, val, n_cands, n_keys, q, k)


def test_sweep_long_row_and_column():
    """a query row of 5,000 entries and a column of 50,001 entries"""
    rng = np.random.default_rng(5)
    n_cands, n_keys = 50001, 6000
    cand = [np.arange(n_cands), np.zeros(5000, np.int64)]
    key = [np.zeros(n_cands, np.int64), 1 + np.arange(5000)]
    val = [np.round(rng.random(n_cands) * 9) / 2 + 0.5, np.round(rng.random(5000) * 9) / 2 + 0.5]
    extra = rng.integers(0, n_cands, 20000)
    cand.append(extra); key.append(rng.integers(1, n_keys, extra.size)); val.append(np.round(rng.random(extra.size) * 9) / 2 + 0.5)
    cand, key, val = np.concatenate(cand), np.concatenate(key), np.concatenate(val)
    for measure in (PCC, EUCLIDEAN):
        run_case(measure, cand, key, val, n_cands, n_keys, np.array([0, 17, -1, 40000]), 20)


def test_slopeone_deviations_match_mirror():
    rng = np.random.default_rng(11)
    n_items, n_users = TILE + 5, 300
    cand, key, val = synthetic(rng, n_items, n_users, 30)      # item -> users
    items = Side(cand, key, val, n_items, n_users)
    users = Side(key, cand, val, n_users, n_items)
    q = np.concatenate([rng.permutation(n_items)[:50], [-1]]).astype(np.int64)
    so = SlopeOneSolver(side_csr(items), side_csr(users), q, batch=16)
    dev, freq = so.deviations(0, q.size)
    hd, hf = sweep(SLOPEONE, [items.rows[c] if c >= 0 else {} for c in q.tolist()], np.zeros(q.size), items)
    assert same_bits(dev, hd) and np.array_equal(freq, hf)


def test_topk_ties_and_signed_zeros():
    """mostly ties, +-0.0 mixed; K of 1, 20, the maximum and more than the candidates"""
    rng = np.random.default_rng(3)
    for n_cands in (10, 700):
        cand = np.arange(n_cands); key = np.zeros(n_cands, np.int64); val = np.ones(n_cands)
        side = Side(cand, key, val, n_cands, 1)
        q = np.concatenate([rng.permutation(n_cands)[:30], [-1]]).astype(np.int64)
        for k in (1, 20, capi.KNN_MAX_K):
            knn = CoRatingKnn(COS, side_csr(side), 1, side.means, q, k)
            S = rng.choice(np.array([0.0, -0.0, 1.0, -1.0, 0.5]), size=(q.size, n_cands), p=[0.3, 0.3, 0.2, 0.1, 0.1])
            knn.d_S.upload(np.ascontiguousarray(S[:, knn.lab2id]))
            knn.topk()
            ids, vals, counts = knn.neighbours()
            for t in range(q.size):
                hi, hv = top_k(*sequence(S, q, t), k)
                assert counts[t] == hi.size
                assert np.array_equal(ids[t, :counts[t]], hi) and same_bits(vals[t, :counts[t]], hv)


def test_k_above_the_limit():
    side = Side(np.arange(4), np.zeros(4, np.int64), np.ones(4), 4, 1)
    with pytest.raises(ValueError, match=str(capi.KNN_MAX_K)):
        CoRatingKnn(PCC, side_csr(side), 1, side.means, np.array([0]), capi.KNN_MAX_K + 1)
    knn = CoRatingKnn(PCC, side_csr(side), 1, side.means, np.array([0]), capi.KNN_MAX_K)
    with pytest.raises(capi.QRecError) as e:
        capi.knn_topk(1, knn.d_S, 4, knn.m, knn.d_q_label, knn.d_test_code, knn.d_lab2id, 4, capi.KNN_MAX_K + 1, knn.d_ids, knn.d_vals,
                      knn.d_counts, knn.d_ws, knn.ws_bytes)
    assert e.value.code == capi.ERR_UNSUPPORTED


def model_lines(text):
    """the printed lines from 'Initializing model' up to the measure block, as gen_golden_knn.py keeps them"""
    out, on = [], False
    for ln in text.splitlines():
        if ln.startswith("Initializing model"):
            on = True
        elif ln.startswith("The result") or ln.startswith("Evaluating"):
            on = False
        if on:
            out.append(ln)
    return out


# ---- the classes against the reference's runs ------------------------------------------------------------------------------
def run_class(model, sim, z, meta):
    from qrec_amd.model.rating.ItemKNN import ItemKNN
    from qrec_amd.model.rating.SlopeOne import SlopeOne
    from qrec_amd.model.rating.UserKNN import UserKNN
    cls = {"UserKNN": UserKNN, "ItemKNN": ItemKNN, "SlopeOne": SlopeOne}[model]
    train = [[f"u{u}", f"i{i}", float(r)] for u, i, r in zip(z["train_uid"].tolist(), z["train_iid"].tolist(), z["train_r"].tolist())]
    test = [[f"u{u}" if u >= 0 else f"xu{un}", f"i{i}" if i >= 0 else f"xi{inn}", float(r)]
            for u, i, un, inn, r in zip(z["test_uid"].tolist(), z["test_iid"].tolist(), z["test_uname"].tolist(),
                                        z["test_iname"].tolist(), z["test_r"].tolist())]
    conf = conf_from_text(f"""ratings=x
ratings.setup=-columns 0 1 2
model.name={model}
evaluation.setup=-testSet y
item.ranking=off -topN -1
similarity={sim}
num.neighbors={K}
output.setup=off -dir {os.path.join(ROOT, 'results')}""")
    raw = []
    orig = cls.predictForRating

    class Rec(cls):
        def predictForRating(self, u, i):
            p = orig(self, u, i)
            raw.append(float(p))
            return p

    Rec.__name__ = cls.__name__
    m = Rec(conf, train, test)
    buf = io.StringIO()
    with redirect_stdout(buf):
        measure = m.execute()
    bd = [row[3] for row in m.data.testData]
    return m, measure, np.array(raw), np.array(bd), model_lines(buf.getvalue())


FT_RUNS = [("UserKNN", "pcc"), ("UserKNN", "cos"), ("UserKNN", "euclidean"), ("ItemKNN", "pcc"), ("ItemKNN", "cos"),
           ("ItemKNN", "euclidean"), ("SlopeOne", "cos")]


@pytest.mark.parametrize("model,sim", FT_RUNS)
def test_class_matches_filmtrust_run(model, sim):
    meta_all, z = load_knn("filmtrust")
    tag = model if model == "SlopeOne" else f"{model}_{sim}"
    meta = meta_all[tag]
    m, measure, raw, bd, lines = run_class(model, sim, z, meta)
    assert same_bits(raw, z[tag + "_pred"]) and same_bits(bd, z[tag + "_pred_bounded"])
    assert measure == meta["measure"]
    want = meta["printed"]
    if model == "SlopeOne":       # the item names of this run are i<id> / xi<name>
        assert [ln for ln in lines if ln.endswith(" finished.")] == ["item " + n + " finished." for n in m.data.testSet_i]
        assert len(lines) == len(want)
        return
    assert lines == want
    side = "user" if model == "UserKNN" else "item"
    top = m.topUsers if side == "user" else m.topItems
    ids_map = m.data.user if side == "user" else m.data.item
    names = list(m.data.testSet_u if side == "user" else m.data.testSet_i)
    tpos = {n: k for k, n in enumerate(names)}
    cnt = z[tag + "_nb_count"]
    for t, q in enumerate(names):
        got_ids = [ids_map[n] if n in ids_map else -1 - tpos[n] for n, _ in top[q]]
        assert got_ids == z[tag + "_nb_ids"][t, :cnt[t]].tolist()
        assert same_bits([s for _, s in top[q]], z[tag + "_nb_sims"][t, :cnt[t]])
    # two runs give the same bytes
    m2, _, raw2, _, _ = run_class(model, sim, z, meta)
    assert same_bits(raw, raw2)
    assert np.array_equal(m.knn.d_S.numpy(), m2.knn.d_S.numpy())


def test_class_matches_lastfm_run():
    meta_all, z = load_knn("lastfm")
    meta = meta_all["UserKNN_pcc"]
    m, measure, raw, bd, lines = run_class("UserKNN", "pcc", z, meta)
    assert same_bits(raw, z["UserKNN_pcc_pred"]) and same_bits(bd, z["UserKNN_pcc_pred_bounded"])
    assert measure == meta["measure"] and lines == meta["printed"]
    ids, vals, counts = m.knn.neighbours()
    assert np.array_equal(counts, z["UserKNN_pcc_nb_count"])
    assert np.array_equal(ids[:, :K], z["UserKNN_pcc_nb_ids"]) and same_bits(vals[:, :K], z["UserKNN_pcc_nb_sims"])


# ---- the Yelp2018 shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side_name", ["user", "item"])
def test_yelp_shape_samples(side_name):
    p = yelp_problem()
    us = Side(p["u"], p["i"], p["r"], p["n_users"], p["n_items"])
    its = Side(p["i"], p["u"], p["r"], p["n_items"], p["n_users"])
    side = us if side_name == "user" else its
    qids = p["q_user"] if side_name == "user" else p["q_item"]
    rows = p["user_csr"] if side_name == "user" else p["item_csr"]
    knn = CoRatingKnn(PCC, rows, p["n_items"] if side_name == "user" else p["n_users"], side.means, qids, K)
    knn.run()
    ids, vals, counts = knn.neighbours()
    rng = np.random.default_rng(1)
    early = qids.size // 16                     # the mirror's earlier-query values are swept for the first queries only
    sample = np.sort(rng.choice(early, 64, replace=False))
    last = int(sample.max()) + 1
    need = np.unique(qids[sample][qids[sample] >= 0])
    qrows = [side.rows[c] if c >= 0 else {} for c in qids[:last].tolist()]
    qmeans = np.array([side.means[c] if c >= 0 else 0.0 for c in qids[:last].tolist()])
    Sh = np.zeros((last, side.n))
    for a in range(0, last, 256):            # full rows, 256 queries at a time
        Sh[a:a + 256] = sweep(PCC, qrows[a:a + 256], qmeans[a:a + 256], side)
    assert same_bits(knn.similarities(sample), Sh[sample])
    for t in sample.tolist():
        hi, hv = top_k(*sequence(Sh[:t + 1], qids[:t + 1], t), K)
        assert np.array_equal(ids[t, :counts[t]], hi) and same_bits(vals[t, :counts[t]], hv), t
    # 2,000 sampled test rows: the device's predictions equal the mirror's over the device's neighbour lists
    n = p["test_u"].size
    rows_s = np.sort(rng.choice(n, 2000, replace=False))
    tpos = {int(c) if c >= 0 else -10 - k: k for k, c in enumerate(qids.tolist())}
    if side_name == "user":
        query = np.array([tpos[int(u)] for u in p["test_u"]]); other = p["test_i"]
        base = np.array([us.means[u] for u in p["test_u"].tolist()])
    else:
        query = np.array([p["test_item_query"][k] for k in range(n)]); other = p["test_u"]
        base = np.array([its.means[i] if i >= 0 else p["global_mean"] for i in p["test_i"].tolist()])
    pred, status = knn.predict(0 if side_name == "user" else 1, query[rows_s], other[rows_s], base[rows_s], p["user_csr"].sorted_rows(),
                               side.means)
    for a, r in enumerate(rows_s.tolist()):
        t = query[r]
        top = list(zip(ids[t, :counts[t]].tolist(), vals[t, :counts[t]].tolist()))
        want = knn_predict(side_name, int(p["test_u"][r]), int(p["test_i"][r]), top, us, its, p["global_mean"])
        assert same_bits([pred[a]], [want]), r
