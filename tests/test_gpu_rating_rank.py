"""Ranking of SVD, SVDPlusPlus, EE, SREE, RSTE and SocialFD on the device (csrc/rank_forms.hip, ranking.FormRanker): every form
against the numpy mirror (tests/rating_rank_mirror.py) at the shapes where the tile, the padding and the sliced top-N can go wrong,
exact ties against find_k_largest, the edges of the operand builder, the ABI's refusals, the recorded FilmTrust runs of the
reference, and the six classes end to end against the host loop they used to rank with.

Error bound and id rule: tests/rating_rank_mirror.py.  With QREC_RATING_RANK_PARITY naming a file, the worst |device - mirror| / S
per form is written there when the module is done (profiles/rating_rank_parity.json is such a file)."""
import importlib
import io
import json
import os
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

import rating_rank_mirror as M
from helpers import check, conf_from_text
from qrec_amd import capi
from qrec_amd.base.recommender import Recommender
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.ranking import DeviceRanker, ranking_measure_strings
from qrec_amd.util.measure import Measure
from qrec_amd.util.qmath import find_k_largest

pytestmark = pytest.mark.gpu

N_USERS = 70
WORST = {}          # form -> worst |device - mirror| / S of this run


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    yield
    path = os.environ.get("QREC_RATING_RANK_PARITY")
    if path and WORST:
        with open(path, "w") as f:
            json.dump(dict(bound=M.RTOL, scale="dot forms: sum|q_k e_k| + |Bi| + |Bu| + |mu|; distance forms: |x|^2 + |y|^2 + |Bi| + |Bu| + |mu|",
                           worst_ratio={k: WORST[k] for k in sorted(WORST)}), f, indent=1, sort_keys=True)


def note(form, worst):
    WORST[form] = max(WORST.get(form, 0.0), worst)
    check(f"{form}: |device - mirror| / S", worst, M.RTOL, inclusive=True)


def batch_users(n):
    """a batch of n users of the N_USERS: the special users 0 .. 3 first (tests/rating_rank_mirror.synthetic), one user twice"""
    users = (np.arange(n) * 7 + (np.arange(n) >= 4) * 3) % N_USERS if n > 4 else np.arange(n)
    users[:min(n, 4)] = np.arange(min(n, 4))
    if n > 8:
        users[8] = users[5]
    return users.astype(np.int32)


# (batch, d, N): every batch size, width and list length of the issue at least once with each of the others' extremes
COMBOS = ((1, 5, 1), (17, 10, 10), (65, 64, 100), (65, 5, 10), (17, 64, 1), (1, 10, 100), (65, 10, 1))


@pytest.mark.parametrize("n_items", (37, 8200))
@pytest.mark.parametrize("form", M.FORMS)
def test_lists_match_the_mirror(form, n_items):
    """37 items: below the 32-item tile pad's second tile and the sliced top-N's 8,192 gate; 8,200: above both, N = 100 still on the
    heap.  Batches of 1, 17 (one 16-user tile and a lane) and 65 (the 64-user pad and one)."""
    for n_b, d, N in COMBOS:
        c = M.synthetic(form, d, N_USERS, n_items)
        users = batch_users(n_b)
        want = M.rank_users(form, users, c["P"], c["Q"], c["rated"], N, **c["kw"])
        ids, sc = M.ranker(c).topk(users, N)
        assert ids.shape == (n_b, N) and ids.dtype == np.int32 and sc.dtype == np.float64
        note(form, M.compare_lists(f"{form} I={n_items} B={n_b} d={d} N={N}", ids, sc, want))


@pytest.mark.parametrize("form", M.FORMS)
def test_fewer_items_than_n_pads_with_minus_one(form):
    c = M.synthetic(form, 5, N_USERS, 7)
    users = batch_users(17)
    want = M.rank_users(form, users, c["P"], c["Q"], c["rated"], 10, **c["kw"])
    ids, sc = M.ranker(c).topk(users, 10)
    assert (ids[:, 7:] == -1).all() and (sc[:, 7:] == 0).all() and (ids[:, :7] >= 0).all()
    # seven scores, all listed: the list is the user's whole column in find_k_largest's order (several masked zeros tie exactly on
    # both sides; the other scores lie far apart), so ids are compared for every user
    assert np.array_equal(ids, want["ids"])
    worst = float(np.max(np.where(want["S"] > 0, np.abs(sc - want["scores"]) / np.where(want["S"] > 0, want["S"], 1.0), np.abs(sc - want["scores"]))))
    note(form, worst)


@pytest.mark.parametrize("n_items", (37, 8200))
@pytest.mark.parametrize("form", M.FORMS)
def test_exact_ties_resolve_as_find_k_largest(form, n_items):
    """small-integer tables: every score is exact, so device and mirror hold the same doubles and the lists must be bit-identical
    to find_k_largest on the mirror's scores -- plateaus of ties, masked zeros and negative scores inside the lists"""
    c = M.synthetic(form, 5, N_USERS, n_items, integer=True)
    users = batch_users(65 if n_items < 100 else 17)
    N = 10
    ids, sc = M.ranker(c).topk(users, N)
    ptr, items = c["rated"]
    zeros_listed = negatives_listed = ties = 0
    for k, u in enumerate(users.tolist()):
        s, _ = M.scores_and_scale(form, u, c["P"], c["Q"], **c["kw"])
        s = s.copy(); s[items[ptr[u]:ptr[u + 1]]] = 0.0
        w_ids, w_sc = find_k_largest(N, s.tolist())
        assert ids[k].tolist() == w_ids and sc[k].tolist() == w_sc, (form, n_items, k, u)
        zeros_listed += int((sc[k] == 0).any()); negatives_listed += int((sc[k] < 0).any()); ties += int(np.unique(sc[k]).size < N)
    assert ties > 0
    if form == "METRIC" and n_items < 100:      # sign -1: most scores are negative, the masked zeros outrank them
        assert zeros_listed > 0 and negatives_listed > 0


def test_dot_route_through_the_forms_is_the_plain_route_bit_for_bit():
    """DOT on the form route against qrec_score_topk's fp64 block route: the same tile loop over the same operand values"""
    from qrec_amd.interactions import CSR
    for n_items in (37, 8200):
        c = M.synthetic("DOT", 10, N_USERS, n_items)
        users = batch_users(65)
        plain = DeviceRanker(c["P"], c["Q"], CSR(c["rated"][0], c["rated"][1]))
        a_ids, a_sc = plain.topk(users, 10)
        b_ids, b_sc = M.ranker(c).topk(users, 10)
        assert np.array_equal(a_ids, b_ids) and a_sc.tobytes() == b_sc.tobytes()


# ---- edges of the operand builder ------------------------------------------------------------------------------------------------
def test_svdpp_user_with_an_empty_rated_row():
    c = M.synthetic("SVDPP", 10, N_USERS, 37)
    ptr = c["kw"]["y_rated"][0]
    assert ptr[1] == ptr[0]                                          # user 0: w = 0, no implicit term
    users = np.array([0, 5, 0], np.int32)
    want = M.rank_users("SVDPP", users, c["P"], c["Q"], c["rated"], 10, **c["kw"])
    plain = M.rank_users("BIASED", users, c["P"], c["Q"], c["rated"], 10, **c["kw"])
    assert np.array_equal(want["scores"][0], plain["scores"][0]) and not np.array_equal(want["scores"][1], plain["scores"][1])
    ids, sc = M.ranker(c).topk(users, 10)
    note("SVDPP", M.compare_lists("SVDPP, empty rated row", ids, sc, want))


def test_rste_users_without_followees_with_zero_weights_and_with_a_repeated_followee():
    c = M.synthetic("RSTE", 10, N_USERS, 37)
    ptr, fids, w, den = c["kw"]["followees"]
    assert ptr[1] == ptr[0] and den[0] == 0                          # user 0 follows nobody
    assert ptr[2] > ptr[1] and (w[ptr[1]:ptr[2]] == 0).all() and den[1] == 0      # user 1: followees, all weights zero
    assert ptr[3] - ptr[2] == 2 and (fids[ptr[2]:ptr[3]] == 3).all() and den[2] != 0      # user 2 follows user 3 twice
    users = np.array([0, 1, 2, 9], np.int32)
    want = M.rank_users("RSTE", users, c["P"], c["Q"], c["rated"], 10, **c["kw"])
    dot = M.rank_users("DOT", users, c["P"], c["Q"], c["rated"], 10, **c["kw"])
    assert np.array_equal(want["scores"][:2], dot["scores"][:2]) and not np.array_equal(want["scores"][2], dot["scores"][2])
    ids, sc = M.ranker(c).topk(users, 10)
    note("RSTE", M.compare_lists("RSTE, builder edges", ids, sc, want))


def test_metric_at_the_lds_cap_and_refused_above_it():
    c = M.synthetic("METRIC", 128, N_USERS, 37)
    users = batch_users(17)
    want = M.rank_users("METRIC", users, c["P"], c["Q"], c["rated"], 10, **c["kw"])
    ids, sc = M.ranker(c).topk(users, 10)
    note("METRIC", M.compare_lists("METRIC d=128", ids, sc, want))
    # d = 129 (ld = 144): refused by both entry points, nothing written
    z = lambda *s: DB.zeros(s, np.float64)
    sentinel_i, sentinel_s = np.full((4, 10), -7, np.int32), np.full((4, 10), -7.25)
    out_i, out_s = DB.from_numpy(sentinel_i), DB.from_numpy(sentinel_s)
    prep = DB.from_numpy(np.full(64, 0x5A, np.uint8))
    with pytest.raises(capi.QRecError) as e:
        capi.rank_form_prepare(capi.RATING_METRIC, z(8, 144), z(129, 129), 129, 144, 8, prep, 1 << 30)
    assert e.value.code == capi.ERR_UNSUPPORTED and "128" in str(e.value)
    with pytest.raises(capi.QRecError) as e:
        capi.score_topk_form(capi.RATING_METRIC, -1.0, z(4, 144), z(8, 144), 129, 144, 4, 8, DB.from_numpy(np.arange(4, dtype=np.int32)), 4,
                             None, None, 10, DB(1 << 20, np.uint8), 1 << 20, out_i, out_s, d_Bu=z(4), d_Bi=z(8), d_H=z(129, 129), d_prep=prep,
                             prep_bytes=1 << 30)
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert np.array_equal(out_i.numpy(), sentinel_i) and np.array_equal(out_s.numpy(), sentinel_s) and (prep.numpy() == 0x5A).all()
    with pytest.raises(ValueError, match="128"):
        M.ranker(M.synthetic("METRIC", 129, 8, 8))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched_and_the_next_call_succeeds():
    c = M.synthetic("EUCLID", 10, N_USERS, 37)
    r = M.ranker(c)
    users = batch_users(17)
    good_ids, good_sc = r.topk(users, 10)
    d_users = DB.from_numpy(users)
    sentinel_i, sentinel_s = np.full((17, 10), -7, np.int32), np.full((17, 10), -7.25)
    out_i, out_s = DB.from_numpy(sentinel_i), DB.from_numpy(sentinel_s)
    need = capi.score_topk_form_scratch_bytes(r.form, r.n_items, 17, r.ld, 10)
    scratch = DB(need, np.uint8)

    def call(**over):
        a = dict(form=r.form, sign=1.0, P=r.t.P, Q=r.t.Q, d=r.d, ld=r.ld, users=d_users, n=17, rp=r.rated[0], ri=r.rated[1], N=10,
                 scratch=scratch, sb=need, ids=out_i, sc=out_s, Bu=r.d_Bu, Bi=r.d_Bi, prep=r.d_prep, pb=r.prep_bytes)
        a.update(over)
        capi.score_topk_form(a["form"], a["sign"], a["P"], a["Q"], a["d"], a["ld"], r.n_users, r.n_items, a["users"], a["n"], a["rp"], a["ri"],
                             a["N"], a["scratch"], a["sb"], a["ids"], a["sc"], mu=r.mu, d_Bu=a["Bu"], d_Bi=a["Bi"], d_prep=a["prep"],
                             prep_bytes=a["pb"])

    refused = [dict(P=None), dict(Q=None), dict(users=None), dict(scratch=None), dict(ids=None), dict(Bu=None), dict(prep=None),
               dict(ld=r.ld + 4), dict(ld=r.ld - 8, d=r.ld - 8), dict(N=0), dict(N=101), dict(sb=need - 1), dict(pb=r.prep_bytes - 1),
               dict(ri=None), dict(rp=None), dict(form=9), dict(sign=0.5)]
    for over in refused:
        with pytest.raises(capi.QRecError) as e:
            call(**over)
        assert e.value.code == -1, over
        assert np.array_equal(out_i.numpy(), sentinel_i) and np.array_equal(out_s.numpy(), sentinel_s), over
    with pytest.raises(capi.QRecError):          # the item side: a buffer one byte short
        capi.rank_form_prepare(r.form, r.t.Q, None, r.d, r.ld, r.n_items, r.d_prep, r.prep_bytes - 1)
    call()
    assert np.array_equal(out_i.numpy(), good_ids) and out_s.numpy().tobytes() == good_sc.tobytes()
    with pytest.raises(ValueError, match="out of range"):
        r.topk(np.array([0, N_USERS], np.int32), 10)


def test_two_calls_give_the_same_bytes_and_the_ranker_follows_its_bound_tables():
    c = M.synthetic("METRIC", 10, N_USERS, 8200)
    r = M.ranker(c)
    users = batch_users(65)
    a = r.topk(users, 10)
    b = r.topk(users, 10)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    Q2 = c["Q"][::-1].copy()
    r.t.upload(c["P"], Q2)                      # the bound tables change under the ranker, as after an epoch ...
    r.update_tables()                           # ... and its own item side is remade from them
    want = M.rank_users("METRIC", users, c["P"], Q2, c["rated"], 10, **c["kw"])
    ids, sc = r.topk(users, 10)
    note("METRIC", M.compare_lists("METRIC, tables replaced", ids, sc, want))
    assert not np.array_equal(ids, a[0])


# ---- the recorded runs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(M.CLASSES))
def test_device_reproduces_the_recorded_lists_and_measures(model):
    c, w = M.recorded(model), M.recorded_mirror(model)
    warm, N = c["warm"], c["rec_ids"].shape[1]
    r = M.ranker(c)
    users = c["users"][warm].astype(np.int32)
    # against the reference's own lists: its ids and scores, the mirror's scale and near-tie flags
    ref = dict(w, ids=c["rec_ids"][warm].astype(np.int64), scores=c["rec_scores"][warm])
    from qrec_amd.interactions import user_item_csr
    tu, ti = [], []
    for k in warm.tolist():
        for i in c["test_rows"][k]:
            if i >= 0:
                tu.append(int(c["users"][k])); ti.append(i)
    r.set_test(user_item_csr(np.array(tu, np.int32), np.array(ti, np.int32), np.ones(len(tu)), c["P"].shape[0], c["Q"].shape[0]))
    ids, sc, per_cut = r.topk(users, N, cuts=c["top"])
    note(c["form"], M.compare_lists(f"{model}: device against the recorded lists", ids, sc, ref))
    assert not w["near"].any()                  # no excluded user in these fixtures: nobody can straddle a cut
    cold = np.flatnonzero(c["users"] < 0)
    per_n = {}
    for n in c["top"]:
        hits = np.zeros(c["users"].size, np.int64); dcg = np.zeros(c["users"].size)
        hits[warm], dcg[warm] = per_cut[n]
        hits[cold], dcg[cold] = M.hits_and_dcg(c["rec_ids"][cold], [c["test_rows"][k] for k in cold.tolist()], n)
        per_n[n] = (hits, dcg)
    assert ranking_measure_strings([len(t) for t in c["test_rows"]], per_n, c["top"]) == c["measure"]


# ---- the classes ----------------------------------------------------------------------------------------------------------------------------
def _build(model, out):
    """the class on the recorded FilmTrust split, 2 epochs, item.ranking=on -topN 10,20, output off"""
    c = M.recorded(model)
    z, meta = c["z"], c["meta"]
    cls = getattr(importlib.import_module(f"qrec_amd.model.rating.{model}"), model)
    text = meta["conf"].replace("num.max.epoch=3", "num.max.epoch=2").replace("-dir ./results/", f"-dir {out}/")
    assert "num.max.epoch=2" in text and "item.ranking=on -topN 10,20" in text and "output.setup=off" in text
    conf = conf_from_text(text)
    uname = lambda a: f"u{a}" if a >= 0 else f"xu{-1 - a}"
    iname = lambda b: f"i{b}" if b >= 0 else f"xi{-1 - b}"
    rows = [[f"u{a}", f"i{b}", float(r)] for a, b, r in zip(z["train_u"].tolist(), z["train_i"].tolist(), z["train_r"].tolist())]
    test = [[uname(a), iname(b), float(r)] for a, b, r in zip(z["test_uid"].tolist(), z["test_iid"].tolist(), z["test_rating"].tolist())]
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    if "raw_follower" in z.files:
        rel = [[uname(a), uname(b), float(w)] for a, b, w in zip(z["raw_follower"].tolist(), z["raw_followee"].tolist(), z["raw_weight"].tolist())]
        return cls(conf, rows, test, rel)
    return cls(conf, rows, test)


def _mirror_kw(model, m):
    from qrec_amd.social import followee_csr_by_user
    form, sign = M.CLASSES[model]
    kw = dict(mu=m.data.globalMean, sign=sign)
    for name in ("Bu", "Bi", "Y", "H"):
        if hasattr(m, name):
            kw[name] = getattr(m, name)
    rated = m.data.rated_csr()
    rated = (rated.indptr, rated.indices)
    if form == "SVDPP":
        kw["y_rated"] = rated
    if form == "RSTE":
        kw["followees"] = followee_csr_by_user(m); kw["alpha"] = m.alpha
    return form, rated, kw


@pytest.mark.parametrize("model", sorted(M.CLASSES))
def test_class_ranks_on_the_device_like_its_host_loop(model, tmp_path):
    """trained here, then ranked both ways on the same tables: rank_measure_all_test_users returns the strings of
    Measure.rankingMeasure over the host loop's lists (before the device path existed it returned None), rank_all_test_users the
    loop's lists under the id rule, cold users included, and a second call the same bytes"""
    top, N = [10, 20], 20
    with redirect_stdout(io.StringIO()):
        m = _build(model, tmp_path)
        final = m.execute()
        fast = m.rank_measure_all_test_users(top, N)
        again = m.rank_measure_all_test_users(top, N)
        dev = m.rank_all_test_users(N)
        dev2 = m.rank_all_test_users(N)
        host = Recommender.rank_all_test_users(m, N)          # the loop these classes ranked with: predictForRanking per user
    assert fast is not None and fast == again == final and fast[0] == "Top 10\n" and len(fast) == 10
    assert fast == Measure.rankingMeasure(m.data.testSet_u, host, top)
    users = list(m.data.testSet_u)
    assert list(dev) == users == list(host) and dev == dev2
    form, rated, kw = _mirror_kw(model, m)
    warm = [k for k, u in enumerate(users) if m.data.containsUser(u)]
    assert 0 < len(warm) < len(users)
    cold = [u for u in users if not m.data.containsUser(u)]
    assert all(dev[u] == host[u] for u in cold)                  # the constant-score list, exactly
    uid = np.array([m.data.user[users[k]] for k in warm], np.int32)
    want = M.rank_users(form, uid, m.P, m.Q, rated, N, **kw)
    as_arrays = lambda rl: (np.array([[m.data.item[i] for i, _ in rl[users[k]]] for k in warm], np.int64),
                            np.array([[s for _, s in rl[users[k]]] for k in warm], np.float64))
    d_ids, d_sc = as_arrays(dev)
    h_ids, h_sc = as_arrays(host)
    note(form, M.compare_lists(f"{model}: device lists against the mirror", d_ids, d_sc, want))
    M.compare_lists(f"{model}: host loop against the mirror", h_ids, h_sc, want)
    clear = ~want["near"]
    assert np.array_equal(d_ids[clear], h_ids[clear])
