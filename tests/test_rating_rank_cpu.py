"""The ranking forms of the six rating models, on the host: the numpy mirror in the expanded form the device computes
(tests/rating_rank_mirror.py) against the recorded runs of the reference (tests/golden/rating_rank_*_filmtrust.npz), the cap on
near-tie users, the measure strings, and the sign of every distance form."""
from types import SimpleNamespace

import numpy as np
import pytest

import rating_rank_mirror as M
from qrec_amd.ranking import ranking_measure_strings
from qrec_amd.util.qmath import find_k_largest

MODELS = sorted(M.CLASSES)


def test_every_class_ran_its_ranking_path_as_written():
    meta = M.meta()
    assert sorted(meta) == MODELS
    for model in MODELS:
        assert meta[model]["ranking_path_unmodified"] is True, model
        assert "item.ranking=on -topN 10,20" in meta[model]["conf"] and "num.factors=8" in meta[model]["conf"]
        assert len(meta[model]["epochs"]) == 3


@pytest.mark.parametrize("model", MODELS)
def test_recorded_lists_hold_the_near_tie_cap_on_their_own(model):
    """the reference's own lists: neighbours of the recorded top 20 further apart than 2e-12 S, for all but 2 % of the users"""
    c, w = M.recorded(model), M.recorded_mirror(model)
    sc = c["rec_scores"][c["warm"]]
    ids = c["rec_ids"][c["warm"]]
    assert np.array_equal(ids, w["ids"]) or w["near"].any()          # S below is the mirror's, listed by the same ids
    S = w["S"]
    close = np.any(sc[:, :-1] - sc[:, 1:] <= 2 * M.RTOL * np.maximum(S[:, :-1], S[:, 1:]), axis=1)
    assert close.mean() <= M.NEAR_TIE_CAP, (model, int(close.sum()))
    assert w["near"].mean() <= M.NEAR_TIE_CAP, (model, int(w["near"].sum()))      # ... and with the 21st score, from the mirror


@pytest.mark.parametrize("model", MODELS)
def test_mirror_reproduces_the_recorded_lists(model):
    c, w = M.recorded(model), M.recorded_mirror(model)
    worst = M.compare_lists(model, c["rec_ids"][c["warm"]], c["rec_scores"][c["warm"]], w)
    print(f"{model}: worst |recorded - mirror| / S = {worst:.3e}")
    for cut in c["top"]:                                        # a prefix of a list is the list of the smaller N
        M.compare_lists(f"{model} top {cut}", c["rec_ids"][c["warm"]], c["rec_scores"][c["warm"]], w, cut=cut)


@pytest.mark.parametrize("model", MODELS)
def test_mirror_and_measure_strings_equal_the_recorded_measures(model):
    c, w = M.recorded(model), M.recorded_mirror(model)
    N = c["rec_ids"].shape[1]
    ids = np.empty_like(c["rec_ids"], dtype=np.int64)
    ids[c["warm"]] = w["ids"]
    cold = np.flatnonzero(c["users"] < 0)
    cold_ids, _ = find_k_largest(N, [c["kw"]["mu"]] * c["Q"].shape[0])      # base/iterativeRecommender.py:79-80
    ids[cold] = cold_ids
    assert cold.size and np.array_equal(ids[cold], c["rec_ids"][cold])
    lens = [len(t) for t in c["test_rows"]]
    per_n = {n: M.hits_and_dcg(ids, c["test_rows"], n) for n in c["top"]}
    assert ranking_measure_strings(lens, per_n, c["top"]) == c["measure"]


def _fake(model, c, u=0):
    """just enough of a recommender for the class's own predictForRanking"""
    data = SimpleNamespace(containsUser=lambda name: True, user={"u": u}, item={k: k for k in range(c["Q"].shape[0])},
                           globalMean=c["kw"]["mu"], trainingSize=lambda: (c["P"].shape[0], c["Q"].shape[0], 0))
    return SimpleNamespace(data=data, P=c["P"], Q=c["Q"], Bu=c["kw"].get("Bu"), Bi=c["kw"].get("Bi"), H=c["kw"].get("H"),
                           num_items=c["Q"].shape[0])


@pytest.mark.parametrize("model,sign", [("EE", 1.0), ("SREE", 1.0), ("SocialFD", -1.0)])
def test_the_sign_of_the_distance_is_the_class_s(model, sign):
    """the class's own predictForRanking ranks like the mirror with this sign and unlike the mirror with the other one"""
    import importlib
    cls = getattr(importlib.import_module(f"qrec_amd.model.rating.{model}"), model)
    assert M.CLASSES[model][1] == sign
    form = M.CLASSES[model][0]
    c = M.synthetic(form, 5, 9, 37, seed=3)
    for u in range(9):
        want = np.asarray(cls.predictForRanking(_fake(model, c, u), "u"), dtype=np.float64)
        kw = dict(c["kw"], sign=sign)
        got, S = M.scores_and_scale(form, u, c["P"], c["Q"], **kw)
        assert np.all(np.abs(got - want) <= M.RTOL * S), (model, u)
        flipped, _ = M.scores_and_scale(form, u, c["P"], c["Q"], **dict(kw, sign=-sign))
        ids = M.topk(got, 10)[0]
        assert np.array_equal(ids, np.array(find_k_largest(10, want.tolist())[0]))
        assert not np.array_equal(ids, M.topk(flipped, 10)[0]), (model, u)
    # and on the recorded run: the other sign does not reproduce the reference's lists
    r = M.recorded(model)
    users = r["users"][r["warm"]][:40]
    other = M.rank_users(r["form"], users, r["P"], r["Q"], r["rated"], 20, **dict(r["kw"], sign=-sign))
    assert not np.array_equal(other["ids"], r["rec_ids"][r["warm"]][:40])
    assert np.array_equal(M.recorded_mirror(model)["ids"][:40], r["rec_ids"][r["warm"]][:40])


def test_topk_shortcut_is_find_k_largest():
    """the mirror's argpartition shortcut against the definition, ties and short catalogues included"""
    rng = np.random.default_rng(0)
    for n, N, ints in ((37, 10, False), (37, 10, True), (7, 10, False), (11, 10, True), (300, 100, False), (300, 1, True)):
        for _ in range(20):
            s = rng.integers(-3, 4, n).astype(np.float64) if ints else rng.standard_normal(n)
            ids, sc = M.topk(s, N)
            w_ids, w_sc = find_k_largest(N, s.tolist())
            assert ids.tolist() == w_ids and sc.tolist() == w_sc
