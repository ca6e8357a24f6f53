"""The social-trust rating models on the host: the numpy mirror (tests/social_mirror.py) against the recorded runs of the
reference, the level schedule's ordering of every conflict, level-by-level execution against the sequential walk, and the
five names resolving to classes."""
import json
import os
import random

import numpy as np
import pytest

import social_mirror as M
from helpers import GOLDEN
from qrec_amd.social import Relations, UserSteps, level_schedule, sequential_schedule

MODELS = ("SoRec", "SoReg", "SocialMF", "RSTE", "SREE")


def load(model):
    meta = json.load(open(os.path.join(GOLDEN, "golden_social_meta.json")))[model]
    return meta, np.load(os.path.join(GOLDEN, f"social_{model.lower()}_filmtrust.npz"))


def test_the_five_social_models_resolve_to_classes():
    from qrec_amd.QRec import resolve_model
    from qrec_amd.base.socialRecommender import SocialRecommender
    for name in MODELS:
        cls = resolve_model(name)
        assert cls.__name__ == name and issubclass(cls, SocialRecommender)


@pytest.mark.parametrize("model", MODELS)
def test_host_mirror_reproduces_the_reference_run(model):
    meta, z = load(model)
    r = M.run(model, meta, z)
    assert r["init_ok"] and r["orders_ok"]
    np.testing.assert_allclose(r["P"], z["P"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(r["Q"], z["Q"], rtol=1e-10, atol=1e-13)
    for k in ("Z", "Bu", "Bi"):
        if k in z.files:
            np.testing.assert_allclose(r[k], z[k], rtol=1e-10, atol=1e-13)
    for got, ep in zip(r["losses"], meta["epochs"]):
        assert got == pytest.approx(ep["loss"], rel=1e-11)
    assert np.array_equal(np.array(random.getstate()[1], dtype=np.uint32), z["py_state"])
    if "test_pred" in z.files:       # rating runs: the measures come from these predictions
        lo, hi = float(z["order0_r"].min()), float(z["order0_r"].max())
        P, Q, g = r["P"], r["Q"], r["graph"]
        alpha = M.opt(M.conf_value(meta["conf"], "RSTE"), "-alpha") if model == "RSTE" else None
        known = (z["test_uid"] >= 0) & (z["test_iid"] >= 0)
        for u, i, want in zip(z["test_uid"][known].tolist(), z["test_iid"][known].tolist(), z["test_pred"][known].tolist()):
            p = M.rste_predict(P, Q, g, u, i, alpha) if model == "RSTE" else P[u].dot(Q[i])
            p = hi if p > hi else lo if p < lo else p
            assert p == pytest.approx(want, abs=5.0001e-4)           # the reference stores them rounded to 3 decimals


def test_soreg_similarity_equals_the_reference():
    meta, z = load("SoReg")
    r = M.run("SoReg", meta, z)
    sp, sim = r["pass"], r["sim"]
    fe = [sim[u][f] for u in sp.users for f in sp.g.fe(u)]
    fr = [sim[u][g] for u in sp.users for g in sp.g.fr(u)]
    assert np.array_equal(np.array(fe), z["sim_followee"]) and np.array_equal(np.array(fr), z["sim_follower"])


def test_product_pearson_sp_is_the_reference_formula():
    from qrec_amd.util.qmath import pearson_sp
    rng = np.random.default_rng(3)
    for _ in range(200):
        a = {int(k): float(v) for k, v in zip(rng.integers(0, 12, 6), rng.integers(1, 9, 6) / 2)}
        b = {int(k): float(v) for k, v in zip(rng.integers(0, 12, 6), rng.integers(1, 9, 6) / 2)}
        assert pearson_sp(a, b) == M.pearson_sp(a, b)
    assert pearson_sp({}, {1: 2.0}) == 0 and pearson_sp({1: 2.0}, {1: 3.0}) == 1


# ---- schedules ---------------------------------------------------------------------------------------------------------------
def random_graph(rng, n_users, n_rel, hub=True):
    """relations with self-follows, duplicates, users without followees and (optionally) a hub followed by many"""
    a = rng.integers(0, n_users, n_rel); b = rng.integers(0, n_users, n_rel)
    if hub:
        b[rng.random(n_rel) < 0.3] = 0
    a[:5] = b[:5] = np.arange(5)                         # self-follows
    a = np.concatenate([a, a[:7]]); b = np.concatenate([b, b[:7]])   # duplicate relations
    a[a == n_users - 1] = 1                               # the last user follows nobody
    return M.Graph(a.tolist(), b.tolist(), (rng.integers(1, 5, a.size) / 4).tolist())


def user_steps_of(sp: M.UserPass):
    fe = [list(sp.g.fe(u)) for u in sp.users]
    fr = [list(sp.g.fr(u)) for u in sp.users]
    ptr = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
    cat = lambda ls: np.array([x for l in ls for x in l], dtype=np.int32)
    out = UserSteps(np.array(sp.users, dtype=np.int32), ptr(fe), cat(fe), np.ones(sum(map(len, fe))))
    if sp.kind == "SoReg":
        out.fr_ptr, out.fr_ids, out.fr_w = ptr(fr), cat(fr), np.ones(sum(map(len, fr)))
    return out


def product_schedule(sp, n_users):
    if isinstance(sp, M.RelationPass):
        rel = Relations(np.array([u for u, _, _ in sp.rel], np.int32), np.array([v for _, v, _ in sp.rel], np.int32),
                        np.zeros(len(sp.rel)), np.zeros(len(sp.rel)))
        return rel.schedule(n_users)
    return user_steps_of(sp).schedule(n_users)


def levels_of(sched):
    return [sched.order[sched.level_ptr[L]:sched.level_ptr[L + 1]].tolist() for L in range(sched.n_levels)]


def assert_orders_every_conflict(sp, sched):
    level = np.empty(sp.n_steps, dtype=np.int64)
    for L, steps in enumerate(levels_of(sched)):
        level[steps] = L
    assert sorted(sched.order.tolist()) == list(range(sp.n_steps))
    last_w, last_r = {}, {}
    for k in range(sp.n_steps):              # every earlier conflicting step sits on an earlier level
        reads, writes = sp.reads_writes(k)
        for r in reads:
            if r in last_w:
                assert level[last_w[r]] < level[k]
        for w in writes:
            for j in (last_w.get(w), *last_r.get(w, ())):
                if j is not None:
                    assert level[j] < level[k]
        for r in reads:
            last_r.setdefault(r, []).append(k)
        for w in writes:
            last_w[w] = k


def graphs():
    out = []
    for model in ("SoReg", "SocialMF", "SoRec"):
        meta, z = load(model)
        out.append((model, M.Graph(z["raw_follower"].tolist(), z["raw_followee"].tolist(), z["raw_weight"].tolist()), meta["n_users"]))
    rng = np.random.default_rng(7)
    for n_users, n_rel in ((40, 200), (300, 900), (12, 80)):
        g = random_graph(rng, n_users, n_rel)
        for model in ("SoReg", "SREE", "SoRec"):
            out.append((model, g, n_users))
    return out


@pytest.mark.parametrize("case", range(12))
def test_level_schedule_orders_every_conflict(case):
    model, g, n_users = graphs()[case]
    sp = M.RelationPass(g, n_users) if model == "SoRec" else M.UserPass(model, g, sim=None)
    sched = product_schedule(sp, n_users)
    assert_orders_every_conflict(sp, sched)
    assert sched.n_levels <= sp.n_steps
    seq = sequential_schedule(sp.n_steps)
    assert_orders_every_conflict(sp, seq) if sp.n_steps else None


def test_level_schedule_of_a_chain_and_of_independent_steps():
    # three steps writing one row: three levels; three steps on three rows: one level
    s = level_schedule(3, np.zeros(4, np.int64), np.zeros(0, np.int32), np.arange(4), np.array([1, 1, 1]))
    assert s.n_levels == 3
    s = level_schedule(3, np.zeros(4, np.int64), np.zeros(0, np.int32), np.arange(4), np.array([0, 1, 2]))
    assert s.n_levels == 1 and s.order.tolist() == [0, 1, 2]
    # write-after-read: step 1 writes the row step 0 read
    s = level_schedule(2, np.array([0, 1, 1]), np.array([1]), np.arange(3), np.array([0, 1]))
    assert s.n_levels == 2


@pytest.mark.parametrize("model", ("SoRec", "SoReg", "SocialMF", "SREE"))
def test_level_by_level_execution_is_the_sequential_walk_bit_for_bit(model):
    """the mirror's social pass on the real schedule, steps of a level shuffled, against the plain walk"""
    meta, z = load(model)
    rng = random.Random(5)
    U = meta["n_users"]

    def shuffled_levels(sp):
        lv = levels_of(product_schedule(sp, U))
        for level in lv:
            rng.shuffle(level)
        return lv
    a = M.run(model, meta, z)
    b = M.run(model, meta, z, schedule=shuffled_levels)
    for k in ("P", "Q", "Z", "Bu", "Bi"):
        if k in a:
            assert np.array_equal(a[k], b[k]), k
    assert a["losses"] == b["losses"]
