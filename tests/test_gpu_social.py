"""The social-trust rating models on the device: every new kernel entry against the host mirror (tests/social_mirror.py) on
synthetic problems, the level schedule against width 1 bit for bit, run-to-run determinism, every class end to end against
the recorded reference run, and one epoch of every model at an Epinions-like shape."""
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

import social_mirror as M
from helpers import conf_from_text
from test_social_cpu import load, random_graph
from qrec_amd import capi
from qrec_amd.engine import DeviceTables, MfSgd, SocialSgd
from qrec_amd.social import Relations, UserSteps, sequential_schedule

pytestmark = pytest.mark.gpu

DIMS = (5, 10, 64, 65, 200)


def steps_of(sp: M.UserPass):
    w = (lambda u, f: sp.sim[u][f]) if sp.kind == "SoReg" else (lambda u, f: sp.g.fe(u)[f])
    fe = [[(f, w(u, f)) for f in sp.g.fe(u)] for u in sp.users]
    ptr = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
    ids = lambda ls: np.array([f for l in ls for f, _ in l], dtype=np.int32)
    ws = lambda ls: np.array([x for l in ls for _, x in l], dtype=np.float64)
    out = UserSteps(np.array(sp.users, dtype=np.int32), ptr(fe), ids(fe), ws(fe))
    if sp.kind == "SoReg":
        fr = [[(g, sp.sim[u][g]) for g in sp.g.fr(u)] for u in sp.users]
        out.fr_ptr, out.fr_ids, out.fr_w = ptr(fr), ids(fr), ws(fr)
    return out


def relations_of(rp: M.RelationPass):
    return Relations(np.array([u for u, _, _ in rp.rel], np.int32), np.array([v for _, v, _ in rp.rel], np.int32),
                     np.array([t for _, _, t in rp.rel], np.float64), np.array(rp.weight, np.float64))


def problem(seed, n_users=60, n_items=50, n_rel=300, n_rows=400):
    rng = np.random.default_rng(seed)
    g = random_graph(rng, n_users, n_rel)
    rows = list(zip(rng.integers(0, n_users, n_rows).tolist(), rng.integers(0, n_items, n_rows).tolist(),
                    (rng.integers(1, 9, n_rows) / 2).tolist()))
    sim = {}
    for u in range(n_users):
        for f in g.fe(u):
            if f not in sim.get(u, {}):
                s = float(rng.random() - 0.3)
                sim.setdefault(u, {})[f] = s; sim.setdefault(f, {})[u] = s
    return g, rows, sim, rng


def arrays(rows):
    return (np.array([u for u, _, _ in rows], np.int32), np.array([i for _, i, _ in rows], np.int32),
            np.array([r for _, _, r in rows], np.float64))


def tables(rng, U, I, d):
    return rng.random((U, d)) / 3, rng.random((I, d)) / 3


def run_social(kind, g, sim, P0, Q0, extra, lr, coef, regZ=0.0, sched=None, start=None):
    """the device's social pass alone; returns tables and the folded loss"""
    t = DeviceTables(P0, Q0, np.float64)
    if kind == "SoRec":
        rp = M.RelationPass(g, P0.shape[0])
        s = SocialSgd(t, 1, kind, relations_of(rp), Z=extra, schedule=sched(rp) if sched else None)
    else:
        sp = M.UserPass(kind, g, sim)
        s = SocialSgd(t, 1, kind, steps_of(sp), schedule=sched(sp) if sched else None)
    s.d_stats.upload_head(np.array([start or 0.0]))
    loss = s.social_pass(lr, coef, regZ)
    P, Q = t.download()
    return P, Q, (s.Z() if kind == "SoRec" else None), loss, s


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", ("SoRec", "SoReg", "SocialMF", "SREE"))
def test_social_pass_matches_the_mirror(kind, d):
    g, rows, sim, rng = problem(d)
    U = 60
    P0, Q0 = tables(rng, U, 50, d)
    Z0 = rng.random((U, d)) / 10
    P, Q, Z, loss, _ = run_social(kind, g, sim, P0, Q0, Z0, 0.05, 0.3, 0.1, start=12.5)
    Pm, Zm = P0.copy(), Z0.copy()
    if kind == "SoRec":
        sp = M.RelationPass(g, U); slots = np.zeros(sp.n_slots)
        for k in range(sp.n_steps):
            sp.step(Pm, Zm, k, 0.05, 0.3, 0.1, slots)
        np.testing.assert_allclose(Z, Zm, rtol=1e-12, atol=1e-14)
    else:
        sp = M.UserPass(kind, g, sim); slots = np.zeros(sp.n_slots)
        for k in range(sp.n_steps):
            sp.step(Pm, k, 0.05, 0.3, slots)
    np.testing.assert_allclose(P, Pm, rtol=1e-12, atol=1e-14)
    assert np.array_equal(Q, Q0)
    assert loss == pytest.approx(M.fold(12.5, slots), rel=1e-12)


@pytest.mark.parametrize("d", DIMS)
def test_rste_rating_pass_matches_the_mirror(d):
    g, rows, _, rng = problem(100 + d)
    P0, Q0 = tables(rng, 60, 50, d)
    lists = [[(f, g.fe(u)[f]) for f in g.fe(u)] for u in range(60)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ids = np.array([f for l in lists for f, _ in l], np.int32); w = np.array([x for l in lists for _, x in l])
    den = np.array([np.array([x for _, x in l]).sum() for l in lists], dtype=np.float64)
    t = DeviceTables(P0, Q0, np.float64)
    s = SocialSgd(t, len(rows), "RSTE", (ptr, ids, w, den))
    loss = s.rating_pass(*arrays(rows), 0.02, 0.001, 0.002, alpha=0.6)
    Pm, Qm = P0.copy(), Q0.copy()
    lm = M.rating_rste(Pm, Qm, g, rows, 0.02, 0.6, 0.001, 0.002)
    P, Q = t.download()
    np.testing.assert_allclose(P, Pm, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(Q, Qm, rtol=1e-11, atol=1e-14)
    assert loss == pytest.approx(lm, rel=1e-12)


@pytest.mark.parametrize("d", DIMS)
def test_variant_4_is_socialmf_rating_pass_on_copies(d):
    _, rows, _, rng = problem(200 + d)
    P0, Q0 = tables(rng, 60, 50, d)
    t = DeviceTables(P0, Q0, np.float64)
    loss = MfSgd(t, len(rows), capi.MF_SOCIALMF).epoch(*arrays(rows), 0.03, 0.02, 0.01)
    Pm, Qm = P0.copy(), Q0.copy()
    lm = M.rating_pmf(Pm, Qm, rows, 0.03, 0.02, 0.01, copies=True)
    P, Q = t.download()
    np.testing.assert_allclose(P, Pm, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(Q, Qm, rtol=1e-11, atol=1e-14)
    assert loss == pytest.approx(lm, rel=1e-12)
    # and it is not PMF's view semantics
    Pv, Qv = P0.copy(), Q0.copy()
    M.rating_pmf(Pv, Qv, rows, 0.03, 0.02, 0.01)
    assert not np.allclose(Q, Qv, rtol=1e-13, atol=0)


@pytest.mark.parametrize("d", (10, 200))
@pytest.mark.parametrize("kind", ("SoRec", "SoReg", "SocialMF", "SREE"))
def test_level_schedule_equals_width_1_bitwise_and_runs_repeat(kind, d):
    g, _, sim, rng = problem(300 + d, n_users=200, n_rel=1500)
    P0, Q0 = tables(rng, 200, 20, d)
    Z0 = rng.random((200, d)) / 10
    a = run_social(kind, g, sim, P0, Q0, Z0, 0.05, 0.3, 0.1)
    assert a[4].schedule.n_levels < a[4].n_steps and a[4].n_waves > 1       # a real schedule
    b = run_social(kind, g, sim, P0, Q0, Z0, 0.05, 0.3, 0.1, sched=lambda sp: sequential_schedule(sp.n_steps))
    c = run_social(kind, g, sim, P0, Q0, Z0, 0.05, 0.3, 0.1)
    for x in (b, c):
        assert np.array_equal(a[0].view(np.uint64), x[0].view(np.uint64))
        if kind == "SoRec":
            assert np.array_equal(a[2].view(np.uint64), x[2].view(np.uint64))
        assert np.float64(a[3]).view(np.uint64) == np.float64(x[3]).view(np.uint64)


@pytest.mark.parametrize("model", ("SoRec", "SoReg", "SocialMF", "RSTE", "SREE"))
def test_model_end_to_end_reproduces_reference_run(model, tmp_path):
    import importlib
    from qrec_amd.util.io import FileIO
    cls = getattr(importlib.import_module(f"qrec_amd.model.rating.{model}"), model)
    meta, z = load(model)
    name = lambda c: f"u{c}" if c >= 0 else f"x{-1 - c}"
    path = tmp_path / "trust.txt"
    path.write_text("".join(f"{name(x)} {name(y)} {w!r}\n" for x, y, w in zip(z["raw_follower"].tolist(), z["raw_followee"].tolist(),
                                                                             z["raw_weight"].tolist())))
    rows = [[f"u{a}", f"i{b}", float(r)] for a, b, r in zip(z["order0_u"].tolist(), z["order0_i"].tolist(), z["order0_r"].tolist())]
    test = [[name(a), f"i{b}" if b >= 0 else f"xi{-1 - b}", float(r)]      # an unknown name keeps one code over all its rows
            for a, b, r in zip(z["test_uid"].tolist(), z["test_iid"].tolist(), z["test_rating"].tolist())]
    conf = conf_from_text(meta["conf"])
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    with redirect_stdout(io.StringIO()):
        m = cls(conf, rows, test, FileIO.loadRelationship(conf, str(path)))
        measure = m.execute()
    assert len(m.social.relation) == meta["relations_kept"]
    np.testing.assert_allclose(m.P, z["P"], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(m.Q, z["Q"], rtol=1e-10, atol=1e-13)
    for k in ("Z", "Bu", "Bi"):
        if k in z.files:
            np.testing.assert_allclose(getattr(m, k), z[k], rtol=1e-10, atol=1e-13)
    assert m.lastLoss == pytest.approx(meta["epochs"][-1]["loss"], rel=1e-11)
    assert len(measure) == len(meta["measure"])
    for g, w in zip(measure, meta["measure"]):
        if ":" in w:
            assert g.split(":")[0] == w.split(":")[0]
            assert float(g.split(":")[1]) == pytest.approx(float(w.split(":")[1]), rel=1e-9)
        else:
            assert g == w
    assert np.array_equal(capi.state_from_python(random.getstate()), z["py_state"])


def epinions_like(seed=11, n_users=40_000, n_items=140_000, n_ratings=660_000, n_edges=490_000):
    """a seeded Epinions-like shape: power-law activity for ratings and trust (synth.gen_edges), ratings in shuffled order"""
    from qrec_amd.synth import gen_edges
    rng = np.random.default_rng(seed)
    u, i = gen_edges(n_users, n_items, n_ratings, seed)
    perm = rng.permutation(u.size); u, i = u[perm], i[perm]
    a, b = gen_edges(n_users, n_users, n_edges, seed + 1)
    r = (rng.integers(1, 11, u.size) / 2).astype(np.float64)
    return u.astype(np.int32), i.astype(np.int32), r, a.astype(np.int32), b.astype(np.int32), rng


def test_one_epinions_shape_epoch_of_every_model_is_finite():
    from qrec_amd.social import synthetic_graph_steps
    U, I, d = 40_000, 140_000, 10
    u, i, r, a, b, rng = epinions_like()
    for kind in ("SoRec", "SoReg", "SocialMF", "RSTE", "SREE"):
        P0, Q0 = rng.random((U, d)) / 3, rng.random((I, d)) / 3
        t = DeviceTables(P0, Q0, np.float64)
        steps = synthetic_graph_steps(kind, U, a, b, np.ones(a.size))
        s = SocialSgd(t, u.size, kind, steps, Z=rng.random((U, d)) / 10, Bu=rng.random(U) / 10, Bi=rng.random(I) / 10)
        loss = s.rating_pass(u, i, r, 0.005, 0.01, 0.01, 0.01, 3.0, alpha=0.5)
        if kind != "RSTE":
            loss = s.social_pass(0.005, 0.1, 0.1)
        P, Q = t.download()
        assert np.isfinite(loss) and np.isfinite(P).all() and np.isfinite(Q).all(), kind
        if kind == "SoRec":
            assert np.isfinite(s.Z()).all()
