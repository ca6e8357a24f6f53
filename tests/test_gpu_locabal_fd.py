"""LOCABAL and SocialFD on the device: each of the four kernel entries against the host mirror (tests/locabal_fd_mirror.py) on
a synthetic problem built so that every path runs, the width limit, empty passes, run-to-run and wave-count determinism,
and both classes end to end against the recorded reference runs."""
import functools
import io
import math
import random
from collections import Counter
from contextlib import redirect_stdout

import numpy as np
import pytest

import locabal_fd_mirror as L
from helpers import conf_from_text
from social_mirror import Graph, fold
from test_locabal_fd_cpu import load
from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer
from qrec_amd.engine import DeviceTables, SocialHSgd
from qrec_amd.social import Edges, UserSteps

pytestmark = pytest.mark.gpu

DIMS = (5, 10, 64, 65, 128)
U, I, N_REL, N_ROWS = 60, 50, 300, 400
# RSTE's serial rating pass in test_gpu_social.py
TABLE_TOL = dict(rtol=1e-11, atol=1e-14)
LOSS_REL = 1e-12
LR, REGU, REGI, REGS, ALPHA, ETA, BETA, MEAN = 0.0005, 0.01, 0.02, 0.05, 0.4, 0.1, 0.2, 0.55


@functools.lru_cache(maxsize=None)
def problem(d):
    """60 users, 50 items, 300 relations (12 self-follows, duplicates), 400 rating rows in all three SocialFD bands; half
    of the users sit far from the items under H (distance >= 1), the others near; a third of the users has no weight"""
    rng = np.random.default_rng(1000 + d)
    a = rng.integers(0, U, N_REL); b = rng.integers(0, U, N_REL)
    a[:12] = b[:12] = np.arange(12)                                   # self-follows
    a = np.concatenate([a, a[:7]]); b = np.concatenate([b, b[:7]])    # duplicate relations
    g = Graph(a.tolist(), b.tolist(), (rng.integers(1, 5, a.size) / 4).tolist())
    rows = list(zip(rng.integers(0, U, N_ROWS).tolist(), rng.integers(0, I, N_ROWS).tolist(),
                    rng.choice([0.2, 0.4, 0.5, 0.6, 0.8, 1.0], N_ROWS).tolist()))
    far = 2 * (1.5 / math.sqrt(d) + 1 / 6)                            # |H^T (x - y)|^2 starts near 9 for these users, near 0.1 for the rest
    P0 = rng.random((U, d)) * np.where(np.arange(U) % 2 == 0, far, 1 / 3)[:, None]
    Q0 = rng.random((I, d)) / 3
    Hfd = rng.random((d, d)) * 4 / d
    Hloc = rng.random((d, d)) / d
    Bu, Bi = rng.random(U) / 5, rng.random(I) / 5
    W = 1 / (1 + np.log(rng.permutation(U) + 1.0)); W[rng.permutation(U)[:U // 3]] = 0.0
    S = {}
    for x, y, _ in g.relation:
        S.setdefault(x, {})[y] = float(rng.random() - 0.2)
    edges = [(x, y, S[x][y]) for x in S for y in S[x]]
    for arr in (P0, Q0, Hfd, Hloc, Bu, Bi, W):
        arr.setflags(write=False)
    return dict(g=g, rows=rows, P0=P0, Q0=Q0, Hfd=Hfd, Hloc=Hloc, Bu=Bu, Bi=Bi, W=W, edges=edges, steps=L.fd_steps(g, U))


def arrays(rows):
    return (np.array([u for u, _, _ in rows], np.int32), np.array([i for _, i, _ in rows], np.int32),
            np.array([r for _, _, r in rows], np.float64))


def edges_of(edges):
    return Edges(np.array([u for u, _, _ in edges], np.int32), np.array([k for _, k, _ in edges], np.int32),
                 np.array([s for _, _, s in edges], np.float64))


def steps_of(steps):
    ptr = np.concatenate([[0], np.cumsum([len(f) for _, f in steps])]).astype(np.int64)
    ids = np.array([f for _, fol in steps for f in fol], dtype=np.int32)
    return UserSteps(np.array([u for u, _ in steps], np.int32), ptr, ids, np.ones(ids.size))


ENTRIES = ("locabal_rating", "locabal_social", "socialfd_rating", "socialfd_social")
START = 12.5                  # the running loss a social pass adds its terms onto


@functools.lru_cache(maxsize=None)
def mirror(entry, d):
    """the mirror's result of one entry (numpy's dot), computed once: dict(P, Q, H, Bu, Bi, loss, count)"""
    pr = problem(d)
    ops = L.NumpyOps()
    P, Q, Bu, Bi = pr["P0"].copy(), pr["Q0"].copy(), pr["Bu"].copy(), pr["Bi"].copy()
    H = (pr["Hloc"] if entry.startswith("locabal") else pr["Hfd"]).copy()
    count = Counter()
    if entry == "locabal_rating":
        loss = L.rating_locabal(P, Q, pr["W"], pr["rows"], LR, REGU, REGI, ops, count)
    elif entry == "locabal_social":
        slots = np.zeros(len(pr["edges"]))
        L.social_locabal(P, H, pr["edges"], LR, ALPHA, REGS, slots, ops, count)
        loss = fold(START, slots)
    elif entry == "socialfd_rating":
        loss = L.rating_socialfd(P, Q, Bu, Bi, H, pr["rows"], LR, REGU, REGI, ETA, ALPHA, MEAN, ops, count)
    else:
        slots = np.zeros(sum(len(f) for _, f in pr["steps"]))
        L.social_socialfd(P, H, pr["steps"], LR, ETA, BETA, slots, ops, count)
        loss = fold(START, slots)
    return dict(P=P, Q=Q, H=H, Bu=Bu, Bi=Bi, loss=float(loss), count=count)


def device(entry, d, n_waves=0, empty=False):
    """one entry on the device through engine.SocialHSgd; dict(P, Q, H, Bu, Bi, loss)"""
    pr = problem(d)
    t = DeviceTables(pr["P0"], pr["Q0"], np.float64)
    rows = [] if empty else pr["rows"]
    if entry.startswith("locabal"):
        s = SocialHSgd(t, len(rows), "LOCABAL", edges_of([] if empty else pr["edges"]), pr["Hloc"], W=pr["W"], n_waves=n_waves)
    else:
        s = SocialHSgd(t, len(rows), "SocialFD", steps_of([] if empty else pr["steps"]), pr["Hfd"], Bu=pr["Bu"], Bi=pr["Bi"],
                       n_waves=n_waves)
    if entry == "locabal_rating":
        loss = s.rating_pass(*arrays(rows), LR, REGU, REGI)
    elif entry == "locabal_social":
        loss = s.social_pass(LR, alpha=ALPHA, regS=REGS, start=START)
    elif entry == "socialfd_rating":
        loss = s.rating_pass(*arrays(rows), LR, REGU, REGI, ETA, ALPHA, MEAN)
    else:
        loss = s.social_pass(LR, eta=ETA, beta=BETA, start=START)
    P, Q = t.download()
    Bu, Bi = s.biases() if entry.startswith("socialfd") else (pr["Bu"], pr["Bi"])
    return dict(P=P, Q=Q, H=s.H(), Bu=Bu, Bi=Bi, loss=loss)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k], dtype=np.float64).view(np.uint64), np.asarray(b[k], dtype=np.float64).view(np.uint64))
               for k in ("P", "Q", "H", "Bu", "Bi", "loss"))


@pytest.mark.parametrize("d", DIMS)
def test_the_synthetic_problem_takes_every_path_at_least_ten_times(d):
    c = mirror("socialfd_rating", d)["count"]
    assert min(c["high"], c["mid"], c["low_near"], c["low_far"]) >= 10, c
    c = mirror("locabal_rating", d)["count"]
    assert min(c["weighted"], c["unweighted"]) >= 10, c
    c = mirror("locabal_social", d)["count"]
    assert min(c["self_loop"], c["same_user_again"]) >= 10, c
    assert mirror("socialfd_social", d)["count"]["self_loop"] >= 10
    for e in ENTRIES:
        m = mirror(e, d)
        assert all(np.isfinite(m[k]).all() for k in ("P", "Q", "H", "Bu", "Bi", "loss")), e


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_matches_the_mirror(entry, d):
    want, got = mirror(entry, d), device(entry, d)
    for k in ("P", "Q", "H", "Bu", "Bi"):
        dev = float(np.max(np.abs(got[k] - want[k]) / (TABLE_TOL["atol"] / TABLE_TOL["rtol"] + np.abs(want[k]))))
        print(f"parity {entry} d={d} {k}: max |got - want| / (atol/rtol + |want|) = {dev:.3e}")
    print(f"parity {entry} d={d} loss: rel = {abs(got['loss'] - want['loss']) / abs(want['loss']):.3e}")
    for k in ("P", "Q", "H", "Bu", "Bi"):
        np.testing.assert_allclose(got[k], want[k], err_msg=k, **TABLE_TOL)
    assert got["loss"] == pytest.approx(want["loss"], rel=LOSS_REL)
    pr = problem(d)
    if entry.endswith("social"):                                   # a social pass touches neither Q nor the biases
        assert np.array_equal(got["Q"], pr["Q0"]) and np.array_equal(got["Bu"], pr["Bu"])
    if entry == "locabal_rating":
        assert np.array_equal(got["H"], pr["Hloc"])


@pytest.mark.parametrize("d", (10, 128))
@pytest.mark.parametrize("entry", ENTRIES)
def test_two_launches_and_every_wave_count_give_the_same_bits(entry, d):
    a = device(entry, d)
    assert same_bits(a, device(entry, d))
    if entry != "locabal_rating":                                  # one wavefront by construction
        for nw in (1, 3, 16):
            assert same_bits(a, device(entry, d, n_waves=nw)), nw


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_pass_with_zero_steps_is_a_no_op(entry):
    pr = problem(10)
    got = device(entry, 10, empty=True)
    assert np.array_equal(got["P"], pr["P0"]) and np.array_equal(got["Q"], pr["Q0"])
    assert np.array_equal(got["H"], pr["Hloc"] if entry.startswith("locabal") else pr["Hfd"])
    assert np.array_equal(got["Bu"], pr["Bu"]) and np.array_equal(got["Bi"], pr["Bi"])
    assert got["loss"] == (0.0 if entry.endswith("rating") else START)


def test_width_129_is_unsupported_by_all_four_entries_and_touches_nothing():
    d, n = 129, 8
    rng = np.random.default_rng(9)
    host = dict(P=rng.random((U, d)), Q=rng.random((I, d)), H=rng.random((d, d)), Bu=rng.random(U), Bi=rng.random(I),
                loss=np.array([7.0]), slots=np.full(n, 3.0))
    dev = {k: DeviceBuffer.from_numpy(v) for k, v in host.items()}
    idx = DeviceBuffer.from_numpy(np.arange(n, dtype=np.int32))
    ptr = DeviceBuffer.from_numpy(np.arange(n + 1, dtype=np.int64))
    val = DeviceBuffer.from_numpy(np.full(n, 0.5))
    w = DeviceBuffer.from_numpy(np.ones(U))
    calls = (
        lambda: capi.locabal_sgd_ordered(dev["P"], dev["Q"], d, d, w, idx, idx, val, n, LR, REGU, REGI, dev["loss"]),
        lambda: capi.locabal_social_pass(dev["P"], dev["H"], d, d, idx, idx, val, n, LR, ALPHA, REGS, dev["slots"]),
        lambda: capi.socialfd_sgd_ordered(dev["P"], dev["Q"], dev["Bu"], dev["Bi"], dev["H"], d, d, idx, idx, val, n, LR, REGU, REGI, ETA,
                                          ALPHA, MEAN, dev["loss"]),
        lambda: capi.socialfd_social_pass(dev["P"], dev["H"], d, d, idx, n, ptr, idx, LR, ETA, BETA, dev["slots"]),
    )
    for call in calls:
        with pytest.raises(capi.QRecError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED and "128" in str(e.value)
    for k, v in host.items():
        assert np.array_equal(dev[k].numpy().reshape(v.shape), v), k


@pytest.mark.parametrize("model", ("LOCABAL", "SocialFD"))
def test_model_end_to_end_reproduces_reference_run(model, tmp_path):
    from qrec_amd.QRec import resolve_model
    from qrec_amd.util.io import FileIO
    cls = resolve_model(model)
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
    for k in ("P", "Q", "H", "Bu", "Bi"):
        if k in z.files:
            np.testing.assert_allclose(getattr(m, k), z[k], rtol=1e-10, atol=1e-13, err_msg=k)
    assert m.lastLoss == pytest.approx(meta["epochs"][-1]["loss"], rel=1e-11)
    assert len(measure) == len(meta["measure"])
    for g, w in zip(measure, meta["measure"]):
        if ":" in w:
            assert g.split(":")[0] == w.split(":")[0]
            assert float(g.split(":")[1]) == pytest.approx(float(w.split(":")[1]), rel=1e-9)
        else:
            assert g == w
    assert np.array_equal(capi.state_from_python(random.getstate()), z["py_state"])
