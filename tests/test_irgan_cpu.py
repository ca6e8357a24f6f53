"""CPU side of IRGAN: the float64 mirror (tests/irgan_mirror.py) held to the reference's recorded run and to its float64 re-run
(tests/golden/tf_irgan_*.npz), the two rules of the reference's loop the issue singles out (the B-fold regulariser, the first
train_size rows), the draw rule against numpy's own np.random.choice, and the preconditions of the GPU tests' built cases."""
import numpy as np
import pytest

import irgan_cases as C
import irgan_mirror as M
from helpers import rel_err


def test_mirror_reproduces_the_float64_run_of_the_reference_on_the_recorded_draws():
    z, r = C.load(), C.mirror_run()
    assert rel_err(r["losses_d"], C.yard("losses_d")) < C.MIRROR_TOL
    assert rel_err(r["losses_g"], C.yard("losses_g")) < C.MIRROR_TOL
    for v in ("d_P", "d_Q", "d_b"):
        assert rel_err(r["grad0"][v], C.yard(f"grad0_{v}")) < C.MIRROR_TOL, v
    for v in ("g_P", "g_Q", "g_b"):
        assert rel_err(r["grad1"][v], C.yard(f"grad1_{v}")) < C.MIRROR_TOL, v
    assert len(r["snaps"]) == C.N_SNAPS
    for k, snap in enumerate(r["snaps"]):
        for v in C.VARS:
            assert rel_err(snap[v], C.yard(f"snap{k}_{v}")) < C.MIRROR_TOL, (k, v)
    for v in C.VARS:                                   # the run ends on the last snapshot, and the float32 run is near it
        assert np.array_equal(C.yard(f"final_{v}"), C.yard(f"snap5_{v}"))
        assert rel_err(r["snaps"][-1][v], z[f"final_{v}"]) < C.trained_bound(f"final_{v}", z), v


def test_the_float32_run_is_as_far_from_the_float64_run_as_expected():
    """the floors the GPU bounds are built from: generator variables 1e-6 .. 1e-3, discriminator variables below 1e-5"""
    z = C.load()
    for v in C.VARS:
        f = C.floor_of(f"final_{v}", z)
        assert 0 < f < (1e-3 if v.startswith("g_") else 1e-5), (v, f)


def test_the_regulariser_enters_once_per_slot_and_lambda_alone_is_refused():
    """pre_loss is a [B] vector and minimize differentiates its sum: B lambda, not lambda.  The scalar-loss reading misses the
    recorded first-step gradient and the recorded losses by far more than the bound the right one meets"""
    right, wrong = C.mirror_run(True), C.mirror_run(False)
    for v in ("d_P", "d_Q"):
        assert rel_err(right["grad0"][v], C.yard(f"grad0_{v}")) < C.MIRROR_TOL
        assert rel_err(wrong["grad0"][v], C.yard(f"grad0_{v}")) > 1e-3, v
    assert rel_err(wrong["losses_d"], C.yard("losses_d")) > 1e-6
    assert rel_err(wrong["snaps"][0]["d_P"], C.yard("snap0_d_P")) > 1e-4
    # directly: the gradient of a row that occurs once is dz q + B lambda p
    rng = np.random.default_rng(0)
    P, Q, b = rng.normal(size=(4, 3)), rng.normal(size=(5, 3)), rng.normal(size=5)
    u, i, y = np.array([0, 1, 1, 2]), np.array([4, 0, 0, 3]), np.array([1.0, 0.0, 0.0, 1.0])
    r = M.discriminator_gradients(P, Q, b, u, i, y, 0.1)
    assert np.allclose(r["gP"][0], r["dz"][0] * Q[4] + 4 * 0.1 * P[0], rtol=1e-13)
    assert np.allclose(r["gb"][0], r["dz"][1] + r["dz"][2] + 2 * 4 * 0.1 * b[0], rtol=1e-13)      # two occurrences: twice B lambda b
    assert not r["gP"][3].any()


def test_only_the_first_train_size_rows_reach_the_discriminator():
    z, m = C.load(), C.META
    order, pos, calls = z["user_order"].tolist(), C.positives(z), C.draw_calls(z)
    rows = M.get_data_rows(order, pos, [c[1] for c in calls[:len(order)]])
    assert rows[0].size == 3 * m["n_train"] and m["train_size"] == m["n_train"]              # get_data returns three times as many
    batches = M.discriminator_batches(rows, m["train_size"], m["batch_size"])
    assert len(batches) == m["n_d_steps"] == -(-m["train_size"] // m["batch_size"])
    assert [b[0].size for b in batches] == [m["batch_size"]] * (len(batches) - 1) + [m["train_size"] - m["batch_size"] * (len(batches) - 1)]
    for got, want in zip(batches, C.discriminator_batches(z)):
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    last_user_reached = batches[-1][0][-1]
    assert order.index(int(last_user_reached)) < len(order) - 1                                 # the users at the end are never seen
    assert m["n_uniforms"] == C.n_uniforms_of_an_epoch(z) == z["draw_items"].size


def test_the_draw_rule_is_numpys_choice_given_its_uniforms():
    """np.random.choice(n, K, p=p) = searchsorted(cumsum(p) / cumsum(p)[-1], random_sample(K), 'right'): so consuming random_sample(K)
    leaves the global stream where choice leaves it"""
    rng = np.random.default_rng(1)
    w = rng.random(300); w[rng.integers(0, 300, 40)] = 0
    p = w / w.sum()
    np.random.seed(5)
    want = np.random.choice(np.arange(300), size=77, p=p)
    after_choice = np.random.get_state()[1].copy()
    np.random.seed(5)
    x = np.random.random_sample(77)
    assert np.array_equal(np.random.get_state()[1], after_choice)
    assert np.array_equal(M.draw(w, x), want)
    assert C.in_band(M.cdf(w), x, want, 0.0).all()
    assert not C.in_band(M.cdf(w), x, (want + 1) % 300).all()


def test_recorded_negatives_are_never_positives_and_samples_follow_the_mirrors_distribution():
    z = C.load()
    pos, calls, nu_t = C.positives(z), C.draw_calls(z), len(z["user_order"])
    for u, neg in calls[:nu_t]:
        assert neg.size == M.NEG_PER_POS * len(pos[u]) and not set(neg.tolist()) & set(pos[u])
    for u, s in calls[nu_t:]:
        assert s.size == M.GEN_PER_POS * len(pos[u])
    # get_data's weights at the initial generator: every recorded negative has a positive weight in the mirror
    m = M.Mirror(C.initial(), C.META["lr"], C.META["regU"])
    for u, neg in calls[:nu_t]:
        assert (m.negatives_weights(u, pos[u])[neg] > 0).all()


@pytest.mark.parametrize("d", C.WIDTHS)
@pytest.mark.parametrize("n_items", C.N_ITEMS)
def test_built_cases_keep_their_logits_in_the_band_in_float32_too(n_items, d):
    """|z| / T <= 10 in float64 and in float32, and the float32 evaluation of the distributions stays within the draw band of the
    float64 one, for every user of every case the GPU tests draw from"""
    v, csr = C.kernel_case(n_items, d)
    for dt in (np.float64, np.float32):
        for u in range(0, C.N_USERS, 7):
            zl = M.logits(v["g_P"], v["g_Q"], v["g_b"], u, dt)
            assert zl.dtype == dt and np.abs(zl).max() / M.TEMPERATURE <= C.LOGIT_BAND
    for u in range(6):
        pos = C.pos_of(csr, u)
        z64, z32 = (M.logits(v["g_P"], v["g_Q"], v["g_b"], u, dt) for dt in (np.float64, np.float32))
        if pos.size < n_items:
            w64, w32 = M.negative_weights(z64, pos) if pos.size else np.exp(z64 / 0.2), M.negative_weights(z32, pos) if pos.size else np.exp(z32 / np.float32(0.2))
            assert np.abs(M.cdf(w64) - M.cdf(w32)).max() < C.CDF_BAND / 10
        if pos.size:
            assert np.abs(M.cdf(M.mixture(z64, pos)[1]) - M.cdf(M.mixture(z32, pos)[1])).max() < C.CDF_BAND / 10


def test_numpys_own_sampler_passes_the_chi_square_the_throughput_test_uses():
    """the throughput test's statistic at its draw count, applied to np.random.choice itself: pooled bins of expected count >= 5,
    rejected at the 1e-6 level"""
    z = C.load()
    pos = C.positives(z)
    m = M.Mirror(C.initial(), C.META["lr"], C.META["regU"])
    rng = np.random.RandomState(3)
    for u in z["user_order"].tolist():
        w = m.negatives_weights(u, pos[u])
        n = M.NEG_PER_POS * len(pos[u]) * C.CHI2_REPEATS
        s = rng.choice(w.size, n, p=w / w.sum())
        assert C.chi_square_p(np.bincount(s, minlength=w.size), w / w.sum(), n) > C.CHI2_LEVEL, u
    # and the statistic has power: draws from the distribution WITHOUT the temperature are refused
    u = z["user_order"].tolist()[0]
    w, flat = m.negatives_weights(u, pos[u]), M.negative_weights(M.logits(m.p["g_P"], m.p["g_Q"], m.p["g_b"], u), pos[u], T=1.0)
    n = M.NEG_PER_POS * len(pos[u]) * C.CHI2_REPEATS * 50
    s = rng.choice(w.size, n, p=flat / flat.sum())
    assert C.chi_square_p(np.bincount(s, minlength=w.size), w / w.sum(), n) < 1.0
