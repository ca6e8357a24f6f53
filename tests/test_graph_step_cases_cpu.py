"""tests/graph_step_cases.py checked without a device: at every case of the GPU table the plain float32 numpy restatement of the same
operation (oracle/tfmodels.py where it has one) stays within TOL / 3 of the float64 reference under the measure the GPU test uses --
so that a kernel that misses 1e-5 is wrong, not unlucky -- and the cases have the properties they promise."""
import numpy as np
import pytest

import graph_step_cases as GC
from helpers import encode_forced_signs
from oracle import tfmodels as T

HEADROOM = GC.TOL / 3


def _headroom(name, e, case):
    assert e < HEADROOM, f"{name} at {case}: the fp32 restatement is {e:.2e} from the fp64 reference (change the input, not the bound)"
    return f"{e:.1e}"


def _rel(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


# ---- batch BPR ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GC.BPR_CASES, ids=GC.case_id)
def test_bpr_restatement_is_within_headroom_of_the_fp64_reference(case):
    """the scatter as fp32 np.add.at over three random orders of the 3 B lookups (what float atomics may do)"""
    B, d, ld = case
    div, reg, nonzero = GC.BPR_ARGS[case]
    t = GC.bpr_inputs(*case)
    nu, f = t["nu"], np.float32
    prev = t["prev"] if nonzero else None
    want_loss, dE, scale, _, _ = GC.bpr_ref(t["S"], t["u"], t["i"], t["j"], nu, div, reg, prev=prev)
    Ebar = (t["S"] / f(div)).astype(f)
    loss, du, di, dj = T.bpr_batch_loss_and_grads(Ebar[t["u"]], Ebar[nu + t["i"]], Ebar[nu + t["j"]], f(reg), GC.BPR_EPS)
    rows, adds = np.concatenate([t["u"], nu + t["i"], nu + t["j"]]), np.concatenate([du, di, dj])
    seen = dict(loss=_headroom("bpr loss", _rel(loss, want_loss), case))
    rng = np.random.default_rng(B)
    for k in range(3):
        order = rng.permutation(3 * B)
        got = np.zeros_like(Ebar) if prev is None else prev.copy()
        np.add.at(got, rows[order], adds[order])
        seen[f"dE, order {k}"] = _headroom("bpr dE", GC.row_error(got, dE, scale), case)
    print(case, seen)


@pytest.mark.parametrize("case", GC.BPR_CASES, ids=GC.case_id)
def test_bpr_cases_hold_what_they_promise(case):
    B, d, ld = case
    div, reg, _ = GC.BPR_ARGS[case]
    t = GC.bpr_inputs(*case)
    u, i, j, nu, ni = t["u"], t["i"], t["j"], t["nu"], t["ni"]
    assert (nu, ni) == ((37, 29) if case in GC.BPR_SMALL else (1500, 1100))
    assert u.min() >= 0 and u.max() < nu and min(i.min(), j.min()) >= 0 and max(i.max(), j.max()) < ni
    assert np.setdiff1d(np.arange(nu), u).size >= 1 and np.setdiff1d(np.arange(ni), np.concatenate([i, j])).size >= 1
    score = GC.bpr_scores(t, div)
    assert np.abs(score[~t["placed"]]).max() < GC.SCORE_CEILING, "an ordinary score saturates sigmoid"
    if B >= 2:
        assert (u[0], i[0], j[0]) == (u[1], i[1], j[1])
    if B >= 3:
        same = i == j
        assert same.any() and (score[same] == 0).all()
    if case not in GC.BPR_SMALL:
        assert t["placed"].sum() == 8
        assert (np.abs(score[t["placed"]] - GC.SATURATED) < 0.01).sum() == 4 and (np.abs(score[t["placed"]] + GC.SATURATED) < 0.01).sum() == 4
    if case in GC.BPR_WRAPPED:
        words = GC.bpr_ref(t["S"], u, i, j, nu, div, reg)[3][:(nu + ni + 31) // 32]
        mixed = np.count_nonzero((words != 0) & (words != 0xFFFFFFFF))
        assert mixed > words.size // 2, "the row mask should have set and clear bits in most words"


def test_bpr_arguments_are_spread_over_the_cases():
    assert set(GC.BPR_ARGS) == set(GC.BPR_CASES)
    divs = [a[0] for a in GC.BPR_ARGS.values()]
    assert divs.count(1.0) == divs.count(3.0) == len(GC.BPR_CASES) // 2
    assert [a[1] for a in GC.BPR_ARGS.values()].count(0.0) == 1
    assert [a[2] for a in GC.BPR_ARGS.values()].count(True) == len(GC.BPR_CASES) // 2
    assert {c[2] for c in GC.BPR_SMALL} == {c[2] for c in GC.BPR_WRAPPED} == {32, 64, 128, 256}
    groups = {32: 4096, 64: 4096, 128: 2048, 256: 1024}
    assert all(groups[ld] < B <= 2 * groups[ld] for B, _, ld in GC.BPR_WRAPPED) and all(B > 2 * groups[ld] for B, _, ld in GC.BPR_THREE_TRIPS)


def test_bpr_reference_agrees_with_central_differences():
    """d loss / d S by central differences, float64, 9 rows of 5 columns; h = 1e-6: truncation h^2 ~ 1e-12, rounding 1e-16 / h = 1e-10"""
    rng = np.random.default_rng(3)
    nu, S = 4, rng.standard_normal((9, 5))
    u, i, j = np.array([0, 1, 1, 3]), np.array([0, 2, 2, 4]), np.array([1, 2, 0, 3])
    _, dE, _, _, _ = GC.bpr_ref(S, u, i, j, nu, 3.0, 0.01)
    num, h = np.zeros_like(S), 1e-6
    for idx in np.ndindex(*S.shape):
        keep = S[idx]
        S[idx] = keep + h; up = GC.bpr_ref(S, u, i, j, nu, 3.0, 0.01)[0]
        S[idx] = keep - h; down = GC.bpr_ref(S, u, i, j, nu, 3.0, 0.01)[0]
        S[idx] = keep
        num[idx] = (up - down) / (2 * h)
    # dE is the gradient w.r.t. the MEAN rows S / div
    assert np.abs(dE / float(np.float32(3.0)) - num).max() < 1e-7


# ---- BUIR batch -----------------------------------------------------------------------------------------------------------------------
def restated_buir(t):
    """oracle/tfmodels.py::BUIR.loss_and_grads between the two propagations and the optimizer, for the same arguments as buir_ref"""
    f = np.float32
    ui, ii = t["u"], t["nu"] + t["i"]
    online, target = (t["S_on"] / f(t["div"])).astype(f), (t["S_tar"] / f(t["div"])).astype(f)
    xu, xi = online[ui], online[ii]
    qu = np.tanh(xu @ t["W"] + t["b"], dtype=f); qi = np.tanh(xi @ t["W"] + t["b"], dtype=f)
    l1, dqu = T.BUIR._cos_loss_grad(qu, target[ii])
    l2, dqi = T.BUIR._cos_loss_grad(qi, target[ui])
    dpu = dqu * (f(1) - qu * qu); dpi = dqi * (f(1) - qi * qi)
    rows = np.concatenate([ui, ii])
    return l1 + l2, np.concatenate([xu, xi]), np.concatenate([dpu, dpi]), rows, np.concatenate([(dpu @ t["W"].T).astype(f), (dpi @ t["W"].T).astype(f)])


@pytest.mark.parametrize("case", GC.BUIR_CASES, ids=GC.case_id)
def test_buir_restatement_is_within_headroom_of_the_fp64_reference(case):
    B, d, ld = case
    t = GC.buir_inputs(*case)
    prev = t["prev"] if GC.BUIR_ARGS[case][2] else None
    want_loss, Xb, Gb, dS, scale = GC.buir_ref(t["S_on"], t["S_tar"], t["W"], t["b"], t["u"], t["i"], t["nu"], t["div"], prev)
    loss, X, G, rows, dx = restated_buir(t)
    seen = dict(loss=_headroom("buir loss", _rel(loss, want_loss), case), Xb=_headroom("buir Xb", GC.plain_row_error(X, Xb), case),
                Gb=_headroom("buir Gb", GC.plain_row_error(G, Gb), case))
    rng = np.random.default_rng(B)
    for k in range(3):
        order = rng.permutation(2 * B)
        got = np.zeros_like(t["S_on"]) if prev is None else prev.copy()
        np.add.at(got, rows[order], dx[order])
        seen[f"dS, order {k}"] = _headroom("buir dS", GC.row_error(got, dS, scale), case)
    print(case, seen)


@pytest.mark.parametrize("case", GC.BUIR_CASES, ids=GC.case_id)
def test_buir_cases_hold_what_they_promise(case):
    B, d, ld = case
    L, zero_bias, _ = GC.BUIR_ARGS[case]
    t = GC.buir_inputs(*case)
    nu = t["nu"]
    assert (nu, t["ni"]) == (300, 260) and t["div"] == L + 1 and L in (1, 2)
    assert np.abs(t["W"]).max() <= np.sqrt(6.0 / (2 * d)) and t["W"].shape == (d, d)
    assert not t["S_on"][GC.BUIR_ZERO_USER].any() and not t["S_tar"][nu + GC.BUIR_ZERO_ITEM].any()
    assert np.count_nonzero(~t["S_on"].any(1)) == 1 and np.count_nonzero(~t["S_tar"].any(1)) == 1
    assert (t["u"][0], t["i"][0]) == (GC.BUIR_ZERO_USER, GC.BUIR_ZERO_ITEM)
    assert bool(t["b"].any()) != zero_bias
    _, _, Gb, _, _ = GC.buir_ref(t["S_on"], t["S_tar"], t["W"], t["b"], t["u"], t["i"], nu, t["div"])
    assert not Gb[0].any(), "an all-zero target row gives no gradient"
    if zero_bias and B >= 3:                                  # q = 0: the clamp of |q| -> dPre = -that / 2 * 1e6
        assert np.allclose(np.linalg.norm(Gb[1]), 0.5e6, rtol=1e-9)


def test_buir_arguments_are_spread_over_the_cases():
    assert set(GC.BUIR_ARGS) == set(GC.BUIR_CASES)
    small = set(GC.BUIR_SMALL)
    for pos in range(3):
        values = {a[pos] for a in GC.BUIR_ARGS.values()}
        assert values == {a[pos] for c, a in GC.BUIR_ARGS.items() if c in small} == {a[pos] for c, a in GC.BUIR_ARGS.items() if c not in small}
    groups = {32: 8192, 64: 4096, 128: 2048}
    assert {c[2] for c in GC.BUIR_SMALL} == {32, 64, 128} and all(groups[ld] < B <= 2 * groups[ld] for B, _, ld in GC.BUIR_WRAPPED)


def test_buir_reference_agrees_with_central_differences():
    rng = np.random.default_rng(4)
    nu, d = 3, 4
    S_on, S_tar, W, b = rng.standard_normal((7, d)), rng.standard_normal((7, d)), rng.standard_normal((d, d)) * 0.5, rng.standard_normal((1, d)) * 0.3
    u, i = np.array([0, 2, 2]), np.array([1, 1, 3])
    _, _, _, dS, _ = GC.buir_ref(S_on, S_tar, W, b, u, i, nu, 2.0)
    num, h = np.zeros_like(S_on), 1e-6
    for idx in np.ndindex(*S_on.shape):
        keep = S_on[idx]
        S_on[idx] = keep + h; up = GC.buir_ref(S_on, S_tar, W, b, u, i, nu, 2.0)[0]
        S_on[idx] = keep - h; down = GC.buir_ref(S_on, S_tar, W, b, u, i, nu, 2.0)[0]
        S_on[idx] = keep
        num[idx] = (up - down) / (2 * h)
    assert np.abs(dS / 2.0 - num).max() < 1e-7            # dS is un-divided: the gradient w.r.t. the mean rows S_on / div


# ---- perturbation --------------------------------------------------------------------------------------------------------------------
def restated_perturb(x, noise, eps=GC.PERTURB_EPS):
    """SimGCL.py:33-35 in float32, the forced signs decoded as include/qrec_hip.h states them"""
    f = np.float32
    a = np.abs(noise)
    mag = np.where(a >= 4, a - f(4), np.where(a >= 2, a - f(2), noise)).astype(f)
    sign = np.where(a >= 4, f(0), np.where(a >= 2, np.sign(noise), np.sign(x))).astype(f)
    nz, _ = T.l2_normalize_rows(mag)
    return (x + (sign * nz) * f(eps)).astype(f)


@pytest.mark.parametrize("case", GC.PERTURB_CASES, ids=GC.case_id)
def test_perturb_restatement_is_within_headroom_of_the_fp64_reference(case):
    n, d, ld = case
    t = GC.perturb_inputs(*case)
    seen = {}
    for v in range(2):
        delta = GC.perturb_delta_ref(t["x"], t["noise"][v])
        e = restated_perturb(t["x"], t["noise"][v])
        seen[f"view {v}"] = _headroom("perturb delta", GC.delta_error(e, t["x"], delta), case)
        want = t["acc0"].astype(np.float64) + t["x"].astype(np.float64) + delta
        seen[f"accum {v}"] = _headroom("perturb accum", GC.plain_row_error((t["acc0"] + e).astype(np.float32), want), case)
    rows = GC.replay_rows(n, ld)[:8]
    drawn = GC.philox_noise(rows, d, ld, GC.PERTURB_SEED, GC.PERTURB_STREAMS[0])
    e = restated_perturb(t["x"][rows], drawn.astype(np.float32))
    seen["drawn"] = _headroom("perturb delta, drawn noise", GC.delta_error(e, t["x"][rows], GC.perturb_delta_ref(t["x"][rows], drawn)), case)
    print(case, seen)


@pytest.mark.parametrize("case", GC.PERTURB_CASES, ids=GC.case_id)
def test_perturb_cases_hold_what_they_promise(case):
    n, d, ld = case
    t = GC.perturb_inputs(*case)
    assert (t["x"] == 0).any()
    for v, nz in enumerate(t["noise"]):
        mag, forced = GC.decode_noise(nz)
        assert np.count_nonzero(~nz.any(1)) == (n >= 3) and (mag >= 0).all() and (mag <= 1).all()
        assert forced[0, 1] != 2 and t["x"][0, 1] == 0 and forced[0, 4] != 2
        if n * d > 1000:
            assert {-1.0, 0.0, 1.0, 2.0} == set(np.unique(forced))
    assert t["marked"].sum() >= 1
    if case in GC.PERTURB_SUBSET_CASES:
        assert 0.05 * n < t["marked"].sum() < 0.15 * n
    if case in GC.PERTURB_WRAPPED:
        wrap = GC.PERTURB_ROWS_PER_TRIP[ld]
        rows = GC.replay_rows(n, ld)
        assert wrap < n <= 2 * wrap and {0, wrap - 1, wrap, n - 1} <= set(rows.tolist()) and rows.size <= 4 * GC.REPLAY_ROWS


def test_perturb_arguments_are_spread_over_the_cases():
    assert set(GC.PERTURB_ARGS) == set(GC.PERTURB_CASES)
    small = set(GC.PERTURB_SMALL)
    for pos in range(2):
        assert {True, False} == {a[pos] for c, a in GC.PERTURB_ARGS.items() if c in small} == {a[pos] for c, a in GC.PERTURB_ARGS.items() if c not in small}
    assert {c[2] for c in GC.PERTURB_SMALL} == {32, 64, 256} and {c[2] for c in GC.PERTURB_WRAPPED} == {32, 64, 128, 256}
    assert sum(c in small for c in GC.PERTURB_SUBSET_CASES) == 1 and len(GC.PERTURB_SUBSET_CASES) == 2


def test_forced_sign_encoding_round_trips():
    u = np.array([0.0, 0.25, 0.75, 0.5], np.float32)
    mag, forced = GC.decode_noise(encode_forced_signs(u, np.array([1, -1, 0, 1])))
    assert np.array_equal(mag, u) and forced.tolist() == [1.0, -1.0, 0.0, 1.0]
    assert GC.decode_noise(u)[1].tolist() == [2.0] * 4


# ---- element-wise ---------------------------------------------------------------------------------------------------------------------
def _elementwise_distances():
    """the largest |fp32 numpy restatement - fp64 reference| of every element-wise output over the three sizes"""
    f = np.float32
    worst = dict(scale_copy=0.0, ema=0.0, theta=0.0, m=0.0, v=0.0)
    for n in GC.ELEMENTWISE_N:
        t = GC.elementwise_inputs(n)
        worst["scale_copy"] = max(worst["scale_copy"], np.abs(GC.SCALE_ALPHA * t["src"] - GC.scale_copy_ref(t["src"])).max())
        ema = (t["target"] * GC.EMA_TAU + t["src"] * (f(1) - GC.EMA_TAU)).astype(f)
        worst["ema"] = max(worst["ema"], np.abs(ema - GC.ema_ref(t["target"], t["src"])).max())
        theta, opt, l2 = t["theta"].copy(), T.AdamTF114((n,), GC.ADAM_LR), f(GC.ADAM_L2[n])
        for alpha, G in zip(GC.adam_alphas(), t["grads"]):
            assert float(opt.alpha()) == alpha
            opt.step(theta, (GC.ADAM_GRAD_SCALE * G + l2 * theta).astype(f))
        for name, got, want in zip(("theta", "m", "v"), (theta, opt.m, opt.v), GC.adam_ref(t["theta"], t["grads"], GC.ADAM_L2[n])):
            assert got.dtype == f
            worst[name] = max(worst[name], np.abs(got - want).max())
    return worst


def test_elementwise_abs_tols_are_three_times_the_restatements_distance():
    """each constant is 3 x the measured distance, rounded up to two digits"""
    worst = _elementwise_distances()
    print({k: f"{v:.2e}" for k, v in worst.items()})
    for name, const in (("scale_copy", GC.ABS_TOL_SCALE_COPY), ("ema", GC.ABS_TOL_EMA), ("theta", GC.ABS_TOL_ADAM_THETA), ("m", GC.ABS_TOL_ADAM_M),
                        ("v", GC.ABS_TOL_ADAM_V)):
        assert 3 * worst[name] <= const <= 3 * worst[name] * 1.1, (name, worst[name], const)


def test_elementwise_sizes_sit_where_the_grid_wraps():
    per_trip = 2048 * 256 * 4
    assert GC.ELEMENTWISE_N == [4, per_trip, 2 * per_trip + 260] and all(n % 4 == 0 for n in GC.ELEMENTWISE_N)
    assert set(GC.ADAM_L2.values()) == {0.0, 0.01} and GC.ADAM_L2[GC.ELEMENTWISE_N[-1]] != 0
