"""CPU side of DiffNet / DHCF: the float64 mirror (tests/diffusion_mirror.py) against the reference's own recorded runs, its
gradients against finite differences, the product's host-side graph builders against the mirror, the class lookup, and the
headroom under 2^24 on which the bit-for-bit dense-layer cases of tests/test_gpu_dense_layer.py rest."""
import numpy as np
import pytest
import scipy.sparse as sp

import dense_layer_cases as D
import diffusion_cases as C
import diffusion_mirror as M
from helpers import check, rel_err


def _replay(name):
    """the mirror through the fixture's batches: (losses, first-step gradients, trained variables)"""
    m, z = C.load(name)
    nu, ni = m["n_users"], m["n_items"]
    names = C.VARS[name]
    opt = M.Adam([z[f"init_{v}"] for v in names], m["lr"])
    if name == C.DIFFNET:
        S = M.social_matrix(nu, z["follower"], z["followee"]); A = M.rating_matrix(nu, ni, z["train_uid"], z["train_iid"])
    else:
        Au, Ai = M.dhcf_operators(nu, ni, z["train_uid"], z["train_iid"])
        H = sp.block_diag([Au, Ai]).tocsr()
    losses, first = [], None
    for k, u, i, j in C.batches(z):
        U, V, W = opt.p[0], opt.p[1], opt.p[2:]
        if name == C.DIFFNET:
            loss, dU, dV, dW = M.diffnet_loss_grads(U, V, W, S, A, u, i, j, m["regU"])
        else:
            loss, dU, dV, dW = M.dhcf_loss_grads(U, V, W, H, u, i, j, m["regU"], masks=C.dhcf_masks(m, z, k))
        losses.append(loss)
        if k == 0:
            first = [dU, dV] + dW
        opt.step([dU, dV] + dW)
    return m, z, np.array(losses), first, opt.p


@pytest.mark.parametrize("name", [C.DIFFNET, C.DHCF])
def test_mirror_reproduces_the_reference_run(name):
    """losses of all steps and first-step gradients at 1e-5; trained variables at max(1e-5, 2.5 floors), the floor being the
    committed float32 run's distance from the committed float64 run of the same batches and masks"""
    m, z, losses, first, final = _replay(name)
    assert losses.size == m["n_steps"] >= 12
    check(f"{name} losses vs the reference run", rel_err(losses, z["losses"][:, 0]), C.GRAD_TOL)
    for v, g, p in zip(C.VARS[name], first, final):
        check(f"{name} first-step gradient of {v}", rel_err(g, z[f"grad0_{v}"]), C.GRAD_TOL)
        floor = C.floor_of(name, f"final_{v}", z)
        check(f"{name} floor of {v} (recorded)", floor, 1.0, kind="info")
        check(f"{name} trained {v} vs the reference run", rel_err(p, z[f"final_{v}"]), C.trained_bound(name, f"final_{v}", z), kind="floor")
        check(f"{name} trained {v} vs the float64 run", rel_err(p, C.YARD[f"{name}/final_{v}"]), C.trained_bound(name, f"final_{v}", z), kind="floor")


def _fd(f, params, grads, rng, n_probe=6, h=1e-6):
    """central differences of f along random directions of every parameter against <grad, direction>"""
    worst = 0.0
    for p, g in zip(params, grads):
        for _ in range(n_probe):
            dirn = rng.standard_normal(p.shape)
            old = p.copy()
            p[...] = old + h * dirn; fp = f()
            p[...] = old - h * dirn; fm = f()
            p[...] = old
            num, ana = (fp - fm) / (2 * h), float((g * dirn).sum())
            worst = max(worst, abs(num - ana) / max(abs(ana), 1e-8))
    return worst


def _toy(rng, nu=23, ni=31, d=5, nnz=140, B=40):
    uid = rng.integers(0, nu, nnz); iid = rng.integers(0, ni, nnz)
    keep = np.unique(np.stack([uid, iid], 1), axis=0)
    uid, iid = keep[:, 0], keep[:, 1]
    b = rng.integers(0, uid.size, B)
    u, i, j = uid[b], iid[b], rng.integers(0, ni, B)
    U, V = rng.standard_normal((nu, d)) * 0.3, rng.standard_normal((ni, d)) * 0.3
    return nu, ni, d, uid, iid, u, i, j, U, V


def test_mirror_gradients_match_finite_differences():
    rng = np.random.default_rng(5)
    nu, ni, d, uid, iid, u, i, j, U, V = _toy(rng)
    fo = rng.integers(0, nu, 50); fe = rng.integers(0, nu, 50)
    S = M.social_matrix(nu, fo, fe); A = M.rating_matrix(nu, ni, uid, iid)
    for L in (1, 2, 3):
        Ws = [rng.standard_normal((2 * d, d)) * 0.5 for _ in range(L)]
        _, dU, dV, dW = M.diffnet_loss_grads(U, V, Ws, S, A, u, i, j, 0.05)
        worst = _fd(lambda: M.diffnet_loss_grads(U, V, Ws, S, A, u, i, j, 0.05)[0], [U, V] + Ws, [dU, dV] + dW, rng)
        check(f"DiffNet mirror, {L} layers: analytic vs central differences", worst, 1e-5)
    Au, Ai = M.dhcf_operators(nu, ni, uid, iid)
    H = sp.block_diag([Au, Ai]).tocsr()
    Ws = [rng.standard_normal((d, d)) * 0.5 for _ in range(2)]
    masks = [(rng.random((nu + ni, d)) >= 0.1).astype(np.float64) for _ in range(2)]
    for mk in (None, masks):
        _, dU, dV, dW = M.dhcf_loss_grads(U, V, Ws, H, u, i, j, 0.05, masks=mk)
        worst = _fd(lambda: M.dhcf_loss_grads(U, V, Ws, H, u, i, j, 0.05, masks=mk)[0], [U, V] + Ws, [dU, dV] + dW, rng)
        check("DHCF mirror: analytic vs central differences", worst, 1e-5)


def test_factored_dhcf_operator_equals_the_formed_product():
    """diag(A_u, A_i) = P Q on the fixture graph: the product's float32 factors against scipy's formed matrices (DHCF.py:33-47)"""
    from qrec_amd.diffusion import dhcf_factor_graphs
    m, z = C.load(C.DHCF)
    nu, ni = m["n_users"], m["n_items"]
    Au, Ai = M.dhcf_operators(nu, ni, z["train_uid"], z["train_iid"])
    H = sp.block_diag([Au, Ai]).tocsr()
    P, Q = dhcf_factor_graphs(nu, ni, z["train_uid"], z["train_iid"])
    assert P.dtype == np.float32 and P.nnz == Q.nnz == 2 * np.unique(np.stack([z["train_uid"], z["train_iid"]], 1), axis=0).shape[0]
    X = np.random.default_rng(0).standard_normal((nu + ni, 8))
    check("factored operator applied to a table vs the formed one", rel_err(P.astype(np.float64) @ (Q.astype(np.float64) @ X), H @ X), 1e-6)
    Pm, Qm = M.dhcf_factors(nu, ni, z["train_uid"], z["train_iid"])
    check("product's factors vs the mirror's", max(rel_err(P.toarray(), Pm.toarray()), rel_err(Q.toarray(), Qm.toarray())), 1e-6)
    check("formed from the factors vs formed by scipy", rel_err((Pm @ Qm).toarray(), H.toarray()), 1e-12)


def test_social_csr_of_the_product_equals_the_mirror():
    from qrec_amd.diffusion import rating_mean_csr, social_csr
    m, z = C.load(C.DIFFNET)
    nu, ni = m["n_users"], m["n_items"]
    assert z["follower"].size == m["n_relations"] and np.unique(z["follower"]).size == m["users_with_followee"] > 200
    S, Sm = social_csr(nu, z["follower"], z["followee"]), M.social_matrix(nu, z["follower"], z["followee"])
    assert S.dtype == np.float32 and np.array_equal(S.toarray().astype(np.float64), Sm.toarray())
    rows = np.asarray(Sm.sum(1)).ravel()
    assert np.allclose(rows[np.unique(z["follower"])], 1.0, atol=1e-6) and (rows[np.setdiff1d(np.arange(nu), z["follower"])] == 0).all()
    A, Am = rating_mean_csr(nu, ni, z["train_uid"], z["train_iid"]), M.rating_matrix(nu, ni, z["train_uid"], z["train_iid"])
    assert np.array_equal(A.toarray().astype(np.float64), Am.toarray())
    # a pair listed twice adds up
    S2 = social_csr(3, np.array([0, 0, 0, 1]), np.array([1, 1, 2, 2]))
    assert S2.toarray().tolist() == [[0.0, 1.0, 0.5], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]


@pytest.mark.parametrize("name", ["DiffNet", "DHCF"])
def test_resolve_model_returns_the_class(name):
    from qrec_amd.QRec import resolve_model
    cls = resolve_model(name)
    assert cls.__name__ == name and hasattr(cls, "trainModel") and hasattr(cls, "predictForRanking")


# ---- the integer cases of the dense-layer tests are exact in fp32 ------------------------------------------------------------------
@pytest.mark.parametrize("ld,d,n", D.EXACT_CASES)
def test_integer_dense_layer_cases_stay_below_two_to_the_24(ld, d, n):
    """tests/test_gpu_dense_layer.py asserts array_equal between fp32 MFMA results and the float64 mirror on these inputs.  That
    holds whatever the summation tree iff no sum of absolute products (+ residual, + prior dX1) reaches 2^24: checked here in
    float64 for every output of every mode, the 69,669-row weight gradient included."""
    t = D.integer_inputs(ld, d, n)
    for a in t.values():
        assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and np.abs(a).max() == 2
    for mode, worst in D.headroom(t).items():
        check("integer dense-layer case: largest sum of |a||b| over all outputs", worst, D.EXACT_LIMIT, ctx=(ld, d, n, mode), kind="info")
        assert worst < D.EXACT_LIMIT


@pytest.mark.parametrize("ld,d,n", D.NGCF_EXACT_CASES + [c[:3] for c in D.NGCF_SUBSET_CASES])
def test_integer_ngcf_layer_cases_stay_below_two_to_the_24(ld, d, n):
    """the same for NGCF's layer, pre = (S + E) W1 + (E * S) W2: |S + E| and |E * S| are at most 4, so the forward stays below 16 d,
    dside = dA1 + dA2 * E and dE below 4 d + 8 d = 12 d, and the weight gradient below 8 n (557,352 at 69,669 rows).  A row subset
    sums a part of what is bounded here."""
    t = D.ngcf_inputs(ld, d, n, integer=True)
    for a in t.values():
        assert a.dtype == np.float32 and np.array_equal(a, np.round(a)) and np.abs(a).max() == 2
    fwd, bwd, wgrad = D.ngcf_headroom(t)
    assert fwd <= 16 * d and bwd <= 12 * d and wgrad <= 8 * n
    for what, worst in (("forward", fwd), ("backward", bwd), ("weight gradient", wgrad)):
        check(f"integer NGCF-layer case: largest sum of |a||b|, {what}", worst, D.EXACT_LIMIT, ctx=(ld, d, n), kind="info")
    assert 16 * 128 < D.EXACT_LIMIT and 8 * 69669 == 557352 < D.EXACT_LIMIT


def test_ngcf_mirror_is_the_backward_of_its_forward():
    """the float64 formulas the GPU test compares with, against central differences of sum(pre * G)"""
    rng = np.random.default_rng(9)
    E, S, G, W1, W2 = (rng.standard_normal(s) for s in ((7, 5), (7, 5), (7, 5), (5, 5), (5, 5)))
    dside, dE, gW1, gW2 = M.ngcf_bwd(G, E, S, W1, W2)
    loss = lambda E, S, W1, W2: float((M.ngcf_fwd(E, S, W1, W2) * G).sum())
    args = [E, S, W1, W2]
    for k, grad in ((0, dE), (1, dside), (2, gW1), (3, gW2)):
        num = np.zeros_like(grad)
        for idx in np.ndindex(grad.shape):
            hi = [a.copy() for a in args]; lo = [a.copy() for a in args]
            hi[k][idx] += 1e-6; lo[k][idx] -= 1e-6
            num[idx] = (loss(*hi) - loss(*lo)) / 2e-6
        assert rel_err(grad, num) < 1e-8, k


@pytest.mark.parametrize("ld,d,n", D.NORM_CASES)
def test_integer_dpre_norm_cases_stay_below_two_to_the_24(ld, d, n):
    """the same for dpre = (dz - z (z.dz)) inv gate: integers times powers of two, every intermediate far below 2^24"""
    t = D.norm_integer_inputs(ld, d, n)
    assert np.abs(t["dAll"]).min() >= 1 and np.abs(t["All"]).min() >= 1 and not t["gate"][:, d:].any() and not t["dZ"][:, d:].any()
    for col_off in (d, 2 * d):
        assert D.norm_headroom(t, d, col_off) < D.EXACT_LIMIT
    # the float64 formula the GPU test compares with, against an independent statement of it on one row
    want = D.dpre_norm_f64(t["dAll"], t["All"], d, t["dZ"], t["inv"], t["gate"], d)
    z = t["All"][0, d:2 * d].astype(np.float64); dz = t["dAll"][0, d:2 * d].astype(np.float64) + t["dZ"][0, :d]
    jac = (np.eye(d) - np.outer(z, z)) * float(t["inv"][0])          # d normalize / d nxt at |nxt| = 1 / inv, z taken as given
    assert np.array_equal(want[0], (jac @ dz) * t["gate"][0, :d])


def test_worst_tile_pins_an_error_the_table_norm_dilutes():
    want = np.ones((70000, 64)); got = want.copy()
    got[32 * 7:32 * 8] *= 1 + 1e-4                                     # one wavefront's tile off by 1e-4
    assert rel_err(got, want) < C.GRAD_TOL < D.worst_tile(got, want)
    assert abs(D.worst_tile(got, want) - 1e-4) < 1e-9 and D.worst_tile(want, want) == 0.0
    z = np.zeros((40, 4)); e = z.copy(); e[35, 1] = 1e-30              # a tile whose reference is zero must be zero
    assert D.worst_tile(z, z) == 0.0 and D.worst_tile(e, z) == np.inf


def test_activation_mirror_backward_matches_finite_differences():
    """activate_f64 and dpre_norm_f64 together are the backward of l2_normalize o dropout o leaky_relu: <dpre, direction> against
    central differences of <z(pre), dz>"""
    rng = np.random.default_rng(8)
    n, d = 5, 7
    pre = rng.standard_normal((n, d)).astype(np.float32).astype(np.float64); mask = (rng.random((n, d)) >= 0.2).astype(np.float64)
    dz = rng.standard_normal((n, d))
    _, z, inv, gate = D.activate_f64(pre, mask, 0.9)
    dpre = D.dpre_norm_f64(dz, z, 0, None, inv, gate, d)
    worst = 0.0
    for _ in range(6):
        dirn = rng.standard_normal((n, d)); h = 1e-6
        num = ((D.activate_f64(pre + h * dirn, mask, 0.9)[1] - D.activate_f64(pre - h * dirn, mask, 0.9)[1]) * dz).sum() / (2 * h)
        worst = max(worst, abs(num - (dpre * dirn).sum()) / abs(num))
    check("activation mirror: analytic vs central differences", worst, 1e-6)
