"""GPU side of DiffNet / DHCF: the dense layer of csrc/dense_layer.hip against the float64 mirror, both trainers on the
reference's recorded runs (tests/golden/tf_diffnet_filmtrust.npz, tf_dhcf_filmtrust.npz; bounds: tests/diffusion_cases.py) and on
synthetic graphs up to the Yelp2018 shape, the drop-in classes end to end.  Every numeric assertion goes through helpers.check."""
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import scipy.sparse as sp

import diffusion_cases as C
import diffusion_mirror as M
from helpers import check, conf_from_text, pad_cols, rel_err, same_bits

pytestmark = pytest.mark.gpu


def _db(a):
    from qrec_amd.capi import DeviceBuffer
    return DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def _pad_w(W, d, ld):
    """(k*d x d) -> [k][ld][ld], zero-padded"""
    out = np.zeros((W.shape[0] // d, ld, ld), np.float32)
    for k in range(out.shape[0]):
        out[k, :d, :d] = W[k * d:(k + 1) * d]
    return out


def _layer_once(n, d, has2, has_r, relu, seed):
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    from qrec_amd.engine import padded_ld
    rng = np.random.default_rng(seed)
    ld = padded_ld(d, np.float32)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    X1, X2, R, dY = f(n, d), (f(n, d) if has2 else None), (f(n, d) if has_r else None), f(n, d)
    X1[::3] = 0.0                                     # empty rows of the sparse product in front (users without a followee)
    if has2:
        X2[1::5] = 0.0
    W = f((2 if has2 else 1) * d, d) * np.float32(0.3)
    dev = lambda a: None if a is None else _db(pad_cols(a, ld))
    dX1o, dX2o, dYd = dev(X1), dev(X2), dev(dY)
    Wd = _db(_pad_w(W, d, ld))
    Y = DeviceBuffer.zeros((n, ld), np.float32)
    capi.dense_layer_fwd(dX1o, dX2o, Wd, dev(R), n, ld, relu, Y)
    Yh = Y.numpy()
    want = M.layer_fwd(X1.astype(np.float64), None if X2 is None else X2.astype(np.float64), W.astype(np.float64),
                       None if R is None else R.astype(np.float64), relu)
    ctx = dict(n=n, d=d, x2=has2, r=has_r, relu=relu)
    check("dense layer forward vs the mirror", rel_err(Yh[:, :d], want), C.GRAD_TOL, ctx=ctx)
    assert not Yh[:, d:].any()
    # backward: dpre (ReLU gate or the plain upstream gradient), dX, gW
    dpre = DeviceBuffer.zeros((n, ld), np.float32)
    if relu:
        capi.dense_layer_dpre_relu(dYd, Y, n, ld, dpre)
        dpre_w = dY.astype(np.float64) * (want > 0)
        assert np.array_equal(dpre.numpy()[:, :d], dY * (Yh[:, :d] > 0))
    else:
        dpre, dpre_w = dYd, dY.astype(np.float64)
    nw = 2 if has2 else 1
    ws = DeviceBuffer(capi.dense_layer_ws_bytes(n, ld, nw), np.uint8)
    g1 = DeviceBuffer.zeros((n, ld), np.float32); g2 = DeviceBuffer.zeros((n, ld), np.float32) if has2 else None
    gW = DeviceBuffer.zeros((nw, ld, ld), np.float32)
    capi.dense_layer_bwd(dpre, dX1o, dX2o, Wd, n, ld, g1, g2, gW, ws)
    if relu:        # the device gate is taken from the device's own Y; where float32 and float64 disagree on the sign of a ~0 entry, follow the device
        dpre_w = dY.astype(np.float64) * (Yh[:, :d] > 0)
    w1, w2, wW = M.layer_bwd(dpre_w, X1.astype(np.float64), None if X2 is None else X2.astype(np.float64), W.astype(np.float64))
    check("dense layer backward dX1 vs the mirror", rel_err(g1.numpy()[:, :d], w1), C.GRAD_TOL, ctx=ctx)
    if has2:
        check("dense layer backward dX2 vs the mirror", rel_err(g2.numpy()[:, :d], w2), C.GRAD_TOL, ctx=ctx)
    gWh = gW.numpy()
    check("dense layer weight gradient vs the mirror", rel_err(np.concatenate([gWh[k, :d, :d] for k in range(nw)]), wW), C.GRAD_TOL, ctx=ctx)
    assert not g1.numpy()[:, d:].any() and not gWh[:, d:, :].any() and not gWh[:, :, d:].any()
    # accumulate: dX1 += on top of what is there
    capi.dense_layer_bwd(dpre, dX1o, dX2o, Wd, n, ld, g1, g2, gW, ws, accumulate_dX1=True)
    check("dense layer backward, accumulating dX1", rel_err(g1.numpy()[:, :d], 2 * w1), C.GRAD_TOL, ctx=ctx)
    return dict(Y=Yh, gW=gWh, g1=g1.numpy())


@pytest.mark.parametrize("d", [8, 50, 64, 100])
def test_dense_layer_forward_and_backward_match_the_mirror(d):
    for n in (1, 77, 1000, 4133):                     # not multiples of the 32-row tile / the 128-row slab, several slabs
        for has2, has_r, relu in ((True, False, True), (False, True, False), (True, True, False), (False, False, True)):
            a = _layer_once(n, d, has2, has_r, relu, seed=n + d)
            if n == 4133:
                same_bits(f"dense layer d={d}", a, _layer_once(n, d, has2, has_r, relu, seed=n + d))


def test_dense_layer_refuses_what_it_cannot_do():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    x = DeviceBuffer.zeros((64, 256), np.float32); w = DeviceBuffer.zeros((256, 256), np.float32)
    with pytest.raises(capi.QRecError, match="32, 64 or 128"):
        capi.dense_layer_fwd(x, None, w, None, 64, 256, False, x)
    x = DeviceBuffer.zeros((300, 32), np.float32); w = DeviceBuffer.zeros((32, 32), np.float32)
    small = DeviceBuffer(capi.dense_layer_ws_bytes(300, 32, 1) - 4, np.uint8)
    with pytest.raises(capi.QRecError, match="workspace"):
        capi.dense_layer_bwd(x, x, None, w, 300, 32, x, None, w, small)


def test_fixed_order_batch_loss_equals_the_gradient_kernels_loss_and_repeats_its_bits():
    """qrec_bpr_batch_loss_slots against the loss qrec_bpr_batch_loss_grad accumulates with fp64 atomics (same per-triplet fp32
    arithmetic up to the lane tree of the dots: 1e-6 on the sum) and against the float64 formula; two launches, the same bits"""
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    rng = np.random.default_rng(2)
    nu, ni, B = 300, 500, 2000
    for ld, d in ((32, 8), (64, 50), (256, 150)):
        S = np.zeros((nu + ni, ld), np.float32); S[:, :d] = rng.standard_normal((nu + ni, d)) * 0.3
        u, i, j = (rng.integers(0, n, B).astype(np.int32) for n in (nu, ni, ni))
        dS, du, di, dj = _db(S), _db(u), _db(i), _db(j)
        dE = DeviceBuffer.zeros(S.shape, np.float32); acc = DeviceBuffer.zeros(1, np.float64)
        capi.bpr_batch_loss_grad(dS, 1.0, nu, nu + ni, ld, du, di, dj, B, 0.0, 0.01, dE, acc)
        runs = []
        for _ in range(2):
            slots = DeviceBuffer.zeros(256, np.float64)
            capi.bpr_batch_loss_slots(dS, 1.0, nu, ld, du, di, dj, B, 0.0, 0.01, slots)
            runs.append(slots.numpy())
        same_bits(f"fixed-order loss ld={ld}", dict(slots=runs[0]), dict(slots=runs[1]))
        S64 = S.astype(np.float64)
        eu, ei, ej = S64[u], S64[nu + i], S64[nu + j]
        y = (eu * (ei - ej)).sum(1)
        want = np.log1p(np.exp(-y)).sum() + 0.005 * ((eu ** 2).sum() + (ei ** 2).sum() + (ej ** 2).sum())
        check("fixed-order loss vs the gradient kernel's", abs(runs[0].sum() - acc.numpy()[0]) / want, 1e-6, ctx=ld)
        check("fixed-order loss vs float64", abs(runs[0].sum() - want) / want, C.GRAD_TOL, ctx=ld)


# ---- trainers on the recorded runs -------------------------------------------------------------------------------------------
def _run_fixture(name):
    from qrec_amd.diffusion import rating_mean_csr, social_csr
    from qrec_amd.graph import DHCFTrainer, DiffNetTrainer, ordered_reductions
    m, z = C.load(name)
    nu, ni = m["n_users"], m["n_items"]
    init = [z[f"init_{v}"] for v in C.VARS[name]]
    with ordered_reductions():
        if name == C.DIFFNET:
            tr = DiffNetTrainer(init[0], init[1], init[2:], social_csr(nu, z["follower"], z["followee"]),
                                rating_mean_csr(nu, ni, z["train_uid"], z["train_iid"]), m["lr"], m["regU"], m["n_layers"])
        else:
            tr = DHCFTrainer(init[0], init[1], init[2:], z["train_uid"], z["train_iid"], m["lr"], m["regU"])
    losses, first = [], None
    for k, u, i, j in C.batches(z):
        kw = {}
        if name == C.DHCF:
            kw["masks"] = [_db(pad_cols(x, tr.ld)) for x in C.dhcf_masks(m, z, k)]
        tr.train_step_async(_db(u), _db(i), _db(j), u.size, **kw)
        losses.append(tr.loss())
        if k == 0:
            gU, gV, gW = tr.gradients()
            first = [np.array(gU), np.array(gV)] + [np.array(w) for w in gW]
    U, V, W = tr.parameters()
    out = dict(losses=np.array(losses))
    for v, g, p in zip(C.VARS[name], first, [U, V] + list(W)):
        out[f"grad_{v}"] = g; out[f"final_{v}"] = p
    return m, z, out


@pytest.mark.parametrize("name", [C.DIFFNET, C.DHCF])
def test_trainer_reproduces_the_reference_run_twice_bit_identically(name):
    """first-step gradients and every loss at 1e-5 of the reference's run; trained variables at max(1e-5, 2.5 floors) of the
    reference's run AND of its float64 re-run (floor = distance between the two committed files); a second run has the same bits.
    DHCF's factored operator sums in another order than the reference's formed scipy product: measured here, same bounds."""
    m, z, a = _run_fixture(name)
    check(f"{name} losses vs the reference run", rel_err(a["losses"], z["losses"][:, 0]), C.GRAD_TOL)
    for v in C.VARS[name]:
        check(f"{name} first-step gradient of {v}", rel_err(a[f"grad_{v}"], z[f"grad0_{v}"]), C.GRAD_TOL)
    for v in C.VARS[name]:
        key, bound = f"final_{v}", C.trained_bound(name, f"final_{v}", z)
        check(f"{name} floor of {v} (recorded)", C.floor_of(name, key, z), 1.0, kind="info")
        check(f"{name} trained {v} vs the reference run (absolute, recorded)", rel_err(a[key], z[key]), 1.0, kind="info")
        check(f"{name} trained {v} vs the reference run", rel_err(a[key], z[key]), bound, kind="floor")
        check(f"{name} trained {v} vs the float64 run", rel_err(a[key], C.YARD[f"{name}/{key}"]), bound, kind="floor")
    same_bits(name, a, _run_fixture(name)[2])


# ---- synthetic graphs -------------------------------------------------------------------------------------------------------
def _synthetic(nu, ni, nnz, n_rel, d, B, seed):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, nu, nnz), rng.integers(0, ni, nnz)], 1), axis=0)
    uid, iid = pairs[:, 0].astype(np.int32), pairs[:, 1].astype(np.int32)
    rel = np.unique(np.stack([rng.integers(0, nu, n_rel), rng.integers(0, nu, n_rel)], 1), axis=0)
    b = rng.integers(0, uid.size, B)
    u, i, j = uid[b], iid[b], rng.integers(0, ni, B).astype(np.int32)
    U = (rng.standard_normal((nu, d)) * 0.1).astype(np.float32); V = (rng.standard_normal((ni, d)) * 0.1).astype(np.float32)
    return rng, uid, iid, rel[:, 0], rel[:, 1], u, i, j, U, V


def _diffnet_step_vs_mirror(nu, ni, nnz, n_rel, d, B, L, seed, what):
    from qrec_amd.diffusion import rating_mean_csr, social_csr
    from qrec_amd.graph import DiffNetTrainer, ordered_reductions
    rng, uid, iid, fo, fe, u, i, j, U, V = _synthetic(nu, ni, nnz, n_rel, d, B, seed)
    lim = np.sqrt(6.0 / (3 * d))
    Ws = [rng.uniform(-lim, lim, (2 * d, d)).astype(np.float32) for _ in range(L)]
    S, A = social_csr(nu, fo, fe), rating_mean_csr(nu, ni, uid, iid)
    with ordered_reductions():
        tr = DiffNetTrainer(U, V, Ws, S, A, 0.001, 0.01, L)
    tr.train_step_async(_db(u), _db(i), _db(j), B)
    f64 = lambda x: np.asarray(x, np.float64)
    loss, dU, dV, dW = M.diffnet_loss_grads(f64(U), f64(V), [f64(w) for w in Ws], M.social_matrix(nu, fo, fe), M.rating_matrix(nu, ni, uid, iid),
                                            u, i, j, 0.01)
    gU, gV, gW = tr.gradients()
    check(f"{what}: loss vs the mirror", abs(tr.loss() - loss) / loss, C.GRAD_TOL)
    check(f"{what}: dU vs the mirror", rel_err(gU, dU), C.GRAD_TOL)
    check(f"{what}: dV vs the mirror", rel_err(gV, dV), C.GRAD_TOL)
    for k in range(L):
        check(f"{what}: dW_{k} vs the mirror", rel_err(gW[k], dW[k]), C.GRAD_TOL)
    Fu, Fv = tr.inference_embeddings()          # after the Adam step: against the mirror on the trainer's own new parameters
    U1, V1, W1 = tr.parameters()
    check(f"{what}: scoring table vs the mirror", rel_err(Fu, M.diffnet_final(f64(U1), f64(V1), [f64(w) for w in W1], M.social_matrix(nu, fo, fe),
                                                                            M.rating_matrix(nu, ni, uid, iid))), C.GRAD_TOL)
    assert np.array_equal(Fv, V1)


@pytest.mark.parametrize("L", [1, 3])
def test_diffnet_with_one_and_three_layers_matches_the_mirror(L):
    _diffnet_step_vs_mirror(700, 900, 9000, 2500, 24, 512, L, seed=L, what=f"DiffNet n_layer {L}")


def test_diffnet_one_step_at_the_yelp2018_shape():
    _diffnet_step_vs_mirror(31668, 38048, 1237259, 120000, 64, 2048, 2, seed=7, what="DiffNet, Yelp2018 shape")


class _Factored:
    """diag(A_u, A_i) applied as P (Q x) in float64 -- the formed matrix is close to dense at this shape"""

    def __init__(self, P, Q):
        self.P, self.Q = P, Q
        self.T = self                             # symmetric

    def __matmul__(self, X):
        return self.P @ (self.Q @ X)


def test_dhcf_one_step_at_the_yelp2018_shape():
    """the case the reference's formed A A^T cannot serve; device Philox dropout is switched off by all-ones masks so that the
    mirror sees the same graph"""
    from qrec_amd.graph import DHCFTrainer, ordered_reductions
    nu, ni, d, B = 31668, 38048, 64, 2048
    rng, uid, iid, _, _, u, i, j, U, V = _synthetic(nu, ni, 1237259, 10, d, B, seed=9)
    lim = np.sqrt(6.0 / (2 * d))
    Ws = [rng.uniform(-lim, lim, (d, d)).astype(np.float32) for _ in range(2)]
    masks = [(rng.random((nu + ni, d)) >= 0.1).astype(np.float32) for _ in range(2)]
    with ordered_reductions():
        tr = DHCFTrainer(U, V, Ws, uid, iid, 0.001, 0.01)
    tr.train_step_async(_db(u), _db(i), _db(j), B, masks=[_db(x) for x in masks])
    f64 = lambda x: np.asarray(x, np.float64)
    P, Q = M.dhcf_factors(nu, ni, uid, iid)
    loss, dU, dV, dW = M.dhcf_loss_grads(f64(U), f64(V), [f64(w) for w in Ws], _Factored(P, Q), u, i, j, 0.01, masks=[f64(x) for x in masks])
    gU, gV, gW = tr.gradients()
    check("DHCF, Yelp2018 shape: loss vs the mirror", abs(tr.loss() - loss) / loss, C.GRAD_TOL)
    check("DHCF, Yelp2018 shape: dU vs the mirror", rel_err(gU, dU), C.GRAD_TOL)
    check("DHCF, Yelp2018 shape: dV vs the mirror", rel_err(gV, dV), C.GRAD_TOL)
    for k in range(2):
        check(f"DHCF, Yelp2018 shape: dW_{k + 1} vs the mirror", rel_err(gW[k], dW[k]), C.GRAD_TOL)


def test_dhcf_device_dropout_keeps_nine_in_ten_and_inference_has_none():
    from qrec_amd.graph import DHCFTrainer
    rng, uid, iid, _, _, u, i, j, U, V = _synthetic(600, 800, 8000, 10, 16, 256, seed=3)
    Ws = [rng.uniform(-0.4, 0.4, (16, 16)).astype(np.float32) for _ in range(2)]
    tr = DHCFTrainer(U, V, Ws, uid, iid, 0.001, 0.01, seed=11)
    tr.train_step_async(_db(u), _db(i), _db(j), 256)
    gate = tr.gate[0].numpy()[:, :16]
    check("DHCF device dropout: kept fraction", abs(float((gate != 0).mean()) - 0.9), 0.01, kind="statistical")
    Ui, Vi = tr.inference_embeddings()
    U1, V1, W1 = tr.parameters()
    f64 = lambda x: np.asarray(x, np.float64)
    P, Q = M.dhcf_factors(600, 800, uid, iid)
    wu, wv = M.dhcf_inference(f64(U1), f64(V1), [f64(w) for w in W1], _Factored(P, Q))
    check("DHCF inference tables vs the mirror", max(rel_err(Ui, wu), rel_err(Vi, wv)), C.GRAD_TOL)


# ---- drop-in classes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "throughput"])
@pytest.mark.parametrize("name", ["DiffNet", "DHCF"])
def test_class_trains_and_evaluates_in_both_modes(name, mode, monkeypatch):
    from qrec_amd.QRec import resolve_model
    monkeypatch.setenv("QREC_MODE", mode)
    fixture = C.DIFFNET if name == "DiffNet" else C.DHCF
    m, z = C.load(fixture)
    conf = conf_from_text(m["conf"])
    conf["num.factors"] = "16"; conf["num.max.epoch"] = "3"; conf["batch_size"] = "2000"
    uid, iid = z["train_uid"].tolist(), z["train_iid"].tolist()
    train = [[f"u{u}", f"i{i}", 1.0] for u, i in zip(uid, iid)]
    test = [[f"u{u}", f"i{(i * 7 + 3) % m['n_items']}", 1.0] for u, i in zip(uid[::19], iid[::19])]
    random.seed(31); np.random.seed(31)
    buf = io.StringIO()
    with redirect_stdout(buf):
        if name == "DiffNet":
            relation = [[f"u{a}", f"u{b}", 1.0] for a, b in zip(z["follower"].tolist(), z["followee"].tolist())]
            model = resolve_model(name)(conf, train, test, relation)
        else:
            model = resolve_model(name)(conf, train, test)
        measure = model.execute()
    losses = [float(l.split("loss:")[1]) for l in buf.getvalue().splitlines() if l.startswith("training:")]
    n_batches = -(-len(train) // 2000)
    assert len(losses) == 3 * n_batches and np.isfinite(losses).all()
    check(f"{name} class, {mode}: last epoch's mean loss over the first's", np.mean(losses[-n_batches:]) / np.mean(losses[:n_batches]), 1.0, kind="statistical")
    assert any(x.startswith("Recall") for x in measure) and any(x.startswith("NDCG") for x in measure)
    wide = 16 if name == "DiffNet" else 48
    assert model.U.shape == (m["n_users"], wide) and model.V.shape == (m["n_items"], wide) and np.isfinite(model.U).all()
