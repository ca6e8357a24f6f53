"""GPU side of CFGAN: the kernels of csrc/cfgan.hip against the float64 mirror (tests/cfgan_mirror.py) on lists built to hold the
shapes they can go wrong on (tests/cfgan_cases.py::kernel_case), the trainer on the reference's recorded run
(tests/golden/tf_cfgan_filmtrust.npz), the evaluation's sparse block fill, and the drop-in class end to end.  Every numeric assertion
goes through helpers.check."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import cfgan_cases as C
import cfgan_mirror as M
from helpers import check, conf_from_text, rel_err, same_bits

pytestmark = pytest.mark.gpu


def _trainer(p, lr=0.002, alpha=C.ALPHA, keep=True):
    from qrec_amd.autoencoder import CfganTrainer
    return CfganTrainer(p["G_W1"], p["G_b1"], p["D_W1"], p["D_b1"], lr, alpha, keep_gradients=keep)


def _flat(p):
    return {k: np.asarray(v).reshape(-1) if k.startswith("D_") else np.asarray(v) for k, v in p.items()}


def _kernels_once(ni, B):
    """a discriminator step on one trainer and a generator step on another, both from the case's variables"""
    p, L = C.kernel_case(ni, B)
    td, tg = _trainer(p), _trainer(p)
    Ld = td.dis_step_async(L)
    out = dict(td.slots(Ld), losses=td.losses.numpy()[:2].copy())
    out.update({f"grad_{k}": v for k, v in _flat(td.raw_gradients("D")).items()})
    out.update({f"after_{k}": v for k, v in _flat(td.parameters()).items() if k.startswith("D_")})
    tg.gen_step_async(L)
    out.update({f"grad_{k}": v for k, v in tg.raw_gradients("G").items()})
    out.update({f"after_{k}": v for k, v in tg.parameters().items() if k.startswith("G_")})
    return p, L, td, tg, out


@pytest.mark.parametrize("B", C.BATCHES)
@pytest.mark.parametrize("ni", C.ITEM_COUNTS)
def test_kernels_match_the_float64_mirror_and_repeat_their_bits(ni, B):
    p, L, td, tg, a = _kernels_once(ni, B)
    w = M.sparse_parts(p, L, C.ALPHA)
    ctx = dict(n_items=ni, B=B, rated=L.n_in, live=L.n_live)
    check("CFGAN sampled forward r_hat per live slot vs the mirror", rel_err(a["r"], w["r"]), C.GRAD_TOL, ctx=ctx)
    check("CFGAN delta per live slot vs the mirror", rel_err(a["delta"], w["delta"]), C.GRAD_TOL, ctx=ctx)
    check("CFGAN a_r per batch row vs the mirror", rel_err(a["a_r"], w["a_r"]), C.GRAD_TOL, ctx=ctx)
    check("CFGAN a_f per batch row vs the mirror", rel_err(a["a_f"], w["a_f"]), C.GRAD_TOL, ctx=ctx)
    check("CFGAN D_loss vs the mirror", abs(a["losses"][0] - w["d_loss"]) / abs(w["d_loss"]), C.GRAD_TOL, ctx=ctx)
    check("CFGAN G_loss vs the mirror", abs(a["losses"][1] - w["g_loss"]) / abs(w["g_loss"]), C.GRAD_TOL, ctx=ctx)
    for k in C.VARS:
        check(f"CFGAN gradient of {k} vs the mirror", rel_err(a[f"grad_{k}"], w["grads"][k]), C.GRAD_TOL, ctx=ctx)
    # one Adam step of each optimizer from the mirror's gradients
    after = M.Adam(0.002, M.G_VARS).step(M.Adam(0.002, M.D_VARS).step(M.cast(p, np.float64), w["grads"]), w["grads"])
    for k in C.VARS:
        check(f"CFGAN {k} after one step vs the mirror", rel_err(a[f"after_{k}"], after[k]), C.GRAD_TOL, ctx=ctx)
    # the saturated position: r_hat rounds to 1, r_hat (1 - r_hat) is an exact 0 and so are delta and its column of the gradient
    sat = L.lv_item == C.SATURATED_ITEM
    assert sat.sum() == B and (a["r"][sat] == 1.0).all() and not a["delta"][sat].any() and (a["delta"][~sat] != 0).all()
    assert not a["grad_G_W1"][:, C.SATURATED_ITEM].any() and a["grad_G_b1"][C.SATURATED_ITEM] == 0
    # the item no row rated: an exactly zero gradient row, and with m = v = 0 the row is bit-unchanged
    assert not a["grad_G_W1"][C.UNRATED_ITEM].any()
    assert np.array_equal(a["after_G_W1"][C.UNRATED_ITEM], p["G_W1"][C.UNRATED_ITEM])
    assert a["grad_G_W1"][C.EVERY_ROW_ITEM].any()
    assert td.padding_is_zero() and tg.padding_is_zero()
    if B >= 5:
        assert (L.users == L.users[1]).sum() >= 3
    same_bits(f"CFGAN kernels n_items={ni} B={B}", a, _kernels_once(ni, B)[4])


def test_a_row_touched_in_one_step_and_not_in_the_next_still_moves_by_its_momentum():
    """two generator steps on two batches: row X of G_W1 takes gradient in the first (user 0 rated X), none in the second (its only
    rater is not drawn), and Adam's first moment still moves it"""
    from qrec_amd.autoencoder import cfgan_lists
    ni, X = 257, 200
    rng = np.random.default_rng(11)
    p, _ = C.kernel_case(ni, 5)
    mk = lambda users, rated: cfgan_lists(np.array(users, np.int32), ni, np.repeat(np.arange(len(users)), [len(r) for r in rated]),
                                          np.concatenate(rated), np.ones(sum(len(r) for r in rated), np.float32) * 2,
                                          np.repeat(np.arange(len(users)), 3), np.tile([5, 90, 250], len(users)), [0], [90])
    first, second = mk([0, 1], [np.array([1, X]), np.array([1, 7])]), mk([1, 2], [np.array([1, 7]), np.array([1, 30, 31])])
    tr = _trainer(p)
    tr.gen_step_async(first); g1 = tr.raw_gradients("G")["G_W1"]; W1 = tr.parameters()["G_W1"]
    tr.gen_step_async(second); g2 = tr.raw_gradients("G")["G_W1"]; W2 = tr.parameters()["G_W1"]
    touched = g1[X] != 0
    assert touched.sum() == 5 and not g2[X].any()             # X's gradient lives on row 0's five mask positions
    assert (W2[X][touched] != W1[X][touched]).all() and np.array_equal(W2[X][~touched], p["G_W1"][X][~touched])
    q, opt = M.cast(p, np.float64), M.Adam(0.002, M.G_VARS)
    for L in (first, second):
        q = opt.step(q, M.sparse_parts(q, L, C.ALPHA)["grads"])
    check("CFGAN G_W1 after two steps vs the mirror", rel_err(W2, q["G_W1"]), C.GRAD_TOL)
    check("CFGAN the momentum-only move of row X vs the mirror", rel_err((W2[X] - W1[X])[touched], (q["G_W1"][X] - W1[X])[touched]), 1e-3,
          kind="info")
    assert tr.padding_is_zero()


@pytest.mark.parametrize("bias", [25.0, -25.0])
def test_discriminator_logits_beyond_20_give_the_guarded_logarithm_not_infinity(bias):
    """D_fake = 1 (resp. D_real = 0) in float32: the 1e-4 guards give log(1e-4)"""
    p, L = C.kernel_case(33, 5)
    p = dict(p, D_b1=np.array([bias], np.float32))
    tr = _trainer(p)
    tr.dis_step_async(L)
    w = M.sparse_parts(p, L, C.ALPHA)
    assert (np.abs(w["logit_real"]) > 20).all() and (np.abs(w["logit_fake"]) > 20).all()
    got = tr.losses.numpy()[:2]
    assert np.isfinite(got).all()
    check("CFGAN D_loss at saturated logits vs the mirror", abs(got[0] - w["d_loss"]) / abs(w["d_loss"]), C.GRAD_TOL, ctx=dict(bias=bias))
    check("CFGAN G_loss at saturated logits vs the mirror", abs(got[1] - w["g_loss"]) / abs(w["g_loss"]), C.GRAD_TOL, ctx=dict(bias=bias))
    check("CFGAN D_loss at saturated logits vs -log(1e-4)", abs(got[0] + np.log(1e-4)) / abs(np.log(1e-4)), 1e-3, ctx=dict(bias=bias))
    assert all(np.isfinite(v).all() for v in tr.parameters().values())


def test_kernels_refuse_unsupported_sizes_and_bad_arguments():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    _, L = C.kernel_case(33, 1)
    tr = _trainer(C.kernel_case(33, 1)[0])
    Ld = tr.forward(L)
    z = DeviceBuffer.zeros(4096, np.float32)
    big = capi.CFGAN_MAX_ITEMS + 32
    with pytest.raises(capi.QRecError) as e:
        capi.cfgan_forward(z, z, z, big, big, Ld, 0.01, tr.ws, tr.losses)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.QRecError) as e:
        capi.cfgan_gen_sweep(z, z, z, z, z, z, big, big, Ld, tr.ws, 1e-3, 0.9, 0.999, 1e-8)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.QRecError) as e:
        capi.score_topk_sparse_row_sigmoid_bias(z, z, big, big, z, 1, z, z, z, 10, z, z, z)
    assert e.value.code == capi.ERR_UNSUPPORTED
    for call in (lambda: capi.cfgan_forward(z, z, z, 33, 40, Ld, 0.01, tr.ws, tr.losses),              # ld not a multiple of 32
                 lambda: capi.cfgan_forward(z, z, z, 33, 32, Ld, 0.01, tr.ws, tr.losses),              # ld below n_items
                 lambda: capi.cfgan_forward(z, z, None, 33, 64, Ld, 0.01, tr.ws, tr.losses),           # a null table
                 lambda: capi.cfgan_gen_sweep(z, z, None, z, z, z, 33, 64, Ld, tr.ws, 1e-3, 0.9, 0.999, 1e-8),
                 lambda: capi.score_topk_sparse_row_sigmoid_bias(z, z, 64, 33, z, 1, z, z, z, 101, z, z, z)):      # N above 100
        with pytest.raises(capi.QRecError) as e:
            call()
        assert e.value.code == -1 and len(str(e.value)) > 20
    with pytest.raises(ValueError):
        tr.forward(C.kernel_case(5, 1)[1])                       # lists over another item count
    with pytest.raises(RuntimeError):
        _trainer(C.kernel_case(5, 1)[0], keep=False).raw_gradients("G")


# ---- the recorded run ---------------------------------------------------------------------------------------------------------------
def _run_fixture(device_lists=False):
    z, m = C.load(), C.META
    tr = _trainer(C.initial(z), m["lr"], m["alpha"])
    d_losses, g_losses, first = [], [], {}
    for k, L in enumerate(C.list_batches()):
        L = L.device_copy() if device_lists else L
        if k == 0:                                    # the first epoch step by step: the gradients of its D step and of its first G step
            Ld = tr.dis_step_async(L); first.update(_flat(tr.raw_gradients("D")))
            tr.gen_step_async(Ld); first.update(tr.raw_gradients("G"))
            tr.gen_step_async(Ld); tr.gen_step_async(Ld)
        else:
            tr.train_epoch_async(L)
        d_losses.append(tr.d_loss()); g_losses.append(tr.g_losses())
    out = dict(d_losses=np.array(d_losses), g_losses=np.array(g_losses))
    for k, v in _flat(tr.parameters()).items():
        out[f"final_{k}"] = v; out[f"grad0_{k}"] = first[k]
    assert tr.padding_is_zero()
    return z, out


def test_trainer_reproduces_the_reference_run_twice_bit_identically():
    """first D-step and first G-step gradients and all 48 losses at 1e-5 of the reference's run; the four trained variables at
    max(1e-5, 2.5 floors) of the reference's run and of its float64 re-run (floor = distance between the two committed files); a second
    run has the same bits, and so has a run whose lists are handed over in device buffers"""
    z, a = _run_fixture()
    assert a["g_losses"].shape == (12, 3)
    check("CFGAN the 12 D losses vs the reference run", rel_err(a["d_losses"], z["d_losses"]), C.GRAD_TOL)
    check("CFGAN the 36 G losses vs the reference run", rel_err(a["g_losses"], z["g_losses"]), C.GRAD_TOL)
    for v in C.VARS:
        check(f"CFGAN first-step gradient of {v}", rel_err(a[f"grad0_{v}"], z[f"grad0_{v}"]), C.GRAD_TOL)
    for v in C.VARS:
        key, bound = f"final_{v}", C.trained_bound(f"final_{v}", z)
        check(f"CFGAN floor of {v} (recorded)", C.floor_of(key, z), 1.0, kind="info")
        check(f"CFGAN trained {v} vs the reference run", rel_err(a[key], z[key]), bound, kind="floor")
        check(f"CFGAN trained {v} vs the float64 run", rel_err(a[key], C.yard()[key]), bound, kind="floor")
    # entries of G_W1 that never received gradient are the initial bits
    same = np.ones(z["init_G_W1"].size, bool); same[z["final_G_W1_idx"]] = False
    assert np.array_equal(a["final_G_W1"].ravel()[same], z["init_G_W1"].ravel()[same])
    same_bits("CFGAN trainer", a, _run_fixture()[1])
    same_bits("CFGAN trainer, lists handed over in device buffers", a, _run_fixture(device_lists=True)[1])


# ---- evaluation: sigmoid(C[u] G_W1 + G_b1), rated items to 0, top-N ---------------------------------------------------------------
def _rated_csr(uid, iid, vals, n_users):
    from qrec_amd.interactions import CSR
    order = np.lexsort((iid, uid))
    indptr = np.zeros(n_users + 1, np.int64); np.cumsum(np.bincount(uid, minlength=n_users), out=indptr[1:])
    return CSR(indptr, iid[order].astype(np.int32), np.asarray(vals)[order].astype(np.float64))


def _check_lists(what, ids, scores, want, rated_mask, tol=C.GRAD_TOL):
    """``want``: the mirror's scores [users, items] before masking; ``rated_mask``: True at rated train items"""
    rows = np.arange(ids.shape[0])[:, None]
    check(f"{what}: returned scores vs the mirror's at the same ids", rel_err(scores, want[rows, ids]), tol)
    assert not rated_mask[rows, ids].any()
    left = np.where(rated_mask, 0.0, want)
    left[rows, ids] = -np.inf
    check(f"{what}: best left-out mirror score above a list's last score", float((left.max(1) - scores[:, -1]).max()), tol, inclusive=True)
    assert (np.diff(scores, axis=1) <= 0).all()


def test_evaluation_scores_and_ranks_like_the_mirror_for_all_test_users():
    from qrec_amd.ranking import SparseRowSigmoidRanker
    z, m = C.load(), C.META
    tr = _trainer(C.initial(z), m["lr"], m["alpha"], keep=False)
    for L in C.list_batches():
        tr.train_epoch_async(L)
    rated = _rated_csr(z["train_uid"], z["train_iid"], z["train_r"], m["n_users"])
    users = np.unique(z["test_uid"][z["test_uid"] >= 0]).astype(np.int32)
    R = C.ratings_matrix(z)
    ids, scores = SparseRowSigmoidRanker(tr.W, tr.b, m["n_users"], m["n_items"], tr.ld, rated).topk(users, 10)
    _check_lists("CFGAN evaluation, recorded run", ids, scores, M.scores(tr.parameters(), R[users]), R[users] != 0)


@pytest.mark.parametrize("ni", [33, 477, 1030])
def test_sparse_block_fill_with_users_of_1_7_and_300_rated_items(ni):
    """the fill is an SpMM from the rated CSR: users of 1, 7 and min(300, n_items - 13) rated items among 70 others (two 64-user
    panels), every list as long as the ranker serves, against the float64 product"""
    from qrec_amd.capi import DeviceBuffer
    from qrec_amd.ranking import SparseRowSigmoidRanker
    rng = np.random.default_rng(ni)
    nu, ld = 73, -(-ni // 32) * 32
    counts = [1, 7, min(300, ni - 13)] + rng.integers(1, min(ni - 13, 40), nu - 3).tolist()
    uid = np.repeat(np.arange(nu), counts); iid = np.concatenate([rng.permutation(ni)[:c] for c in counts])
    vals = rng.integers(1, 9, uid.size) / 2
    rated = _rated_csr(uid, iid, vals, nu)
    R = np.zeros((nu, ni)); R[uid, iid] = vals
    p = dict(G_W1=rng.uniform(-0.2, 0.2, (ni, ni)).astype(np.float32), G_b1=rng.uniform(-1, 1, ni).astype(np.float32))
    W = np.zeros((ni, ld), np.float32); W[:, :ni] = p["G_W1"]
    b = np.zeros(ld, np.float32); b[:ni] = p["G_b1"]
    ranker = SparseRowSigmoidRanker(DeviceBuffer.from_numpy(W), DeviceBuffer.from_numpy(b), nu, ni, ld, rated)
    users = rng.permutation(nu).astype(np.int32)
    N = min(12, ni - max(counts))
    ids, scores = ranker.topk(users, N)
    _check_lists(f"CFGAN block fill n_items={ni}", ids, scores, M.scores(p, R[users]), R[users] != 0)
    ids2, scores2 = ranker.topk(users, N)
    same_bits(f"CFGAN block fill n_items={ni}", dict(ids=ids, scores=scores), dict(ids=ids2, scores=scores2))


# ---- the drop-in class ------------------------------------------------------------------------------------------------------------------
def test_class_on_the_recorded_batches_gives_the_reference_measure_strings(monkeypatch, tmp_path):
    from qrec_amd.QRec import resolve_model
    monkeypatch.chdir(tmp_path)                    # the log and the measure file are written under the working directory
    monkeypatch.setenv("QREC_MODE", "throughput")  # one path whatever the mode says
    m, z = C.META, C.load()
    train, test = C.train_test_lists()
    model = resolve_model("CFGAN")(conf_from_text(m["conf"]), train, test)
    buf = io.StringIO()
    with redirect_stdout(buf):
        model.readConfiguration(); model.initializing_log(); model.initModel()
        model.G_W1, model.G_b1, model.D_W1, model.D_b1 = (z[f"init_{v}"] for v in C.VARS)
        model.injected_lists = C.list_batches()
        model.trainModel()
        model.evalRanking()
    lines = [l for l in buf.getvalue().splitlines() if l.startswith("epoch:")]
    assert len(lines) == m["n_epochs"] and lines[0].startswith("epoch: 0 D_loss: ") and " G_loss " in lines[0]
    printed = np.array([[float(l.split()[3]), float(l.split()[5])] for l in lines])
    check("CFGAN class: printed D losses vs the reference run", rel_err(printed[:, 0], z["d_losses"]), C.GRAD_TOL)
    check("CFGAN class: printed G losses vs the reference run", rel_err(printed[:, 1], z["g_losses"][:, 2]), C.GRAD_TOL)
    assert [s.strip() for s in model.measure] == [s.strip() for s in m["measure"]]
    # the host scores of predictForRanking are the mirror's
    user = next(u for u in model.data.testSet_u if model.data.containsUser(u))
    want = M.scores(model.trainer.parameters(), model.data.row(user)[None, :])[0]
    check("CFGAN class: predictForRanking vs the mirror", rel_err(model.predictForRanking(user), want), C.GRAD_TOL)


def test_class_trains_and_evaluates_on_its_own_draws(monkeypatch, tmp_path):
    import random
    from qrec_amd.QRec import resolve_model
    monkeypatch.chdir(tmp_path); monkeypatch.setenv("QREC_QUIET", "1")
    train, test = C.train_test_lists()
    model = resolve_model("CFGAN")(conf_from_text(C.META["conf"]), train, test)
    with redirect_stdout(io.StringIO()):
        model.readConfiguration(); model.initializing_log(); model.initModel()
        model.S_zr = model.S_pm = 0.05
        random.seed(5); np.random.seed(5)
        model.trainModel()
        model.evalRanking()
    assert len(model.batches) == C.META["n_epochs"] and np.isfinite(model.trainer.d_loss()) and np.isfinite(model.trainer.g_loss())
    p, d_losses, g_losses, _, _ = M.train(model.initial_variables(), [model.recorded_lists(k) for k in range(len(model.batches))],
                                          C.META["lr"], 0.01)
    check("CFGAN class: last D loss vs the mirror on the class's own batches", abs(model.trainer.d_loss() - d_losses[-1]) / abs(d_losses[-1]), C.GRAD_TOL)
    check("CFGAN class: last G loss vs the mirror on the class's own batches", abs(model.trainer.g_loss() - g_losses[-1, 2]) / abs(g_losses[-1, 2]), C.GRAD_TOL)
    assert any(s.startswith("Recall:") for s in model.measure)
