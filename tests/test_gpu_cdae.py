"""GPU side of CDAE: the kernels of csrc/autoencoder.hip against the float64 mirror (tests/cdae_mirror.py) on lists built to hold
the shapes they can go wrong on (tests/cdae_cases.py::kernel_case), the trainer on the reference's recorded run
(tests/golden/tf_cdae_filmtrust.npz), the sigmoid + bias evaluation, and the drop-in class end to end.  Every numeric assertion
goes through helpers.check."""
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

import cdae_cases as C
import cdae_mirror as M
from helpers import check, conf_from_text, rel_err, same_bits

pytestmark = pytest.mark.gpu


def _trainer(p, lr=0.01, reg=0.01):
    from qrec_amd.autoencoder import CdaeTrainer
    return CdaeTrainer(p["W_enc"], p["W_dec"], p["b_enc"], p["b_dec"], p["V"], lr, reg)


def _kernels_once(nh, B):
    p, L, reg = C.kernel_case(nh, B)
    tr = _trainer(p, reg=reg)
    tr.forward_backward(L)
    out = dict(h=tr.h.numpy()[:B, :nh], dz=tr.dz.numpy()[:B, :nh], g=tr.g.numpy()[:L.n_live], loss=np.array([tr.loss()]))
    out.update({f"grad_{k}": v for k, v in tr.raw_gradients().items()})
    return p, L, reg, tr, out


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("nh", [20, 24, 128, 200])
def test_kernels_match_the_float64_mirror_and_repeat_their_bits(nh, B):
    p, L, reg, tr, a = _kernels_once(nh, B)
    w = M.sparse_parts(p, L, reg)
    ctx = dict(nh=nh, B=B, kept=L.n_in, live=L.n_live)
    check("CDAE encoder h vs the mirror", rel_err(a["h"], w["h"]), C.GRAD_TOL, ctx=ctx)
    check("CDAE decoder g per live slot vs the mirror", rel_err(a["g"], w["g"]), C.GRAD_TOL, ctx=ctx)
    check("CDAE loss vs the mirror", abs(a["loss"][0] - w["loss"]) / w["loss"], C.GRAD_TOL, ctx=ctx)
    check("CDAE hidden backward dz vs the mirror", rel_err(a["dz"], w["dz"]), C.GRAD_TOL, ctx=ctx)
    for k in C.VARS:
        check(f"CDAE gradient of {k} vs the mirror", rel_err(a[f"grad_{k}"], w["raw"][k]), C.GRAD_TOL, ctx=ctx)
    # the clamp: every slot of the saturated item has y < 1e-6, so its gradient is an exact zero and its term -log(1e-6) or -log(1 - 1e-6)
    sat = L.lv_item == C.SATURATED_ITEM
    assert sat.any() and (w["logits"][sat] < -14).all() and not a["g"][sat].any()
    assert (a["g"][~sat] != 0).all()
    # items live in no row and kept in none: exact zero rows; the padding columns of every table and gradient stay zero
    dead = list(C.DEAD_ITEMS)
    assert not a["grad_W_enc"][dead].any() and not a["grad_W_dec"][:, dead].any() and not a["grad_b_dec"][dead].any()
    absent_users = np.setdiff1d(np.arange(C.N_USERS), L.users)
    assert not a["grad_V"][absent_users].any()
    assert tr.padding_is_zero()
    if B >= 5:      # the same user three times: one reg * V term per occurrence
        u = L.users[1]
        assert (L.users == u).sum() >= 3
        check("CDAE gradient of V at the user drawn three times", rel_err(a["grad_V"][u], w["raw"]["V"][u]), C.GRAD_TOL, ctx=ctx)
    if B == 64:
        assert (np.diff(L.lv_cptr)[C.EVERY_ROW_ITEM] == B - 1) and L.lv_ptr[1] == 0          # live in every row but the empty one
    same_bits(f"CDAE kernels nh={nh} B={B}", a, _kernels_once(nh, B)[4])


def test_kernels_refuse_a_width_above_the_supported_one():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    z = DeviceBuffer.zeros(4096, np.float32)
    with pytest.raises(capi.QRecError) as e:
        capi.cdae_encode(z, z, z, 4, 4, 257, 288, z, 1, z, z, z, z)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.QRecError) as e:
        capi.cdae_decode(z, z, 4, 300, 320, z, 1, z, z, z, z, z)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        _trainer(dict(W_enc=np.zeros((4, 257)), W_dec=np.zeros((257, 4)), b_enc=np.zeros(257), b_dec=np.zeros(4), V=np.zeros((3, 257))))


# ---- the recorded run ---------------------------------------------------------------------------------------------------------------
def _run_fixture(device_lists=False):
    z, m = C.load(), C.META
    tr = _trainer(C.initial(z), m["lr"], m["regU"])
    losses, first = [], None
    for L in C.list_batches():
        L = L.device_copy() if device_lists else L
        tr.train_step_async(L)
        losses.append(tr.loss())
        if first is None:
            raw, p0 = tr.raw_gradients(), C.initial(z)
            first = {k: raw[k] + (np.float32(m["regU"]) * p0[k] if k != "V" else 0) for k in C.VARS}
    out = dict(losses=np.array(losses))
    for k, v in tr.parameters().items():
        out[f"final_{k}"] = v; out[f"grad_{k}"] = first[k]
    return z, out


def test_trainer_reproduces_the_reference_run_twice_bit_identically():
    """first-step gradients and all 12 losses at 1e-5 of the reference's run; trained variables at max(1e-5, 2.5 floors) of the
    reference's run and of its float64 re-run (floor = distance between the two committed files); a second run has the same bits"""
    z, a = _run_fixture()
    check("CDAE losses vs the reference run", rel_err(a["losses"], z["losses"][:, 0]), C.GRAD_TOL)
    for v in C.VARS:
        check(f"CDAE first-step gradient of {v}", rel_err(a[f"grad_{v}"], z[f"grad0_{v}"]), C.GRAD_TOL)
    for v in C.VARS:
        key, bound = f"final_{v}", C.trained_bound(f"final_{v}", z)
        check(f"CDAE floor of {v} (recorded)", C.floor_of(key, z), 1.0, kind="info")
        check(f"CDAE trained {v} vs the reference run", rel_err(a[key], z[key]), bound, kind="floor")
        check(f"CDAE trained {v} vs the float64 run", rel_err(a[key], C.YARD[f"{C.NAME}/{key}"]), bound, kind="floor")
    same_bits("CDAE trainer", a, _run_fixture()[1])
    same_bits("CDAE trainer, lists handed over in device buffers", a, _run_fixture(device_lists=True)[1])


# ---- evaluation: sigmoid(h W_dec + b_dec), rated items to 0, top-N --------------------------------------------------------------------
def _rated_csr(uid, iid, vals, n_users):
    from qrec_amd.interactions import CSR
    order = np.lexsort((iid, uid))
    indptr = np.zeros(n_users + 1, np.int64); np.cumsum(np.bincount(uid, minlength=n_users), out=indptr[1:])
    return CSR(indptr, iid[order].astype(np.int32), vals[order].astype(np.float64))


def _rank(tr, rated, users, N=10):
    from qrec_amd.ranking import SigmoidBiasRanker
    hidden = tr.hidden(np.arange(tr.nu, dtype=np.int32), rated.indptr, rated.indices, rated.values.astype(np.float32))
    ranker = SigmoidBiasRanker(hidden, tr.W_dec, tr.b_dec, tr.nu, tr.ni, tr.nh, tr.ld, rated)
    return ranker.topk(users, N)


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
    z, m = C.load(), C.META
    tr = _trainer(C.initial(z), m["lr"], m["regU"])
    for L in C.list_batches():
        tr.train_step_async(L)
    rated = _rated_csr(z["train_uid"], z["train_iid"], z["train_r"], m["n_users"])
    users = np.unique(z["test_uid"][z["test_uid"] >= 0]).astype(np.int32)
    R = C.ratings_matrix(z)
    check("CDAE hidden(users) vs the mirror", rel_err(tr.hidden(users, rated.indptr, rated.indices, rated.values.astype(np.float32)).numpy()[:users.size, :tr.nh],
                                                     M.hidden(tr.parameters(), users, R[users])), C.GRAD_TOL)
    ids, scores = _rank(tr, rated, users)
    _check_lists("CDAE evaluation, recorded run", ids, scores, M.scores(tr.parameters(), users, R[users]), R[users] != 0)


def test_evaluation_puts_rated_items_last_when_every_logit_is_negative():
    """on logits a rated item (set to 0) would outrank every item of a user whose logits are all negative; after the sigmoid it is
    below all of them"""
    rng = np.random.default_rng(3)
    nu, ni, nh = 40, 1003, 24
    p = dict(W_enc=rng.uniform(-0.1, 0.1, (ni, nh)), W_dec=rng.uniform(-0.05, 0.05, (nh, ni)), b_enc=rng.uniform(-0.3, 0.3, nh),
             b_dec=rng.uniform(-4.0, -2.0, ni), V=rng.uniform(-0.1, 0.1, (nu, nh)))
    p = {k: v.astype(np.float32) for k, v in p.items()}
    tr = _trainer(p)
    uid = np.repeat(np.arange(nu), 30); iid = np.concatenate([rng.permutation(ni)[:30] for _ in range(nu)])
    rated = _rated_csr(uid, iid, np.ones(uid.size), nu)
    R = np.zeros((nu, ni), np.float32); R[uid, iid] = 1
    users = np.arange(nu, dtype=np.int32)
    want = M.scores(p, users, R)
    assert (want < 0.5).all()                                    # every logit negative
    ids, scores = _rank(tr, rated, users)
    _check_lists("CDAE evaluation, all-negative logits", ids, scores, want, R != 0)
    assert (scores > 0).all()


# ---- the drop-in class ------------------------------------------------------------------------------------------------------------------
def _measure_of(strings):
    out = {}
    for s in strings:
        if ":" in s:
            k, v = s.strip().split(":")
            out[k] = float(v)
    return out


def test_class_trains_the_recorded_conf_and_evaluates_like_the_mirror_on_its_own_batches(monkeypatch, tmp_path):
    from qrec_amd.QRec import resolve_model
    from qrec_amd.util.measure import Measure
    from qrec_amd.util.qmath import find_k_largest
    monkeypatch.setenv("QREC_MODE", "exact")
    monkeypatch.chdir(tmp_path)                    # the log and the measure file are written under the working directory
    m = C.META
    train, test = C.train_test_lists()
    model = resolve_model("CDAE")(conf_from_text(m["conf"]), train, test)
    buf = io.StringIO()
    with redirect_stdout(buf):
        model.readConfiguration(); model.initializing_log(); model.initModel()
        random.seed(41); np.random.seed(41)
        model.trainModel()
        model.evalRanking()
    lines = [l for l in buf.getvalue().splitlines() if "loss=" in l]
    assert len(lines) == m["n_steps"] and lines[0].startswith("[1] Epoch: 0001 loss= ")
    got = _measure_of(model.measure)
    # the float64 mirror trained on the batches the class drew, evaluated on the host by the reference's rule
    lists = [model.recorded_lists(k) for k in range(m["n_steps"])]
    p, losses, _ = M.train(model.initial_variables(), lists, m["lr"], m["regU"])
    check("CDAE class: printed losses vs the mirror on the class's own batches",
          rel_err([float(l.split("loss=")[1]) for l in lines], losses), C.GRAD_TOL)
    R = np.zeros((model.num_users, model.num_items))
    for u, i, r in train:
        R[model.data.user[u], model.data.item[i]] = r
    recList = {}
    for user in model.data.testSet_u:
        if model.data.containsUser(user):
            uid = model.data.user[user]
            s = M.scores(p, [uid], R[[uid]])[0]
            s[R[uid] != 0] = 0
        else:
            s = [model.data.globalMean] * model.num_items
        ids, sc = find_k_largest(10, s)
        recList[user] = [(model.data.id2item[i], v) for i, v in zip(ids, sc)]
    want = _measure_of(Measure.rankingMeasure(model.data.testSet_u, recList, [10]))
    for key in ("Recall", "NDCG"):
        check(f"CDAE class: {key}@10 vs the host evaluation of the mirror", abs(got[key] - want[key]), 0.002, inclusive=True, kind="statistical")
    assert got["Recall"] > 0.2
    # trainModel itself consumed nothing before its first step's draws: the first batch is a direct draw from the same seeds
    np.random.seed(41)
    rnd = random.Random(41)
    want_mask = np.random.binomial(1, m["corruption_level"], (model.batch_size, model.num_items))
    indptr, items, _ = model._rated
    rated = [set(items[indptr[u]:indptr[u + 1]].tolist()) for u in range(model.num_users)]
    want_users, want_negs = M.draw_batch(rnd, model.num_users, model.num_items, rated, model.batch_size)
    users, bits, neg_ptr, neg_items = model.batches[0]
    assert users.tolist() == want_users
    assert np.array_equal(np.unpackbits(bits)[:want_mask.size].reshape(want_mask.shape), want_mask)
    assert [set(neg_items[neg_ptr[b]:neg_ptr[b + 1]].tolist()) for b in range(model.batch_size)] == want_negs


# ---- throughput mode: the batch drawn on the device ---------------------------------------------------------------------------------
def _device_stream(seed=5):
    from qrec_amd.autoencoder import DeviceBatchStream
    z, m = C.load(), C.META
    rated = _rated_csr(z["train_uid"], z["train_iid"], z["train_r"], m["n_users"])
    return rated, DeviceBatchStream(rated.indptr, rated.indices, rated.values.astype(np.float32), m["n_items"], 64, 0.9, seed)


def _ascending(ptr, idx):
    return all((np.diff(idx[a:b]) > 0).all() for a, b in zip(ptr[:-1], ptr[1:]))


def test_device_drawn_lists_hold_sets_of_unrated_negatives_ascending_and_consistent_in_both_views():
    """three steps of batch 64 on the subset, read back: negatives unrated and unique per row, at most 5 |rated| of them; every
    live positive a kept input with its rating; both lists ascending, their item-major views the same entries; the keep rate over
    all evaluated positions within 4 standard deviations of co; a second draw of a step has the same bits, another step differs"""
    rated, ds = _device_stream()
    m, R = C.META, C.ratings_matrix()
    kept = evaluated = 0
    drawn = []
    for step in range(3):
        L = ds.draw(step).host()
        cand = ds.cand_count.numpy()
        L.validate()
        drawn.append(L)
        assert L.users.min() >= 0 and L.users.max() < m["n_users"]
        for b in range(64):
            u = L.users[b]
            n_rated = int(rated.indptr[u + 1] - rated.indptr[u])
            it, lab = L.lv_item[L.lv_ptr[b]:L.lv_ptr[b + 1]], L.lv_label[L.lv_ptr[b]:L.lv_ptr[b + 1]]
            neg, pos = it[lab == 0], it[lab == 1]
            assert not R[u, neg].any() and np.unique(neg).size == neg.size and neg.size <= 5 * n_rated
            assert (R[u, pos] != 0).all() and np.array_equal(pos, L.in_item[L.in_ptr[b]:L.in_ptr[b + 1]])
            assert np.array_equal(L.in_val[L.in_ptr[b]:L.in_ptr[b + 1]], R[u, pos])
            assert n_rated < cand[b] <= 6 * n_rated and it.size <= cand[b]
        assert _ascending(L.lv_ptr, L.lv_item) and _ascending(L.in_ptr, L.in_item)
        assert _ascending(L.lv_cptr, L.lv_crow) and _ascending(L.in_cptr, L.in_crow)
        lv_row = np.repeat(np.arange(64), np.diff(L.lv_ptr)); lv_citem = np.repeat(np.arange(L.n_items), np.diff(L.lv_cptr))
        assert np.array_equal(np.sort(L.lv_cslot), np.arange(L.n_live))
        assert np.array_equal(lv_row[L.lv_cslot], L.lv_crow) and np.array_equal(L.lv_item[L.lv_cslot], lv_citem)
        in_row = np.repeat(np.arange(64), np.diff(L.in_ptr)); in_citem = np.repeat(np.arange(L.n_items), np.diff(L.in_cptr))
        order = np.lexsort((in_row, L.in_item))                     # the row-major input entries in item-major order
        assert np.array_equal(in_row[order], L.in_crow) and np.array_equal(L.in_item[order], in_citem)
        assert np.array_equal(L.in_val[order], L.in_cval)
        kept += L.n_live; evaluated += int(cand.sum())
    sd = np.sqrt(0.9 * 0.1 / evaluated)
    check("CDAE device stream: keep rate over the evaluated positions vs co, in standard deviations", abs(kept / evaluated - 0.9) / sd, 4.0,
          ctx=dict(evaluated=evaluated, kept=kept), kind="statistical")
    again = ds.draw(0).host()
    same_bits("CDAE device stream, step 0 drawn twice", {k: getattr(drawn[0], k) for k in L.NAMES}, {k: getattr(again, k) for k in L.NAMES})
    assert not np.array_equal(drawn[0].users, drawn[1].users)
    assert np.unique(np.concatenate([d.users for d in drawn])).size > 100          # 192 uniform draws over 291 users


def test_device_lists_and_the_same_lists_from_the_host_train_to_the_same_bits_under_ordered_reductions():
    """the paired check of tests/device_stream.py: the device-drawn lists fed as they are, and read back and fed through the
    host-list path, both with ordered reductions, give bit-identical tables and losses"""
    from qrec_amd.graph import ordered_reductions
    z, m = C.load(), C.META
    _, ds = _device_stream()
    with ordered_reductions(True):
        a, b = _trainer(C.initial(z), m["lr"], m["regU"]), _trainer(C.initial(z), m["lr"], m["regU"])
        la, lb = [], []
        for step in range(3):
            L = ds.draw(step)
            host = L.host()
            a.train_step_async(L); la.append(a.loss())
            b.train_step_async(host); lb.append(b.loss())
    assert all(np.isfinite(la)) and la[0] != la[1]
    same_bits("CDAE device-list path vs host-list path", dict(a.parameters(), losses=np.array(la)), dict(b.parameters(), losses=np.array(lb)))


def test_class_trains_in_throughput_mode_without_consuming_the_host_generators(monkeypatch, tmp_path):
    from qrec_amd.QRec import resolve_model
    monkeypatch.setenv("QREC_MODE", "throughput"); monkeypatch.setenv("QREC_SEED", "7"); monkeypatch.setenv("QREC_QUIET", "1")
    monkeypatch.chdir(tmp_path)
    train, test = C.train_test_lists()
    model = resolve_model("CDAE")(conf_from_text(C.META["conf"]), train, test)
    with redirect_stdout(io.StringIO()):
        model.readConfiguration(); model.initializing_log(); model.initModel()
        random.seed(1); np.random.seed(1)
        before = (random.getstate(), np.random.get_state()[1].copy())
        model.trainModel()
        assert random.getstate() == before[0] and np.array_equal(np.random.get_state()[1], before[1])
        model.evalRanking()
    assert np.isfinite(model.trainer.loss()) and _measure_of(model.measure)["Recall"] > 0.2
