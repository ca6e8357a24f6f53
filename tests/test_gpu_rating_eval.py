"""The rating evaluation on the device (csrc/rating_eval.hip, engine.RatingEvaluator): unrounded predictions of the six
forms against the numpy mirror (tests/rating_eval_mirror.py), the boundary kernel against checkRatingBoundary, the folded
error sums against Python's sum, bound buffers, determinism, refusals, the recorded FilmTrust runs, and the twelve classes
end to end with the device evaluator against the host loops."""
import glob
import importlib
import io
import json
import os
import random
from contextlib import redirect_stdout
from types import SimpleNamespace

import numpy as np
import pytest

import rating_eval_cases as K
import rating_eval_mirror as M
from helpers import GOLDEN, check, conf_from_text
from qrec_amd import capi
from qrec_amd.base.recommender import Recommender
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.engine import DeviceTables, MfSgd, RatingEvaluator
from qrec_amd.util.measure import Measure

pytestmark = pytest.mark.gpu

# a launch holds at most this many pairs side by side (one per wavefront); a longer list wraps the grid-stride loop
BLOCK_CAP_PAIRS = capi.RATING_MAX_BLOCKS * capi.RATING_BLOCK_WAVES
COUNTS = (1, 63, 64, 65, BLOCK_CAP_PAIRS + 65)
DIMS = (5, 10, 64, 65, 128, 200)
RAW_TOL = 1e-11      # x max(1, |value|): dots of <= 256 terms with sums of ~28 (dot forms) / ~73 (METRIC, d = 128) round below 1e-12


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    yield


def test_the_block_cap_is_the_one_the_library_was_built_with():
    assert (capi.RATING_MAX_BLOCKS, capi.RATING_BLOCK_WAVES) == (256, 8) and COUNTS[-1] > BLOCK_CAP_PAIRS


@pytest.mark.parametrize("form,d", [(f, d) for f in M.FORMS for d in DIMS if not (f == "METRIC" and d > capi.SOCIAL_H_MAX_D)])
def test_unrounded_predictions_match_the_mirror(form, d):
    """every count: cold user, cold item, both cold, a user without followees and one with a single followee, an SVD++ user
    with one rated item and one with 300, a repeated user (rating_eval_cases.synthetic).  METRIC stages H in LDS and stops
    at d = 128 (the refusal above it has its own test)."""
    for n in COUNTS:
        c = K.synthetic(form, d, n)
        if n >= 63:
            assert (c["uid"] < 0).any() and (c["iid"] < 0).any() and ((c["uid"] < 0) & (c["iid"] < 0)).any()
            assert (c["uid"] == 0).any() and (c["uid"] == 1).any() and (c["uid"] == 2).sum() >= 2
        want = M.raw_predictions(form, c["uid"], c["iid"], c["P"], c["Q"], **c["kw"])
        got = K.evaluator(c).raw_predictions()
        assert got.shape == want.shape and np.isfinite(got).all()
        worst = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
        check(f"{form} d={d} n={n}: |device - mirror| / max(1, |mirror|)", worst, RAW_TOL)


def test_boundary_kernel_is_check_rating_boundary():
    x = M.boundary_cases()
    for lo, hi in ((0.5, 4.0), (-1.0, 6.0)):
        rec = SimpleNamespace(data=SimpleNamespace(rScale=[lo, hi]))
        want = np.array([Recommender.checkRatingBoundary(rec, v) for v in x.tolist()], dtype=np.float64)
        buf = DB.from_numpy(x)
        capi.rating_boundary(buf, x.size, lo, hi)
        got = buf.numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (x[bad][:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())


@pytest.mark.parametrize("form", ("DOT", "METRIC"))
def test_folded_sums_are_pythons_sums(form):
    c = K.synthetic(form, 10, COUNTS[-1])
    ev = K.evaluator(c)
    pred = ev.predictions()
    s_abs, s_sq = ev.error_sums()
    res = [[None, None, r, p] for r, p in zip(c["rating"].tolist(), pred.tolist())]
    # Python 3.10's sum() is a plain left-to-right sum: the absolute-error sum is held to the bit, the MAE string to the byte
    assert np.float64(s_abs).view(np.uint64) == np.float64(sum(abs(e[2] - e[3]) for e in res)).view(np.uint64)
    got, want = ev.measure(), Measure.ratingMeasure(res)
    assert got[0] == want[0]
    # Measure.RMSE squares with ** 2, the C library's pow, and e ** 2 != e * e for about one rating-shaped error in 10^4: the
    # squared-error sum is held to 1e-12 relative, not to the bit
    want_sq = sum((e[2] - e[3]) ** 2 for e in res)
    check(f"{form}: squared-error sum against Python's", abs(s_sq - want_sq) / want_sq, 1e-12)
    assert got[1].startswith("RMSE:") and got[1].endswith("\n")
    check(f"{form}: RMSE against Measure's", abs(float(got[1][5:]) - float(want[1][5:])) / float(want[1][5:]), 1e-12)
    assert got == M.measure(c["rating"], pred)


def test_no_pairs_measure_like_measure():
    c = K.synthetic("DOT", 10, 1)
    for k in ("uid", "iid", "rating"):
        c[k] = c[k][:0]
    ev = K.evaluator(c)
    assert ev.predictions().shape == (0,) and ev.measure() == Measure.ratingMeasure([])


def test_evaluator_reads_the_bound_tables_after_an_epoch():
    """one MfSgd epoch moves P, Q, Bu, Bi on the device; measure() with nothing uploaded sees the moved tables"""
    c = K.synthetic("BIASED", 10, 65)
    rng = np.random.default_rng(5)
    U, I = c["P"].shape[0], c["Q"].shape[0]
    t = DeviceTables(c["P"], c["Q"], np.float64)
    sgd = MfSgd(t, 500, capi.MF_SVD, c["kw"]["Bu"], c["kw"]["Bi"])
    kw = c["kw"]
    ev = RatingEvaluator("BIASED", t, c["uid"], c["iid"], c["rating"], c["scale"], kw["user_means"], kw["item_means"], kw["global_mean"],
                         Bu=sgd.d_Bu, Bi=sgd.d_Bi)
    before = ev.measure()
    sgd.epoch(rng.integers(0, U, 500), rng.integers(0, I, 500), rng.integers(1, 9, 500) / 2.0, 0.02, 0.01, 0.01, 0.01, kw["global_mean"])
    after = ev.measure()
    P, Q = t.download()
    Bu, Bi = sgd.biases()
    assert not np.array_equal(P, c["P"]) and not np.array_equal(Bu, kw["Bu"])
    want = M.measure(c["rating"], M.predictions("BIASED", c["uid"], c["iid"], P, Q, c["scale"], **dict(kw, Bu=Bu, Bi=Bi)))
    assert after == want and after != before


@pytest.mark.parametrize("form", M.FORMS)
def test_two_calls_give_the_same_bytes(form):
    ev = K.evaluator(K.synthetic(form, 65, COUNTS[-1]))
    a, b = ev.predictions(), ev.predictions()
    assert a.tobytes() == b.tobytes()
    assert ev.measure() == ev.measure()


def test_refusals_leave_the_output_untouched():
    c = K.synthetic("METRIC", 10, 64)
    sentinel = np.full(64, -7.25)
    out = DB.from_numpy(sentinel)
    z = lambda *s: DB.zeros(s, np.float64)
    idx = DB.from_numpy(np.zeros(64, np.int32))
    with pytest.raises(capi.QRecError) as e:          # METRIC above the LDS cap
        capi.rating_predict(capi.RATING_METRIC, capi.F64, z(4, 129), z(4, 129), 4, 4, 129, 129, idx, idx, 64, out, 3.0, d_Bu=z(4), d_Bi=z(4),
                            d_aux=z(129, 129))
    assert e.value.code == capi.ERR_UNSUPPORTED and "128" in str(e.value)
    with pytest.raises(capi.QRecError, match="fp64"):    # fp32 tables
        capi.rating_predict(capi.RATING_DOT, capi.F32, z(4, 16), z(4, 16), 4, 4, 10, 16, idx, idx, 64, out, 3.0, d_user_mean=z(4),
                            d_item_mean=z(4))
    with pytest.raises(capi.QRecError, match="form"):
        capi.rating_predict(9, capi.F64, z(4, 16), z(4, 16), 4, 4, 10, 16, idx, idx, 64, out, 3.0)
    with pytest.raises(capi.QRecError, match="Bu and Bi"):
        capi.rating_predict(capi.RATING_BIASED, capi.F64, z(4, 16), z(4, 16), 4, 4, 10, 16, idx, idx, 64, out, 3.0)
    assert np.array_equal(out.numpy(), sentinel)
    # ids at or above the table sizes, or below -1: refused by the evaluator before an upload or a launch
    ev = K.evaluator(c)
    good = ev.predictions()
    ev.d_pred.upload(sentinel)
    U, I = c["P"].shape[0], c["Q"].shape[0]
    for col, bad in (("uid", U), ("uid", -2), ("iid", I), ("iid", -2)):
        ids = {"uid": c["uid"].copy(), "iid": c["iid"].copy()}
        ids[col][17] = bad
        with pytest.raises(ValueError, match="test pair ids"):
            ev.set_pairs(ids["uid"], ids["iid"], c["rating"])
        with pytest.raises(ValueError, match="test pair ids"):
            K.evaluator(dict(c, **ids))
    assert np.array_equal(ev.d_pred.numpy(), sentinel)
    assert np.array_equal(ev.predictions(), good)        # and its pairs are the ones it had


@pytest.mark.parametrize("model", sorted(K.RECORDED))
def test_device_reproduces_the_recorded_predictions(model):
    """the recorded run's final tables uploaded: test_pred exactly, but for at most one pair at a rounding boundary"""
    try:
        c = K.recorded(model)
    except KeyError as e:
        pytest.skip(str(e))
    ev = K.evaluator(c)
    raw, got = ev.raw_predictions(), ev.predictions()
    K.assert_equals_recorded(model, got, raw, c["want"])


# ---- the classes -------------------------------------------------------------------------------------------------------------
CLASSES = dict(K.RECORDED, SREE=("social_sree_filmtrust", "golden_social_meta.json", "SREE", "EUCLID"))


def _run_class(model, tmp_path, tag):
    npz, meta_file, key, _ = CLASSES[model]
    meta = json.load(open(os.path.join(GOLDEN, meta_file)))[key]
    z = np.load(os.path.join(GOLDEN, npz + ".npz"))
    cls = getattr(importlib.import_module(f"qrec_amd.model.rating.{model}"), model)
    out = tmp_path / tag
    out.mkdir()
    # the recorded conf, with the prediction file switched on; SREE's recorded run ranks, here it rates
    text = meta["conf"].replace("output.setup=off -dir ./results/", f"output.setup=on -dir {out}/").replace("item.ranking=on", "item.ranking=off")
    assert f"-dir {out}/" in text
    conf = conf_from_text(text)
    name = lambda c: f"u{c}" if c >= 0 else f"x{-1 - c}"
    test = [[name(a) if a >= 0 else f"xu{k}", f"i{b}" if b >= 0 else f"xi{k}", float(r)]
            for k, (a, b, r) in enumerate(zip(z["test_uid"].tolist(), z["test_iid"].tolist(), z["test_rating"].tolist()))]
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    with redirect_stdout(io.StringIO()) as log:
        if "order0" in z.files:
            rows = [[f"u{a}", f"i{b}", float(r)] for (a, b), r in zip(z["order0"].tolist(), z["rating0"].tolist())]
            m = cls(conf, rows, test)
        else:
            from qrec_amd.util.io import FileIO
            path = out / "trust.txt"
            path.write_text("".join(f"{name(x)} {name(y)} {w!r}\n" for x, y, w in zip(z["raw_follower"].tolist(), z["raw_followee"].tolist(),
                                                                                     z["raw_weight"].tolist())))
            rows = [[f"u{a}", f"i{b}", float(r)] for a, b, r in zip(z["order0_u"].tolist(), z["order0_i"].tolist(), z["order0_r"].tolist())]
            m = cls(conf, rows, test, FileIO.loadRelationship(conf, str(path)))
        measure = m.execute()
    files = glob.glob(str(out / "*-rating-predictions*.txt"))
    assert len(files) == 1
    epochs = [line for line in log.getvalue().splitlines() if " epoch " in line and "MAE" in line]
    return m, measure, open(files[0]).read().splitlines(), epochs


@pytest.mark.parametrize("model", sorted(CLASSES))
def test_class_with_the_evaluator_equals_the_class_on_the_host_loops(model, tmp_path, monkeypatch):
    cls = getattr(importlib.import_module(f"qrec_amd.model.rating.{model}"), model)

    def refuse(self, u, i):
        raise AssertionError("a test pair went through predictForRating")
    with monkeypatch.context() as mp:
        mp.setattr(cls, "predictForRating", refuse)
        m, dev, dev_lines, dev_epochs = _run_class(model, tmp_path, "device")
    assert m.rating_evaluator() is not None
    with monkeypatch.context() as mp:
        mp.setattr(cls, "rating_evaluator", lambda self: None)
        _, host, host_lines, host_epochs = _run_class(model, tmp_path, "host")
    assert dev[0] == host[0] and dev[0].startswith("MAE:")
    d_rmse, h_rmse = float(dev[1].split(":")[1]), float(host[1].split(":")[1])
    check(f"{model}: RMSE, device evaluator against the host loop", abs(d_rmse - h_rmse) / h_rmse, 1e-12)
    assert len(dev_lines) == 1748 and dev_lines == host_lines
    assert len(dev_epochs) >= 1 and dev_epochs == host_epochs          # the printed lines carry 7 digits of MAE and RMSE
    assert all(len(row) == 4 for row in m.data.testData)
