"""The rating evaluation on the host: the numpy mirror (tests/rating_eval_mirror.py) that the device kernels are held to is
itself held here to ``Recommender.checkRatingBoundary`` and to the predictions the reference recorded on FilmTrust; the
class hooks that choose between the device evaluator and the host loops; the engine's refusals that need no device."""
from types import SimpleNamespace

import numpy as np
import pytest

import rating_eval_cases as K
import rating_eval_mirror as M
from qrec_amd.base.recommender import Recommender

TWELVE = ("BasicMF", "PMF", "SVD", "SVDPlusPlus", "EE", "SoRec", "SoReg", "SocialMF", "RSTE", "SREE", "LOCABAL", "SocialFD")


def _check_boundary(lo, hi):
    rec = SimpleNamespace(data=SimpleNamespace(rScale=[lo, hi]))
    return lambda x: Recommender.checkRatingBoundary(rec, x)


def test_boundary_rule_is_check_rating_boundary():
    """== on every value: -0.0 against 0.0 below zero compare equal, nothing else may differ"""
    x = M.boundary_cases()
    assert x.size == 300000 + 6 * 7001 + 6
    for lo, hi in ((0.5, 4.0), (-1.0, 6.0)):
        ref = _check_boundary(lo, hi)
        want = np.array([ref(v) for v in x.tolist()], dtype=np.float64)
        got = M.boundary_array(x, lo, hi)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (x[bad][:5].tolist(), got[bad][:5].tolist(), want[bad][:5].tolist())
    assert M.boundary(9.25, 0.5, 4.0) == 4.0 and M.boundary(-3.0, 0.5, 4.0) == 0.5


def test_fma_residual_is_exact():
    from fractions import Fraction
    for v in M.boundary_cases()[::997].tolist():
        y = v * 1000.0
        assert Fraction(M._fma_residual(v, 1000.0, y)) == Fraction(v) * 1000 - Fraction(y)


def test_sree_recording_has_no_predictions():
    """the twelfth rating model's recorded run ranks (item.ranking=on): it carries no test_pred and is not in RECORDED"""
    import os
    z = np.load(os.path.join(K.GOLDEN, "social_sree_filmtrust.npz"))
    assert "test_pred" not in z.files and "SREE" not in K.RECORDED and len(K.RECORDED) == 11


@pytest.mark.parametrize("model", sorted(K.RECORDED))
def test_mirror_reproduces_the_recorded_predictions(model):
    """the run's final tables, the means and the scale from its training rows -> its test_pred, exactly; at most one pair
    per run may differ, and only within 1e-9 of a rounding boundary"""
    try:
        c = K.recorded(model)
    except KeyError as e:
        pytest.skip(str(e))
    assert c["uid"].size == 1747 and int((c["uid"] < 0).sum()) == 10 and int((c["iid"] < 0).sum()) == 41
    raw = M.raw_predictions(c["form"], c["uid"], c["iid"], c["P"], c["Q"], **c["kw"])
    got = M.boundary_array(raw, c["scale"][0], c["scale"][-1])
    K.assert_equals_recorded(model, got, raw, c["want"])


def test_mirror_measure_is_rating_measure():
    from qrec_amd.util.measure import Measure
    c = K.recorded("BasicMF")
    res = [[None, None, r, p] for r, p in zip(c["rating"].tolist(), c["want"].tolist())]
    got, want = M.measure(c["rating"], c["want"]), Measure.ratingMeasure(res)
    assert got[0] == want[0]
    assert float(got[1][5:]) == pytest.approx(float(want[1][5:]), rel=1e-12)       # ** 2 is libm's pow, e * e a product
    assert M.measure([], []) == Measure.ratingMeasure([])


# ---- the hooks -------------------------------------------------------------------------------------------------------------------
def test_only_the_twelve_classes_override_the_hook():
    from qrec_amd.QRec import resolve_model
    from qrec_amd.base.iterativeRecommender import IterativeRecommender
    from qrec_amd.base.socialRecommender import SocialRecommender
    assert Recommender.rating_evaluator(SimpleNamespace()) is None
    for base in (IterativeRecommender, SocialRecommender):
        assert "rating_evaluator" not in vars(base)
    for name in TWELVE:
        cls = resolve_model(name)
        assert "rating_evaluator" in vars(cls), name
        assert cls.rating_evaluator(SimpleNamespace()) is None          # nothing trained yet: the host loop
    for name in ("UserKNN", "ItemKNN", "SlopeOne", "BPR"):
        assert resolve_model(name).rating_evaluator is Recommender.rating_evaluator


class _Stub:
    """what rating_performance / evalRatings touch, with a predictForRating of its own"""
    def __init__(self, evaluator):
        from qrec_amd.base.iterativeRecommender import IterativeRecommender
        self.cls = IterativeRecommender
        self.data = SimpleNamespace(testData=[["a", "x", 3.0], ["b", "y", 1.5]], rScale=[0.5, 4.0])
        self.evaluator, self.calls = evaluator, 0

    def rating_evaluator(self):
        return self.evaluator

    def predictForRating(self, u, i):
        self.calls += 1
        return 2.71828

    def checkRatingBoundary(self, p):
        return Recommender.checkRatingBoundary(self, p)

    def rating_performance_host(self):
        return self.cls.rating_performance_host(self)


def test_rating_performance_keeps_the_host_loop_without_an_evaluator():
    s = _Stub(None)
    got = s.cls.rating_performance(s)
    from qrec_amd.util.measure import Measure
    assert s.calls == 2 and got == Measure.ratingMeasure([[0, 0, 3.0, 2.718], [0, 0, 1.5, 2.718]]) and s.measure == got


def test_rating_performance_uses_the_evaluator_when_there_is_one():
    s = _Stub(SimpleNamespace(measure=lambda: ["MAE:1\n", "RMSE:2\n"]))
    assert s.cls.rating_performance(s) == ["MAE:1\n", "RMSE:2\n"] and s.calls == 0 and s.measure == ["MAE:1\n", "RMSE:2\n"]


def test_rating_test_pairs_are_built_once_with_unknown_names_as_minus_one():
    rec = SimpleNamespace(data=SimpleNamespace(testData=[["a", "x", 3.0], ["zz", "y", 1.5], ["b", "qq", 2.0]], user={"a": 0, "b": 1},
                                               item={"x": 0, "y": 1}))
    u, i, r = Recommender.rating_test_pairs(rec)
    assert u.tolist() == [0, -1, 1] and i.tolist() == [0, 1, -1] and r.tolist() == [3.0, 1.5, 2.0]
    assert u.dtype == np.int32 and i.dtype == np.int32 and r.dtype == np.float64
    assert Recommender.rating_test_pairs(rec)[0] is u


# ---- refusals that need no device ---------------------------------------------------------------------------------------------
def test_engine_refuses_before_touching_the_device():
    from qrec_amd import capi
    from qrec_amd.engine import RatingEvaluator
    z1 = np.zeros(1)
    t32 = SimpleNamespace(dtype=np.dtype(np.float32), d=8, n_users=4, n_items=4)
    with pytest.raises(ValueError, match="fp64"):
        RatingEvaluator("DOT", t32, [0], [0], [1.0], (0.5, 4.0), np.zeros(4), np.zeros(4), 3.0)
    with pytest.raises(ValueError, match="fp64"):
        RatingEvaluator.from_host("DOT", np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32), [0], [0], [1.0], (0.5, 4.0),
                                  np.zeros(4), np.zeros(4), 3.0)
    t = SimpleNamespace(dtype=np.dtype(np.float64), d=capi.SOCIAL_H_MAX_D + 1, n_users=4, n_items=4)
    with pytest.raises(ValueError, match="num.factors <= 128"):
        RatingEvaluator("METRIC", t, [0], [0], [1.0], (0.5, 4.0), np.zeros(4), np.zeros(4), 3.0, Bu=z1, Bi=z1, H=z1)
    with pytest.raises(ValueError, match="num.factors <= 128"):
        RatingEvaluator.from_host("METRIC", np.zeros((4, 129)), np.zeros((4, 129)), [0], [0], [1.0], (0.5, 4.0), np.zeros(4), np.zeros(4), 3.0,
                                  Bu=np.zeros(4), Bi=np.zeros(4), H=np.zeros((129, 129)))
    t = SimpleNamespace(dtype=np.dtype(np.float64), d=8, n_users=4, n_items=5)
    for uid, iid in (([4], [0]), ([0], [5]), ([-2], [0]), ([0], [-2])):
        with pytest.raises(ValueError, match="test pair ids"):
            RatingEvaluator("DOT", t, uid, iid, [1.0], (0.5, 4.0), np.zeros(4), np.zeros(5), 3.0)
    with pytest.raises(ValueError, match="missing"):
        RatingEvaluator("BIASED", t, [0], [0], [1.0], (0.5, 4.0), np.zeros(4), np.zeros(5), 3.0)
