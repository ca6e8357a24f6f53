"""Ranking evaluation of the six rating models whose score is not one plain inner product, on the MI355X: the device path
(ranking.FormRanker, csrc/rank_forms.hip, through ``rank_measure_all_test_users``) beside the host loop it replaces
(``Recommender.rank_all_test_users``: one ``predictForRanking`` call, one mask and one ``find_k_largest`` per test user, then
``Measure.rankingMeasure``) on the same tables.

    python tools/bench_rating_rank.py [--shape filmtrust|epinions_like] [out.json]     # default out: profiles/rating_rank_bench.json

SVD, SVDPlusPlus, EE, SREE, RSTE, SocialFD, d = 10, ``-topN 10,20``, the two workloads of tools/bench_rating_eval.py: FilmTrust
(the recorded training rows and relations; the test users are the users of its 1,747 recorded test pairs) and the Epinions-like
shape (40,000 users, 140,000 items, 660,000 ratings, 490,000 trust edges, seeded) with 2,000 test users of three test items each.
Per model and workload, after one training epoch (so that the tables are a model's, not noise):
  * device_ms: ``rank_measure_all_test_users([10, 20], 20)`` -- item-side preparation, operand rows, scoring, mask, top-N, hit counts,
    read-back and the strings -- the median of 30 calls between two device events, after 3 warm-up calls;
  * host_loop_ms: the loop on the same tables (downloaded first, as the class has them after every epoch), host clock: the median of
    3 runs over all test users at FilmTrust; at the Epinions-like shape ONE run over the first 50 test users, reported per user and
    extrapolated to the 2,000 (``host_loop_ms_extrapolated``: not a measurement of the whole loop);
  * measures_equal: the two paths' measure strings over the users the host loop ran are the same strings.
With --shape the file's other workload is kept as it was."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_rating_eval as E  # noqa: E402

MODELS = ("SVD", "SVDPlusPlus", "EE", "SREE", "RSTE", "SocialFD")
SIGN = {"SocialFD": -1.0}
TOP, N, WARMUP, CALLS, HOST_USERS_LARGE = [10, 20], 20, 3, 30, 50


class RankData(E.HostData):
    """HostData plus what the ranking loops read: testSet_u (insertion order = test rows' order), id2item, trainingSize"""

    def __init__(self, wl, um, im, gm, scale):
        super().__init__(wl, um, im, gm, scale)
        self.id2item = dict(enumerate(self.inames))
        self.testSet_u = {}
        for u, i, r in self.testData:
            self.testSet_u.setdefault(u, {})[i] = r
        self._sizes = (wl["U"], wl["I"], int(wl["u"].size))

    def trainingSize(self):
        return self._sizes

    def userRated(self, u):
        return super().userRated(u) if u in self.user else ([], [])      # trainSet_u is a defaultdict: a cold user rated nothing


def test_users(name, wl):
    """the workload's test pairs: FilmTrust's recorded ones; at the Epinions-like shape 2,000 users x 3 items (1 % unknown users)"""
    if name == "filmtrust":
        return
    rng = np.random.default_rng(13)
    users = rng.choice(wl["U"], 2000, replace=False).astype(np.int32)
    tu = np.repeat(users, 3)
    tu[rng.random(tu.size) < 0.01] = -1
    wl.update(tu=tu, ti=rng.integers(0, wl["I"], tu.size).astype(np.int32), tr=rng.integers(1, 11, tu.size) / 2.0)


def model_over(model, wl, data, rng):
    """the class, un-constructed, over the workload: its tables after one epoch, its bound FormRanker"""
    import importlib

    from qrec_amd.ranking import FormRanker
    t, epoch, (form, buffers), host_attrs = E.build(model, wl, data, rng)
    if epoch is not None:
        epoch()
    kw = dict(buffers)
    if "rated" in kw:
        ptr, items, _ = kw.pop("rated")
        kw["y_rated"] = (ptr, items)
    cls = getattr(importlib.import_module(f"qrec_amd.model.rating.{model}"), model)
    m = cls.__new__(cls)
    m.data, m.num_items, m.modelName, m.foldInfo, m._dp = data, wl["I"], model, "[1]", None
    m.P, m.Q = t.download(np.float64)
    for k, v in host_attrs().items():
        setattr(m, k, v)
    m._form_ranker = FormRanker(form, t, data.rated_csr(), mu=data.globalMean, sign=SIGN.get(model, 1.0), **kw)
    return m, form


def host_loop(m):
    from qrec_amd.base.recommender import Recommender
    from qrec_amd.util.measure import Measure
    with redirect_stdout(io.StringIO()):
        return Measure.rankingMeasure(m.data.testSet_u, Recommender.rank_all_test_users(m, N), TOP)


def restrict(m, users):
    """the same model over the first ``users`` test users only (fresh test CSR on the ranker)"""
    m.data.testSet_u = dict(list(m.data.testSet_u.items())[:users])
    m._test_cache = None
    m._form_ranker.test = None


def bench(model, name, wl, data):
    from qrec_amd import capi
    rng = np.random.default_rng(MODELS.index(model))
    m, form = model_over(model, wl, data, rng)
    row = dict(model=model, form=form, n_test_users=len(data.testSet_u), top=TOP)
    for _ in range(WARMUP):
        dev = m.rank_measure_all_test_users(TOP, N)
    times, a, b = [], capi.Event(), capi.Event()
    for _ in range(CALLS):
        a.record(); dev = m.rank_measure_all_test_users(TOP, N); b.record(); b.sync()
        times.append(b.elapsed_ms_since(a))
    row["device_ms"] = round(float(np.median(times)), 4)
    row["device_ms_min_max"] = [round(min(times), 4), round(max(times), 4)]
    full = m.data.testSet_u
    if name == "filmtrust":
        host_ms, host_all = E.median_wall_ms(lambda: host_loop(m), 3)
        host = host_loop(m)
        row["host_loop_ms"], row["host_loop_ms_all"] = round(host_ms, 2), host_all
        row["host_ms_per_user"] = round(host_ms / len(full), 4)
        row["host_over_device"] = round(host_ms / row["device_ms"], 1)
    else:
        restrict(m, HOST_USERS_LARGE)
        dev = m.rank_measure_all_test_users(TOP, N)
        host_ms, _ = E.median_wall_ms(lambda: host_loop(m), 1)
        host = host_loop(m)
        row["host_users_run"] = HOST_USERS_LARGE
        row["host_ms_per_user"] = round(host_ms / HOST_USERS_LARGE, 3)
        row["host_loop_ms_extrapolated"] = round(host_ms / HOST_USERS_LARGE * len(full), 1)
        row["host_over_device_extrapolated"] = round(row["host_loop_ms_extrapolated"] / row["device_ms"], 1)
    row["measures_equal"] = bool(dev == host)
    row["measure_device"], row["measure_host"] = [x.strip() for x in dev], [x.strip() for x in host]
    m.data.testSet_u = full
    return row


def main():
    args = sys.argv[1:]
    which = None
    if args and args[0] == "--shape":
        which, args = args[1], args[2:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "rating_rank_bench.json")
    from qrec_amd import capi
    capi.init(0)
    res = dict(device=capi.device_info()["arch"], d=E.D, top=TOP, device_calls_timed=CALLS, warmup_calls=WARMUP, workloads={})
    if which and os.path.exists(out_path):
        res["workloads"] = json.load(open(out_path)).get("workloads", {})
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    for name, wl in E.workloads(which).items():
        test_users(name, wl)
        rng = np.random.default_rng(3)
        um, im = rng.random(wl["U"]) * 3 + 1, rng.random(wl["I"]) * 3 + 1
        data = RankData(wl, um, im, float(um.mean()), (float(wl["r"].min()), float(wl["r"].max())))
        rows = []
        res["workloads"][name] = dict(n_users=wl["U"], n_items=wl["I"], n_ratings=int(wl["u"].size), n_relations=int(wl["a"].size),
                                      n_test_users=len(data.testSet_u), models=rows)
        for model in MODELS:
            rows.append(bench(model, name, wl, data))
            print(name, json.dumps(rows[-1]), flush=True)
            with open(out_path, "w") as f:                       # after every model: a run that is cut short leaves its rows
                json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
