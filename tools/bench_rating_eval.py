"""The rating models' evaluation on the MI355X: the device evaluator (engine.RatingEvaluator, csrc/rating_eval.hip) beside
the host loop it replaces (``rating_performance_host``: one ``predictForRating`` call per test pair) and beside the model's
epoch.

    python tools/bench_rating_eval.py [--shape filmtrust|epinions_like] [out.json]     # default out: profiles/rating_eval_bench.json

Twelve models, d = 10, two workloads: FilmTrust (the recorded training rows, kept relations and the 1,747 recorded test
pairs of tests/golden) and the Epinions-like shape of tools/bench_social.py (40,000 users, 140,000 items, 660,000 ratings,
490,000 trust edges, seeded) with 66,000 test pairs, one in a hundred of them naming an unknown user or item.  Per model
and workload:
  * device_eval_ms: ``RatingEvaluator.measure()`` -- predictions, boundary, errors, both folds and the read-back of the two
    sums -- bound to the SGD object's device buffers: the median of 30 calls between two device events, after 3 warm-up calls;
  * host_loop_ms: the class's own ``rating_performance_host`` on the same tables (downloaded first, as the class has them
    after every epoch), host clock; the median of 3 calls at FilmTrust, one call at the Epinions-like shape;
  * epoch_ms: the model's passes over the training rows (each ends in a device synchronisation), the median of 3;
  * mae_equal: the two paths' MAE strings are the same string.
SVD++'s epoch at the Epinions-like shape is not run (every rating rewrites all of its user's Y rows; the heaviest users
rate thousands of items): the row says so.  With --shape the file's other workload is kept as it was."""
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODELS = ("BasicMF", "PMF", "SVD", "SVDPlusPlus", "EE", "SoRec", "SoReg", "SocialMF", "RSTE", "SREE", "LOCABAL", "SocialFD")
D, EPOCHS, WARMUP, CALLS = 10, 3, 3, 30


def workloads(which):
    import bench_social as B
    out = {}
    if which in (None, "filmtrust"):
        wl = B.filmtrust()
        z = np.load(os.path.join(ROOT, "tests", "golden", "social_sorec_filmtrust.npz"))
        wl.update(tu=np.maximum(z["test_uid"], -1).astype(np.int32), ti=np.maximum(z["test_iid"], -1).astype(np.int32), tr=z["test_rating"])
        out["filmtrust"] = wl
    if which in (None, "epinions_like"):
        wl = B.epinions_like()
        rng = np.random.default_rng(12)
        n = 66_000
        tu, ti = rng.integers(0, wl["U"], n).astype(np.int32), rng.integers(0, wl["I"], n).astype(np.int32)
        tu[rng.random(n) < 0.005] = -1; ti[rng.random(n) < 0.005] = -1
        wl.update(tu=tu, ti=ti, tr=rng.integers(1, 11, n) / 2.0)
        out["epinions_like"] = wl
    return out


class HostData:
    """what predictForRating, checkRatingBoundary and rating_performance_host read of data/rating.py's model, over names"""

    def __init__(self, wl, um, im, gm, scale):
        U, I = wl["U"], wl["I"]
        self.unames, self.inames = [f"u{k}" for k in range(U)], [f"i{k}" for k in range(I)]
        self.user, self.item = dict(zip(self.unames, range(U))), dict(zip(self.inames, range(I)))
        self.userMeans, self.itemMeans, self.globalMean = dict(zip(self.unames, um.tolist())), dict(zip(self.inames, im.tolist())), gm
        self.rScale = list(scale)
        self.testData = [[f"u{u}" if u >= 0 else f"xu{k}", f"i{i}" if i >= 0 else f"xi{k}", r]
                         for k, (u, i, r) in enumerate(zip(wl["tu"].tolist(), wl["ti"].tolist(), wl["tr"].tolist()))]
        rows = [dict() for _ in range(U)]
        for u, i, r in zip(wl["u"].tolist(), wl["i"].tolist(), wl["r"].tolist()):
            rows[u][i] = r
        self._rows = rows

    def containsUser(self, u):
        return u in self.user

    def containsItem(self, i):
        return i in self.item

    def userRated(self, u):
        row = self._rows[self.user[u]]
        return [self.inames[i] for i in row], list(row.values())

    def getUserId(self, u):
        return self.user.get(u)

    def rated_csr(self):
        from qrec_amd.interactions import CSR
        ptr = np.zeros(len(self._rows) + 1, np.int64)
        ptr[1:] = np.cumsum([len(r) for r in self._rows])
        return CSR(ptr, np.array([i for r in self._rows for i in r], dtype=np.int32))


def build(model, wl, data, rng):
    """(tables, sgd, epoch(), evaluator kwargs, host attributes()) of one model over the workload"""
    from qrec_amd import capi
    from qrec_amd.engine import DeviceTables, MfSgd, SocialHSgd, SocialSgd, SvdppSgd
    from qrec_amd.social import synthetic_graph_steps
    import bench_social as B
    U, I, n = wl["U"], wl["I"], wl["u"].size
    u, i, r = wl["u"], wl["i"], wl["r"]
    lr, gm = 0.005, data.globalMean
    P0, Q0 = rng.random((U, D)) / 3, rng.random((I, D)) / 3
    Bu0, Bi0 = rng.random(U) / 10, rng.random(I) / 10
    if model in ("BasicMF", "PMF", "SVD", "EE"):
        t = DeviceTables(P0, Q0, np.float64)
        variant = {"BasicMF": capi.MF_BASIC, "PMF": capi.MF_PMF, "SVD": capi.MF_SVD, "EE": capi.MF_EE}[model]
        s = MfSgd(t, n, variant, Bu0, Bi0)
        epoch = lambda: s.epoch(u, i, r, lr, 0.01, 0.01, 0.01, gm)
        if model in ("SVD", "EE"):
            return t, epoch, ("BIASED" if model == "SVD" else "EUCLID", dict(Bu=s.d_Bu, Bi=s.d_Bi)), lambda: dict(zip(("Bu", "Bi"), s.biases()))
        return t, epoch, ("DOT", {}), dict
    if model == "SVDPlusPlus":
        t = DeviceTables(P0, Q0, np.float64)
        rated = data.rated_csr()
        s = SvdppSgd(t, rng.random((I, D)) / 3, Bu0, Bi0, rated, n)
        epoch = (lambda: s.epoch(u, i, r, lr, 0.01, 0.01, 0.01, 0.01, gm)) if n < 100_000 else None
        host = lambda: dict(zip(("Y", "Bu", "Bi"), s.download()))
        return t, epoch, ("SVDPP", dict(Bu=s.d_Bu, Bi=s.d_Bi, Y=s.d_Y, rated=(s.d_indptr, s.d_items, rated.indptr))), host
    if model in ("LOCABAL", "SocialFD"):
        x = B.h_inputs(model, wl, D)
        t = DeviceTables(x["P"], x["Q"], np.float64)
        steps = synthetic_graph_steps(model, U, wl["a"], wl["b"], wl["w"])
        if model == "LOCABAL":
            s = SocialHSgd(t, n, model, steps[0], x["H"], W=steps[1])
        else:
            s = SocialHSgd(t, n, model, steps, x["H"], Bu=x["Bu"], Bi=x["Bi"])

        def epoch():
            s.rating_pass(u, i, x["r"], 0.001, 0.01, 0.01, 0.1, 0.3, 0.5)
            s.social_pass(0.001, alpha=0.4, regS=0.01, eta=0.1, beta=0.1)
        if model == "LOCABAL":
            return t, epoch, ("DOT", {}), dict
        return t, epoch, ("METRIC", dict(Bu=s.d_Bu, Bi=s.d_Bi, H=s.d_H)), lambda: dict(zip(("Bu", "Bi"), s.biases()), H=s.H())
    t = DeviceTables(P0, Q0, np.float64)
    steps = synthetic_graph_steps(model, U, wl["a"], wl["b"], wl["w"])
    s = SocialSgd(t, n, model, steps, Z=rng.random((U, D)) / 10, Bu=Bu0, Bi=Bi0)

    def epoch():
        s.rating_pass(u, i, r, lr, 0.01, 0.01, 0.01, gm, alpha=0.5)
        if model != "RSTE":
            s.social_pass(lr, 0.1, 0.1)
    if model == "RSTE":
        ptr, ids, w, _ = steps
        fol = [{data.unames[f]: x for f, x in zip(ids[ptr[k]:ptr[k + 1]].tolist(), w[ptr[k]:ptr[k + 1]].tolist())} for k in range(U)]
        social = SimpleNamespace(getFollowees=lambda name: fol[data.user[name]] if name in data.user else {})
        return t, epoch, ("RSTE", dict(followees=(s.d_fe_ptr, s.d_fe_ids, s.d_fe_w, s.d_den), alpha=0.5)), lambda: dict(social=social, alpha=0.5)
    if model == "SREE":
        return t, epoch, ("EUCLID", dict(Bu=s.mf.d_Bu, Bi=s.mf.d_Bi)), lambda: dict(zip(("Bu", "Bi"), s.biases()))
    return t, epoch, ("DOT", {}), dict


def median_wall_ms(f, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out)), [round(x, 3) for x in out]


def bench(model, name, wl, data, um, im):
    import importlib

    from qrec_amd import capi
    from qrec_amd.engine import RatingEvaluator
    rng = np.random.default_rng(MODELS.index(model))
    t, epoch, (form, buffers), host_attrs = build(model, wl, data, rng)
    row = dict(model=model, form=form, n_test_pairs=int(wl["tu"].size))
    if epoch is None:
        row["epoch_ms"] = None
        row["epoch_note"] = "unmeasured: SVD++'s epoch at this shape was not run"
    else:
        epoch()                                                  # warm-up: code objects, first touch
        row["epoch_ms"], row["epoch_ms_all"] = median_wall_ms(epoch, EPOCHS)
        row["epoch_ms"] = round(row["epoch_ms"], 3)
    ev = RatingEvaluator(form, t, wl["tu"], wl["ti"], wl["tr"], data.rScale, um, im, data.globalMean, **buffers)
    for _ in range(WARMUP):
        dev = ev.measure()
    times, a, b = [], capi.Event(), capi.Event()
    for _ in range(CALLS):
        a.record(); dev = ev.measure(); b.record(); b.sync()
        times.append(b.elapsed_ms_since(a))
    row["device_eval_ms"] = round(float(np.median(times)), 4)
    row["device_eval_ms_min_max"] = [round(min(times), 4), round(max(times), 4)]
    # the host loop of the class itself, on the tables as the class downloads them after an epoch
    cls = getattr(importlib.import_module(f"qrec_amd.model.rating.{model}"), model)
    m = cls.__new__(cls)
    m.data = data
    m.P, m.Q = t.download(np.float64)
    for k, v in host_attrs().items():
        setattr(m, k, v)
    host_ms, host_all = median_wall_ms(m.rating_performance_host, 3 if name == "filmtrust" else 1)
    row["host_loop_ms"], row["host_loop_ms_all"] = round(host_ms, 2), host_all
    row["host_us_per_pair"] = round(1e3 * host_ms / max(wl["tu"].size, 1), 3)
    row["host_over_device"] = round(host_ms / row["device_eval_ms"], 1)
    row["mae_equal"] = bool(dev[0] == m.measure[0])
    row["measure_device"], row["measure_host"] = [x.strip() for x in dev], [x.strip() for x in m.measure]
    return row


def main():
    args = sys.argv[1:]
    which = None
    if args and args[0] == "--shape":
        which, args = args[1], args[2:]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "rating_eval_bench.json")
    from qrec_amd import capi
    capi.init(0)
    res = dict(device=capi.device_info()["arch"], d=D, device_calls_timed=CALLS, warmup_calls=WARMUP, epochs_timed=EPOCHS, workloads={})
    if which and os.path.exists(out_path):
        res["workloads"] = json.load(open(out_path)).get("workloads", {})
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    for name, wl in workloads(which).items():
        rng = np.random.default_rng(3)
        um, im = rng.random(wl["U"]) * 3 + 1, rng.random(wl["I"]) * 3 + 1
        scale = (float(wl["r"].min()), float(wl["r"].max()))
        data = HostData(wl, um, im, float(um.mean()), scale)
        rows = []
        res["workloads"][name] = dict(n_users=wl["U"], n_items=wl["I"], n_ratings=int(wl["u"].size), n_relations=int(wl["a"].size),
                                      n_test_pairs=int(wl["tu"].size), models=rows)
        for model in MODELS:
            rows.append(bench(model, name, wl, data, um, im))
            print(name, json.dumps(rows[-1]), flush=True)
            with open(out_path, "w") as f:                       # after every model: a run that is cut short leaves its rows
                json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
