#!/usr/bin/env python3
"""Golden runs of the reference's ExpoMF and SERec (model/ranking/ExpoMF.py, model/ranking/SERec.py), recorded by running the
UNMODIFIED reference in-process.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_expo.py [case ...]

Same set-up as gen_golden.py (stubs for numba / mkl / tensorflow, a scratch cwd with a ``dataset`` link, seeded RNGs).  joblib runs
with its sequential backend (under the module stubs loky's workers cannot unpickle the tasks; the result is the same) and OpenBLAS
with one thread, so the float32 runs regenerate byte-identically.  Only ``initModel`` and ``_update_expo`` are wrapped, to copy
state.  Every case is run twice from the same seed:
  ref32  the unmodified run (float32 tables and prior, sgemm posterior and Gram, fp64 solves);
  ref64  the same run with theta, beta and mu cast to float64 at the end of ``initModel``, nothing else touched.
Writes, next to this file, expo_<case>.npz with, per run: every ``row_stride``-th row of theta and beta after each kept epoch, the
ExpoMF prior mu (every item) or a row x column subsample of SERec's mu, the recommendation lists; and the split rows, the
followee counts t_u (SERec) and the Python ``random`` state.  golden_expo_meta.json holds per case the conf, seed, sizes, the
printed training lines of both runs, the measure strings, sha256 of the initial and every epoch's whole tables, and the measured
distance |ref32 - ref64| (max |diff| / max |ref64|) of theta, beta and mu at every epoch.
Running it twice gives byte-identical files.
"""
import os

os.environ["OPENBLAS_NUM_THREADS"] = "1"          # before numpy: sgemm's summation order must not depend on the host

import io  # noqa: E402
import json  # noqa: E402
import random  # noqa: E402
import sys  # noqa: E402
import tempfile  # noqa: E402
from contextlib import redirect_stdout  # noqa: E402

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, install_stubs, sha, write_conf  # noqa: E402
from gen_golden_wrmf import save_npz  # noqa: E402

META = os.path.join(OUT, "golden_expo_meta.json")


def run(conf_path, seed, model, cast64):
    from joblib import parallel_config
    from QRec import QRec
    from util.config import ModelConf
    import base.recommender as br
    import importlib
    cls = getattr(importlib.import_module("model.ranking." + model), model)
    rec = {"epochs": []}
    orig_init, orig_expo, orig_train, orig_rm = cls.initModel, cls._update_expo, cls.trainModel, br.Measure.rankingMeasure

    def initModel(self):
        orig_init(self)
        rec["theta0"], rec["beta0"] = self.theta.copy(), self.beta.copy()
        rec["mu0_dtype"], rec["mu0_first"] = str(self.mu.dtype), float(self.mu.flat[0])
        if model == "SERec":
            rec["t"] = np.asarray(self.T.sum(axis=1)).ravel().astype(np.float64)
        if cast64:
            self.theta, self.beta, self.mu = (self.theta.astype(np.float64), self.beta.astype(np.float64),
                                              self.mu.astype(np.float64))

    def _update_expo(self, X, n_users):
        orig_expo(self, X, n_users)
        rec["epochs"].append(dict(theta=self.theta.copy(), beta=self.beta.copy(), mu=np.array(self.mu, copy=True)))

    def trainModel(self):
        b = io.StringIO()
        with redirect_stdout(b):
            orig_train(self)
        rec["printed"] = b.getvalue().splitlines()
        print(b.getvalue(), end="")

    def rankingMeasure(origin, res, N):
        rec["recList"] = res
        return orig_rm(origin, res, N)

    cls.initModel, cls._update_expo, cls.trainModel = initModel, _update_expo, trainModel
    br.Measure.rankingMeasure = staticmethod(rankingMeasure)
    random.seed(seed); np.random.seed(seed)
    try:
        with redirect_stdout(io.StringIO()), parallel_config(backend="sequential"):
            q = QRec(ModelConf(conf_path))
            m = cls(q.config, q.trainingData, q.testData, q.relation) if model == "SERec" else cls(q.config, q.trainingData, q.testData)
            rec["measure"] = m.execute()
    finally:
        cls.initModel, cls._update_expo, cls.trainModel = orig_init, orig_expo, orig_train
        br.Measure.rankingMeasure = staticmethod(orig_rm)
    rec.update(model=m, py_state=random.getstate(), train_rows=q.trainingData, test_rows=q.testData)
    return rec


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def rec_ids(rec):
    m, rl = rec["model"], rec["recList"]
    users = list(rl.keys())
    N = max(len(v) for v in rl.values())
    ids = np.full((len(users), N), -1, dtype=np.int32)
    for a, un in enumerate(users):
        for b, (iname, _) in enumerate(rl[un]):
            ids[a, b] = m.data.item[iname]
    return users, ids


def case(tmp, name, model, seed, keep, row_stride, mu_rows=None, mu_cols=None, **conf):
    path = os.path.join(tmp, name + ".conf")
    write_conf(path, model__name=model, **conf)
    r32, r64 = run(path, seed, model, False), run(path, seed, model, True)
    m = r64["model"]
    assert sha(r32["theta0"]) == sha(r64["theta0"]) and r32["py_state"] == r64["py_state"]
    arrays = dict(
        train_uid=np.array([m.data.user[r[0]] for r in r64["train_rows"]], dtype=np.int32),
        train_iid=np.array([m.data.item[r[1]] for r in r64["train_rows"]], dtype=np.int32),
        test_uid=np.array([m.data.user.get(r[0], -1) for r in r64["test_rows"]], dtype=np.int32),
        train_r=np.array([r[2] for r in r64["train_rows"]], dtype=np.float64),
        test_iid=np.array([m.data.item.get(r[1], -1) for r in r64["test_rows"]], dtype=np.int32),
        test_uname=np.array([str(r[0]) for r in r64["test_rows"]]), test_iname=np.array([str(r[1]) for r in r64["test_rows"]]),
        py_state=np.array(r64["py_state"][1], dtype=np.uint32))
    if model == "SERec":
        arrays["t"] = r64["t"]
    n_ep = len(r64["epochs"])
    kept = [k for k in keep if k <= n_ep] if keep else list(range(1, n_ep + 1))
    distance, table_sha = [], {}
    for k in range(1, n_ep + 1):
        e32, e64 = r32["epochs"][k - 1], r64["epochs"][k - 1]
        distance.append({key: dist(e32[key], e64[key]) for key in ("theta", "beta", "mu")})
        for tag, e in (("ref32", e32), ("ref64", e64)):
            for key in ("theta", "beta"):
                table_sha["%s_%s%d" % (tag, key, k)] = sha(e[key])
            if k in kept:
                arrays["%s_theta%d" % (tag, k)] = e["theta"][::row_stride].copy()
                arrays["%s_beta%d" % (tag, k)] = e["beta"][::row_stride].copy()
                mu = e["mu"]
                arrays["%s_mu%d" % (tag, k)] = mu.copy() if mu.ndim == 1 else mu[::mu_rows, ::mu_cols].copy()
    for tag, r in (("ref32", r32), ("ref64", r64)):
        users, ids = rec_ids(r)
        arrays["%s_rec_ids" % tag] = ids
    arrays["rec_users"] = np.array([m.data.user.get(un, -1) for un in users], dtype=np.int32)
    arrays["rec_user_names"] = np.array([str(u) for u in users])
    save_npz(os.path.join(OUT, name + ".npz"), arrays)
    meta = dict(name=name, model=model, seed=seed, conf=open(path).read(), n_users=len(m.data.user), n_items=len(m.data.item),
                n_train=len(r64["train_rows"]), n_test=len(r64["test_rows"]), emb_size=m.emb_size, maxEpoch=m.maxEpoch,
                kept_epochs=kept, row_stride=row_stride, mu_rows=mu_rows, mu_cols=mu_cols, mu0_dtype=r64["mu0_dtype"],
                mu0_first=r64["mu0_first"], theta0_sha256=sha(r64["theta0"]), beta0_sha256=sha(r64["beta0"]),
                table_sha256=table_sha, distance_ref32_ref64=distance,
                printed=dict(ref32=r32["printed"], ref64=r64["printed"]), measure=dict(ref32=r32["measure"], ref64=r64["measure"]))
    return meta


FT = dict(ratings="./dataset/FilmTrust/trainset.txt", ratings__setup="-columns 0 1 2",
          evaluation__setup="-testSet ./dataset/FilmTrust/testset.txt", item__ranking="on -topN 10",
          learnRate="-init 0.01 -max 1", reg__lambda="-u 1 -i 0.02 -b 0.02 -s 0.01", output__setup="off -dir ./results/")
LFM = dict(ratings="./dataset/lastfm/ratings.txt", ratings__setup="-columns 0 1 2", evaluation__setup="-ap 0.2",
           item__ranking="on -topN 10", learnRate="-init 0.01 -max 1", reg__lambda="-u 1 -i 0.02 -b 0.02 -s 0.01",
           output__setup="off -dir ./results/")

CASES = {
    # FilmTrust, the stock settings with 20 factors
    "expo_expomf_filmtrust": lambda tmp: case(tmp, "expo_expomf_filmtrust", "ExpoMF", 1, [1, 4, 8], 8, num__factors="20",
                                              num__max__epoch="8", **FT),
    # config/ExpoMF.conf (lastfm, 50 factors, 15 epochs) with -ap 0.2 and output off
    "expo_expomf_lastfm": lambda tmp: case(tmp, "expo_expomf_lastfm", "ExpoMF", 7, [1, 15], 128, num__factors="50",
                                           num__max__epoch="15", **LFM),
    "expo_serec_filmtrust": lambda tmp: case(tmp, "expo_serec_filmtrust", "SERec", 3, [1, 5], 8, mu_rows=64, mu_cols=4,
                                             social="./dataset/FilmTrust/trust.txt", social__setup="-columns 0 1 2",
                                             num__factors="20", num__max__epoch="5", **dict(FT, evaluation__setup="-ap 0.2")),
    "expo_serec_lastfm": lambda tmp: case(tmp, "expo_serec_lastfm", "SERec", 5, [1, 3], 32, mu_rows=128, mu_cols=32,
                                          social="./dataset/lastfm/trusts.txt", social__setup="-columns 0 1",
                                          num__factors="20", num__max__epoch="3", **LFM),
}


def main():
    names = sys.argv[1:] or list(CASES)
    install_stubs()
    tmp = tempfile.mkdtemp(prefix="qrec_golden_expo_")
    os.symlink(os.path.join(REF, "dataset"), os.path.join(tmp, "dataset"))
    os.chdir(tmp)
    metas = json.load(open(META)) if os.path.exists(META) else {}
    for n in names:
        metas[n] = CASES[n](tmp)
        print(n, "ok", {k: metas[n][k] for k in ("n_users", "n_items", "n_train")}, metas[n]["distance_ref32_ref64"][-1], flush=True)
        with open(META, "w") as f:
            json.dump(metas, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
