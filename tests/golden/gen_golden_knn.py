#!/usr/bin/env python3
"""Golden vectors of the reference's memory-based rating models (model/rating/{UserKNN,ItemKNN,SlopeOne}.py), recorded by
running the UNMODIFIED reference in-process.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_knn.py

Same set-up as gen_golden.py (stubs for numba / mkl / tensorflow, a scratch cwd with a ``dataset`` link, seeded RNGs,
PYTHONHASHSEED=0 is set for a child run when the caller did not set it); nothing in the models' arithmetic is touched:
``predictForRating`` is wrapped only to copy what it returns.  Writes, next to this file:
  knn_filmtrust.npz   the stock FilmTrust train / test split (ids, test ratings) and, per run (UserKNN and ItemKNN with pcc, cos
                      and euclidean, SlopeOne), every query's first 20 neighbours (ids; a test-only user or item is -1 - its
                      index in testSet_u / testSet_i) and their similarities, and every test row's prediction before and after
                      checkRatingBoundary
  knn_lastfm.npz      UserKNN / pcc on the lastfm split that gen_golden_wrmf.py draws (-ap 0.2, seed 7): the split with its test
                      ratings, the neighbours and the predictions
  golden_knn_meta.json  confs, measure strings and the model's printed lines per run
Running it twice gives byte-identical files.
"""
import io
import json
import os
import random
import subprocess
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, install_stubs, write_conf  # noqa: E402
from gen_golden_wrmf import save_npz  # noqa: E402

K = 20
FT = dict(ratings="./dataset/FilmTrust/trainset.txt", ratings__setup="-columns 0 1 2",
          evaluation__setup="-testSet ./dataset/FilmTrust/testset.txt", item__ranking="off -topN -1")
LFM = dict(ratings="./dataset/lastfm/ratings.txt", ratings__setup="-columns 0 1 2", evaluation__setup="-ap 0.2",
           item__ranking="off -topN -1")


def model_lines(text):
    """the printed lines from 'Initializing model' up to the measure block (no paths, no timestamps)"""
    out, on = [], False
    for ln in text.splitlines():
        if ln.startswith("Initializing model"):
            on = True
        elif ln.startswith("The result") or ln.startswith("Evaluating"):
            on = False
        if on:
            out.append(ln)
    return out


def run(conf_path, model, seed):
    from QRec import QRec
    from util.config import ModelConf
    import importlib
    cls = getattr(importlib.import_module("model.rating." + model), model)
    preds = []
    orig = cls.predictForRating

    def predictForRating(self, u, i):
        p = orig(self, u, i)
        preds.append(float(p))
        return p

    cls.predictForRating = predictForRating
    random.seed(seed); np.random.seed(seed)
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            q = QRec(ModelConf(conf_path))
            m = cls(q.config, q.trainingData, q.testData)
            measure = m.execute()
    finally:
        cls.predictForRating = orig
    return dict(model=m, measure=measure, preds=preds, train_rows=q.trainingData, test_rows=q.testData,
                printed=model_lines(buf.getvalue()))


def split_arrays(m, train_rows, test_rows):
    return dict(
        train_uid=np.array([m.data.user[r[0]] for r in train_rows], dtype=np.int32),
        train_iid=np.array([m.data.item[r[1]] for r in train_rows], dtype=np.int32),
        train_r=np.array([r[2] for r in train_rows], dtype=np.float64),
        test_uid=np.array([m.data.user.get(r[0], -1) for r in test_rows], dtype=np.int32),
        test_iid=np.array([m.data.item.get(r[1], -1) for r in test_rows], dtype=np.int32),
        test_uname=np.array([str(r[0]) for r in test_rows]), test_iname=np.array([str(r[1]) for r in test_rows]),
        test_r=np.array([r[2] for r in test_rows], dtype=np.float64))


def neighbours(m, model):
    """(ids [Q, K], sims [Q, K], counts [Q]) of topUsers / topItems in testSet_u / testSet_i order"""
    if model == "UserKNN":
        top, ids, tests = m.topUsers, m.data.user, list(m.data.testSet_u)
    else:
        top, ids, tests = m.topItems, m.data.item, list(m.data.testSet_i)
    tpos = {name: k for k, name in enumerate(tests)}
    I = np.zeros((len(tests), K), dtype=np.int32)
    S = np.zeros((len(tests), K), dtype=np.float64)
    n = np.zeros(len(tests), dtype=np.int32)
    for k, name in enumerate(tests):
        lst = top[name][:K]
        n[k] = len(lst)
        for j, (other, s) in enumerate(lst):
            I[k, j] = ids[other] if other in ids else -1 - tpos[other]
            S[k, j] = float(s)
    return I, S, n


def record(tag, conf, model, seed, arrays, metas, split):
    r = run(conf, model, seed)
    m = r["model"]
    if split:
        arrays.update(split_arrays(m, r["train_rows"], r["test_rows"]))
    if model != "SlopeOne":
        I, S, n = neighbours(m, model)
        arrays.update({tag + "_nb_ids": I, tag + "_nb_sims": S, tag + "_nb_count": n})
    arrays[tag + "_pred"] = np.array(r["preds"], dtype=np.float64)
    arrays[tag + "_pred_bounded"] = np.array([row[3] for row in m.data.testData], dtype=np.float64)
    metas[tag] = dict(model=model, seed=seed, conf=open(conf).read(), measure=r["measure"], printed=r["printed"],
                      n_users=len(m.data.user), n_items=len(m.data.item), n_test=len(m.data.testData),
                      globalMean=m.data.globalMean)


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":        # set-iteration order in the reference's split: one fixed hash seed
        env = dict(os.environ, PYTHONHASHSEED="0", PYTHONDONTWRITEBYTECODE="1")
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    install_stubs()
    tmp = tempfile.mkdtemp(prefix="qrec_golden_knn_")
    os.symlink(os.path.join(REF, "dataset"), os.path.join(tmp, "dataset"))
    os.chdir(tmp)
    metas = {}
    ft = {}
    first = True
    for model, sims in (("UserKNN", ("pcc", "cos", "euclidean")), ("ItemKNN", ("pcc", "cos", "euclidean")), ("SlopeOne", ("cos",))):
        for sim in sims:
            tag = model if model == "SlopeOne" else f"{model}_{sim}"
            conf = os.path.join(tmp, tag + ".conf")
            write_conf(conf, model__name=model, similarity=sim, num__neighbors=str(K), output__setup="off -dir ./results/", **FT)
            record(tag, conf, model, 1, ft, metas, first)
            first = False
            print(tag, "done", flush=True)
    save_npz(os.path.join(OUT, "knn_filmtrust.npz"), ft)
    lfm = {}
    conf = os.path.join(tmp, "UserKNN_lastfm.conf")
    write_conf(conf, model__name="UserKNN", similarity="pcc", num__neighbors=str(K), output__setup="off -dir ./results/", **LFM)
    record("UserKNN_pcc", conf, "UserKNN", 7, lfm, metas.setdefault("lastfm", {}), True)
    save_npz(os.path.join(OUT, "knn_lastfm.npz"), lfm)
    out = {"filmtrust": {k: v for k, v in metas.items() if k != "lastfm"}, "lastfm": metas["lastfm"]}
    with open(os.path.join(OUT, "golden_knn_meta.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("ok")


if __name__ == "__main__":
    main()
