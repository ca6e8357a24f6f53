#!/usr/bin/env python3
"""Golden RANKING runs of the reference's six rating models whose ranking score is not one plain inner product
(model/rating/{SVD,SVDPlusPlus,EE,SREE,RSTE,SocialFD}.py), recorded by running the UNMODIFIED reference in-process.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_rating_rank.py

Same set-up as gen_golden.py (stubs for numba / mkl / tensorflow, a scratch cwd with a ``dataset`` link, seeded RNGs,
PYTHONHASHSEED=0 for a child run when the caller did not set it).  Every case: FilmTrust trainset.txt / testset.txt (and
trust.txt for the three social classes), ``item.ranking=on -topN 10,20``, ``num.factors=8``, 3 epochs, the learning rates and
regularisers of the classes' rating fixtures.  Writes, next to this file:
  rating_rank_<model>_filmtrust.npz   the training rows in their initial order, the test rows as codes (a training id, or
                                      -1 - k for the k-th unknown name), the raw relation file as codes (social classes), the
                                      trained tables after the last epoch (P, Q and Bu, Bi, Y, H where the class has them),
                                      the rated CSR in userRated order, RSTE's followee CSR in the order its predictForRanking
                                      walks it, and what evalRanking built: rec_users (testSet_u order, -1 = unknown to the
                                      training set), rec_ids / rec_scores [users, 20]
  golden_rating_rank_meta.json        per case: conf, seed, sizes, globalMean, alpha, every epoch's loss, the measure strings and
                                      ``ranking_path_unmodified`` (whether the class's predictForRanking / evalRanking ran as
                                      written)
Running it twice gives byte-identical files.
"""
import json
import os
import subprocess
import sys
import tempfile
import traceback

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, install_stubs, run_numpy_model, write_conf  # noqa: E402
from gen_golden_wrmf import save_npz  # noqa: E402

BASE = dict(ratings="./dataset/FilmTrust/trainset.txt", ratings__setup="-columns 0 1 2",
            evaluation__setup="-testSet ./dataset/FilmTrust/testset.txt", item__ranking="on -topN 10,20", num__factors="8",
            num__max__epoch="3", output__setup="off -dir ./results/")
SOCIAL = dict(social="./dataset/FilmTrust/trust.txt", social__setup="-columns 0 1 2")
# model -> (seed, social?, learnRate, reg.lambda, own option line)
CASES = {
    "SVD": (31, False, "-init 0.005 -max 1", "-u 0.01 -i 0.02 -b 0.02 -s 0.1", {}),
    "SVDPlusPlus": (32, False, "-init 0.02 -max 1", "-u 0.01 -i 0.01 -b 0.1 -s 0.1", {"SVDPlusPlus": "-y 0.01"}),
    "EE": (33, False, "-init 0.005 -max 1", "-u 0.005 -i 0.005 -b 0.005 -s 0.1", {}),
    "SREE": (34, True, "-init 0.01 -max 1", "-u 0.01 -i 0.01 -b 0.01 -s 0.1", {"SREE": "-alpha 0.5"}),
    "RSTE": (35, True, "-init 0.01 -max 1", "-u 0.001 -i 0.001 -b 0.1 -s 0.1", {"RSTE": "-alpha 0.6"}),
    "SocialFD": (36, True, "-init 0.01 -max 1", "-u 0.005 -i 0.005 -b 0.01 -s 0.1", {"SocialFD": "-alpha 0.3 -eta 0.1 -beta 0.1"}),
}


def record(model, tmp):
    seed, social, lr, reg, own = CASES[model]
    conf = os.path.join(tmp, model + ".conf")
    write_conf(conf, model__name=model, learnRate=lr, reg__lambda=reg, **BASE, **(SOCIAL if social else {}), **own)
    try:
        rec = run_numpy_model(conf, seed, "model.rating." + model, model, "mf", social=social)
    except Exception as e:                       # the class cannot run its ranking path as written: say so, record nothing else
        tb = traceback.extract_tb(e.__traceback__)[-1]
        return dict(seed=seed, conf=open(conf).read(), ranking_path_unmodified=False,
                    raised=dict(type=type(e).__name__, message=str(e), file=os.path.relpath(tb.filename, REF), line=tb.lineno))
    m = rec["model"]
    user, item = m.data.user, m.data.item
    unknown_u, unknown_i = {}, {}
    ucode = lambda name: user[name] if name in user else -1 - unknown_u.setdefault(name, len(unknown_u))
    icode = lambda name: item[name] if name in item else -1 - unknown_i.setdefault(name, len(unknown_i))
    order0 = rec["order0"]
    z = dict(train_u=np.array([a for a, _, _ in order0], dtype=np.int16), train_i=np.array([b for _, b, _ in order0], dtype=np.int16),
             train_r=np.array([c for _, _, c in order0], dtype=np.float64),
             test_uid=np.array([ucode(r[0]) for r in m.data.testData], dtype=np.int32),
             test_iid=np.array([icode(r[1]) for r in m.data.testData], dtype=np.int32),
             test_rating=np.array([r[2] for r in m.data.testData], dtype=np.float64), P=m.P, Q=m.Q)
    for name in ("Bu", "Bi", "Y", "H"):
        if hasattr(m, name):
            z[name] = np.asarray(getattr(m, name), dtype=np.float64)
    ptr, items = [0], []
    for name in user:                            # id order; userRated order inside a row
        items += [item[j] for j in m.data.userRated(name)[0]]
        ptr.append(len(items))
    z["rated_indptr"] = np.array(ptr, dtype=np.int64); z["rated_items"] = np.array(items, dtype=np.int16)
    if social:
        raw = rec["raw_relation"]
        z["raw_follower"] = np.array([ucode(r[0]) for r in raw], dtype=np.int32)
        z["raw_followee"] = np.array([ucode(r[1]) for r in raw], dtype=np.int32)
        z["raw_weight"] = np.array([r[2] for r in raw], dtype=np.float64)
    if model == "RSTE":
        ptr, ids, w = [0], [], []
        for name in user:                        # the walk of RSTE.py:70-76
            fol = m.social.getFollowees(name)
            for f in fol:
                if m.data.containsUser(f):
                    ids.append(user[f]); w.append(fol[f])
            ptr.append(len(ids))
        z["fe_indptr"] = np.array(ptr, dtype=np.int64); z["fe_ids"] = np.array(ids, dtype=np.int32); z["fe_w"] = np.array(w, dtype=np.float64)
    rl = rec["holder"]["recList"]
    users = list(rl.keys())
    assert users == list(m.data.testSet_u.keys())
    N = max(len(v) for v in rl.values())
    ids = np.full((len(users), N), -1, dtype=np.int32); sc = np.zeros((len(users), N))
    for a, un in enumerate(users):
        for b, (iname, s) in enumerate(rl[un]):
            ids[a, b] = item[iname]; sc[a, b] = s
    z["rec_users"] = np.array([user.get(un, -1) for un in users], dtype=np.int32)
    z["rec_ids"] = ids; z["rec_scores"] = sc
    for k in ("P", "Q", "rec_scores"):
        assert np.isfinite(z[k]).all(), (model, k)
    path = os.path.join(OUT, f"rating_rank_{model.lower()}_filmtrust.npz")
    save_npz(path, z)
    assert os.path.getsize(path) < (1 << 20), (model, os.path.getsize(path))
    return dict(seed=seed, conf=open(conf).read(), ranking_path_unmodified=True, n_users=len(user), n_items=len(item), n_train=len(order0),
                n_test_users=len(users), globalMean=m.data.globalMean, alpha=float(getattr(m, "alpha", 0.0)), topN=m.ranking["-topN"],
                epochs=[dict(epoch=e["epoch"], loss=e["loss"], lr_used=e["lr_used"]) for e in rec["epochs"]], measure=rec["measure"])


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":        # set-iteration order in the reference's data model: one fixed hash seed
        env = dict(os.environ, PYTHONHASHSEED="0", PYTHONDONTWRITEBYTECODE="1")
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    install_stubs()
    tmp = tempfile.mkdtemp(prefix="qrec_golden_rating_rank_")
    os.symlink(os.path.join(REF, "dataset"), os.path.join(tmp, "dataset"))
    os.chdir(tmp)
    only = sys.argv[1:]
    meta_path = os.path.join(OUT, "golden_rating_rank_meta.json")
    metas = json.load(open(meta_path)) if only and os.path.exists(meta_path) else {}
    for model in CASES:
        if only and model not in only:
            continue
        metas[model] = record(model, tmp)
        print(model, "done", metas[model].get("measure", metas[model].get("raised")), flush=True)
    with open(meta_path, "w") as f:
        json.dump(metas, f, indent=1, sort_keys=True)
    print("ok")


if __name__ == "__main__":
    main()
