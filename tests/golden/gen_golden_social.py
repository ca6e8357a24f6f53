#!/usr/bin/env python3
"""Golden runs of the reference's social-trust rating models (model/rating/{SoRec,SoReg,SocialMF,RSTE,SREE}.py), recorded by
running the UNMODIFIED reference in-process.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_social.py

Same set-up as gen_golden.py (stubs for numba / mkl / tensorflow -- SocialMF.py imports tensorflow at the top but its numpy
trainModel never touches it --, a scratch cwd with a ``dataset`` link, seeded RNGs, PYTHONHASHSEED=0 for a child run when
the caller did not set it).  Every case: FilmTrust trainset.txt / testset.txt / trust.txt, d = 10, 3 epochs, the stock
conf's regularisers (learning rates: see CASES); SREE with its stock ``item.ranking=on -topN 10``.  Writes, next to this file:
  social_<model>_filmtrust.npz   the training rows in their initial order, the trained tables after the last epoch (P, Q and
                                 Z or Bu, Bi), the raw relation file as codes (a training user's id, or -1 - k for the k-th
                                 unknown name), the pruned relation list as id pairs, the test rows (user and item codes, as the relation's) with their
                                 predictions
                                 and the Python ``random`` state at the end; SoReg also every edge's Sim in walk order
  golden_social_meta.json        per case: conf, seed, every epoch's loss and learning rate, sha256 of every epoch's training
                                 order and of the initial tables (both regenerable from the seed), measure strings
The initial tables and the later epochs' orders are not stored: np.random.seed(seed) then rand(U, d)/3, rand(I, d)/3 (and
Z = rand(U, d)/10 or Bu, Bi = rand(U)/10, rand(I)/10) gives the former, random.seed(seed) then one random.shuffle of the row
list per epoch the latter.  Running it twice gives byte-identical files.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, install_stubs, run_numpy_model, write_conf  # noqa: E402
from gen_golden_wrmf import save_npz  # noqa: E402

FT = dict(ratings="./dataset/FilmTrust/trainset.txt", social="./dataset/FilmTrust/trust.txt", ratings__setup="-columns 0 1 2",
          social__setup="-columns 0 1 2", evaluation__setup="-testSet ./dataset/FilmTrust/testset.txt", num__factors="10",
          num__max__epoch="3", output__setup="off -dir ./results/")
# model -> (seed, item.ranking, learnRate, reg.lambda, own key): the stock config/<model>.conf values, except that the learning
# rate is capped at 0.02 (PMF's fixture rate): SoRec's stock 0.1 and SoReg's 0.05 overflow within the first epoch at d = 10
CASES = {
    "SoRec": (11, "off -topN 10", "-init 0.02 -max 1", "-u 0.05 -i 0.05 -b 0.1 -s 0.1", {"SoRec": "-z 0.1"}),
    "SoReg": (12, "off -topN 10", "-init 0.02 -max 1", "-u 0.02 -i 0.02 -b 0.1 -s 0.02", {"SoReg": "-alpha 0.1"}),
    "SocialMF": (13, "off -topN 30", "-init 0.02 -max 1", "-u 0.05 -i 0.05 -b 0.1 -s 0.1", {}),
    "RSTE": (14, "off -topN 10", "-init 0.01 -max 1", "-u 0.001 -i 0.001 -b 0.1 -s 0.1", {"RSTE": "-alpha 0.6"}),
    "SREE": (15, "on -topN 10", "-init 0.01 -max 1", "-u 0.01 -i 0.01 -b 0.01 -s 0.1", {"SREE": "-alpha 0.5"}),
}


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(model, tmp):
    seed, ranking, lr, reg, own = CASES[model]
    conf = os.path.join(tmp, model + ".conf")
    write_conf(conf, model__name=model, item__ranking=ranking, learnRate=lr, reg__lambda=reg, **FT, **own)
    rec = run_numpy_model(conf, seed, "model.rating." + model, model, "mf", social=True)
    m = rec["model"]
    user = m.data.user
    unknown = {}
    code = lambda name: user[name] if name in user else -1 - unknown.setdefault(name, len(unknown))
    unknown_items = {}
    icode = lambda name: m.data.item[name] if name in m.data.item else -1 - unknown_items.setdefault(name, len(unknown_items))
    raw = rec["raw_relation"]
    order0 = rec["order0"]
    z = dict(order0_u=np.array([a for a, _, _ in order0], dtype=np.int16), order0_i=np.array([b for _, b, _ in order0], dtype=np.int16),
             order0_r=np.array([c for _, _, c in order0], dtype=np.float64),
             P=m.P, Q=m.Q,
             raw_follower=np.array([code(r[0]) for r in raw], dtype=np.int32), raw_followee=np.array([code(r[1]) for r in raw], dtype=np.int32),
             raw_weight=np.array([r[2] for r in raw], dtype=np.float64),
             rel_u=np.array([user[r[0]] for r in m.social.relation], dtype=np.int32),
             rel_v=np.array([user[r[1]] for r in m.social.relation], dtype=np.int32),
             test_uid=np.array([code(r[0]) for r in m.data.testData], dtype=np.int32),
             test_iid=np.array([icode(r[1]) for r in m.data.testData], dtype=np.int32),
             test_rating=np.array([r[2] for r in m.data.testData], dtype=np.float64),
             py_state=np.array(rec["py_state"][1], dtype=np.uint32))
    if ranking.startswith("off"):
        z["test_pred"] = np.array([r[3] for r in m.data.testData], dtype=np.float64)
    if model == "SoRec":
        z["Z"] = m.Z
    if model == "SREE":
        z["Bu"] = m.Bu; z["Bi"] = m.Bi
    if model == "SoReg":
        fe, fr = [], []
        for name in m.social.user:                 # the walk of SoReg.py:58-71
            if name in user:
                fe += [m.Sim[name][f] for f in m.social.getFollowees(name) if f in user]
                fr += [m.Sim[name][g] for g in m.social.getFollowers(name) if g in user]
        z["sim_followee"] = np.array(fe, dtype=np.float64); z["sim_follower"] = np.array(fr, dtype=np.float64)
    save_npz(os.path.join(OUT, f"social_{model.lower()}_filmtrust.npz"), z)
    tabs = {"P0": rec["P0"], "Q0": rec["Q0"]}
    if "Bu0" in rec:
        tabs.update(Bu0=rec["Bu0"], Bi0=rec["Bi0"])
    return dict(seed=seed, conf=open(conf).read(), n_users=len(user), n_items=len(m.data.item), n_train=len(order0),
                relations_loaded=len(raw), relations_kept=len(m.social.relation), globalMean=m.data.globalMean,
                epochs=[dict(epoch=e["epoch"], loss=e["loss"], lr_used=e["lr_used"], lr_next=e["lr_next"], converged=e["converged"],
                             order_sha256=sha(np.array([(a, b) for a, b, _ in e["order"]], dtype=np.int32))) for e in rec["epochs"]],
                init_sha256={k: sha(v) for k, v in tabs.items()}, measure=rec["measure"])


def main():
    if os.environ.get("PYTHONHASHSEED") != "0":        # set-iteration order in the reference's data model: one fixed hash seed
        env = dict(os.environ, PYTHONHASHSEED="0", PYTHONDONTWRITEBYTECODE="1")
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    install_stubs()
    tmp = tempfile.mkdtemp(prefix="qrec_golden_social_")
    os.symlink(os.path.join(REF, "dataset"), os.path.join(tmp, "dataset"))
    os.chdir(tmp)
    metas = {}
    for model in CASES:
        metas[model] = record(model, tmp)
        print(model, "done", metas[model]["epochs"][-1]["loss"], flush=True)
    with open(os.path.join(OUT, "golden_social_meta.json"), "w") as f:
        json.dump(metas, f, indent=1, sort_keys=True)
    print("ok")


if __name__ == "__main__":
    main()
