#!/usr/bin/env python3
"""Golden runs of the reference's two rating models that carry a dense d x d matrix (model/rating/{LOCABAL,SocialFD}.py),
recorded by running the UNMODIFIED reference in-process.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_locabal_fd.py

Same set-up as gen_golden_social.py (stubs for numba / mkl / tensorflow, a scratch cwd with a ``dataset`` link, seeded RNGs,
PYTHONHASHSEED=0 for a child run when the caller did not set it); LOCABAL's nx.pagerank is the real networkx.  Both cases:
FilmTrust trainset.txt / testset.txt / trust.txt through -testSet (the stock LOCABAL.conf draws a split with -ap 0.2; the
fixture does not), d = 10, 3 epochs, item.ranking=off -topN 10, the stock conf's reg.lambda and own option line (learning
rates: see CASES).  Writes, next to this file:
  social_<model>_filmtrust.npz   everything the other social fixtures hold (the training rows in their initial order, the
                                 trained P, Q, the raw relation file as codes, the pruned relation list as id pairs, the test
                                 rows with their predictions, the Python ``random`` state at the end) and H0, H (the d x d
                                 matrix before and after); SocialFD: Bu, Bi; LOCABAL: ``pr_user`` / ``pr_rank`` / ``pr_w``
                                 (every user of the pruned relation list in graph insertion order, its 1-based PageRank rank
                                 and W = 1/(1 + log(rank))) and ``s_u`` / ``s_k`` / ``s_sim`` (the similarity dict in its walk
                                 order: the outer dict's insertion order, then the inner dict's; a repeated pair keeps its
                                 first position and its last value, which is what a dict does)
  golden_locabal_fd_meta.json    per case: conf, seed, every epoch's loss and learning rate, sha256 of every epoch's training
                                 order and of the initial tables, measure strings
Running it twice gives byte-identical files.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, install_stubs, run_numpy_model, write_conf  # noqa: E402
from gen_golden_social import FT, sha  # noqa: E402
from gen_golden_wrmf import save_npz  # noqa: E402

# model -> (seed, learnRate, reg.lambda, own key): the stock config/<model>.conf values.  Both stock learning rates (0.03 and
# 0.01) keep every table finite over the three epochs at d = 10 (asserted below), so neither is capped.
CASES = {
    "LOCABAL": (16, "-init 0.03 -max 1", "-u 0.01 -i 0.01 -s 0.01 -b 0.01", {"LOCABAL": "-alpha 0.4"}),
    "SocialFD": (17, "-init 0.01 -max 1", "-u 0.005 -i 0.005 -b 0.01 -s 0.1", {"SocialFD": "-alpha 0.3 -eta 0.1 -beta 0.1"}),
}


def record(model, tmp):
    import importlib
    seed, lr, reg, own = CASES[model]
    conf = os.path.join(tmp, model + ".conf")
    write_conf(conf, model__name=model, item__ranking="off -topN 10", learnRate=lr, reg__lambda=reg, **FT, **own)
    cls = getattr(importlib.import_module("model.rating." + model), model)
    plain_init, seen = cls.initModel, {}

    def initModel(self):                       # H as initModel leaves it; run_numpy_model wraps this one in turn
        plain_init(self); seen["H0"] = self.H.copy()
    cls.initModel = initModel
    try:
        rec = run_numpy_model(conf, seed, "model.rating." + model, model, "mf", social=True)
    finally:
        cls.initModel = plain_init
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
             P=m.P, Q=m.Q, H0=seen["H0"], H=m.H,
             raw_follower=np.array([code(r[0]) for r in raw], dtype=np.int32), raw_followee=np.array([code(r[1]) for r in raw], dtype=np.int32),
             raw_weight=np.array([r[2] for r in raw], dtype=np.float64),
             rel_u=np.array([user[r[0]] for r in m.social.relation], dtype=np.int32),
             rel_v=np.array([user[r[1]] for r in m.social.relation], dtype=np.int32),
             test_uid=np.array([code(r[0]) for r in m.data.testData], dtype=np.int32),
             test_iid=np.array([icode(r[1]) for r in m.data.testData], dtype=np.int32),
             test_rating=np.array([r[2] for r in m.data.testData], dtype=np.float64),
             test_pred=np.array([r[3] for r in m.data.testData], dtype=np.float64),
             py_state=np.array(rec["py_state"][1], dtype=np.uint32))
    for k in ("P", "Q", "H"):
        assert np.isfinite(z[k]).all(), (model, k)
    if model == "SocialFD":
        z["Bu"] = m.Bu; z["Bi"] = m.Bi
    else:
        rank = {name: k + 1 for k, name in enumerate(m.W)}          # LOCABAL.py:30-34 fills W in rank order
        nodes = []
        for a, b, _ in m.social.relation:                            # DiGraph insertion order: LOCABAL.py:27-28
            for name in (a, b):
                if name not in nodes:
                    nodes.append(name)
        assert set(nodes) == set(m.W)
        z["pr_user"] = np.array([user[n] for n in nodes], dtype=np.int32)
        z["pr_rank"] = np.array([rank[n] for n in nodes], dtype=np.int32)
        z["pr_w"] = np.array([m.W[n] for n in nodes], dtype=np.float64)
        walk = [(user[a], user[b], m.S[a][b]) for a in m.S for b in m.S[a]]      # LOCABAL.py:68-69
        z["s_u"] = np.array([a for a, _, _ in walk], dtype=np.int32)
        z["s_k"] = np.array([b for _, b, _ in walk], dtype=np.int32)
        z["s_sim"] = np.array([s for _, _, s in walk], dtype=np.float64)
    save_npz(os.path.join(OUT, f"social_{model.lower()}_filmtrust.npz"), z)
    tabs = {"P0": rec["P0"], "Q0": rec["Q0"], "H0": seen["H0"]}
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
    tmp = tempfile.mkdtemp(prefix="qrec_golden_locabal_fd_")
    os.symlink(os.path.join(REF, "dataset"), os.path.join(tmp, "dataset"))
    os.chdir(tmp)
    metas = {}
    for model in CASES:
        metas[model] = record(model, tmp)
        print(model, "done", metas[model]["epochs"][-1]["loss"], flush=True)
    with open(os.path.join(OUT, "golden_locabal_fd_meta.json"), "w") as f:
        json.dump(metas, f, indent=1, sort_keys=True)
    print("ok")


if __name__ == "__main__":
    main()
