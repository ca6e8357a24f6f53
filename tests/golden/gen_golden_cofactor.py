#!/usr/bin/env python3
"""Golden vectors of the reference's CoFactor (model/ranking/CoFactor.py), recorded by running the UNMODIFIED reference
in-process.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cofactor.py [case ...]

Same set-up as gen_golden_wrmf.py.  Nothing in the model's arithmetic is touched: ``initModel`` and
``Measure.rankingMeasure`` are wrapped only to copy what they see, and -- the model has no per-epoch hook -- a ``print``
is put into the reference module's globals that copies the tables when it is called as ``print('epoch:', epoch, 'loss:',
loss)`` and then prints.  Writes, next to this file:
  cofactor_filmtrust.npz    FilmTrust (-testSet, -b 1), 20 factors, 3 epochs, CoFactor=-k 5 -gamma 0.01 -filter 2
  cofactor_filmtrust_b.npz  FilmTrust, 10 factors, 2 epochs, CoFactor=-k 2 -gamma 0.05 -filter 5, reg.lambda -u 0.5
  cofactor_lastfm.npz       the stock CoFactor.conf (lastfm, -ap 0.2 -b 1, 7 epochs), epochs 1 and 7 kept
  golden_cofactor_meta.json confs, seeds, losses, measure strings, sizes, sha256 of the whole tables
Per case: the train / test rows; in ``<case>_sppmi.npz`` the SPPMI as a CSR by item id whose rows hold the neighbours in the
dict's insertion order (``sppmi_ptr``, ``sppmi_idx``) and the values of the entries with neighbour > item in that traversal
(``sppmi_val_upper``: (a, b) and (b, a) hold the same bits, asserted here); per kept epoch every ``row_stride``-th row of X and Y,
of G every ``row_stride``-th of the rows of the items with contexts, and w, c at those items -- everywhere else G, w, c stay
trainModel's seeded draws, and the sha256 of every whole table is in the meta file, so all of w and c is pinned; the Python
``random`` state; the recommendation lists; per test user the gap between the reference's N-th and (N + 1)-th
candidate score (``rec_gap``: a list whose gap is positive but below the tables' parity bound is not comparable; at most 1 % of a
case's test users may be such, asserted here.  An exact tie, gap 0, is decided by the selection rule and stays comparable).
Running it twice gives byte-identical files.
"""
import builtins
import io
import json
import os
import random
import sys
import tempfile
from contextlib import redirect_stdout

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, install_stubs, sha, write_conf  # noqa: E402
from gen_golden_wrmf import save_npz  # noqa: E402

TABLES = ("X", "Y", "G", "w", "c")
MAX_UNSEPARATED = 0.01          # share of the test users whose reference lists may be left out of the comparison
SEPARATION = 1e-9               # ... a gap below this share of the largest |Y| entry (the tables' parity bound)


def run_cofactor(conf_path, seed):
    from QRec import QRec
    from util.config import ModelConf
    import model.ranking.CoFactor as mod
    import base.recommender as br
    CoFactor = mod.CoFactor
    rec = {"epochs": []}
    orig_init, orig_rm = CoFactor.initModel, br.Measure.rankingMeasure

    def initModel(self):
        orig_init(self)
        rec["X0"], rec["Y0"] = self.P * 10, self.Q * 10
        rec["SPPMI"] = {a: dict(row) for a, row in self.SPPMI.items()}

    def spy(*args, **kw):
        if len(args) == 4 and args[0] == "epoch:" and args[2] == "loss:":
            m = rec["live"]
            rec["epochs"].append(dict(epoch=int(args[1]), loss=float(args[3]), **{t: getattr(m, t).copy() for t in TABLES}))
        builtins.print(*args, **kw)

    def rankingMeasure(origin, res, N):
        rec["recList"] = res
        return orig_rm(origin, res, N)

    CoFactor.initModel = initModel
    mod.print = spy
    br.Measure.rankingMeasure = staticmethod(rankingMeasure)
    random.seed(seed); np.random.seed(seed)
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            q = QRec(ModelConf(conf_path))
            m = CoFactor(q.config, q.trainingData, q.testData)
            rec["live"] = m
            rec["measure"] = m.execute()
    finally:
        CoFactor.initModel = orig_init
        del mod.print
        br.Measure.rankingMeasure = staticmethod(orig_rm)
    rec.update(model=m, py_state=random.getstate(), train_rows=q.trainingData, test_rows=q.testData,
               printed=[ln for ln in buf.getvalue().splitlines() if ln.startswith("epoch:")])
    return rec


def score_gaps(m, users, N):
    """per test user: the gap between the N-th and the (N + 1)-th largest candidate of base/recommender.py:143-150 (rated items
    set to 0), from the trained tables"""
    gaps = np.zeros(len(users), dtype=np.float64)
    for a, un in enumerate(users):
        cand = np.array(m.predictForRanking(un), dtype=np.float64)
        for item in m.data.userRated(un)[0]:
            cand[m.data.item[item]] = 0
        top = np.sort(cand)[::-1][:N + 1]
        gaps[a] = top[N - 1] - top[N]
    return gaps


def pack(rec, name, keep_epochs, row_stride):
    m = rec["model"]
    I = len(m.data.item)
    arrays = dict(
        train_uid=np.array([m.data.user[r[0]] for r in rec["train_rows"]], dtype=np.int32),
        train_iid=np.array([m.data.item[r[1]] for r in rec["train_rows"]], dtype=np.int32),
        train_r=np.array([r[2] for r in rec["train_rows"]], dtype=np.float64),
        test_uid=np.array([m.data.user.get(r[0], -1) for r in rec["test_rows"]], dtype=np.int32),
        test_iid=np.array([m.data.item.get(r[1], -1) for r in rec["test_rows"]], dtype=np.int32),
        test_uname=np.array([str(r[0]) for r in rec["test_rows"]]), test_iname=np.array([str(r[1]) for r in rec["test_rows"]]),
        py_state=np.array(rec["py_state"][1], dtype=np.uint32),
        loss=np.array([e["loss"] for e in rec["epochs"]], dtype=np.float64))
    rows = [[] for _ in range(I)]
    for a, row in rec["SPPMI"].items():
        rows[m.data.item[a]] = [(m.data.item[b], v) for b, v in row.items()]
    ptr = np.zeros(I + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    idx = np.array([b for r in rows for b, _ in r], dtype=np.int32)
    val = np.array([v for r in rows for _, v in r], dtype=np.float64)
    row_of = np.repeat(np.arange(I, dtype=np.int32), np.diff(ptr))
    upper = idx > row_of                  # the value of (a, b) is that of (b, a), bit for bit: keep it once
    lo, hi = np.minimum(idx, row_of).astype(np.int64), np.maximum(idx, row_of).astype(np.int64)
    key = lo * I + hi
    assert np.array_equal(val[~upper][np.argsort(key[~upper], kind="stable")], val[upper][np.argsort(key[upper], kind="stable")])
    sppmi = dict(sppmi_ptr=ptr, sppmi_idx=idx, sppmi_val_upper=val[upper])
    ctx = np.flatnonzero(np.diff(ptr) > 0)
    kept = keep_epochs or [e["epoch"] for e in rec["epochs"]]
    table_sha = {}
    for e in rec["epochs"]:
        assert all(np.isfinite(e[t]).all() for t in TABLES)
        if e["epoch"] in kept:
            for t in TABLES:
                key = "%s%d" % (t, e["epoch"])
                # G, w, c change only at the items with contexts (ctx): elsewhere they are trainModel's draws to the end
                arrays[key] = e[t][::row_stride].copy() if t in "XY" else e[t][ctx][::row_stride].copy() if t == "G" else e[t][ctx].copy()
                table_sha[key] = sha(e[t])
    rl = rec["recList"]
    users = list(rl.keys())
    N = max(len(v) for v in rl.values())
    ids = np.full((len(users), N), -1, dtype=np.int32)
    for a, un in enumerate(users):
        for b, (iname, _) in enumerate(rl[un]):
            ids[a, b] = m.data.item[iname]
    gaps = score_gaps(m, users, N)
    y_max = float(np.abs(m.Y).max())
    # gap == 0 is a tie of bit-equal scores (items with the same raters and no contexts get the same row of Y; rated items are
    # all 0): the selection rule decides it, not the arithmetic, so those lists stay in the comparison and are only counted
    tied = int((gaps == 0).sum())
    unsep = int(((gaps > 0) & (gaps < SEPARATION * y_max)).sum())
    assert unsep <= MAX_UNSEPARATED * len(users), (name, unsep, len(users))
    arrays.update(rec_users=np.array([m.data.user.get(un, -1) for un in users], dtype=np.int32),
                  rec_user_names=np.array([str(u) for u in users]), rec_ids=ids, rec_gap=gaps)
    deg = np.diff(ptr)
    return arrays, sppmi, dict(name=name, n_users=len(m.data.user), n_items=I, n_train=len(rec["train_rows"]),
                        n_test=len(rec["test_rows"]), emb_size=m.emb_size, regU=m.regU, regR=m.regR, negCount=m.negCount,
                        filter=m.filter, maxEpoch=m.maxEpoch,
                        epochs=[dict(epoch=e["epoch"], loss=e["loss"]) for e in rec["epochs"]], printed=rec["printed"],
                        measure=rec["measure"], X0_sha256=sha(rec["X0"]), Y0_sha256=sha(rec["Y0"]),
                        sppmi_rows=int((deg > 0).sum()), sppmi_entries=int(ptr[-1]), sppmi_longest_row=int(deg.max()),
                        unseparated_lists=unsep, tied_lists=tied, y_max=y_max, kept_epochs=kept, row_stride=row_stride, table_sha256=table_sha)


def _filmtrust(tmp, name, seed, factors, epochs, cofactor, reg, stride):
    conf = os.path.join(tmp, name + ".conf")
    write_conf(conf, ratings="./dataset/FilmTrust/trainset.txt", ratings__setup="-columns 0 1 2", model__name="CoFactor",
               evaluation__setup="-testSet ./dataset/FilmTrust/testset.txt -b 1", item__ranking="on -topN 10,20",
               num__factors=str(factors), num__max__epoch=str(epochs), CoFactor=cofactor, learnRate="-init 0.01 -max 1",
               reg__lambda=reg, output__setup="off -dir ./results/")
    rec = run_cofactor(conf, seed)
    arrays, sppmi, meta = pack(rec, name, None, stride)
    save_npz(os.path.join(OUT, name + ".npz"), arrays)
    save_npz(os.path.join(OUT, name + "_sppmi.npz"), sppmi)
    meta.update(seed=seed, conf=open(conf).read())
    return meta


def case_filmtrust(tmp):
    return _filmtrust(tmp, "cofactor_filmtrust", 1, 20, 3, "-k 5 -gamma 0.01 -filter 2", "-u 1 -i 0.02 -b 0.02", 4)


def case_filmtrust_b(tmp):
    return _filmtrust(tmp, "cofactor_filmtrust_b", 2, 10, 2, "-k 2 -gamma 0.05 -filter 5", "-u 0.5 -i 0.02 -b 0.02", 4)


def case_lastfm(tmp):
    conf = os.path.join(tmp, "cofactor_lfm.conf")
    # config/CoFactor.conf as shipped, output off (nothing else differs)
    text = open(os.path.join(REF, "config", "CoFactor.conf")).read()
    kv = dict(ln.strip().split("=", 1) for ln in text.splitlines() if "=" in ln)
    kv["output.setup"] = "off -dir ./results/"
    with open(conf, "w") as f:
        for k, v in kv.items():
            f.write(f"{k}={v}\n")
    rec = run_cofactor(conf, 7)
    last = rec["epochs"][-1]["epoch"]
    arrays, sppmi, meta = pack(rec, "cofactor_lastfm", [1, last], 16)
    save_npz(os.path.join(OUT, "cofactor_lastfm.npz"), arrays)
    save_npz(os.path.join(OUT, "cofactor_lastfm_sppmi.npz"), sppmi)
    meta.update(seed=7, conf=open(conf).read())
    return meta


CASES = dict(cofactor_filmtrust=case_filmtrust, cofactor_filmtrust_b=case_filmtrust_b, cofactor_lastfm=case_lastfm)


def main():
    install_stubs()
    tmp = tempfile.mkdtemp(prefix="qrec_golden_cofactor_")
    os.symlink(os.path.join(REF, "dataset"), os.path.join(tmp, "dataset"))
    os.chdir(tmp)
    path = os.path.join(OUT, "golden_cofactor_meta.json")
    names = sys.argv[1:] or list(CASES)
    metas = json.load(open(path)) if os.path.exists(path) and sys.argv[1:] else {}
    for n in names:
        m = CASES[n](tmp)
        metas[m["name"]] = m
        print(m["name"], "ok", {k: m[k] for k in ("n_users", "n_items", "n_train", "sppmi_rows", "sppmi_entries", "unseparated_lists")})
    with open(path, "w") as f:
        json.dump(metas, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
