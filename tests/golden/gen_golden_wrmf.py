#!/usr/bin/env python3
"""Golden vectors of the reference's WRMF (model/ranking/WRMF.py), recorded by running the UNMODIFIED reference in-process.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_wrmf.py

Same set-up as gen_golden.py (stubs for numba / mkl / tensorflow, a scratch cwd with a ``dataset`` link, seeded RNGs);
nothing in the model's arithmetic is touched: ``initModel``, ``isConverged`` and ``Measure.rankingMeasure`` are wrapped
only to copy what they see.  Writes, next to this file:
  wrmf_filmtrust.npz   FilmTrust, the stock WRMF.conf's settings (20 factors, reg.lambda -u 1) for 3 epochs: the train /
                       test rows, every 4th row of X and Y after every epoch, the Python ``random`` state, the recommendation lists
  wrmf_lastfm.npz      the stock WRMF.conf (lastfm, -ap 0.2, 7 epochs): the split rows, every 16th row of X and Y after epochs
                       1 and 7, the same state and lists
  golden_wrmf_meta.json  confs, seeds, per-epoch losses, measure strings, sizes, sha256 of the whole tables
The fixtures stay small: X0 / Y0 are np.random.seed(seed); rand(U, d) / 3 * 10, rand(I, d) / 3 * 10 (base initModel's draws,
WRMF.py:14-15; only their sha256 is kept), and of the trained tables one row in ``row_stride`` is kept -- every row of X and Y still
enters the next epoch's loss, which is kept for every epoch.
Running it twice gives byte-identical files.
"""
import io
import json
import os
import random
import sys
import tempfile
import zipfile
from contextlib import redirect_stdout

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import OUT, REF, install_stubs, sha, write_conf  # noqa: E402


def run_wrmf(conf_path, seed):
    from QRec import QRec
    from util.config import ModelConf
    from model.ranking.WRMF import WRMF
    import base.recommender as br
    rec = {"epochs": []}
    orig_init, orig_conv, orig_rm = WRMF.initModel, WRMF.isConverged, br.Measure.rankingMeasure

    def initModel(self):
        orig_init(self)
        rec["X0"], rec["Y0"] = self.X.copy(), self.Y.copy()

    def isConverged(self, epoch):
        rec["epochs"].append(dict(epoch=epoch, loss=float(self.loss), X=self.X.copy(), Y=self.Y.copy()))
        return orig_conv(self, epoch)

    def rankingMeasure(origin, res, N):
        rec["recList"] = res
        return orig_rm(origin, res, N)

    WRMF.initModel, WRMF.isConverged = initModel, isConverged
    br.Measure.rankingMeasure = staticmethod(rankingMeasure)
    random.seed(seed); np.random.seed(seed)
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            q = QRec(ModelConf(conf_path))
            m = WRMF(q.config, q.trainingData, q.testData)
            rec["measure"] = m.execute()
    finally:
        WRMF.initModel, WRMF.isConverged = orig_init, orig_conv
        br.Measure.rankingMeasure = staticmethod(orig_rm)
    rec.update(model=m, py_state=random.getstate(), train_rows=q.trainingData, test_rows=q.testData,
               printed=[ln for ln in buf.getvalue().splitlines() if ln.startswith("epoch:")])
    return rec


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (byte-identical output from run to run)"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def pack(rec, name, keep_epochs, row_stride):
    m = rec["model"]
    arrays = dict(
        train_uid=np.array([m.data.user[r[0]] for r in rec["train_rows"]], dtype=np.int32),
        train_iid=np.array([m.data.item[r[1]] for r in rec["train_rows"]], dtype=np.int32),
        train_r=np.array([r[2] for r in rec["train_rows"]], dtype=np.float64),
        test_uid=np.array([m.data.user.get(r[0], -1) for r in rec["test_rows"]], dtype=np.int32),
        test_iid=np.array([m.data.item.get(r[1], -1) for r in rec["test_rows"]], dtype=np.int32),
        test_uname=np.array([str(r[0]) for r in rec["test_rows"]]), test_iname=np.array([str(r[1]) for r in rec["test_rows"]]),
        py_state=np.array(rec["py_state"][1], dtype=np.uint32),
        loss=np.array([e["loss"] for e in rec["epochs"]], dtype=np.float64))
    kept = keep_epochs or [e["epoch"] for e in rec["epochs"]]
    table_sha = {}
    for e in rec["epochs"]:
        if e["epoch"] in kept:
            arrays["X%d" % e["epoch"]] = e["X"][::row_stride].copy(); arrays["Y%d" % e["epoch"]] = e["Y"][::row_stride].copy()
            table_sha["X%d" % e["epoch"]] = sha(e["X"]); table_sha["Y%d" % e["epoch"]] = sha(e["Y"])
    rl = rec["recList"]
    users = list(rl.keys())
    N = max(len(v) for v in rl.values())
    ids = np.full((len(users), N), -1, dtype=np.int32)
    for a, un in enumerate(users):
        for b, (iname, _) in enumerate(rl[un]):
            ids[a, b] = m.data.item[iname]
    arrays.update(rec_users=np.array([m.data.user.get(un, -1) for un in users], dtype=np.int32),
                  rec_user_names=np.array([str(u) for u in users]), rec_ids=ids)
    return arrays, dict(name=name, n_users=len(m.data.user), n_items=len(m.data.item), n_train=len(rec["train_rows"]),
                        n_test=len(rec["test_rows"]), emb_size=m.emb_size, regU=m.regU, maxEpoch=m.maxEpoch,
                        epochs=[dict(epoch=e["epoch"], loss=e["loss"]) for e in rec["epochs"]], printed=rec["printed"],
                        measure=rec["measure"], X0_sha256=sha(rec["X0"]), Y0_sha256=sha(rec["Y0"]),
                        kept_epochs=kept, row_stride=row_stride, table_sha256=table_sha)


def case_filmtrust(tmp):
    conf = os.path.join(tmp, "wrmf_ft.conf")
    write_conf(conf, ratings="./dataset/FilmTrust/trainset.txt", ratings__setup="-columns 0 1 2", model__name="WRMF",
               evaluation__setup="-testSet ./dataset/FilmTrust/testset.txt", item__ranking="on -topN 10,20",
               num__factors="20", num__max__epoch="3", WRMF="-alpha 10 -lamba 1", learnRate="-init 0.01 -max 1",
               reg__lambda="-u 1 -i 0.02 -b 0.02", output__setup="off -dir ./results/")
    rec = run_wrmf(conf, 1)
    arrays, meta = pack(rec, "wrmf_filmtrust", None, 4)
    save_npz(os.path.join(OUT, "wrmf_filmtrust.npz"), arrays)
    meta.update(seed=1, conf=open(conf).read())
    return meta


def case_lastfm(tmp):
    conf = os.path.join(tmp, "wrmf_lfm.conf")
    # config/WRMF.conf as shipped, output off (nothing else differs)
    write_conf(conf, ratings="./dataset/lastfm/ratings.txt", ratings__setup="-columns 0 1 2", model__name="WRMF",
               evaluation__setup="-ap 0.2", item__ranking="on -topN 10", num__factors="20", num__max__epoch="7",
               WRMF="-alpha 10 -lamba 1", learnRate="-init 0.01 -max 1", reg__lambda="-u 1 -i 0.02 -b 0.02",
               output__setup="off -dir ./results/")
    rec = run_wrmf(conf, 7)
    last = rec["epochs"][-1]["epoch"]
    arrays, meta = pack(rec, "wrmf_lastfm", [1, last], 16)
    save_npz(os.path.join(OUT, "wrmf_lastfm.npz"), arrays)
    meta.update(seed=7, conf=open(conf).read())
    return meta


def main():
    install_stubs()
    tmp = tempfile.mkdtemp(prefix="qrec_golden_wrmf_")
    os.symlink(os.path.join(REF, "dataset"), os.path.join(tmp, "dataset"))
    os.chdir(tmp)
    metas = [case_filmtrust(tmp), case_lastfm(tmp)]
    with open(os.path.join(OUT, "golden_wrmf_meta.json"), "w") as f:
        json.dump({m["name"]: m for m in metas}, f, indent=1, sort_keys=True)
    for m in metas:
        print(m["name"], "ok", {k: m[k] for k in ("n_users", "n_items", "n_train")})


if __name__ == "__main__":
    main()
