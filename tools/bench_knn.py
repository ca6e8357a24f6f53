"""UserKNN / ItemKNN / SlopeOne timing on the MI355X (engine.CoRatingKnn, engine.SlopeOneSolver, knn.hip).

    python tools/bench_knn.py [out.json]          # default out: profiles/knn_bench.json

For UserKNN/pcc, ItemKNN/pcc and SlopeOne at FilmTrust (tests/golden/knn_filmtrust.npz) and at the Yelp2018 shape
(synth.make_dataset("yelp2018") with ratings drawn, seeded, from FilmTrust's rating histogram): the wall time of the sweep, the
top-K and the predictions (each ends in a device synchronisation), the co-rating contributions -- (query, candidate, key)
triples, counted from the CSRs -- and the achieved contributions/s, and the one-core host-mirror time (tests/test_knn_cpu.py)
at FilmTrust.  The per-kernel split comes from a run of this script under rocprofv3 --kernel-trace --stats.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _csrs(u, i, r, nu, ni):
    from qrec_amd.interactions import dedup_user_item, user_item_csr
    du, di, dr = dedup_user_item(u, i, r, ni)
    return (user_item_csr(du, di, dr, nu, ni, assume_unique=True), user_item_csr(di, du, dr, ni, nu, assume_unique=True))


def _means(csr):
    return np.bincount(csr.row_ids(), weights=csr.values, minlength=csr.n_rows) / np.maximum(np.diff(csr.indptr), 1)


def _problem(nu, ni, u, i, r, test_u, test_i):
    user_csr, item_csr = _csrs(u, i, r, nu, ni)
    q_user = np.array(list(dict.fromkeys(test_u.tolist())), dtype=np.int64)
    q_item = np.array(list(dict.fromkeys(test_i.tolist())), dtype=np.int64)
    ipos = {c: k for k, c in enumerate(q_item.tolist())}
    um = _means(user_csr)
    return dict(n_users=nu, n_items=ni, u=u, i=i, r=r, user_csr=user_csr, item_csr=item_csr, q_user=q_user, q_item=q_item,
                test_u=test_u, test_i=test_i, test_item_query=np.array([ipos[c] for c in test_i.tolist()], dtype=np.int64),
                user_means=um, item_means=_means(item_csr), global_mean=float(sum(um.tolist()) / um.size))


def filmtrust_histogram():
    z = np.load(os.path.join(ROOT, "tests", "golden", "knn_filmtrust.npz"))
    vals, counts = np.unique(z["train_r"], return_counts=True)
    return vals, counts / counts.sum()


def yelp_problem(seed: int = 2018):
    """the Yelp2018 shape, ratings drawn from FilmTrust's histogram"""
    from qrec_amd.synth import make_dataset
    g = make_dataset("yelp2018")
    vals, p = filmtrust_histogram()
    r = np.random.default_rng(seed).choice(vals, size=g["train_u"].size, p=p)
    return _problem(g["n_users"], g["n_items"], g["train_u"].astype(np.int64), g["train_i"].astype(np.int64), r,
                    g["test_u"].astype(np.int64), g["test_i"].astype(np.int64))


def filmtrust_problem():
    z = np.load(os.path.join(ROOT, "tests", "golden", "knn_filmtrust.npz"))
    u, i = z["train_uid"].astype(np.int64), z["train_iid"].astype(np.int64)
    return _problem(int(u.max()) + 1, int(i.max()) + 1, u, i, z["train_r"], z["test_uid"].astype(np.int64), z["test_iid"].astype(np.int64))


def contributions(rows, inverted, queries):
    """sum over the queries' row entries of the key's column length: the (query, candidate, key) triples the sweep adds"""
    col_len = np.diff(inverted.indptr)
    lens = np.diff(rows.indptr)
    total = 0
    for c in queries[queries >= 0].tolist():
        total += int(col_len[rows.indices[rows.indptr[c]:rows.indptr[c] + lens[c]]].sum())
    return total


def sync():
    from qrec_amd import capi
    capi._check(capi.load().qrec_stream_sync(None))


def timed(fn):
    sync(); t0 = time.perf_counter(); out = fn(); sync()
    return out, (time.perf_counter() - t0) * 1e3


def bench_knn(p, side, reps=3):
    from qrec_amd import capi
    from qrec_amd.engine import CoRatingKnn
    rows, inv = (p["user_csr"], p["item_csr"]) if side == "user" else (p["item_csr"], p["user_csr"])
    qids = p["q_user"] if side == "user" else p["q_item"]
    means = p["user_means"] if side == "user" else p["item_means"]
    knn = CoRatingKnn(capi.KNN_PCC, rows, inv.n_rows, means, qids, 20)
    if side == "user":
        qpos = {c: k for k, c in enumerate(qids.tolist())}
        query, other = np.array([qpos[c] for c in p["test_u"].tolist()]), p["test_i"]
        base = p["user_means"][p["test_u"]]
    else:
        query, other, base = p["test_item_query"], p["test_u"], p["item_means"][p["test_i"]]
    members = p["user_csr"].sorted_rows()
    best = {}
    for _ in range(reps):
        for name, fn in (("sweep", knn.sweep), ("topk", knn.topk),
                         ("predict", lambda: knn.predict(0 if side == "user" else 1, query, other, base, members, means))):
            _, ms = timed(fn)
            best[name] = min(best.get(name, 1e30), ms)
    n = contributions(rows, inv, qids)
    return dict(queries=int(qids.size), candidates=int(rows.n_rows), test_rows=int(query.size), contributions=n,
                ms=best, ms_total=sum(best.values()), contributions_per_s=n / (best["sweep"] * 1e-3))


def bench_slopeone(p, reps=3):
    from qrec_amd.engine import SlopeOneSolver
    so = SlopeOneSolver(p["item_csr"], p["user_csr"], p["q_item"])
    base = p["user_means"][p["test_u"]]
    best = 1e30
    for _ in range(reps):
        _, ms = timed(lambda: so.predict(p["test_item_query"], p["test_u"], base))
        best = min(best, ms)
    n = contributions(p["item_csr"], p["user_csr"], p["q_item"])
    return dict(queries=int(p["q_item"].size), candidates=int(p["n_items"]), batch=so.batch, contributions=n, ms_sweep_and_predict=best,
                contributions_per_s=n / (best * 1e-3))


def host_mirror_ms(p):
    """one core, the host mirror's sweep + sequence + top-K of every query (FilmTrust)"""
    from test_knn_cpu import PCC, Side, sequence, sweep, top_k
    out = {}
    for side in ("user", "item"):
        s = Side(p["u"], p["i"], p["r"], p["n_users"], p["n_items"]) if side == "user" else Side(p["i"], p["u"], p["r"], p["n_items"], p["n_users"])
        q = p["q_user"] if side == "user" else p["q_item"]
        t0 = time.perf_counter()
        S = sweep(PCC, [s.rows[c] if c >= 0 else {} for c in q.tolist()], np.array([s.means[c] if c >= 0 else 0 for c in q.tolist()]), s)
        for t in range(q.size):
            top_k(*sequence(S, q, t), 20)
        out[side] = (time.perf_counter() - t0) * 1e3
    return out


def main():
    from qrec_amd import capi
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "knn_bench.json")
    capi.init(0)
    res = dict(device=capi.device_info(), cases={})
    ft = filmtrust_problem()
    res["cases"]["filmtrust"] = dict(UserKNN_pcc=bench_knn(ft, "user"), ItemKNN_pcc=bench_knn(ft, "item"), SlopeOne=bench_slopeone(ft),
                                     host_mirror_one_core_ms=host_mirror_ms(ft))
    print(json.dumps({"filmtrust": res["cases"]["filmtrust"]}), flush=True)
    y = yelp_problem()
    res["cases"]["yelp2018"] = dict(UserKNN_pcc=bench_knn(y, "user", 2), ItemKNN_pcc=bench_knn(y, "item", 2), SlopeOne=bench_slopeone(y, 1))
    print(json.dumps({"yelp2018": res["cases"]["yelp2018"]}), flush=True)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
