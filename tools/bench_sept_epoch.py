#!/usr/bin/env python3
"""What SEPT's per-epoch perturbed graph costs both ways, for one joint epoch, at FilmTrust + trust and at a synthetic Yelp2018-shape
graph with 10 followees per user (-drop_rate 0.3, d = 64, two layers):

  exact mode       host time of get_adj_mat(is_subgraph=True): the two random.sample replays + the scipy sum and row-sum scaling
                   (graph.sept_perturbed_adjacency), then _View.set_matrix: two SpMM plans (M and M^T) built and uploaded
  throughput mode  device time of SeptGraphSampler.draw (two permutations + qrec_sept_perturbed_values), between two events
  the known cost   the perturbed view's forward SpMM over the whole union structure (device-drawn values, dropped entries 0) against the
                   same product over the host-built compact CSR of the same keep lists, alternated in one run

Writes profiles/sept_throughput.json (``--out`` to write elsewhere).  ``--paired S`` adds the paired-modes procedure of
tests/test_gpu_sept_throughput.py over S seeds (FilmTrust + trust, 6 epochs): mean and standard error of Recall@10 / NDCG@10 differences
between throughput mode and exact mode on the same stream, and the max-normalised table distance."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qrec_amd import capi                                                   # noqa: E402
from qrec_amd.capi import DeviceBuffer as DB                                # noqa: E402
from qrec_amd.graph import SeptGraphSampler, SpmmPlan, _View, _scaled_by_row_sums, sept_perturbed_adjacency   # noqa: E402

RATE, DIM, LAYERS = 0.3, 64, 2


def filmtrust():
    z = np.load(os.path.join(ROOT, "tests", "golden", "sept_graphs_filmtrust.npz"))
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_meta.json")))["sept_graphs_filmtrust"]
    return meta["n_users"], meta["n_items"], z["train_uid"], z["train_iid"], z["follower"], z["followee"]


def yelp_shape():
    from qrec_amd.synth import make_dataset
    d = make_dataset("yelp2018")
    nu = d["n_users"]
    rng = np.random.default_rng(0)
    fo = np.repeat(np.arange(nu, dtype=np.int32), 10)
    return nu, d["n_items"], d["train_u"].astype(np.int32), d["train_i"].astype(np.int32), fo, rng.integers(0, nu, fo.size).astype(np.int32)


def compact_csr(nu, ni, uid, iid, fo, fe, keep, skeep):
    """the perturbed graph of explicit keep lists with the exact path's arithmetic (graph.sept_perturbed_adjacency without the draw)"""
    import scipy.sparse as sp
    n = nu + ni
    up = sp.csr_matrix((np.ones(keep.size, np.float32), (uid[keep], nu + iid[keep].astype(np.int64))), shape=(n, n))
    soc = sp.csr_matrix((np.ones(skeep.size, np.float32), (fo[skeep], fe[skeep])), shape=(n, n))
    return _scaled_by_row_sums(up + up.T + soc.multiply(soc)).tocsr()


def events_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    e0, e1, ts = capi.Event(), capi.Event(), []
    for _ in range(reps):
        e0.record(); fn(); e1.record(); e1.sync()
        ts.append(e1.elapsed_ms_since(e0))
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), reps=reps)


def measure(name, nu, ni, uid, iid, fo, fe):
    n, ld = nu + ni, DIM
    out = dict(graph=name, n_users=nu, n_items=ni, training_rows=int(uid.size), follow_pairs=int(fo.size), drop_rate=RATE, d=DIM)
    # exact mode, host: replay + scipy, then two plans + upload; the first set_matrix also pays the row -> XCD map, later epochs reuse it
    random.seed(0)
    words = capi.state_from_python(random.getstate())
    view = _View(n, ld, LAYERS)
    host = []
    for epoch in range(4):
        t0 = time.perf_counter(); M = sept_perturbed_adjacency(words, nu, ni, uid, iid, fo, fe, RATE); t1 = time.perf_counter()
        view.set_matrix(M, split_row=nu); capi.device_sync(); t2 = time.perf_counter()
        host.append((t1 - t0, t2 - t1))
    out["exact_mode_host"] = dict(replay_and_scipy_ms=float(np.median([h[0] for h in host[1:]]) * 1e3),
                                  two_plans_and_upload_ms=float(np.median([h[1] for h in host[1:]]) * 1e3),
                                  first_epoch_two_plans_and_upload_ms=host[0][1] * 1e3, epochs_timed=3)
    # throughput mode, device
    t0 = time.perf_counter(); smp = SeptGraphSampler(nu, ni, uid, iid, fo, fe); capi.device_sync()
    out["one_time_host_setup_s"] = time.perf_counter() - t0
    vals, vals_t = DB(max(smp.nnz, 1), np.float32), DB(max(smp.nnz, 1), np.float32)
    k = [0]

    def draw():
        k[0] += 1
        smp.draw(RATE, 7, (1 << 32) + 2 * k[0], vals, vals_t)
    out["throughput_mode_device_draw"] = events_ms(draw, 30)
    # the known cost: SpMM over the union structure vs over the compact CSR of the same keep lists
    kr, ks = smp.sizes(RATE)
    keep, skeep = smp.d_keep.numpy()[:kr], smp.d_skeep.numpy()[:ks]
    M = compact_csr(nu, ni, uid, iid, fo, fe, keep, skeep); M.sort_indices()
    chunk = view.plan.row_chunk
    kw = dict(split_row=nu, row_chunk=chunk) if chunk is not None else dict(split_row=nu, chunks=1)
    union = SpmmPlan(smp.indptr, smp.indices, np.zeros(smp.nnz, np.float32), ld, **kw).with_values(vals)
    compact = SpmmPlan(M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(np.float32), ld, **kw)
    X = DB.from_numpy((np.random.default_rng(1).standard_normal((n, ld)) * 0.1).astype(np.float32))
    Y1, Y2 = DB.zeros((n, ld), np.float32), DB.zeros((n, ld), np.float32)
    capi.spmm_csr(union, X, Y1, ld); capi.spmm_csr(compact, X, Y2, ld)
    a, b = Y1.numpy(), Y2.numpy()
    out["spmm_union_vs_compact_rel_err"] = float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))
    inner = 20
    t_union, t_compact = [], []
    for rep in range(8):                                                     # alternated, so that both see the same neighbours on the machine
        for plan, Y, ts in ((union, Y1, t_union), (compact, Y2, t_compact)):
            r = events_ms(lambda: [capi.spmm_csr(plan, X, Y, ld) for _ in range(inner)], 1, warmup=1 if rep == 0 else 0)
            ts.append(r["median_ms"] / inner)
    out["forward_spmm"] = dict(union_structure_nnz=smp.nnz, compact_nnz=int(M.nnz), nnz_ratio=smp.nnz / max(int(M.nnz), 1),
                               union_structure_ms=float(np.median(t_union)), compact_csr_ms=float(np.median(t_compact)),
                               time_ratio=float(np.median(t_union) / np.median(t_compact)), products_per_sample=inner, samples=len(t_union))
    return out


def paired(seeds: int):
    import tempfile
    from pathlib import Path
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import device_stream as DS
    import sept_stream as SS
    d, dist = [], []
    with tempfile.TemporaryDirectory() as tmp:
        problem = SS.social_problem("SEPT", Path(tmp), epochs=6, batch=2000, extra="-n_layer 2 -ss_rate 0.005 -drop_rate 0.3 -ins_cnt 5")
        for s in range(seeds):
            a = SS.run_mode("SEPT", problem, "throughput", 100 + s)
            b = SS.run_mode("SEPT", problem, "exact", 100 + s)
            d.append(np.array(a["values"]) - np.array(b["values"])); dist.append(DS.table_distance(a["arrays"], b["arrays"]))
    D = np.array(d)
    mean, se = D.mean(0), D.std(0, ddof=1) / np.sqrt(seeds)
    return dict(procedure="throughput (float atomics, union structure) vs exact (ordered, host CSR) on the same stream, FilmTrust + trust, 6 epochs",
                seeds=seeds, recall10_mean_d=float(mean[1]), recall10_se=float(se[1]), ndcg10_mean_d=float(mean[3]), ndcg10_se=float(se[3]),
                recall10_abs_mean_plus_2se=float(abs(mean[1]) + 2 * se[1]), ndcg10_abs_mean_plus_2se=float(abs(mean[3]) + 2 * se[3]),
                table_distance_max=float(max(dist)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sept_throughput.json"))
    ap.add_argument("--paired", type=int, default=0, help="seeds of the paired-modes procedure (0: skip)")
    ap.add_argument("--skip-yelp", action="store_true")
    args = ap.parse_args()
    capi.init(0)
    res = dict(device=capi.device_info()["arch"], graphs=[measure("FilmTrust + trust", *filmtrust())])
    if not args.skip_yelp:
        res["graphs"].append(measure("synthetic Yelp2018 shape, 10 followees per user", *yelp_shape()))
    if args.paired:
        res["paired_modes"] = paired(args.paired)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
