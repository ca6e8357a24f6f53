#!/usr/bin/env python3
"""bench.py -- BPR triplet-updates/sec on the MI355X hot path (BASELINE.json metric).

One EPOCH = one full pass of the reference's BPR epoch (model/ranking/BPR.py:29-43) over the synthetic
Yelp2018-shape interaction matrix (31,668 x 38,048, ~1.25 M train triplets, d=64): negative sampling for every
triplet (device Philox sampler) -> fused gather / dot / sigmoid / SGD scatter kernel (throughput mode) -> epoch-end
regulariser reductions -> loss, convergence test and bold-driver learning-rate update (the reference's isConverged)
on the device.  Inputs are resident in HBM before the timed region; the host only enqueues.

One STEP = `epochs_per_step` consecutive epochs: an epoch is 0.6 ms, so K = 20 single epochs would be a 12 ms sample;
the bench repeats epochs inside a step until the K timed steps cover >= --min-seconds (0.3 s).  `value` does not
depend on that grouping (triplets / second); `ms_per_step` is per step, `config.ms_per_epoch` per epoch.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full  # + every other figure and check of the line (below)
    python bench.py --gpus N --steps K --warmup W          # N > 1 typed like this: bench.py starts its own N ranks (below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run does what its headline figure needs and nothing else: set-up, warm-up, the K timed steps, --dump-outputs if given,
the JSON line.  --full adds the legs that take runs of their own (marked [--full] below): CPU baselines, the order-exact mode,
the Recall@20 comparisons with a reference, other shapes and configurations, the HBM-resident roofline, and for N > 1 the
weak-scaling leg, the other item-table layout and config #4.  They run after the timed steps and do not change the headline.

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment re-executes itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free port>` with
the same arguments: one rank per GPU, rank 0's JSON line on the caller's stdout.  Under a launcher (WORLD_SIZE set) it is
one of the ranks.  The layout can be steered by flag or, for a caller whose command line is fixed, by environment:
--dist-mode / QREC_DIST_MODE (replicated | sharded), --scaling (weak | strong).

N > 1, one process per GPU (qrec_amd/dist.py; collectives are RCCL bound directly by libqrec_hip.so, torch.distributed
/gloo is only the control plane).  Users (rows of P, triplets, sampler) are sharded by rank.  --dist-mode replicated
(default): item table replicated, a delta all-reduce per reconciliation, the epoch's last one fused with the loss terms.  --dist-mode
sharded: item table row-sharded, per batch an all-to-all of the distinct rows a rank's triplets touch and of their
updates.  --scaling strong (default since round 4: BASELINE.json quotes the metric on THE Yelp2018 shape at 1/2/4/8 GPUs): the same
31,668 users split over the ranks = `value`; [--full] the weak-scaling figure (every rank its own 31,668 users) is timed next to it and
reported as `weak_scaling` under its aggregate shape; --scaling weak makes that leg `value`.  --sync-per-epoch (default: 1 up to two ranks, 2 beyond):
how often the ranks' item rows are reconciled inside an epoch.

Rank 0 prints ONE JSON line.  Besides the contract fields it carries
  roofline     -- the SGD kernel's algorithmic bytes/launch over its mean launch time (HIP events on the launch
                  stream of the timed steps) against 8 TB/s HBM peak;
  multi_gpu    -- N > 1: what RCCL reports per rank, kernel time per rank, collectives and bytes per epoch;
and with --full also
  roofline_hbm_resident -- the same kernel on an HBM-sized problem (a single-GPU slice of BASELINE config #4: 1.25 M x 1 M,
                  d=128, 1.15 GB of tables); its p_update: how the item-major kernel writes P[u] there ("rmw": sc1 load + store
                  instead of an atomic delta, chosen by engine.resolve_p_update from the collision density;
                  `roofline_hbm_resident_atomic` = the same slice with atomic deltas);
  exact_mode   -- the order-exact mode (the one that meets the bit-exact-stream / 1e-5 numeric contract) timed on
                  the same workload;
  cpu_baseline -- the CPU port of the same epoch (oracle/, plain C, fp64, 1 thread) timed on this box's host cores
                  on a bounded sample; reference_loop_here: the reference's own interpreter-bound form (oracle/npref.py)
                  timed on this host; reference_python: the unmodified reference's figure (another host);
  recall_at_20 -- the paired harness (tools/paired_recall.py): fresh runs of the timed mode against order-exact fp64 training on the same
                  negatives, on the bench's own graph and on the planted-community graph of the same shape (datasets[]: recall, abs_diff,
                  rel_diff at the reference's peak epoch and at the last one); N > 1: the same over the real communicator;
  other_configs -- BASELINE configs #2, #3, #5 and the evaluation, measured by this very run (HIP events, >= 20 repetitions);
                  N > 1: other_configs.config4_sharded, each rank's share of BASELINE config #4 in north_star's layout (row-sharded
                  item table, per-batch all-to-all) and that layout's paired Recall@20;
  weak_scaling, value_sharded / value_replicated -- N > 1, strong scaling: the weak-scaling leg and the other item-table layout.
Under --full, --no-cpu-baseline drops cpu_baseline and --no-extras every other --full leg.
Sharded layout options: --shard-batch, --shard-pipeline, --no-plan-inside.
Every timed region starts from a collected Python heap with the cyclic collector off (settled_heap).

--dump-outputs DIR (one process only): after the timed steps, what the last step handed its caller -- the trained tables P (users x d)
and Q (items x d, float32) and that step's per-epoch loss and learning rate with the final rate (float64) -- as DIR/<name>.npy, at most
64 MB in all (larger tables: a fixed, seeded sample of their rows).  Inputs are seeded, and in such a run the epochs of a step follow from
the arguments alone (--epochs-per-step, else --min-seconds over --steps nominal epochs of NOMINAL_EPOCH_S) instead of a clock
calibration, so that the same arguments give the same computation on every run and every build.  The Hogwild kernel's update order
is still a race: two runs of the Yelp2018 shape (--steps 20) agreed in the learning rates exactly, in the loss to 2e-4 and in the
tables to 8e-3 (relative norms), so a comparison of two builds needs a tolerance of that order.
"""
from __future__ import annotations

import argparse
import contextlib
import gc
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
DIM = 64
LR0, MAX_LR, REG_U, REG_I = 0.01, 1.0, 0.001, 0.001   # config/BPR.conf:9-10
FLUSH_EVERY = 16
SEED = 2018
NOMINAL_EPOCH_S = 0.6e-3        # the Yelp2018-shape epoch: sets the epochs per step of a --dump-outputs run
DUMP_BUDGET = 64 << 20          # bytes of all --dump-outputs arrays together


def bytes_per_triplet(d: int) -> int:
    """3 rows read + 3 rows written (fp32) + 3 int32 ids."""
    return 6 * d * 4 + 12


def recall_at_n(ids: np.ndarray, users: np.ndarray, test_u: np.ndarray, test_i: np.ndarray, n_items: int) -> float:
    """util/measure.py:106-109: mean over test users of |top-N ∩ test items| / |test items|."""
    test_keys = np.unique(test_u.astype(np.int64) * n_items + test_i)
    rec_keys = (users.astype(np.int64)[:, None] * n_items + ids).ravel()
    hit = np.isin(rec_keys, test_keys).reshape(ids.shape).sum(1)
    cnt = np.bincount(test_u, minlength=int(users.max()) + 1)[users]
    return float((hit / cnt).mean())


def evaluate_recall(P, Q, data, indptr, items, N=20):
    """Recall@N of (P, Q) on the held-out edges through the product's device ranker."""
    from qrec_amd.interactions import CSR
    from qrec_amd.ranking import DeviceRanker
    users = np.unique(data["test_u"]).astype(np.int32)
    ids, _ = DeviceRanker(np.ascontiguousarray(P, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32),
                          CSR(indptr, items)).topk(users, N)
    return recall_at_n(ids, users, data["test_u"], data["test_i"], data["n_items"])


def cpu_baseline(u, i, indptr, n_items, U, seconds=12.0):
    """The same epochs on the host, timed: oracle sampler (CPython MT19937 replay) + the plain-C fp64
    restatement of BPR.optimization + the epoch-end reductions, single thread, ~`seconds` of work."""
    from oracle import c as O
    rng = np.random.default_rng(0)
    P = rng.random((U, DIM)) / 3; Q = rng.random((n_items, DIM)) / 3
    mt = O.MT.cpython_seed(0)
    done, epochs, t0 = 0, 0, time.perf_counter()
    while True:
        j = O.bpr_sample_epoch(mt, indptr, i, n_items)
        O.bpr_sgd(P, Q, u, i, j, LR0, REG_U, REG_I)
        O.sumsq(P); O.sumsq(Q)
        done += u.size; epochs += 1
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    # ... and the interpreter-bound form the reference itself runs in (oracle/npref.py: one Python iteration and seven numpy row
    # statements per triplet, random.choice negatives), timed HERE on a bounded sample -- the reference cannot travel to this box
    from oracle import npref
    import random as _random
    Pn = rng.random((U, DIM)) / 3; Qn = rng.random((n_items, DIM)) / 3
    t1 = time.perf_counter()
    _, n_loop, _ = npref.bpr_epoch(Pn, Qn, indptr, i, n_items, LR0, REG_U, REG_I, rng=_random.Random(0), max_triplets=200_000)
    dt_loop = time.perf_counter() - t1
    return {"value": done / dt, "unit": "triplet-updates/s", "cores": 1, "kind": "port",
            "sample": f"{epochs} epochs ({done} triplets, {dt:.1f} s), C fp64 port of BPR.py:29-53 + CPython-stream sampler",
            "reference_loop_here": {"value": n_loop / dt_loop, "unit": "triplet-updates/s", "cores": 1, "kind": "port",
                                    "what": "a RESTATEMENT of the reference's interpreter-bound loop, leaner than the reference's own (ints instead of "
                                            "string-keyed dict look-ups, locals instead of attribute access, no method call per triplet): per triplet one "
                                            "CPython iteration, random.choice, seven numpy row statements (BPR.py:28-53) -- oracle/npref.py, timed on this "
                                            "host; the unmodified reference is `reference_python` (another host)",
                                    "sample": f"{n_loop} triplets of the same epoch ({dt_loop:.1f} s), d = {DIM}, fp64"},
            "reference_python": {"value": 58930.0, "unit": "triplet-updates/s", "cores": 1,
                                 "host": "survey container (8 vCPU Xeon 2.1 GHz KVM), not this box: the Python reference cannot travel",
                                 "source": "BASELINE.md s2: unmodified BPR.trainModel, same shape, fp64"}}


def recall_case(mode, dataset, lr0, epochs, every=5, seed=SEED, world=1, layout="replicated", syncs=1):
    """The metric's second half (north_star: "Recall@20 within +-0.002 of reference"): a fresh `epochs`-epoch training in the timed mode
    against order-exact fp64 training (the oracle's restatement of BPR.py:45-53 + the bold driver) from the same tables on the SAME
    negatives, both ranked by the device ranker -- tools/paired_recall.py.  Recall at the reference's peak epoch and at the last one,
    |diff| absolute and relative, loss gap."""
    from tools import paired_recall as PR
    case = dict(dataset=dataset, lr0=lr0, seed=seed, mode=mode, epochs=epochs, eval_every=every, world=world, layout=layout, syncs=syncs)
    r = PR.run_case(case, recall_case.cache, recall_case.datasets)
    return {"dataset": dataset, "lr0": lr0, "epochs": epochs, "mode": mode,
            "recall": r["peak"]["recall_gpu"], "recall_exact_order": r["peak"]["recall_exact_order"], "peak_epoch": r["peak"]["epoch"],
            "abs_diff": r["peak"]["abs_diff"], "rel_diff": r["peak"]["rel_diff"],
            "final": {k: r["final"][k] for k in ("epoch", "recall_gpu", "recall_exact_order", "abs_diff", "rel_diff", "loss_rel_gap")},
            "worst_mark": {k: r["worst_mark"][k] for k in ("epoch", "abs_diff")}, "bar": r["bar"], "within_bar_at_peak": r["within_bar_at_peak"],
            "same_bold_driver_decisions": r["same_bold_driver_decisions"]}


recall_case.cache, recall_case.datasets = {}, {}


def recall_bpr_conf(mode, seeds=16):
    """The reference's own BPR workload (config/BPR.conf: lastfm, 50 factors, learnRate 0.01 -max 1, reg 0.001, 100 epochs), scored once
    after the LAST epoch as the reference does, over `seeds` seeds (initial tables + negatives): the signed gap throughput mode - order-exact
    fp64 training per seed, its mean +- standard error, and beside it the yardstick with no GPU in it -- the same sequential fp64 training in
    another visiting order (tools/paired_recall.py plan_bpr_conf / summarize_seeds)."""
    from tools import paired_recall as PR
    cases = PR.plan_bpr_conf(seeds=range(1, seeds + 1), rounds=(None,), modes=(mode,))
    res = [PR.run_case(c, recall_case.cache, recall_case.datasets) for c in cases]
    (row,) = PR.summarize_seeds(res)
    g = row["final_gap"]
    per_seed = np.abs(np.array([r["final"]["signed_diff"] for r in res if "final" in r]))
    return {"dataset": "lastfm", "conf": "config/BPR.conf (num.factors 50, learnRate -init 0.01 -max 1, reg 0.001, 100 epochs), Recall after the last epoch",
            "mode": mode, "lr0": 0.01, "epochs": 100, "seeds": row["seeds"],
            "recall_exact_order_mean": row["recall_exact_order_mean"], "recall_exact_order_sd_over_seeds": row["recall_exact_order_sd_over_seeds"],
            "final_gap_signed": {k: g[k] for k in ("n", "mean_signed", "se", "sd", "mean_abs", "max_abs")},
            # what ONE run looks like (the reader is to see 0.002-0.006, not only the mean's 0.0004)
            "per_seed_abs_gap": {"mean": float(per_seed.mean()), "p90": float(np.quantile(per_seed, 0.9)), "max": float(per_seed.max()),
                                 "runs_inside_the_bar": int((per_seed <= 0.002).sum()), "runs": int(per_seed.size)},
            "abs_diff": abs(g["mean_signed"]), "abs_diff_is": "|mean over seeds of the signed final-epoch gap|", "bar": 0.002,
            "within_bar": bool(abs(g["mean_signed"]) <= 0.002),
            "final_gap_recall_at_10": row["final_gap_other_topn"]["10"],
            "order_only_yardstick": {**row["order_null_final_gap"], "what": "sequential fp64 training of the same triplets on the same negatives in one fixed random "
                                                                              "visiting order, minus the same in the reference's order: no GPU involved"},
            "per_run_note": "a single run cannot be held to +-0.002 here: 1,884 test users, a bold driver in its bounce regime (no two runs take the same "
                            "decisions), the reference's own Recall@20 spreads `recall_exact_order_sd_over_seeds` from seed to seed; the order-exact mode "
                            "(the drop-in default) reproduces the reference to 1e-10"}


def recall_legs(mode, shape):
    """`recall_at_20` of the N = 1 line: the bench's own (structureless) shape for continuity with rounds 1-3, and the planted-community
    graph of the same size, on which order-exact training reaches Recall@20 0.12 and the bar can fail -- at BPR.conf's
    rate (0.01: 40 epochs to the peak) and at five times that rate (20 epochs)."""
    legs = []
    if shape == "yelp2018":
        legs.append(recall_case(mode, "yelp2018", LR0, 25))
        legs.append(recall_case(mode, "yelp2018-clustered", LR0, 40))
        legs.append(recall_case(mode, "yelp2018-clustered", 5 * LR0, 20))
        legs.append(recall_bpr_conf(mode))
    else:
        legs.append(recall_case(mode, shape, LR0, 25))
    head = legs[0]
    return {"gpu_throughput_mode": head["final"]["recall_gpu"], "cpu_port_exact_order": head["final"]["recall_exact_order"],
            "abs_diff": head["final"]["abs_diff"], "rel_diff": head["final"]["rel_diff"], "epochs": head["epochs"], "dataset": head["dataset"],
            "datasets": legs, "harness": "tools/paired_recall.py (same negatives, same tables, same bold driver; reference = order-exact fp64)"}


def exact_mode_rate(capi, u, items, indptr, n_items, P0, Q0):
    """The order-exact mode on the same workload: CPython-stream negatives from the native host replay, triplets
    applied strictly in the reference's order on the device (fp64 tables, the drop-in classes' default)."""
    import random
    from qrec_amd.engine import BprSgd, DeviceTables
    words = capi.state_from_python(random.Random(1).getstate())
    t0 = time.perf_counter()
    j = capi.mt_bpr_sample_epoch(words, indptr, items, n_items)
    t_sample = time.perf_counter() - t0
    t = DeviceTables(P0.astype(np.float64), Q0.astype(np.float64), np.float64)
    s = BprSgd(t, u, items); s.set_negatives(j)
    capi.device_sync()
    t0 = time.perf_counter()
    s.epoch_ordered(LR0, REG_U, REG_I)            # synchronous: schedule, upload, kernel, loss read back
    dt_single = time.perf_counter() - t0
    # steady state, as the BPR class runs it: the host side of epoch k + 1 (sampler replay, schedule, upload on a side stream)
    # under the kernel of epoch k
    side, n_ep = capi.Stream(), 4
    prep = s.prepare_ordered(j, slot=0, stream=side.handle); side.sync()
    capi.device_sync()
    t0 = time.perf_counter()
    for k in range(n_ep):
        s.run_prepared(prep, LR0, REG_U, REG_I)
        if k + 1 < n_ep:
            j = capi.mt_bpr_sample_epoch(words, indptr, items, n_items)
            prep = s.prepare_ordered(j, slot=(k + 1) & 1, stream=side.handle); side.sync()
        s.epoch_stats()                           # reads the loss terms back: the per-epoch host decision point
    dt = (time.perf_counter() - t0) / n_ep
    return {"value": u.size / dt, "unit": "triplet-updates/s", "dtype": "f64", "epoch_s": dt, "epochs_timed": n_ep,
            "epoch_s_unpipelined": dt_single, "host_sampler_s": t_sample,
            "parity": "index stream bit-exact vs the recorded reference run; P, Q 1e-10, loss 1e-11 (tests/test_gpu_bpr.py)"}


def hbm_resident_roofline(capi, schedule="user", p_update="atomic"):
    """BASELINE config #4, single-GPU slice (U=1.25 M, I=1 M, d=128, 25 M triplets, uniform items): 1.15 GB of tables,
    far beyond the 256 MiB Infinity Cache, so the gather+SGD kernel's traffic is real HBM traffic.
    ``p_update``: one policy, or a tuple of policies timed on the same arrays (a dict keyed by policy is returned)."""
    from qrec_amd.engine import BprSgd, DeviceTables
    rng = np.random.default_rng(0)
    U2, I2, n2, d2 = 1_250_000, 1_000_000, 25_000_000, 128
    u2 = np.sort(rng.integers(0, U2, n2, dtype=np.int32)); i2 = rng.integers(0, I2, n2, dtype=np.int32)
    blk = (rng.random((50_000, d2)) / 3).astype(np.float32)
    P2 = np.empty((U2, d2), np.float32); Q2 = np.empty((I2, d2), np.float32)
    for a in (P2, Q2):
        for k in range(0, a.shape[0], 50_000):
            a[k:k + 50_000] = blk[:min(50_000, a.shape[0] - k)]
    j2 = rng.integers(0, I2, n2, dtype=np.int32)
    t = DeviceTables(P2, Q2, np.float32)
    out = {}
    for pol in ((p_update,) if isinstance(p_update, str) else tuple(p_update)):
        t.upload(P2, Q2)
        s = BprSgd(t, u2, i2, None, schedule=schedule, p_update=pol)
        s.set_negatives(j2)
        e0, e1 = capi.Event(), capi.Event(); ts = []
        with settled_heap(capi):
            for _ in range(5):
                e0.record(); s.epoch_throughput_async(LR0, REG_U, REG_I); e1.record(); e1.sync(); ts.append(e1.elapsed_ms_since(e0))
        ms = float(np.median(ts[1:])); alg = n2 * bytes_per_triplet(d2)
        out[pol] = {"workload": f"BPR d={d2}, {U2}x{I2}, {n2} triplets/epoch, {schedule}-major (config #4 single-GPU slice, tables 1.15 GB)", "schedule": schedule,
                    "p_update": s.p_update, "p_update_requested": pol, "collision_density": s.collision,
                    "bound": "hbm", "achieved": alg / ms / 1e6, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": alg / ms / 1e6 / HBM_PEAK_GBPS,
                    "avg_launch_ms": ms, "algorithmic_bytes_per_launch": alg, "triplet_updates_per_s": n2 / ms * 1e3}
        del s
    return out[p_update] if isinstance(p_update, str) else out


def write_outputs(out_dir: str, P: np.ndarray, Q: np.ndarray, log: np.ndarray, final_lr: float) -> list:
    """--dump-outputs: the timed path's result as <name>.npy.  Tables that do not fit DUMP_BUDGET are cut to the same seeded sample
    of their rows on every run."""
    os.makedirs(out_dir, exist_ok=True)
    out = {"loss": np.ascontiguousarray(log[:, 0], dtype=np.float64), "lr": np.ascontiguousarray(log[:, 1], dtype=np.float64),
           "final_lr": np.array([final_lr], dtype=np.float64)}
    room = DUMP_BUDGET - sum(a.nbytes for a in out.values()) - 4096 * 5          # npy headers
    frac = min(1.0, room / (P.nbytes + Q.nbytes))
    for name, t in (("P", P), ("Q", Q)):
        if frac < 1.0:
            t = t[np.sort(np.random.default_rng(SEED).choice(t.shape[0], int(t.shape[0] * frac), replace=False))]
        out[name] = np.ascontiguousarray(t, dtype=np.float32)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(out)


@contextlib.contextmanager
def settled_heap(capi):
    """A timed region starts with the garbage of the EARLIER legs already gone and runs without the cyclic collector: a DeviceBuffer that
    dies inside a collection is a hipFree, hipFree waits for the device, and freeing another leg's gigabyte tables costs milliseconds --
    paid by whichever leg happens to be allocating Python objects when the collector's counters run over.  (Round 5: the NGCF step of
    `other_configs` read 2.27 ms instead of 0.41 right after the two HBM-resident legs, LightGCN before and SimGCL after it unchanged.)
    Nothing of the timed work is skipped: the collector only ever frees what is unreachable."""
    gc.collect()
    capi.device_sync()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _time_events(capi, fn, reps, warm=3):
    """median of `reps` HIP-event timings (ms) of fn() on the null stream"""
    e0, e1 = capi.Event(), capi.Event()
    ts = []
    with settled_heap(capi):
        for k in range(warm + reps):
            e0.record(); fn(); e1.record(); e1.sync()
            if k >= warm:
                ts.append(e1.elapsed_ms_since(e0))
    return float(np.median(ts))


def other_configs(capi, yelp, budget_s=22.0):
    """SURVEY s8(d) configs #2, #3, #5 and the evaluation, measured HERE by the driver's own run (round 4; rounds 1-3 had them only as
    builder-run files under profiles/): HIP events, >= 20 repetitions each, bounded to ~`budget_s` seconds of wall clock.
      #2  BPR d=64 on the ML-1M shape (6,040 x 3,706, 1,000,209 triplets/epoch): one epoch of the default schedule;
      #3  LightGCN L=3 d=64 batch 2048 at the Yelp2018 shape: the training step (model/ranking/LightGCN.py:27-41) and its
          propagation SpMM alone (algorithmic bytes 8 nnz + 4 (N+1) + 2 N d 4);
      #5  NGCF (2 layers) and SimGCL (L=2, lambda 0.5, eps 0.1) steps at the same shape (NGCF.py:27-41, SimGCL.py:92-111);
      eval  full-rank scoring + mask + top-20 of all 31,668 users against 38,048 items (base/recommender.py:127-179)."""
    from qrec_amd.capi import DeviceBuffer as DB
    from qrec_amd.engine import BprSgd, DeviceTables, balanced_chunk
    from qrec_amd.graph import LightGCNTrainer, NGCFTrainer, SimGCLTrainer, joint_norm_adjacency, unique_first_appearance
    from qrec_amd.interactions import CSR
    from qrec_amd.ranking import DeviceRanker
    from qrec_amd.synth import make_dataset, to_csr
    t_begin = time.perf_counter()
    out, rng = {}, np.random.default_rng(0)
    # ---- config #2
    d = make_dataset("ml1m"); U, I = d["n_users"], d["n_items"]
    indptr, ind = to_csr(U, d["train_u"], d["train_i"])
    u = np.repeat(np.arange(U, dtype=np.int32), np.diff(indptr)).astype(np.int32); n = int(ind.size)
    t = DeviceTables((rng.random((U, DIM)) / 3).astype(np.float32), (rng.random((I, DIM)) / 3).astype(np.float32), np.float32)
    chunk = balanced_chunk(n)
    s = BprSgd(t, u, ind, CSR(indptr, ind), schedule="item", chunk=chunk); s.sample_negatives_device(1, 0)
    ms = _time_events(capi, lambda: s.epoch_throughput_async(LR0, REG_U, REG_I, chunk=chunk, flush_every=FLUSH_EVERY), 20)
    out["bpr_ml1m_shape"] = {"workload": f"BPR d={DIM} ML-1M-shape {U}x{I}, {n} triplets/epoch, item-major", "ms_per_epoch_kernel": ms,
                             "triplet_updates_per_s": n / ms * 1e3, "roofline_frac": n * bytes_per_triplet(DIM) / ms / 1e6 / HBM_PEAK_GBPS, "reps": 20}
    del s, t
    # ---- the Yelp2018-shape graph (configs #3, #5)
    nu, ni = yelp["n_users"], yelp["n_items"]; N = nu + ni
    adj = joint_norm_adjacency(nu, ni, yelp["train_u"], yelp["train_i"])
    nn = int(yelp["train_u"].size); perm = rng.permutation(nn); B = 2048
    hu, hi = yelp["train_u"][perm].astype(np.int32), yelp["train_i"][perm].astype(np.int32)
    hj = rng.integers(0, ni, nn).astype(np.int32)
    du, di, dj = DB.from_numpy(hu), DB.from_numpy(hi), DB.from_numpy(hj)
    U0 = (rng.standard_normal((nu, DIM)) * 0.005).astype(np.float32); V0 = (rng.standard_normal((ni, DIM)) * 0.005).astype(np.float32)

    def step_ms(step, steps=40):
        with settled_heap(capi):
            for k in range(5):
                step(k)
            capi.device_sync()
            e0, e1 = capi.Event(), capi.Event()
            e0.record()
            for k in range(steps):
                step(5 + k)
            e1.record(); e1.sync()
            return e1.elapsed_ms_since(e0) / steps

    tr = LightGCNTrainer(U0, V0, adj, 3, lr=0.001, reg=1e-4)
    ms = step_ms(lambda k: tr.train_step_async(du.ptr + 4 * k * B, di.ptr + 4 * k * B, dj.ptr + 4 * k * B, B))
    spmm_ms = _time_events(capi, lambda: capi.spmm_csr(tr.plan, tr.E, tr.A, tr.ld, d_accum=tr.S), 20)
    nnz = int(tr.plan.nnz); alg = 8 * nnz + 4 * (N + 1) + 2 * N * DIM * 4
    traffic = traffic_c = None
    cfile = os.path.join(ROOT, "profiles", "r06_lightgcn_hbm_counters.json")
    if os.path.exists(cfile):
        cj = json.load(open(cfile))
        traffic = cj.get("yelp2018", {}).get("spmm_forward_with_layer_sum", {}).get("l2_miss_MB_per_launch", 0) * 1e6 or None
        traffic_c = cj.get("yelp2018-clustered", {}).get("spmm_forward_with_layer_sum", {}).get("l2_miss_MB_per_launch", 0) * 1e6 or None
    # the same product on a graph WITH structure (both graphs on the line): the planted-community graph of the same shape
    dc = make_dataset("yelp2018-clustered")
    adj_c = joint_norm_adjacency(dc["n_users"], dc["n_items"], dc["train_u"], dc["train_i"])
    from qrec_amd.graph import SpmmPlan
    plan_c = SpmmPlan(adj_c[0], adj_c[1], adj_c[2], tr.ld, split_row=dc["n_users"])
    spmm_c_ms = _time_events(capi, lambda: capi.spmm_csr(plan_c, tr.E, tr.A, tr.ld, d_accum=tr.S), 20)
    alg_c = 8 * int(plan_c.nnz) + 4 * (N + 1) + 2 * N * DIM * 4
    ACHIEVABLE_GBPS = 6300.0        # /opt/skills/guides/MI355X_MICROARCH.md: ~6.3 TB/s achievable of the 8 TB/s spec
    out["lightgcn_step"] = {"workload": f"LightGCN L=3 d={DIM} batch {B} Yelp2018-shape N={N} nnz={nnz}", "ms_per_step": ms, "steps_timed": 40,
                            "triplets_per_s": B / ms * 1e3, "epoch_s": ms * -(-nn // B) / 1e3,
                            "spmm": {"kernel": "spmm_kernel<16> + spmm_fixup_kernel<16>", "avg_us": spmm_ms * 1e3, "reps": 20, "algorithmic_bytes": alg,
                                     "achieved_GBps": alg / spmm_ms / 1e6, "frac": alg / spmm_ms / 1e6 / HBM_PEAK_GBPS, "bound": "hbm (normalised: the operand is cache resident)",
                                     "traffic": traffic, "traffic_source": "profiles/r06_lightgcn_hbm_counters.json (static: rocprofv3 PMC passes run by the builder on "
                                                                            "this kernel in round 6; bytes past the XCD L2s per launch of THIS launch type, FETCH_SIZE doubled)" if traffic else None,
                                     "graph": "structureless (Zipf degrees, no communities): the worst case for locality",
                                     "on_the_planted_community_graph": {"graph": "yelp2018-clustered: same shape, 64 planted communities, 80 % of a user's edges inside the user's community",
                                                                        "avg_us": spmm_c_ms * 1e3, "algorithmic_bytes": alg_c, "frac": alg_c / spmm_c_ms / 1e6 / HBM_PEAK_GBPS,
                                                                        "traffic": traffic_c, "over_fetch_vs_algorithmic": (traffic_c / alg_c) if traffic_c else None,
                                                                        "roofline_l2miss_frac": (traffic_c / spmm_c_ms / 1e6 / 6300.0) if traffic_c else None},
                                     # the bound the kernel is actually on: every XCD's 4 MiB L2 misses most of the gathered operand, the misses are served by the
                                     # Infinity Cache / HBM side at what that side achieves
                                     "roofline_l2miss": ({"bound": "bytes past the XCD L2s (counters) / live time, against the ~6.3 TB/s the memory side achieves",
                                                          "achieved": traffic / spmm_ms / 1e6, "peak": ACHIEVABLE_GBPS, "unit": "GB/s", "frac": traffic / spmm_ms / 1e6 / ACHIEVABLE_GBPS,
                                                          "over_fetch_vs_algorithmic": traffic / alg} if traffic else None)}}
    del tr, plan_c
    if time.perf_counter() - t_begin < budget_s:
        lim = np.sqrt(6 / 128)
        W = [[rng.uniform(-lim, lim, (DIM, DIM)).astype(np.float32) for _ in range(2)] for _ in range(2)]
        tr = NGCFTrainer(U0, V0, W, adj, 0.002, 1e-3)
        ms = step_ms(lambda k: tr.train_step_async(du.ptr + 4 * k * B, di.ptr + 4 * k * B, dj.ptr + 4 * k * B, B))
        out["ngcf_step"] = {"workload": f"NGCF 2 layers d={DIM} batch {B} keep 0.9 Yelp2018-shape", "ms_per_step": ms, "steps_timed": 40, "triplets_per_s": B / ms * 1e3,
                            "epoch_s": ms * -(-nn // B) / 1e3}
        del tr
    if time.perf_counter() - t_begin < budget_s:
        lim = np.sqrt(6.0 / (nu + DIM))
        tr = SimGCLTrainer(rng.uniform(-lim, lim, (nu, DIM)).astype(np.float32), rng.uniform(-lim, lim, (ni, DIM)).astype(np.float32), adj, 2, 0.001, 1e-4, 0.5, 0.1,
                           max_unique=B)
        steps = 45
        uu = [unique_first_appearance(hu[k * B:(k + 1) * B]) for k in range(steps)]
        vv = [(unique_first_appearance(hi[k * B:(k + 1) * B]) + nu).astype(np.int32) for k in range(steps)]
        duu, dvv = [DB.from_numpy(x) for x in uu], [DB.from_numpy(x) for x in vv]
        ms = step_ms(lambda k: tr.train_step_async(du.ptr + 4 * k * B, di.ptr + 4 * k * B, dj.ptr + 4 * k * B, B, duu[k], uu[k].size, dvv[k], vv[k].size), steps - 5)
        out["simgcl_step"] = {"workload": f"SimGCL L=2 lambda 0.5 eps 0.1 tau 0.2 d={DIM} batch {B} Yelp2018-shape", "ms_per_step": ms, "steps_timed": steps - 5,
                              "triplets_per_s": B / ms * 1e3, "epoch_s": ms * -(-nn // B) / 1e3}
        del tr
    if time.perf_counter() - t_begin < budget_s + 4:
        indptr, ind = to_csr(nu, yelp["train_u"], yelp["train_i"])
        Ue = (rng.random((nu, DIM)) / 3 - 0.1).astype(np.float32); Ve = (rng.random((ni, DIM)) / 3 - 0.1).astype(np.float32)
        rk = DeviceRanker(Ue, Ve, CSR(indptr, ind)); users = np.arange(nu, dtype=np.int32)
        rk.topk(users, 20)                                     # allocates the scratch
        d_users = DB.from_numpy(users)
        ms = _time_events(capi, lambda: capi.score_topk(rk.dU, rk.dV, rk.code, rk.d, rk.ld, ni, d_users, nu, rk.rated[0], rk.rated[1], 20, rk._scratch,
                                                        rk._d_ids, rk._d_sc), 20, warm=2)
        flop = 2.0 * nu * ni * DIM
        out["evaluation"] = {"workload": f"full-rank scoring + mask-to-0 + top-20, {nu} users x {ni} items, d={DIM}, fp32 tables", "gpu_ms": ms, "reps": 20,
                             "nominal_tflops": flop / ms / 1e9, "bound": "mfma",
                             "frac": flop / ms / 1e9 / 2500.0, "peak": 2500.0, "unit": "TFLOP/s (bf16 dense MFMA: where the route spends the nominal flops)",
                             "all_fp32_route_floor_ms": flop / 157.3e12 * 1e3,
                             "note": "nominal flops = 2 x users x items x d.  The fused route spends them in bf16 MFMA (threshold + filter passes over the whole "
                                     "users x items product) and re-scores only the survivors with the fp32 MFMA sequence, so the rate is priced against the bf16 "
                                     "dense peak (`frac`); `all_fp32_route_floor_ms` = what the same product costs at the 157 TF fp32 MFMA peak -- a floor the fused route sits "
                                     "ON, not a utilisation (the fp32-filter route measures 2.4 ms).  "
                                     "ids and scores identical to the block route and the reference's heap procedure (tests/test_gpu_eval.py)"}
    out["seconds"] = time.perf_counter() - t_begin
    return out


def launch_own_ranks(n: int):
    """`python bench.py --gpus N` outside a launcher: become `torch.distributed.run` with N ranks of this very command line
    (exec, so rank 0's single JSON line is the only thing on the caller's stdout and the exit code is the launcher's)."""
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC: RCCL between processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")                   # the launcher would set it anyway, with a warning on stderr
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush(); sys.stderr.flush()
    os.execvpe(cmd[0], cmd, env)


def multi_gpu_recall(capi, qd, control, comm, world, rank, layout, mode, dataset, lr0, epochs, every, shard_batch, syncs):
    """`recall_at_20` of the N > 1 line (strong scaling: the SAME users split over the ranks, so the run is directly comparable to
    order-exact training of the whole problem): every rank trains its block through the real communicator exactly as the timed
    epochs do (tools/paired_recall.train_rank); at the marks the pieces are assembled on rank 0 over the control plane and ranked;
    rank 0 then re-draws every rank's negatives (the sampler is a function of (seed + 7919 rank, epoch, stored order)) and runs the
    reference.  Returns the comparison on rank 0, None elsewhere."""
    from tools import paired_recall as PR
    d = PR.load_dataset(dataset)
    P0, Q0 = PR.initial_tables(d, 3)
    t, sgd, chunk, lo, hi, groups = PR.build_rank(d, mode, world, rank, layout, P0, Q0, shard_batch, syncs)
    marks = set(range(every, epochs + 1, every)) | {epochs}
    rows_p, rows_q = -(-d["n_users"] // world), -(-d["n_items"] // world)
    pad = lambda a, r: np.concatenate([a, np.zeros((r - a.shape[0], a.shape[1]), a.dtype)]) if a.shape[0] < r else a
    rec = {}

    def on_mark(epoch, Pr, Qr):
        allP = control.allgather_host(pad(Pr, rows_p))
        allQ = control.allgather_host(pad(Qr, rows_q)) if layout == "sharded" else None
        if rank == 0:
            Pp = [allP[r][:qd.user_block(d["n_users"], world, r)[1] - qd.user_block(d["n_users"], world, r)[0]] for r in range(world)]
            Qp = [allQ[r] for r in range(world)] if allQ is not None else [Qr]
            rec[epoch] = PR.recall20(*PR.assemble(Pp, Qp, world, layout, d["n_items"]), d)

    log = PR.train_rank(d, sgd, t, chunk, lr0, SEED, epochs, marks, world, rank, comm, layout, on_mark, capi.Stream(), groups=groups)
    control.barrier()
    out = None
    if rank == 0:
        samplers = [sgd] + [PR.build_rank(d, mode, world, r, layout, P0, Q0, shard_batch, syncs)[1] for r in range(1, world)]
        g = {"recall": rec, "loss": [float(x) for x in log[:, 0]], "lr": [float(x) for x in log[:, 1]]}
        ref = PR.reference_run(d, PR.negatives_of(samplers, SEED), lr0, epochs, marks, P0, Q0)
        r = PR.compare({}, g, ref)
        out = {"dataset": dataset, "lr0": lr0, "epochs": epochs, "mode": mode, "ranks": world, "layout": layout,
               "recall": r["peak"]["recall_gpu"], "recall_exact_order": r["peak"]["recall_exact_order"], "peak_epoch": r["peak"]["epoch"],
               "abs_diff": r["peak"]["abs_diff"], "rel_diff": r["peak"]["rel_diff"],
               "final": {k: r["final"][k] for k in ("epoch", "recall_gpu", "recall_exact_order", "abs_diff", "rel_diff", "loss_rel_gap")},
               "worst_mark": {k: r["worst_mark"][k] for k in ("epoch", "abs_diff")}, "bar": r["bar"], "within_bar_at_peak": r["within_bar_at_peak"],
               "same_bold_driver_decisions": r["same_bold_driver_decisions"],
               "harness": "tools/paired_recall.py over the real communicator (same negatives, same tables, same bold driver; reference = order-exact fp64 "
                          "training of the whole problem on rank 0's host)"}
    control.barrier()
    return out


def config4_sharded_leg(capi, qd, control, comm, world, rank, shard_batch, syncs, users=1_250_000, items=1_000_000, triplets=25_000_000, d=128, epochs=3):
    """BASELINE.json config #4 in north_star's layout, on the ranks of THIS run (round 5): every rank holds its own `users` users' rows of P
    and its interleaved 1 / world share of the `items` item rows (d = 128), trains `triplets` triplets per epoch whose items are uniform
    over the WHOLE catalogue, and fetches / returns the distinct item rows of every exchange batch over the communicator
    (qrec_amd/dist.py ShardedItemExchange: per batch an all-to-all of row ids' rows out and of their updates back).  At world 8 this IS
    config #4: 10 M users x 1 M items, 200 M triplets per epoch, 5.6 GB of tables.  Negatives are drawn once on the host (the device
    sampler is the main leg's business); `epochs` timed epochs after one warm-up, barrier + device sync on both sides, max over ranks."""
    from qrec_amd.engine import BprSgd, DeviceTables, balanced_chunk
    rng = np.random.default_rng(4000 + rank)
    u2 = np.sort(rng.integers(0, users, triplets, dtype=np.int32)); i2 = rng.integers(0, items, triplets, dtype=np.int32)
    j2 = rng.integers(0, items, triplets, dtype=np.int32)
    rows_q = len(range(rank, items, world))
    blk = (rng.random((min(50_000, max(users, rows_q)), d)) / 3).astype(np.float32)
    P2 = np.empty((users, d), np.float32); Q2 = np.empty((rows_q, d), np.float32)
    for a in (P2, Q2):
        for k in range(0, a.shape[0], blk.shape[0]):
            a[k:k + blk.shape[0]] = blk[:min(blk.shape[0], a.shape[0] - k)]
    t = DeviceTables(P2, Q2, np.float32)
    del P2, Q2
    n_batches = qd.agree_on_batches(control, triplets, shard_batch, split_from=1 << 19, min_batches=syncs)
    chunk = balanced_chunk(triplets)
    sgd = BprSgd(t, u2, i2, None, schedule="item", n_items=items, batches=n_batches, chunk=chunk)
    sgd.set_negatives(j2)
    step = qd.ShardedStep(comm, qd.ShardedItemExchange(comm, items, t.ld, t.Q), n_batches)
    stream = capi.Stream()
    sgd.start_device_driver(LR0, log_capacity=epochs + 2)
    capi.device_sync()
    pairs = []

    def run(m):
        for _ in range(m):
            pair = (capi.Event(), capi.Event()); pairs.append(pair)
            step.prepare(sgd, stream)
            sgd.epoch_device_async(REG_U, REG_I, MAX_LR, tol=0.0, chunk=chunk, flush_every=FLUSH_EVERY, stream=stream, dist=step, events=pair)

    def sync():
        control.barrier(); stream.sync(); capi.device_sync(); control.barrier()
    gc.collect()          # (the earlier legs' tables go before the clock starts, not inside it)
    run(1); sync()
    moved0 = step.exchange.bytes_moved
    t0 = time.perf_counter(); run(epochs); sync()
    dt = float(control.allreduce_host(np.array([time.perf_counter() - t0]), op="max")[0]) / epochs
    moved = float(control.allreduce_host(np.array([(step.exchange.bytes_moved - moved0) / epochs]))[0])
    kernel_ms = float(np.mean([b.elapsed_ms_since(a) for a, b in pairs[1:]]))
    per_rank = control.allgather_host(np.array([kernel_ms]))[:, 0]
    loss = float(sgd.driver_log()[-1, 0])
    alg = triplets * bytes_per_triplet(d)
    out = {"workload": f"BPR d={d}, {world} x {users} users x {items} items, {world} x {triplets} triplets/epoch; item table row-sharded x{world} "
                       f"({rows_q} rows = {rows_q * t.ld * 4 / 1e6:.0f} MB per rank), {n_batches} exchange batches per epoch and rank"
                       + (" = BASELINE config #4" if (world, users, items, triplets, d) == (8, 1_250_000, 1_000_000, 25_000_000, 128) else ""),
           "ms_per_epoch": dt * 1e3, "triplet_updates_per_s_job": world * triplets / dt, "batches_per_epoch": n_batches,
           "bytes_leaving_all_ranks_per_epoch": moved, "bytes_leaving_one_rank_per_triplet": moved / world / triplets,
           "epoch_ms_per_rank_by_events": {"min": float(per_rank.min()), "max": float(per_rank.max()), "all": [float(x) for x in per_rank],
                                           "what": "HIP events around a rank's whole epoch on its stream: SGD batches + gathers + exchanges + applies"},
           "algorithmic_GBps_per_rank": alg / dt / 1e9, "frac_of_8TBps_per_rank": alg / dt / 1e9 / HBM_PEAK_GBPS,
           "predicted_link_ms_per_epoch": {"all_links_1071GBps": moved / world / 1071e9 * 1e3, "one_link_153GBps": moved / world / 153e9 * 1e3,
                                           "what": "bytes leaving one rank per epoch / link rate; arithmetic, not measured"},
           "final_loss_rank0": loss, "negatives": "uniform, drawn once on the host", "epochs_timed": epochs}
    del sgd, step, t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", default="yelp2018")
    ap.add_argument("--min-seconds", type=float, default=0.3, help="epochs are repeated inside a step until the timed region lasts this long")
    ap.add_argument("--epochs-per-step", type=int, default=0, help="fix the inner repeat instead of calibrating it")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every other leg of the line: CPU baselines, exact_mode, recall_at_20, other_configs, "
                         "roofline_hbm_resident; N > 1: the weak-scaling leg, the other item-table layout, config4_sharded (off: the headline alone)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip exact_mode / roofline_hbm_resident / recall_at_20 / other_configs / the weak-scaling leg")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=0, help="triplets per work item of the SGD kernel (0 = engine.balanced_chunk: the length in 26..40 that spreads the "
                                                         "epoch's chunks most evenly over the persistent groups)")
    ap.add_argument("--flush-every", type=int, default=0, help="item-major schedule: triplets between flushes of the register-resident Q[i] (0 = default)")
    ap.add_argument("--schedule", choices=("item", "user"), default="item",
                    help="visiting order of the epoch's triplets in the Hogwild kernel (DESIGN.md s4)")
    ap.add_argument("--p-update", choices=("auto", "atomic", "rmw"), default="auto",
                    help="item-major: how P[u] is written -- atomic delta, sc1 load + store, or by the collision density (engine.resolve_p_update; "
                         "the Yelp2018 shape resolves to atomic)")
    ap.add_argument("--dist-mode", choices=("replicated", "sharded"), default=os.environ.get("QREC_DIST_MODE", "replicated"))
    ap.add_argument("--scaling", choices=("strong", "weak"), default="strong",
                    help="N > 1.  strong (default; BASELINE.json quotes the metric on THE Yelp2018 shape at 1/2/4/8 GPUs): the same 31,668 users "
                         "split over the ranks -- `value`; a weak-scaling leg (every rank its own 31,668 users: an N x 31,668-user problem) is "
                         "timed next to it and reported as `weak_scaling`.  weak: that leg alone, as `value`, labelled with its aggregate shape")
    ap.add_argument("--sync-per-epoch", type=int, default=int(os.environ.get("QREC_REPLICATED_SYNCS", "0")),
                    help="reconciliations of the ranks' item rows per epoch: delta all-reduces of the replicated layout, minimum number of exchange "
                         "batches of the sharded one.  0 = dist.reconciliations_per_epoch: 1 up to two ranks, 2 beyond (the smallest count whose paired "
                         "Recall@20 runs stay inside +-0.002 at the peak and at the last epoch: the table in that function's docstring); "
                         "1 = the epoch close's fused all-reduce alone")
    ap.add_argument("--recall-dataset", default="auto", help="N > 1: dataset of the Recall@20 leg (auto: yelp2018-clustered for the Yelp2018 shape)")
    ap.add_argument("--recall-epochs", type=int, default=0, help="epochs of that leg (0: 40 at BPR.conf's rate on the clustered graph, else 25)")
    ap.add_argument("--shard-batch", type=int, default=1 << 20,
                    help="sharded mode: triplets per exchange batch and rank (2^20: at most 2^21 distinct item rows in a rank's cache, 1 GiB at "
                         "d = 128; an epoch of 2^19 triplets or more is split into at least two batches, so that the next epoch's plan hides "
                         "in front of the last one)")
    ap.add_argument("--config4-triplets", type=int, default=-1,
                    help="N > 1: triplets per epoch and rank of the `config4_sharded` leg (its users and items scale along: 25 M = BASELINE config "
                         "#4's share of one of 8 GPUs = the default; the one-device functional tests default to 0 and pass a small number; 0 skips it)")
    ap.add_argument("--shard-pipeline", action="store_true",
                    help="sharded mode: fetch batch k + 1 under batch k's SGD kernel, on a second stream and communicator (one more batch of "
                         "staleness).  Off by default: at the Yelp2018 shape the fetch is 10 MB per batch and the gather/copy kernels "
                         "running beside the atomic-bound SGD grid cost it more than they hide (world 1: 0.85 vs 0.75 ms/epoch, "
                         "profiles/r03_sharded_world1.json); it is for shapes whose exchange outlasts the batch's SGD (config #4)")
    ap.add_argument("--no-shard-pipeline", action="store_true", help="(accepted for compatibility: the default)")
    ap.add_argument("--no-plan-inside", action="store_true",
                    help="sharded mode: plan every epoch at its own start, with the host waiting for the stream to run dry (default: the "
                         "next epoch's plan is enqueued in front of the current epoch's last batch, its row counts read back behind an event)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's trained tables, per-epoch loss and learning rate as DIR/<name>.npy "
                         "(one process only; the epochs per step then follow from the arguments, not from a clock calibration)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and (args.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        ap.error("--dump-outputs writes one process's tables: run it with --gpus 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_own_ranks(args.gpus)           # does not return

    # stdout carries ONE line, the result.  Libraries print there too -- RCCL writes its version banner to C stdio's
    # stdout, flushed at exit, i.e. AFTER a Python print -- so file descriptor 1 is pointed at stderr for the whole run and
    # the JSON line goes to the saved original descriptor at the end.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and args.gpus > 1:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} ranks")
    # QREC_FORCE_DIST=1 drives the multi-GPU branch with world size 1 (the gpurun boxes have one GPU): same code path
    # as N > 1 -- delta / apply kernels, the real RCCL communicator -- the collectives degenerate to copies.
    use_dist = world > 1 or os.environ.get("QREC_FORCE_DIST") == "1"
    # Test hook for the 1-GPU development boxes: QREC_DIST_TEST_ONE_DEVICE=1 puts every rank on device 0 with the staged
    # gloo transport (RCCL refuses two ranks on one device).  Not a bench result; the output line says so.
    one_device = os.environ.get("QREC_DIST_TEST_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    control = comm = qd = None
    from qrec_amd import capi
    capi.load()       # BEFORE torch is imported: libqrec_hip.so then binds /opt/rocm's HIP runtime (and, next to it, its librccl)
                      # and not the older one bundled with torch, on which the sampler's side stream does not overlap the
                      # SGD kernel (measured: 0.67 vs 0.61 ms per epoch).  torch is the CPU control plane only.
    if use_dist:
        from qrec_amd import dist as qd
        control = qd.ControlPlane.from_env()
    from qrec_amd.capi import DeviceBuffer
    from qrec_amd.engine import BprSgd, DeviceTables, balanced_chunk
    from qrec_amd.interactions import CSR
    from qrec_amd.synth import make_dataset, to_csr
    capi.init(local_rank)
    if use_dist:
        with qd.watchdog(f"rank {rank} of {world}: creating the RCCL communicator (ncclCommInitRank waits for ALL ranks)", float(os.environ.get("QREC_PREFLIGHT_TIMEOUT", "90"))):
            comm = qd.make_comm(control)
    # first contact with the communicator, before anything is timed: a tiny all-reduce and a ragged all-to-all round trip, checked, under a
    # watchdog -- a wrong value raises, a hang ends the process with one line on stderr (qrec_amd/dist.py preflight)
    pre = qd.preflight(comm, stream=None, timeout_s=float(os.environ.get("QREC_PREFLIGHT_TIMEOUT", "90"))) if use_dist else None

    # ---- workload: resident in HBM before timing ------------------------------------------
    data = make_dataset(args.shape)
    U, I = data["n_users"], data["n_items"]
    indptr, items = to_csr(U, data["train_u"], data["train_i"])
    u = np.repeat(np.arange(U, dtype=np.int32), np.diff(indptr)).astype(np.int32)
    n_full = int(items.size)
    Q0 = (np.random.default_rng(999).random((I, DIM)) / 3).astype(np.float32)    # same on all ranks
    sharded = use_dist and args.dist_mode == "sharded"
    flush_every = args.flush_every or FLUSH_EVERY
    extra_comms = []
    # The step's kernels and collectives run on an explicit non-blocking stream, not the null stream: the legacy null
    # stream synchronises implicitly with every blocking stream of the process, and an RCCL communicator brings its own --
    # measured at world 1 (QREC_FORCE_DIST=1): 0.670 ms/epoch on the null stream, 0.626 on this one, 0.610 with no
    # communicator in the process at all.
    main_stream = capi.Stream()

    def sync_all():
        if use_dist:
            control.barrier()
        capi.device_sync()          # hipDeviceSynchronize on the runtime all of this process's GPU work runs on
        if use_dist:
            control.barrier()

    layout_of_the_line = sharded

    def run_leg(strong: bool, steps: int, warmup: int, min_seconds: float, dump: bool, layout_sharded: bool | None = None):
        """one timed run: warm-up steps, then EXACTLY `steps` steps between barrier + device sync on both sides, max over ranks.
        ``layout_sharded``: the item table's layout for THIS leg (None = the line's own, --dist-mode)"""
        sharded = layout_of_the_line if layout_sharded is None else (layout_sharded and use_dist)
        if strong and world > 1:     # the SAME users split over the ranks: rank r trains the r-th contiguous block (qrec_amd/dist.py)
            lo, hi, l_indptr, l_items = qd.shard_positive_csr(indptr, items, world, rank)
            l_u = np.repeat(np.arange(hi - lo, dtype=np.int32), np.diff(l_indptr)).astype(np.int32)
            P0 = (np.random.default_rng(1000).random((U, DIM)) / 3).astype(np.float32)[lo:hi]
        else:          # one GPU -- or weak scaling: every rank its own population of U users with the same interaction structure
            l_indptr, l_items, l_u = indptr, items, u
            P0 = (np.random.default_rng(1000 + rank).random((U, DIM)) / 3).astype(np.float32)   # rand/3, iterativeRecommender.py:37-38
        n = int(l_items.size)
        Q0_local = qd.shard_item_rows(Q0, world, rank) if sharded else Q0
        tables = DeviceTables(P0, Q0_local, np.float32)
        CHUNK = args.chunk or balanced_chunk(n)     # triplets per work item: the count that spreads evenly over the 4,096 persistent groups
        syncs = qd.reconciliations_per_epoch(world, args.sync_per_epoch) if use_dist else 1
        if sharded:
            n_batches = qd.agree_on_batches(control, n, args.shard_batch, split_from=1 << 19, min_batches=syncs)
        else:
            n_batches = syncs
        sgd = BprSgd(tables, l_u, l_items, CSR(l_indptr, l_items), schedule=args.schedule, n_items=I, batches=n_batches, chunk=CHUNK, p_update=args.p_update)
        # one launch per epoch: at least 8 rounds of the persistent grid whatever the epoch's size (engine.grid_for_epoch; nothing changes at
        # the Yelp2018 shape's 1.25 M triplets, a two-rank share of it runs chunks of 16)
        CHUNK, GROUPS = (CHUNK, 0) if args.chunk else sgd.launch_grid()
        sampler_seed = SEED + 7919 * rank
        dstep = None
        if use_dist and sharded:
            pipe = None
            if args.shard_pipeline and not args.no_shard_pipeline:
                # a second communicator for the fetch stream: two collectives of ONE communicator must not be in flight on two streams
                pipe = (comm if one_device else qd.make_comm(control), capi.Stream())
            extra_comms.extend(x[0] for x in (pipe,) if x is not None and x[0] is not comm)
            dstep = qd.ShardedStep(comm, qd.ShardedItemExchange(comm, I, tables.ld, tables.Q, pipeline=pipe), n_batches,
                                   plan_inside=not args.no_plan_inside)
        elif use_dist:
            dstep = qd.ReplicatedStep(comm, qd.ReplicatedTableSync(comm, tables.Q))
        # device copies of the initial state: every step restarts training from it (see step())
        d_P0, d_Q0 = DeviceBuffer.from_numpy(tables._pad(P0)), DeviceBuffer.from_numpy(tables._pad(Q0_local))
        ev, pool = [], []
        counter = {"epoch": 0}
        main = main_stream

        def epoch():
            """sampler (side stream) | SGD kernel -> [N > 1: collectives] -> epoch close (BPR.py:40 loss terms, isConverged,
            updateLearningRate) all on the device; the host only enqueues (sharded mode: plus ONE read-back of the exchange's
            row counts per epoch).  tol = 0: every epoch runs."""
            k = counter["epoch"]; counter["epoch"] += 1
            pair = pool.pop() if pool else (capi.Event(), capi.Event())
            ev.append(pair)
            sgd.take_prefetched_negatives(k, main)                      # BPR.py:35-37 (sampled under epoch k-1)
            if sharded:
                dstep.prepare(sgd, main)
                # the next epoch's sampler is enqueued from inside (same place on the device: behind the start event) -- the
                # epoch's last batch is preceded by the next epoch's plan, which waits for those negatives
                sgd.epoch_device_async(REG_U, REG_I, MAX_LR, tol=0.0, chunk=CHUNK, variant=args.variant, stream=main, flush_every=flush_every,
                                       events=pair, dist=dstep, after_start=lambda: sgd.prefetch_negatives_device(sampler_seed, k + 1))
                return
            sgd.epoch_device_async(REG_U, REG_I, MAX_LR, tol=0.0, chunk=CHUNK, variant=args.variant, stream=main,
                                   flush_every=flush_every, events=pair, dist=dstep, groups=GROUPS)   # BPR.py:45-53,40 + iterativeRecommender.py:88-104
            sgd.prefetch_negatives_device(sampler_seed, k + 1)          # side stream, under the SGD kernel

        def restart():
            """Every step is a fresh training run of `inner` epochs from the initial tables and learning rate (device-to-
            device copies inside the timed region -- extra work, not skipped work): the bold driver (BPR.conf: -max 1) halves
            the rate whenever sampling noise raises the loss, so a single run of many hundred epochs ends at a vanishing
            rate, while the reference trains 100 epochs at most; this keeps every timed epoch in the regime of a real run."""
            capi.memcpy_d2d(tables.P, d_P0, d_P0.nbytes, main); capi.memcpy_d2d(tables.Q, d_Q0, d_Q0.nbytes, main)
            if dstep is not None and dstep.mode == "replicated":
                capi.memcpy_d2d(dstep.sync_q.start, d_Q0, d_Q0.nbytes, main)
            capi.memcpy_d2d(sgd.d_drv, d_drv0, d_drv0.nbytes, main)

        # calibration: how many epochs make a step, so that K steps last >= --min-seconds (same on every rank)
        cal, inner_max = 5, 400
        sgd.start_device_driver(LR0, log_capacity=args.epochs_per_step or inner_max)
        d_drv0 = DeviceBuffer.from_numpy(sgd.d_drv.numpy())
        capi.device_sync()            # set-up work sits on the null stream; the epochs run on `main`
        sgd.prefetch_negatives_device(sampler_seed, 0)
        epoch(); epoch(); sync_all()
        t0 = time.perf_counter()
        for _ in range(cal - 2):
            epoch()
        sync_all()
        t_epoch = (time.perf_counter() - t0) / (cal - 2)
        if args.epochs_per_step:
            inner = args.epochs_per_step
        elif dump and args.dump_outputs:       # the outputs must not depend on the clock: nominal epochs, not the measured ones
            inner = min(inner_max, max(1, math.ceil(round(min_seconds / (steps * NOMINAL_EPOCH_S), 6))))
        else:
            inner = min(inner_max, max(1, math.ceil(min_seconds / (steps * t_epoch))))
            if use_dist:
                inner = int(control.allreduce_host(np.array([inner], dtype=np.int64), op="max")[0])

        def step():
            restart()
            for _ in range(inner):
                epoch()

        pool.extend((capi.Event(), capi.Event()) for _ in range((warmup + steps) * inner))   # not inside the timed loop
        with settled_heap(capi):      # an earlier leg's tables (the N > 1 line times two legs) are freed before the clock starts, not inside it
            for _ in range(warmup):
                step()
            sync_all()
            first_timed = counter["epoch"]
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            sync_all()
            elapsed = time.perf_counter() - t0
        if use_dist:
            elapsed = float(control.allreduce_host(np.array([elapsed]), op="max")[0])
        total = counter["epoch"]
        drv = sgd.driver_state()
        if drv["failed"]:
            raise SystemExit("Loss = NaN or Infinity")            # iterativeRecommender.py:84-86
        assert drv["epochs"] == inner and not drv["converged"], drv
        log = sgd.driver_log()
        if dump and os.environ.get("QREC_DIST_TEST_DUMP"):     # functional tests: every rank leaves its tables and its driver log behind
            np.savez(os.path.join(os.environ["QREC_DIST_TEST_DUMP"], f"rank{rank}.npz"), Q=tables.Q.numpy(), P=tables.P.numpy(),
                     log=log, lr=drv["lr"], epochs_per_step=inner)
        dumped = None
        if dump and args.dump_outputs:        # after the clock: the last step's result, as its caller receives it
            P, Q = tables.download(np.float32)
            dumped = write_outputs(args.dump_outputs, P, Q, log, drv["lr"])
        kernel_ms = [ev[k][1].elapsed_ms_since(ev[k][0]) for k in range(first_timed, total)]
        leg = {"n": n, "chunk": CHUNK, "inner": inner, "elapsed": elapsed, "steps": steps, "final_loss": float(log[-1, 0]), "final_lr": drv["lr"],
               "avg_kernel_ms": float(np.mean(kernel_ms)), "n_batches": n_batches, "q_floats": int(tables.Q.nbytes // 4), "moved": None,
               "fetch_pipelined": False, "plan": None, "ld": tables.ld, "P0": P0, "p_update": sgd.p_update, "collision_density": sgd.collision,
               "dumped": dumped}
        if sharded:
            leg["moved"] = float(control.allreduce_host(np.array([dstep.exchange.bytes_moved / max(total, 1)]))[0])
            leg["fetch_pipelined"] = dstep.exchange.pipeline is not None
            leg["plan"] = ("ahead, on a plan stream" if dstep.exchange.plan_ahead is not None else
                           "inside the previous epoch, in front of its last batch" if dstep.plan_inside and dstep.n_batches >= 2 else "at the epoch's start")
        return leg

    strong = args.scaling == "strong" and world > 1
    extras = args.full and not args.no_extras          # the same on every rank: the N > 1 legs below are collective
    leg = run_leg(strong, args.steps, args.warmup, args.min_seconds, dump=True)
    n, CHUNK, inner, elapsed, avg_kernel_ms = leg["n"], leg["chunk"], leg["inner"], leg["elapsed"], leg["avg_kernel_ms"]
    weak_leg = None
    if strong and extras:       # the weak-scaling figure next to it: every rank its own U users (an N x U-user problem)
        weak_leg = run_leg(False, max(2, args.steps // 2), 1, args.min_seconds / 2, dump=False)
    # north_star's layout as a first-class figure of the same line: the SAME strong-scaling problem with the item table
    # row-sharded and a per-batch all-to-all -- `value_sharded` beside `value` (which runs the replicated layout unless --dist-mode says otherwise)
    other_layout_leg = None
    if use_dist and world > 1 and strong and extras:
        other_layout_leg = run_leg(True, max(2, args.steps // 2), 1, args.min_seconds / 2, dump=False, layout_sharded=not sharded)
    alg_bytes = n * bytes_per_triplet(DIM)
    moved = leg["moved"]
    multi = None
    if use_dist:
        # what the run looked like from every rank: the SGD kernel's mean launch time per rank (HIP events on the rank's own
        # stream) and what RCCL itself reports for the communicator (ncclCommCount / UserRank / CuDevice)
        q = comm.query() if hasattr(comm, "query") else {"ranks": comm.world, "rank": comm.rank, "device": local_rank}
        per_rank = control.allgather_host(np.array([avg_kernel_ms, float(q["ranks"]), float(q["rank"]), float(q["device"]), float(n)]))
        lib = None
        if hasattr(comm, "query"):
            path, ver = capi.comm_library()
            lib = {"library": path, "version": ver}
        payload = None if sharded else leg["q_floats"] * 4 + 24          # the fused all-reduce: item-table deltas + 3 fp64 loss terms
        syncs = leg["n_batches"] if not sharded else None
        inner_payload = payload                                                  # an inner reconciliation covers the whole table too
        # link-time arithmetic for the collectives of one epoch (NOT a measurement): a ring all-reduce moves 2 (G-1)/G x payload over
        # each rank's links; xGMI is point-to-point, 7 links x ~153 GB/s per GPU (MI355X_MICROARCH.md) -- one ring uses one link per
        # direction, a fully connected 8-GPU node can run up to 7 rings side by side
        wire = (2.0 * (world - 1) / world * (payload + (syncs - 1) * inner_payload)) if (payload and world > 1) else 0.0
        predicted = None if sharded else {"one_ring_153GBps": wire / 153e9 * 1e3, "seven_rings_1071GBps": wire / 1071e9 * 1e3,
                                          "what": "ring all-reduce wire bytes per rank and epoch / link rate; arithmetic, not measured"}
        if sharded and moved is not None and world > 1:
            predicted = {"all_links_1071GBps": moved / world / 1071e9 * 1e3, "one_link_153GBps": moved / world / 153e9 * 1e3,
                         "what": "bytes leaving one rank per epoch / link rate; arithmetic, not measured"}
        # the line is only a multi-GPU line if RCCL says so: every rank in a communicator of `world` ranks, every rank on its own device
        # (the one-device functional test shares device 0 over the staged transport and says so in the line)
        devices = [int(x) for x in per_rank[:, 3]]
        if not one_device and (int(per_rank[:, 1].min()) != world or int(per_rank[:, 1].max()) != world or len(set(devices)) != world):
            raise SystemExit(f"bench.py --gpus {world}: the communicator reports {sorted(set(int(x) for x in per_rank[:, 1]))} ranks on devices {devices}; "
                             f"expected {world} ranks on {world} distinct devices -- no line is printed for a run that was not what it claims to be")
        multi = {"preflight": pre, "rccl_ranks": int(per_rank[:, 1].min()), "rccl_ranks_agree": bool((per_rank[:, 1] == per_rank[0, 1]).all()),
                 "rank_devices": [int(x) for x in per_rank[:, 3]], "rccl": lib,
                 "transport": "rccl" if hasattr(comm, "query") else type(comm).__name__,
                 "kernel_ms_per_rank": {"min": float(per_rank[:, 0].min()), "max": float(per_rank[:, 0].max()),
                                        "all": [float(x) for x in per_rank[:, 0]]},
                 "triplets_per_epoch_per_rank": [int(x) for x in per_rank[:, 4]],
                 "collectives_per_epoch": ({"all_to_all_batches": leg["n_batches"], "calls": 3 * leg["n_batches"] + 1,
                                            "bytes_leaving_all_ranks": moved} if sharded else
                                           {"all_reduce": syncs, "payload_bytes_per_rank": payload,
                                            "inner_payload_bytes_per_rank": inner_payload,
                                            "ring_wire_bytes_per_rank": wire}),
                 "predicted_link_ms_per_epoch": predicted}

    recall_multi, recall_ran = None, False                # recall_multi is rank 0's; recall_ran is the same on every rank
    if world > 1 and strong and extras:      # every rank takes part
        ds = args.recall_dataset
        if ds == "auto":
            ds = "yelp2018-clustered" if args.shape == "yelp2018" else (args.shape if data["test_u"].size else None)
        if ds is not None:
            recall_ran = True
            ep = args.recall_epochs or (40 if ds == "yelp2018-clustered" else 25)
            recall_multi = multi_gpu_recall(capi, qd, control, comm, world, rank, args.dist_mode if use_dist else "replicated", args.schedule, ds,
                                            LR0, ep, 5, args.shard_batch, qd.reconciliations_per_epoch(world, args.sync_per_epoch))

    config4 = None
    if args.config4_triplets < 0:
        args.config4_triplets = 0 if one_device else 25_000_000
    if world > 1 and extras and args.config4_triplets > 0:      # every rank takes part
        scale = args.config4_triplets / 25_000_000
        config4 = config4_sharded_leg(capi, qd, control, comm, world, rank, args.shard_batch, qd.reconciliations_per_epoch(world, args.sync_per_epoch),
                                      users=max(1000, int(1_250_000 * scale)), items=max(1000, int(1_000_000 * scale)), triplets=args.config4_triplets)
        if strong and recall_ran and args.dist_mode != "sharded":      # (a condition every rank evaluates alike: the leg is collective)
            # ... and the Recall@20 of THAT layout: the paired run of the strong-scaling leg again with the item table row-sharded (at config
            # #4's own size a CPU reference is 30 s per epoch: the layout is judged at the Yelp2018 shape, like the replicated one)
            # (the dataset and epochs the first Recall leg resolved, not a second resolution of "auto")
            rs = multi_gpu_recall(capi, qd, control, comm, world, rank, "sharded", args.schedule, ds, LR0, ep, 5,
                                  args.shard_batch, qd.reconciliations_per_epoch(world, args.sync_per_epoch))
            if rank == 0:
                config4["recall_at_20_of_the_layout"] = rs

    if rank == 0:
        n_job = n_full if (strong or world == 1) else world * n
        value = n_job * args.steps * inner / elapsed
        achieved = alg_bytes / (avg_kernel_ms * 1e-3) / 1e9
        traffic = None
        tfile = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if os.path.exists(tfile) and not sharded:
            tj = json.load(open(tfile))
            if tj.get("workload") == f"bpr-{args.shape}-d{DIM}-{args.schedule}":
                traffic = tj.get("bytes_per_launch")
        kernel = {"item": "bpr_hogwild_item_kernel<16,4>" + (" (P[u] by sc1 load + store)" if leg.get("p_update") == "rmw" else ""),
                  "user": "bpr_hogwild_kernel<16,4,plain-load,atomic>"}[args.schedule]
        shape_name = "Yelp2018-shape" if args.shape == "yelp2018" else args.shape
        if world == 1:
            par = "1 GPU" + (f" (QREC_FORCE_DIST: {args.dist_mode} multi-GPU path at world 1)" if use_dist else "")
            workload = f"BPR d={DIM} {shape_name} {U}x{I}"
        else:
            how = (f"item table row-sharded x{world}: per-batch RCCL all-to-all of distinct rows + their updates" if sharded else
                   f"item table replicated: {leg['n_batches']} fused RCCL all-reduce(s) of deltas (+ loss terms) per epoch")
            if strong:
                par = f"the {U} users split x{world}, {how}"
                workload = f"BPR d={DIM} {shape_name} {U}x{I} (strong scaling: the one problem over {world} GPUs)"
            else:
                par = f"{world} x {U} users (every rank its own population), {how}"
                workload = f"BPR d={DIM} {world}x{U} users x {I} items = {world * U}x{I}, {world * n} triplets/epoch (weak scaling of the {shape_name} per GPU)"
        out = {
            **({"INVALID_AS_BENCH": "QREC_DIST_TEST_ONE_DEVICE: all ranks shared one GPU over gloo (functional test only)"} if one_device else {}),
            "metric": "BPR triplet-updates/sec", "value": value, "unit": "triplet-updates/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if (strong or world == 1) else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": workload,
                       "mode": f"throughput: device Philox sampler + Hogwild atomic-delta SGD, {args.schedule}-major",
                       "p_update": leg["p_update"], "collision_density": leg["collision_density"],
                       "triplets_per_epoch_per_gpu": n, "triplets_per_epoch_job": n_job, "epochs_per_step": inner,
                       "step": f"a fresh {inner}-epoch training run from the initial tables and learning rate", "ms_per_epoch": elapsed / (args.steps * inner) * 1e3,
                       "timed_seconds": elapsed, "chunk": CHUNK, "parallelism": par,
                       "lr": LR0, "reg": REG_U, "final_loss": leg["final_loss"], "final_lr": leg["final_lr"],
                       "epoch_close": "device (no host sync inside the timed region)" if not sharded else "device; one row-count read-back per epoch for the exchange",
                       "dist_mode": args.dist_mode if use_dist else None,
                       **({"xgmi_bytes_per_epoch_all_ranks": moved, "batches_per_epoch": leg["n_batches"],
                           "fetch_pipelined": leg["fetch_pipelined"], "plan": leg["plan"]} if sharded else {})},
            **({"multi_gpu": multi} if multi is not None else {}),
            **({"dumped_outputs": {"dir": args.dump_outputs, "arrays": leg["dumped"]}} if leg["dumped"] else {}),
            "roofline": {"bound": "hbm", "kernel": kernel,
                         "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic,
                         "traffic_source": ("profiles/hbm_traffic.json: rocprofv3 PMC passes of this command run by the builder (static; "
                                            "not re-measured in this run)") if traffic is not None else None,
                         "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": avg_kernel_ms,
                         "note": ("events bracket the epoch's batches incl. their exchanges" if (sharded or (use_dist and leg["n_batches"] > 1)) else
                                  "tables (17.8 MB) are cache resident at this shape; bound = L2 atomic units, see DESIGN.md"),
                         **({"atomic_unit_floor_static": {"ms": 0.547, "of_this_kernel": 0.547 / avg_kernel_ms, "source": "profiles/r03_ubench_atomics4.txt "
                                                          "(static, builder-measured in round 3, not re-measured in this run): the item-major epoch's two atomic row "
                                                          "updates per triplet ALONE, no loads, no arithmetic = 308 G dword atomics/s = one dword per clock on each of "
                                                          "the 128 L2 channels"}}
                            if args.schedule == "item" and args.shape == "yelp2018" and not use_dist else {})},
        }
        if weak_leg is not None:
            wv = world * weak_leg["n"] * weak_leg["steps"] * weak_leg["inner"] / weak_leg["elapsed"]
            out["weak_scaling"] = {"value": wv, "unit": "triplet-updates/s", "workload": f"BPR d={DIM} {world}x{U} users x {I} items = {world * U}x{I}, "
                                   f"{world * weak_leg['n']} triplets/epoch: every rank its own {U}-user population (NOT the Yelp2018 problem: {world} of them side by side)",
                                   "ms_per_epoch": weak_leg["elapsed"] / (weak_leg["steps"] * weak_leg["inner"]) * 1e3, "steps": weak_leg["steps"],
                                   "epochs_per_step": weak_leg["inner"], "kernel_ms": weak_leg["avg_kernel_ms"]}
        if other_layout_leg is not None:
            ol = other_layout_leg
            key = "value_replicated" if sharded else "value_sharded"
            out[key] = {"value": n_full * ol["steps"] * ol["inner"] / ol["elapsed"], "unit": "triplet-updates/s",
                        "layout": ("item table replicated, delta all-reduce per reconciliation" if sharded else
                                   f"item table row-sharded x{world}, per-batch RCCL all-to-all of distinct rows + their updates (north_star's layout)"),
                        "workload": f"the same strong-scaling problem: BPR d={DIM} {shape_name} {U}x{I} over {world} GPUs",
                        "ms_per_epoch": ol["elapsed"] / (ol["steps"] * ol["inner"]) * 1e3, "steps": ol["steps"], "epochs_per_step": ol["inner"],
                        "kernel_ms": ol["avg_kernel_ms"], "batches_per_epoch": ol["n_batches"],
                        **({"xgmi_bytes_per_epoch_all_ranks": ol["moved"]} if ol["moved"] is not None else {})}
        if recall_multi is not None:
            out["recall_at_20"] = recall_multi
        if config4 is not None:
            out.setdefault("other_configs", {})["config4_sharded"] = config4
        if world == 1 and not use_dist:
            if args.full and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(u, items, indptr, I, U)
                out["vs_cpu_port"] = value / out["cpu_baseline"]["value"]
                out["vs_reference_loop_here"] = value / out["cpu_baseline"]["reference_loop_here"]["value"]
            if extras:
                out["recall_at_20"] = recall_legs(args.schedule, args.shape)
                out["exact_mode"] = exact_mode_rate(capi, u, items, indptr, I, leg["P0"], Q0)
                # the HBM-resident slice of config #4 (1.15 GB of tables: real HBM traffic) under what `auto` resolves to at that size: item-major,
                # P[u] written by sc1 load + store where users rarely collide (engine.resolve_p_update: collision density 0.003 there) -- and, beside
                # it, the same slice with atomic deltas (what rounds 1-5 ran)
                from qrec_amd.engine import P_RMW_MAX_COLLISION, resolve_schedule
                sch, _ = resolve_schedule(25_000_000, None)
                both = hbm_resident_roofline(capi, schedule=sch, p_update=("auto", "atomic"))
                out["roofline_hbm_resident"] = both["auto"]
                out["roofline_hbm_resident"]["chosen_by"] = (f"engine.resolve_schedule + engine.resolve_p_update (QREC_SCHEDULE / QREC_P_UPDATE = auto): "
                                                             f"load + store where groups x sum_u p_u^2 <= {P_RMW_MAX_COLLISION}")
                out["roofline_hbm_resident"]["recall_at_20_at_this_size"] = {
                    "source": "profiles/r06_item_rmw.json (builder-measured in round 6, tools/paired_recall.py: xl25m-clustered, 650 k users, 25.3 M triplets per epoch, "
                              "d = 128, collision density 0.008, against order-exact fp64 training on the same negatives; static here)",
                    "abs_diff_peak_and_last_epoch": {"lr0 0.01, 30 epochs, load + store": [0.0010, 0.0002], "lr0 0.05, 12 epochs, load + store": [0.0011, 0.0002],
                                                     "lr0 0.01, 30 epochs, atomic deltas": [0.0008, 0.0002], "lr0 0.05, 12 epochs, atomic deltas": [0.0010, 0.0003]},
                    "bar": 0.002}
                out["roofline_hbm_resident_atomic"] = both["atomic"]
                if args.shape == "yelp2018":
                    out["other_configs"] = other_configs(capi, data)
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if use_dist:
        control.barrier()
        for extra in extra_comms:
            extra.destroy()
        if comm is not None:
            comm.destroy()
        control.shutdown()


if __name__ == "__main__":
    main()
