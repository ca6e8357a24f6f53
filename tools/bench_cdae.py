#!/usr/bin/env python3
"""Steady-state time of one CDAE training step (device events) at the reference's lastfm shape (1,892 x 17,632, the stock conf:
batch 256, -nh 128, -co 0.9) and the Yelp2018 shape (31,668 x 38,048, same batch and width), on synthetic ratings of those sizes.
Figures per shape, from the same batches in the same run:

  step_device_lists   the five kernels + two Adam launches, lists already on the device (what the step itself costs)
  step_host_lists     the same with the host lists validated, packed and uploaded inside the timed region (what exact mode runs)
  dense_torch_step    a straightforward dense fp32 step of the same batch with torch matmuls on the same device: four
                      batch x n_items arrays, two dense products each way, Adam by element-wise torch ops -- the form the
                      reference writes, the comparison that says what the sparse form bought
  host_list_build     CPU time to draw a batch (mask, users, negatives) and build its lists -- host work, not a device time

  throughput_draw     one batch drawn and its lists built on the device (QREC_MODE=throughput's stream)
  throughput_step     that draw followed by the step on its lists (what throughput mode runs)

All device figures are device-event times of single calls, the variants alternated inside one loop.

    python tools/bench_cdae.py [--out profiles/cdae_bench.json] [--reps 30] [--warmup 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qrec_amd import capi                                                              # noqa: E402
from qrec_amd.autoencoder import CdaeTrainer, DeviceBatchStream, lists_from_entries, rated_rows           # noqa: E402

SHAPES = {"lastfm": dict(nu=1892, ni=17632, nnz=92834, nh=128, B=256),
          "yelp2018": dict(nu=31668, ni=38048, nnz=1237259, nh=128, B=256)}
N_BATCHES = 8
CO = 0.9


def synthetic(nu, ni, nnz, nh, B, seed=0):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, nu, nnz), rng.integers(0, ni, nnz)], 1), axis=0)
    uid, iid = pairs[:, 0], pairs[:, 1].astype(np.int32)
    indptr = np.zeros(nu + 1, np.int64); np.cumsum(np.bincount(uid, minlength=nu), out=indptr[1:])
    vals = (rng.integers(1, 11, iid.size) / 2).astype(np.float32)
    xav = lambda *s: rng.uniform(-np.sqrt(6.0 / sum(s)), np.sqrt(6.0 / sum(s)), s).astype(np.float32)
    p = dict(W_enc=xav(ni, nh), W_dec=xav(nh, ni), b_enc=np.zeros(nh, np.float32), b_dec=np.zeros(ni, np.float32), V=xav(nu, nh))
    return rng, (indptr, iid, vals), p


def draw_lists(rng, rated, ni, B):
    """a batch with the reference's distribution: uniform users, 5 |rated| uniform unrated negatives, Bernoulli(co) mask"""
    indptr, items, vals = rated
    users = rng.integers(0, indptr.size - 1, B).astype(np.int32)
    pr, pi, pv = rated_rows(users, indptr, items, vals)
    cnt = np.diff(indptr)[users]
    nr = np.repeat(np.arange(B), 5 * cnt)
    nn = rng.integers(0, ni, nr.size)
    is_rated = np.isin(nr.astype(np.int64) * ni + nn, pr.astype(np.int64) * ni + pi)
    nr, nn = nr[~is_rated], nn[~is_rated]                    # the rejected draws are dropped, not redrawn: a few per cent fewer negatives
    mask = rng.random((B, ni)) < CO
    return lists_from_entries(users, ni, pr, pi, pv, nr, nn, lambda r, i: mask[r, i])


def interleaved_ms(fns: dict, reps, warmup):
    """every variant timed by the same clock (device events on the null stream around one call), alternated inside one loop so
    that clock and thermal drift fall on all of them alike; median and spread of `reps` timings each after `warmup` untimed rounds"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    capi.device_sync()
    a, b, ms = capi.Event(), capi.Event(), {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a.record(); fn(); b.record(); b.sync()
            ms[k].append(b.elapsed_ms_since(a))
    out = {}
    for k, v in ms.items():
        v = np.sort(v)
        out[k] = dict(median_ms=float(np.median(v)), p10_ms=float(v[len(v) // 10]), p90_ms=float(v[(9 * len(v)) // 10]), reps=reps)
    return out


def dense_torch_step(p, lists, lr, reg):
    """the dense form on the device with torch: returns a callable running one forward / backward / Adam step"""
    import torch
    dev = torch.device("cuda")
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    P = {k: t(v) for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in P.items()}; v2 = {k: torch.zeros_like(v) for k, v in P.items()}
    B, ni = lists[0].B, lists[0].n_items
    dense = []
    for L in lists:
        X = np.zeros((B, ni), np.float32); pos = np.zeros((B, ni), np.float32); neg = np.zeros((B, ni), np.float32)
        rows = np.repeat(np.arange(B), np.diff(L.lv_ptr))
        X[np.repeat(np.arange(B), np.diff(L.in_ptr)), L.in_item] = L.in_val
        pos[rows[L.lv_label == 1], L.lv_item[L.lv_label == 1]] = 1; neg[rows[L.lv_label == 0], L.lv_item[L.lv_label == 0]] = 1
        # the mask: ones at the live and kept positions; the positions it zeroes elsewhere carry no loss either way
        dense.append((torch.tensor(L.users.astype(np.int64), device=dev), t(X), t(pos), t(neg), t(((pos + neg) > 0).astype(np.float32))))
    state = dict(k=0)

    def step():
        u, X, pos, neg, mask = dense[state["k"] % len(dense)]; state["k"] += 1
        x = mask * X
        h = torch.sigmoid(x @ P["W_enc"] + P["b_enc"] + P["V"][u])
        y = torch.sigmoid(h @ P["W_dec"] + P["b_dec"])
        yc = torch.clamp(y * mask, min=1e-6)
        ds = (-(pos * mask) / yc + (neg * mask) / (1 - yc)) / (B * ni) * (y * mask >= 1e-6) * mask * y * (1 - y)
        dh = ds @ P["W_dec"].T
        dz = dh * h * (1 - h)
        gV = torch.zeros_like(P["V"]).index_add_(0, u, dz + reg * P["V"][u])
        g = dict(W_enc=x.T @ dz + reg * P["W_enc"], W_dec=h.T @ ds + reg * P["W_dec"], b_enc=dz.sum(0) + reg * P["b_enc"],
                 b_dec=ds.sum(0) + reg * P["b_dec"], V=gV)
        for k in P:
            m[k] += (g[k] - m[k]) * 0.1; v2[k] += (g[k] * g[k] - v2[k]) * 0.001
            P[k] -= (m[k] * lr) / (torch.sqrt(v2[k]) + 1e-8)
    return step


def bench_shape(name, reps, warmup):
    s = SHAPES[name]
    rng, rated, p = synthetic(**s)
    t0 = time.perf_counter()
    lists = [draw_lists(rng, rated, s["ni"], s["B"]) for _ in range(N_BATCHES)]
    build_ms = (time.perf_counter() - t0) * 1e3 / N_BATCHES
    tr = CdaeTrainer(p["W_enc"], p["W_dec"], p["b_enc"], p["b_dec"], p["V"], 0.001, 0.01)
    on_device = [L.device_copy() for L in lists]
    k = dict(n=0)

    def step(src):
        tr.train_step_async(src[k["n"] % N_BATCHES]); k["n"] += 1
    stream = DeviceBatchStream(*rated, s["ni"], s["B"], CO, seed=0)
    tr_t = CdaeTrainer(p["W_enc"], p["W_dec"], p["b_enc"], p["b_dec"], p["V"], 0.001, 0.01)      # throughput mode trains its own copy

    def throughput_step():
        tr_t.train_step_async(stream.draw(k["n"])); k["n"] += 1
    out = dict(shape=s, kept_inputs_per_batch=int(np.mean([L.n_in for L in lists])), live_slots_per_batch=int(np.mean([L.n_live for L in lists])),
               dense_positions_per_batch=s["B"] * s["ni"], host_list_build=dict(mean_ms=build_ms, batches=N_BATCHES))
    dense = dense_torch_step(p, lists, 0.001, 0.01)            # torch's kernels run on the null stream, as the events do
    out.update(interleaved_ms(dict(step_device_lists=lambda: step(on_device), step_host_lists=lambda: step(lists),
                                   throughput_draw=lambda: stream.draw(0), throughput_step=throughput_step, dense_torch_step=dense),
                              reps, warmup))
    assert np.isfinite(tr.loss()) and np.isfinite(tr_t.loss())
    out["dense_over_sparse"] = out["dense_torch_step"]["median_ms"] / out["step_device_lists"]["median_ms"]
    out["dense_over_throughput"] = out["dense_torch_step"]["median_ms"] / out["throughput_step"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", default="lastfm,yelp2018")
    a = ap.parse_args()
    capi.init()
    res = dict(tool="tools/bench_cdae.py", device=capi.device_info(), mode="exact (ordered sums; the kernels use no float atomic in any mode)",
               throughput_mode="batch drawn and lists built on the device, then the same kernels", shapes={})
    for name in a.shapes.split(","):
        res["shapes"][name] = bench_shape(name, a.reps, a.warmup)
        print(name, json.dumps({k: v for k, v in res["shapes"][name].items() if k != "shape"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
