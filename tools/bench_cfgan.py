#!/usr/bin/env python3
"""Steady-state time of one CFGAN epoch (device events: one discriminator step and three generator steps on one batch) at the
FilmTrust shape (1,508 x 2,071), the reference's lastfm shape under the stock conf (1,892 x 17,632, batch 128) and the Yelp2018
shape (31,668 x 38,048: 17 GB of G_W1 and its two Adam slots), on synthetic ratings of those sizes with the class's own
S_zr = S_pm = 0.001.  Figures per shape, from the same batches in the same run:

  epoch_device_lists  the four forward passes, the discriminator step and the three sweeps, lists already on the device
  epoch_host_lists    the same with the host lists validated, packed and uploaded inside the timed region (what the class runs)
  sweep               qrec_cfgan_gen_sweep alone: one read and one write of G_W1, m, v (24 bytes per entry) with the sparse gradient
                      injected; ``roofline_fraction`` = 24 n_items ld bytes / time / 8 TB/s (the MI355X's HBM peak; about
                      6.3 TB/s is what streaming kernels achieve)
  forward             qrec_cfgan_forward alone (sampled forward pass, discriminator logits, delta, losses)
  eval_call           one qrec_score_topk_sparse_row_sigmoid_bias call for ``eval_users`` users: the sparse block fill, the sigmoid +
                      bias pass, the rated mask and the top-10 together (the fill has no entry point of its own)
  dense_torch_epoch   the same epoch in the dense form the reference writes, with torch ops on the same device: C @ G_W1, autograd-free
                      hand-written gradients, Adam by element-wise ops over the whole table (skipped with --no-dense)
  host_draw           CPU time of one next_batch draw loop in plain Python (random.choice on name lists) plus building its lists
  mirror_epoch        the float64 numpy mirror (tests/cfgan_mirror.py, sparse form) on the host, FilmTrust shape only

All device figures are device-event times of single calls, the variants alternated inside one loop.

    python tools/bench_cfgan.py [--out profiles/cfgan_bench.json] [--shapes filmtrust,lastfm,yelp2018] [--reps 20] [--warmup 5]

``--out`` is updated shape by shape: a later call with other ``--shapes`` keeps the shapes already in the file."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qrec_amd import capi                                                              # noqa: E402
from qrec_amd.autoencoder import CfganTrainer, cfgan_lists, rated_rows                 # noqa: E402
from qrec_amd.interactions import CSR                                                  # noqa: E402

SHAPES = {"filmtrust": dict(nu=1508, ni=2071, nnz=35497, B=128),
          "lastfm": dict(nu=1892, ni=17632, nnz=92834, B=128),
          "yelp2018": dict(nu=31668, ni=38048, nnz=1237259, B=128)}
N_BATCHES = 4
S_ZR = S_PM = 0.001
ALPHA, LR = 0.01, 0.002
PEAK_BYTES_PER_S = 8e12


def synthetic(nu, ni, nnz, B, seed=0):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, nu, nnz), rng.integers(0, ni, nnz)], 1), axis=0)
    uid, iid = pairs[:, 0], pairs[:, 1].astype(np.int32)
    indptr = np.zeros(nu + 1, np.int64); np.cumsum(np.bincount(uid, minlength=nu), out=indptr[1:])
    vals = (rng.integers(1, 11, iid.size) / 2).astype(np.float32)
    lim = np.sqrt(6.0 / (2 * ni))
    block = rng.uniform(-lim, lim, (min(ni, 2048), ni)).astype(np.float32)             # a 38,048^2 table of fresh draws takes minutes on the host
    W = np.tile(block, (-(-ni // block.shape[0]), 1))[:ni]
    p = dict(G_W1=W, G_b1=np.zeros(ni, np.float32), D_W1=rng.uniform(-lim, lim, 2 * ni).astype(np.float32), D_b1=np.zeros(1, np.float32))
    return rng, (indptr, iid, vals), p


def draw_lists(rated, ni, B):
    """next_batch's loop in plain Python, as the class runs it: choice(userList), then the N_zr and mask negatives by rejection"""
    indptr, items, vals = rated
    user_names = [f"u{k}" for k in range(indptr.size - 1)]
    item_names = [f"i{k}" for k in range(ni)]
    item_id = {n: k for k, n in enumerate(item_names)}
    users = np.empty(B, np.int32)
    zr, pm = ([], []), ([], [])
    for n in range(B):
        u = int(random.choice(user_names)[1:])
        users[n] = u
        mine = {item_names[i] for i in items[indptr[u]:indptr[u + 1]]}
        for count, (rows, its) in ((int(S_ZR * ni), zr), (int(S_PM * ni), pm)):
            for _ in range(count):
                ng = random.choice(item_names)
                while ng in mine:
                    ng = random.choice(item_names)
                rows.append(n); its.append(item_id[ng])
    return cfgan_lists(users, ni, *rated_rows(users, indptr, items, vals), pm[0], pm[1], zr[0], zr[1])


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


def dense_torch_epoch(p, lists):
    """the dense form on the device with torch: returns a callable running D, G, G, G on one batch"""
    import torch
    dev = torch.device("cuda")
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    P = {k: t(v) for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in P.items()}; v2 = {k: torch.zeros_like(v) for k, v in P.items()}
    B, ni = lists[0].B, lists[0].n_items
    dense = []
    for L in lists:
        C = np.zeros((B, ni), np.float32); mask = np.zeros((B, ni), np.float32); zr = np.zeros((B, ni), np.float32)
        rows = np.repeat(np.arange(B), np.diff(L.lv_ptr))
        C[np.repeat(np.arange(B), np.diff(L.in_ptr)), L.in_item] = L.in_val
        mask[rows, L.lv_item] = 1; zr[rows, L.lv_item] = L.lv_label
        dense.append((t(C), t(mask), t(zr)))
    state = dict(k=0)

    def adam(keys, g):
        for k in keys:
            m[k] += (g[k] - m[k]) * 0.1; v2[k] += (g[k] * g[k] - v2[k]) * 0.001
            P[k] -= (m[k] * LR) / (torch.sqrt(v2[k]) + 1e-8)

    def forward(C, mask):
        r = torch.sigmoid(C @ P["G_W1"] + P["G_b1"])
        fake = r * mask
        Dr = torch.sigmoid(torch.cat([C, C], 1) @ P["D_W1"] + P["D_b1"])
        Df = torch.sigmoid(torch.cat([fake, C], 1) @ P["D_W1"] + P["D_b1"])
        return r, fake, Dr, Df

    def epoch():
        C, mask, zr = dense[state["k"] % len(dense)]; state["k"] += 1
        r, fake, Dr, Df = forward(C, mask)
        a_r = -Dr * (1 - Dr) / (Dr + 1e-4) / B; a_f = Df * (1 - Df) / (1 - Df + 1e-4) / B
        adam(("D_W1", "D_b1"), dict(D_W1=torch.cat([C, C], 1).T @ a_r + torch.cat([fake, C], 1).T @ a_f, D_b1=(a_r.sum() + a_f.sum()).reshape(1)))
        for _ in range(3):
            r, fake, Dr, Df = forward(C, mask)
            a_f = Df * (1 - Df) / (1 - Df + 1e-4) / B
            delta = (-a_f[:, None] * P["D_W1"][None, :ni] + ALPHA * zr * fake) * mask * r * (1 - r)
            adam(("G_W1", "G_b1"), dict(G_W1=C.T @ delta, G_b1=delta.sum(0)))
    return epoch


def bench_shape(name, reps, warmup, dense, eval_users):
    from qrec_amd.capi import DeviceBuffer
    from qrec_amd.ranking import SparseRowSigmoidRanker
    s = SHAPES[name]
    rng, rated, p = synthetic(**s)
    ni, B = s["ni"], s["B"]
    random.seed(0)
    t0 = time.perf_counter()
    lists = [draw_lists(rated, ni, B) for _ in range(N_BATCHES)]
    draw_ms = (time.perf_counter() - t0) * 1e3 / N_BATCHES
    tr = CfganTrainer(p["G_W1"], p["G_b1"], p["D_W1"], p["D_b1"], LR, ALPHA)
    on_device = [L.device_copy() for L in lists]
    k = dict(n=0)

    def epoch(src):
        tr.train_epoch_async(src[k["n"] % N_BATCHES]); k["n"] += 1
    Lf = tr.forward(on_device[0])

    def sweep():
        capi.cfgan_gen_sweep(tr.W, tr.mW, tr.vW, tr.b, tr.mb, tr.vb, ni, tr.ld, Lf, tr.ws, 1e-4, 0.9, 0.999, 1e-8)
    n_eval = min(eval_users, s["nu"])
    ranker = SparseRowSigmoidRanker(tr.W, tr.b, s["nu"], ni, tr.ld, CSR(rated[0], rated[1], rated[2].astype(np.float64)))
    d_users = DeviceBuffer.from_numpy(np.arange(n_eval, dtype=np.int32))
    scratch = DeviceBuffer(ranker._scratch_bytes(n_eval, 10), np.uint8)
    d_ids, d_sc = DeviceBuffer((n_eval, 10), np.int32), DeviceBuffer((n_eval, 10), np.float32)
    # forward right before sweep: the sweep reads the delta of the lists it is handed from the workspace
    fns = dict(epoch_device_lists=lambda: epoch(on_device), epoch_host_lists=lambda: epoch(lists), forward=lambda: tr.forward(on_device[0]),
               sweep=sweep, eval_call=lambda: ranker._score_topk(d_users, n_eval, 10, scratch, d_ids, d_sc))
    dense_note = "skipped (--no-dense)"
    if dense:
        try:
            fns["dense_torch_epoch"] = dense_torch_epoch(p, lists)     # torch's kernels run on the null stream, as the events do
        except RuntimeError as e:                                      # a torch build that does not see the device: the partner is missing, not the product
            dense, dense_note = False, f"torch could not use the device: {e}"
    out = dict(shape=s, rated_entries_per_batch=int(np.mean([L.n_in for L in lists])), mask_positions_per_batch=int(np.mean([L.n_live for L in lists])),
               flagged_positions_per_batch=int(np.mean([L.lv_label.sum() for L in lists])), table_bytes=3 * 4 * ni * tr.ld, eval_users=n_eval,
               host_draw=dict(mean_ms=draw_ms, batches=N_BATCHES))
    out.update(interleaved_ms(fns, reps, warmup))
    assert np.isfinite(tr.d_loss()) and np.isfinite(tr.g_loss())
    out["sweep"]["bytes"] = 24 * ni * tr.ld
    out["sweep"]["achieved_TBps"] = out["sweep"]["bytes"] / (out["sweep"]["median_ms"] * 1e-3) / 1e12
    out["sweep"]["roofline_fraction"] = out["sweep"]["bytes"] / (out["sweep"]["median_ms"] * 1e-3) / PEAK_BYTES_PER_S
    if dense:
        out["dense_over_sparse"] = out["dense_torch_epoch"]["median_ms"] / out["epoch_device_lists"]["median_ms"]
    else:
        out["dense_torch_epoch"] = f"unmeasured: {dense_note}"
    if name == "filmtrust":
        import cfgan_mirror as M
        t0 = time.perf_counter()
        M.train(p, lists[:1], LR, ALPHA)
        out["mirror_epoch"] = dict(ms=(time.perf_counter() - t0) * 1e3, dtype="float64", form="sparse")
    else:
        out["mirror_epoch"] = "unmeasured"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="filmtrust,lastfm,yelp2018")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--eval-users", type=int, default=1024)
    a = ap.parse_args()
    capi.init()
    res = dict(tool="tools/bench_cfgan.py", shapes={})
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    res["device"] = capi.device_info()
    res["mode"] = "one path (ordered sums; the kernels use no float atomic)"
    for name in a.shapes.split(","):
        res["shapes"][name] = bench_shape(name, a.reps, a.warmup, not a.no_dense, a.eval_users)
        print(name, json.dumps({k: v for k, v in res["shapes"][name].items() if k != "shape"}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
