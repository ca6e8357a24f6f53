#!/usr/bin/env python3
"""Steady-state device time of APR's three operations (qrec_amd/graph.py::AprTrainer, csrc/apr.hip) on synthetic triplets at the
FilmTrust shape (1,508 x 2,071, batch 512), the reference's lastfm shape under the stock APR.conf (1,892 x 17,632, batch 512) and
the Yelp2018 shape (31,668 x 38,048, batch 2,048), d = 64.  Figures per shape, from the same batches in the same interleaved run:

  pretrain_step          zero dE, qrec_apr_batch_loss_grad without perturbations, dense Adam        (atomic and ordered reductions)
  adversarial_step       the same with the perturbed term                                           (atomic and ordered reductions)
  perturb                qrec_apr_perturb: producer, clear of the previous rows, sort, walk + normalise (one mode: it has no atomics)
  perturb_stages         device milliseconds of the four stages of that call, from events the entry point records itself
  perturb_10x_users      the same call, same batch, on tables with ten times the users: the pass does no work per table row
  bpr_tf_step            BprTfTrainer.train_step_async on the same shape and batches: the nearest step the project had before APR
                         (the adversarial step does strictly more: a second gather, a second score, a third loss term)
  dense_torch_perturb    the perturbation update in the dense form the reference writes, torch ops on the same device: autograd
  dense_torch_adv_step   gradient of the loss w.r.t. the whole perturbation tables, row normalisation over the whole tables; the
                         adversarial step by autograd and element-wise Adam (skipped with --no-dense)

    python tools/bench_apr.py [--out profiles/apr_bench.json] [--shapes filmtrust,lastfm,yelp2018] [--reps 30] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qrec_amd import capi                                                              # noqa: E402
from qrec_amd.capi import DeviceBuffer                                                 # noqa: E402
from qrec_amd.graph import AprTrainer, BprTfTrainer, ordered_reductions                # noqa: E402

SHAPES = {"filmtrust": dict(nu=1508, ni=2071, B=512), "lastfm": dict(nu=1892, ni=17632, B=512), "yelp2018": dict(nu=31668, ni=38048, B=2048)}
D, LR, REG, REG_ADV, EPS = 64, 0.003, 0.002, 2.0, 0.5
N_BATCHES = 4


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


def dense_torch(U0, V0, batches):
    """(perturbation update, adversarial step) as callables in the dense form, torch on the device"""
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda")
    U, V = (torch.tensor(a, device=dev, requires_grad=True) for a in (U0, V0))
    dU, dV = (torch.zeros_like(a, requires_grad=True) for a in (U, V))
    m = [torch.zeros_like(a) for a in (U, V)]; v2 = [torch.zeros_like(a) for a in (U, V)]
    idx = [tuple(torch.tensor(x.astype(np.int64), device=dev) for x in b) for b in batches]
    state = dict(k=0)

    def adv_loss(u, i, j):
        up = U[u] + dU[u]
        return REG_ADV * F.softplus(-((up * (V[i] + dV[i])).sum(1) - (up * (V[j] + dV[j])).sum(1))).sum()

    def perturb():
        u, i, j = idx[state["k"] % len(idx)]; state["k"] += 1
        gU, gV = torch.autograd.grad(adv_loss(u, i, j), [dU, dV])
        with torch.no_grad():
            dU.copy_(F.normalize(gU, dim=1, eps=1e-6) * EPS); dV.copy_(F.normalize(gV, dim=1, eps=1e-6) * EPS)

    def step():
        u, i, j = idx[state["k"] % len(idx)]; state["k"] += 1
        loss = F.softplus(-((U[u] * V[i]).sum(1) - (U[u] * V[j]).sum(1))).sum() + REG * 0.5 * ((U[u] ** 2).sum() + (V[i] ** 2).sum()) + adv_loss(u, i, j)
        g = torch.autograd.grad(loss, [U, V])
        with torch.no_grad():
            for t, gt, mt, vt in zip((U, V), g, m, v2):
                mt += (gt - mt) * 0.1; vt += (gt * gt - vt) * 0.001
                t -= (mt * LR) / (torch.sqrt(vt) + 1e-8)
    return perturb, step


def bench_shape(name, reps, warmup, dense):
    s = SHAPES[name]
    nu, ni, B = s["nu"], s["ni"], s["B"]
    rng = np.random.default_rng(0)
    V0 = (rng.standard_normal((ni, D)) * 0.05).astype(np.float32)
    U0 = (rng.standard_normal((nu, D)) * 0.05).astype(np.float32)
    host = []
    for _ in range(N_BATCHES):
        i = rng.integers(0, ni, B)
        host.append((rng.integers(0, nu, B).astype(np.int32), i.astype(np.int32), ((i + 1 + rng.integers(0, ni - 1, B)) % ni).astype(np.int32)))
    dev = [tuple(DeviceBuffer.from_numpy(x) for x in b) for b in host]
    atomic = AprTrainer(U0, V0, LR, REG, REG_ADV, EPS, B)
    with ordered_reductions():
        ordered = AprTrainer(U0, V0, LR, REG, REG_ADV, EPS, B)
        bpr_ordered = BprTfTrainer(U0, V0, LR, REG)
    bpr_atomic = BprTfTrainer(U0, V0, LR, REG)
    wide = AprTrainer(np.tile(U0, (10, 1)), V0, LR, REG, REG_ADV, EPS, B)
    k = dict(n=0)

    def nxt():
        k["n"] += 1
        return dev[k["n"] % N_BATCHES]
    fns = dict(pretrain_step_atomic=lambda: atomic.pretrain_step_async(*nxt(), B), pretrain_step_ordered=lambda: ordered.pretrain_step_async(*nxt(), B),
               adversarial_step_atomic=lambda: atomic.adversarial_step_async(*nxt(), B),
               adversarial_step_ordered=lambda: ordered.adversarial_step_async(*nxt(), B),
               perturb=lambda: atomic.perturb_async(*nxt(), B), perturb_10x_users=lambda: wide.perturb_async(*nxt(), B),
               bpr_tf_step_atomic=lambda: bpr_atomic.train_step_async(*nxt(), B), bpr_tf_step_ordered=lambda: bpr_ordered.train_step_async(*nxt(), B))
    ordered.perturb_async(*dev[0], B)                               # the ordered trainer's steps run on non-zero perturbations too
    dense_note = "skipped (--no-dense)"
    if dense:
        try:
            fns["dense_torch_perturb"], fns["dense_torch_adv_step"] = dense_torch(U0, V0, host)
            fns["dense_torch_perturb"](); fns["dense_torch_adv_step"]()
        except Exception as e:                                      # a torch build that does not see the device: the partner is missing, not the product
            fns.pop("dense_torch_perturb", None); fns.pop("dense_torch_adv_step", None)
            dense, dense_note = False, f"torch could not run it on the device: {e}"
    out = dict(shape=dict(s, d=D, ld=atomic.ld), table_bytes=4 * atomic.n * atomic.ld)
    out.update(interleaved_ms(fns, reps, warmup))
    stages = np.zeros((reps, 4), np.float32)
    for r in range(reps):
        u, v, n = nxt()
        capi.apr_perturb(atomic.E, atomic.D, atomic.nu, atomic.n, atomic.d, atomic.ld, u, v, n, B, REG_ADV, EPS, atomic.touched, atomic.perturb_ws,
                         stage_ms=stages[r])
    med = np.median(stages, 0)
    out["perturb_stages"] = dict(producer_ms=float(med[0]), clear_ms=float(med[1]), sort_ms=float(med[2]), walk_ms=float(med[3]), reps=reps,
                                 note="events recorded by the entry point between its launches; their sum exceeds the untimed call by the event overhead")
    assert all(np.isfinite(t.loss()) for t in (atomic, ordered)) and np.isfinite(atomic.D.numpy()).all()
    out["adversarial_over_bpr_tf_atomic"] = out["adversarial_step_atomic"]["median_ms"] / out["bpr_tf_step_atomic"]["median_ms"]
    out["perturb_10x_users_over_perturb"] = out["perturb_10x_users"]["median_ms"] / out["perturb"]["median_ms"]
    if dense:
        out["dense_perturb_over_perturb"] = out["dense_torch_perturb"]["median_ms"] / out["perturb"]["median_ms"]
        out["dense_adv_step_over_adv_step_atomic"] = out["dense_torch_adv_step"]["median_ms"] / out["adversarial_step_atomic"]["median_ms"]
    else:
        out["dense_torch_perturb"] = out["dense_torch_adv_step"] = f"unmeasured: {dense_note}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="filmtrust,lastfm,yelp2018")
    ap.add_argument("--no-dense", action="store_true")
    a = ap.parse_args()
    capi.init()
    res = dict(tool="tools/bench_apr.py", shapes={})
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    res["device"] = capi.device_info()
    for name in a.shapes.split(","):
        res["shapes"][name] = bench_shape(name, a.reps, a.warmup, not a.no_dense)
        print(name, json.dumps({k: v for k, v in res["shapes"][name].items() if k != "shape"}), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
