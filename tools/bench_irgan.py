#!/usr/bin/env python3
"""Steady-state times of IRGAN's three phases (device events) at FilmTrust (1,508 x 2,071, d = 8 as the fixture), the reference's
lastfm shape (1,892 x 17,632, the stock conf: d = 50, batch 128) and the Yelp2018 shape (31,668 x 38,048, d = 64), on synthetic
ratings of those sizes.  Figures per shape:

  get_data_ms             2 |pos| negatives for every user, drawn on the device in blocks of users, rows assembled there (per epoch)
  discriminator_ms        one batch step: slot gradients, two ordered scatters, two dense Adam launches
  generator_us            one user's step: distribution, 3 |pos| draws, rewards, policy gradient, dense Adam on three variables
  dense_torch_generator_us / dense_torch_discriminator_ms
                          the same steps written in dense torch ops on the same device (softmax, multinomial, index_add, element-wise
                          Adam): the figure to beat
  numpy_generator_us      the float64 numpy mirror of the generator step on one core (tests/irgan_mirror.py) -- host time

Device figures are device-event times of single calls, the variants alternated inside one loop.  generator_us is averaged over the
users of a fixed sample (heavy and light rows alike).  The dense torch steps run in a child process of their own (torch brings its own
HIP runtime; this library binds the system's), on the same synthetic case, timed the same way with torch's events; when torch cannot
use the device the child's error is recorded in place of the figures and the ratios are null.

    python tools/bench_irgan.py [--out profiles/irgan_bench.json] [--reps 30] [--warmup 10] [--shapes filmtrust,lastfm,yelp2018]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qrec_amd import capi                                  # noqa: E402
from qrec_amd.gan import IrganTrainer                      # noqa: E402

SHAPES = {"filmtrust": dict(nu=1508, ni=2071, nnz=35497, d=8, B=128),
          "lastfm": dict(nu=1892, ni=17632, nnz=92834, d=50, B=128),
          "yelp2018": dict(nu=31668, ni=38048, nnz=1237259, d=64, B=128)}
N_USERS_TIMED = 16
LR, REG = 0.001, 0.001


def synthetic(nu, ni, nnz, d, B, seed=0):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, nu, nnz), rng.integers(0, ni, nnz)], 1), axis=0)
    uid, iid = pairs[:, 0], pairs[:, 1].astype(np.int32)
    uid = np.concatenate([uid, np.setdiff1d(np.arange(nu), uid)]); iid = np.concatenate([iid, np.zeros(uid.size - iid.size, np.int32)])
    order = np.lexsort((iid, uid)); uid, iid = uid[order], iid[order]          # every user has at least one rated item
    indptr = np.zeros(nu + 1, np.int64); np.cumsum(np.bincount(uid, minlength=nu), out=indptr[1:])
    v = {}
    for t in "gd":
        v[t + "_P"] = rng.uniform(-0.05, 0.05, (nu, d)).astype(np.float32); v[t + "_Q"] = rng.uniform(-0.05, 0.05, (ni, d)).astype(np.float32)
        v[t + "_b"] = np.zeros(ni, np.float32)
    return rng, (indptr, iid), v


def case(name):
    """the synthetic tables, the users whose steps are timed and the discriminator batch of a shape: the same in parent and child"""
    s = SHAPES[name]
    rng, csr, v = synthetic(**s)
    users = rng.permutation(s["nu"])[:N_USERS_TIMED].tolist()
    B = s["B"]
    batch = (rng.integers(0, s["nu"], B).astype(np.int32), rng.integers(0, s["ni"], B).astype(np.int32), (rng.random(B) < 1 / 3).astype(np.float32))
    return s, rng, csr, v, users, batch


def interleaved(fns: dict, reps, warmup):
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


def dense_torch(v, csr, users, batch):
    """the generator step of one user and the discriminator step of one batch in dense torch ops"""
    import torch
    dev = torch.device("cuda")
    T = {k: torch.tensor(x, device=dev) for k, x in v.items()}
    m = {k: torch.zeros_like(x) for k, x in T.items()}; s = {k: torch.zeros_like(x) for k, x in T.items()}
    pos = {u: torch.tensor(csr[1][csr[0][u]:csr[0][u + 1]].astype(np.int64), device=dev) for u in users}
    bu, bi, by = (torch.tensor(x, device=dev) for x in (batch[0].astype(np.int64), batch[1].astype(np.int64), batch[2]))
    state = dict(k=0)

    def adam(keys, g):
        for k in keys:
            m[k] += (g[k] - m[k]) * 0.1; s[k] += (g[k] * g[k] - s[k]) * 0.001
            T[k] -= (m[k] * LR) / (torch.sqrt(s[k]) + 1e-8)

    def generator():
        u = users[state["k"] % len(users)]; state["k"] += 1
        ps = pos[u]; K = 3 * ps.numel()
        p = torch.softmax(T["g_Q"] @ T["g_P"][u] + T["g_b"], 0)
        pn = 0.8 * p; pn[ps] += 0.2 / ps.numel()
        smp = torch.multinomial(pn, K, replacement=True)
        rew = 2 * (torch.sigmoid(T["d_Q"][smp] @ T["d_P"][u] + T["d_b"][smp]) - 0.5) * p[smp] / pn[smp]
        c = torch.zeros_like(p).index_add_(0, smp, rew); n = torch.zeros_like(p).index_add_(0, smp, torch.ones_like(rew))
        g = -(c - rew.sum() * p) / K
        gP = torch.zeros_like(T["g_P"]); gP[u] = g @ T["g_Q"] + REG * T["g_P"][u]
        adam(("g_P", "g_Q", "g_b"), dict(g_P=gP, g_Q=g[:, None] * T["g_P"][u][None, :] + REG * n[:, None] * T["g_Q"], g_b=g + REG * n * T["g_b"]))

    def discriminator():
        B = bu.numel()
        pu, qi = T["d_P"][bu], T["d_Q"][bi]
        dz = torch.sigmoid((pu * qi).sum(1) + T["d_b"][bi]) - by
        g = dict(d_P=torch.zeros_like(T["d_P"]).index_add_(0, bu, dz[:, None] * qi + B * REG * pu),
                 d_Q=torch.zeros_like(T["d_Q"]).index_add_(0, bi, dz[:, None] * pu + B * REG * qi),
                 d_b=torch.zeros_like(T["d_b"]).index_add_(0, bi, dz + B * REG * T["d_b"][bi]))
        adam(("d_P", "d_Q", "d_b"), g)
    return generator, discriminator


def dense_child(name, reps, warmup):
    """runs in the child process: torch only"""
    import torch
    _, _, csr, v, users, batch = case(name)
    tg, td = dense_torch(v, csr, users, batch)
    fns = dict(dense_torch_generator=tg, dense_torch_discriminator=td)
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ms[k].append(a.elapsed_time(b))
    out = {}
    for k, x in ms.items():
        x = np.sort(x)
        out[k] = dict(median_ms=float(np.median(x)), p10_ms=float(x[len(x) // 10]), p90_ms=float(x[(9 * len(x)) // 10]), reps=reps)
    print("DENSE " + json.dumps(out), flush=True)


def dense_in_child(name, reps, warmup):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dense-child", name, "--reps", str(reps), "--warmup", str(warmup)],
                       capture_output=True, text=True, timeout=600)
    for line in r.stdout.splitlines():
        if line.startswith("DENSE "):
            return json.loads(line[6:])
    return dict(error=(r.stderr.strip().splitlines() or ["no output"])[-1], returncode=r.returncode)


def bench_shape(name, reps, warmup):
    import irgan_mirror as M
    s, rng, csr, v, users, batch = case(name)
    tr = IrganTrainer(v, csr[0], csr[1], LR, REG)
    order = np.arange(s["nu"], dtype=np.int32)
    d_batch = tuple(capi.DeviceBuffer.from_numpy(x) for x in batch)
    k = dict(n=0)

    def generator():
        tr.generator_step(users[k["n"] % len(users)]); k["n"] += 1
    out = dict(shape=s, ld=tr.ld, mean_positives_of_timed_users=float(np.mean(tr.n_pos[users])))
    t = interleaved(dict(generator=generator, discriminator=lambda: tr.discriminator_step(*d_batch)), reps, warmup)
    t.update(interleaved(dict(get_data=lambda: tr.draw_negatives(order, None, step=k["n"], assemble=True)), max(3, reps // 10), 1))
    out["get_data_ms"] = t["get_data"]; out["discriminator_ms"] = t["discriminator"]
    to_us = lambda d: {a.replace("_ms", "_us"): (b * 1e3 if a.endswith("_ms") else b) for a, b in d.items()}
    out["generator_us"] = to_us(t["generator"])
    mir = M.Mirror(v, LR, REG)
    pos = {u: csr[1][csr[0][u]:csr[0][u + 1]] for u in users}
    t0 = time.perf_counter()
    for u in users[:4]:
        p, pn = M.mixture(M.logits(mir.p["g_P"], mir.p["g_Q"], mir.p["g_b"], u), pos[u])
        mir.generator_step(u, pos[u], M.draw(pn, rng.random(3 * pos[u].size)))
    out["numpy_generator_us"] = dict(mean_us=(time.perf_counter() - t0) * 1e6 / 4, users=4)
    assert np.isfinite(tr.loss()) and tr.padding_is_zero()
    dense = dense_in_child(name, reps, warmup)
    if "error" in dense:
        out["dense_torch"] = dense
        out["dense_over_hip_generator"] = out["dense_over_hip_discriminator"] = None
    else:
        out["dense_torch_generator_us"] = to_us(dense["dense_torch_generator"]); out["dense_torch_discriminator_ms"] = dense["dense_torch_discriminator"]
        out["dense_over_hip_generator"] = dense["dense_torch_generator"]["median_ms"] / t["generator"]["median_ms"]
        out["dense_over_hip_discriminator"] = dense["dense_torch_discriminator"]["median_ms"] / t["discriminator"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", default="filmtrust,lastfm,yelp2018")
    ap.add_argument("--dense-child", default=None, help="internal: time the dense torch steps of this shape and print them")
    a = ap.parse_args()
    if a.dense_child:
        return dense_child(a.dense_child, a.reps, a.warmup)
    capi.init()
    res = dict(tool="tools/bench_irgan.py", device=capi.device_info(), shapes={},
               note="plain launches; the generator step is ~14 launches (row weights 4, draw, reward, prep, memset, sort, walk, sums, item pass, "
                    "user row, Adam on the user table) plus one row memset")
    for name in a.shapes.split(","):
        res["shapes"][name] = bench_shape(name, a.reps, a.warmup)
        print(name, json.dumps({k: v for k, v in res["shapes"][name].items() if k != "shape"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
