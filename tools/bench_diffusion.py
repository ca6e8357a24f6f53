#!/usr/bin/env python3
"""Steady-state step time of the DiffNet and DHCF trainers and of the dense-layer kernels (device events), at the reference's
lastfm shape (1,892 x 17,632, batch 2000, d = 50: the stock confs) and the Yelp2018 shape (31,668 x 38,048, d = 64, batch
2048), on synthetic graphs of those sizes.  The forward dense kernel with two operands is timed against qrec_ngcf_dense_fwd at
equal n and ld in the same run (same flops, same tables read and written).

    python tools/bench_diffusion.py [--out profiles/diffusion_bench.json] [--reps 30] [--warmup 10]
    python tools/bench_diffusion.py --model DHCF --steps 40     # a plain loop of steps, for a kernel trace
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qrec_amd import capi                                          # noqa: E402
from qrec_amd.capi import DeviceBuffer                             # noqa: E402
from qrec_amd.diffusion import rating_mean_csr, social_csr         # noqa: E402
from qrec_amd.engine import padded_ld                              # noqa: E402
from qrec_amd.graph import DHCFTrainer, DiffNetTrainer, NGCFTrainer, joint_norm_adjacency   # noqa: E402

SHAPES = {"lastfm": dict(nu=1892, ni=17632, nnz=92834, n_rel=25434, d=50, B=2000),
          "yelp2018": dict(nu=31668, ni=38048, nnz=1237259, n_rel=120000, d=64, B=2048)}


def synthetic(nu, ni, nnz, n_rel, d, B, seed=0):
    rng = np.random.default_rng(seed)
    pairs = np.unique(np.stack([rng.integers(0, nu, nnz), rng.integers(0, ni, nnz)], 1), axis=0)
    uid, iid = pairs[:, 0].astype(np.int32), pairs[:, 1].astype(np.int32)
    rel = np.unique(np.stack([rng.integers(0, nu, n_rel), rng.integers(0, nu, n_rel)], 1), axis=0)
    b = rng.integers(0, uid.size, B)
    U = (rng.standard_normal((nu, d)) * 0.1).astype(np.float32); V = (rng.standard_normal((ni, d)) * 0.1).astype(np.float32)
    xav = lambda r, c: rng.uniform(-np.sqrt(6.0 / (r + c)), np.sqrt(6.0 / (r + c)), (r, c)).astype(np.float32)
    return dict(uid=uid, iid=iid, fo=rel[:, 0], fe=rel[:, 1], u=uid[b], i=iid[b], j=rng.integers(0, ni, B).astype(np.int32), U=U, V=V, xav=xav)


def median_ms(fn, reps, warmup):
    """median and spread of `reps` single-call timings by device events, after `warmup` untimed calls"""
    for _ in range(warmup):
        fn()
    capi.device_sync()
    a, b, ms = capi.Event(), capi.Event(), []
    for _ in range(reps):
        a.record(); fn(); b.record(); b.sync()
        ms.append(b.elapsed_ms_since(a))
    ms = np.sort(ms)
    return dict(median_ms=float(np.median(ms)), p10_ms=float(ms[len(ms) // 10]), p90_ms=float(ms[(9 * len(ms)) // 10]), reps=reps)


def make(model, shape):
    s = SHAPES[shape]; g = synthetic(**s)
    d = s["d"]
    if model == "DiffNet":
        tr = DiffNetTrainer(g["U"], g["V"], [g["xav"](2 * d, d) for _ in range(2)], social_csr(s["nu"], g["fo"], g["fe"]),
                            rating_mean_csr(s["nu"], s["ni"], g["uid"], g["iid"]), 0.001, 0.01, 2)
    elif model == "DHCF":
        tr = DHCFTrainer(g["U"], g["V"], [g["xav"](d, d) for _ in range(2)], g["uid"], g["iid"], 0.001, 0.01)
    else:
        tr = NGCFTrainer(g["U"], g["V"], [[g["xav"](d, d), g["xav"](d, d)] for _ in range(2)],
                         joint_norm_adjacency(s["nu"], s["ni"], g["uid"], g["iid"]), 0.001, 0.01)
    batch = tuple(DeviceBuffer.from_numpy(g[k]) for k in ("u", "i", "j"))
    return tr, batch, s


def kernel_times(shape, reps, warmup):
    """the dense-layer entry points on [n][ld] tables of this shape's joint row count, and qrec_ngcf_dense_fwd beside them"""
    s = SHAPES[shape]
    n, ld = s["nu"] + s["ni"], padded_ld(s["d"], np.float32)
    rng = np.random.default_rng(1)
    t = lambda: DeviceBuffer.from_numpy(rng.standard_normal((n, ld)).astype(np.float32))
    X1, X2, R, dY, Y, g1, g2 = t(), t(), t(), t(), t(), t(), t()
    W = DeviceBuffer.from_numpy((rng.standard_normal((2, ld, ld)) * 0.1).astype(np.float32))
    W2 = capi.DeviceSlice(W, ld * ld, (ld, ld))
    gW = DeviceBuffer.zeros((2, ld, ld), np.float32)
    ws = DeviceBuffer(capi.dense_layer_ws_bytes(n, ld, 2), np.uint8)
    out = dict(n_rows=n, ld=ld)
    out["dense_layer_fwd_two_operands_relu"] = median_ms(lambda: capi.dense_layer_fwd(X1, X2, W, None, n, ld, True, Y), reps, warmup)
    out["ngcf_dense_fwd"] = median_ms(lambda: capi.ngcf_dense_fwd(X1, X2, W, W2, n, ld, Y), reps, warmup)
    out["fwd_two_operands_over_ngcf_dense_fwd"] = out["dense_layer_fwd_two_operands_relu"]["median_ms"] / out["ngcf_dense_fwd"]["median_ms"]
    out["dense_layer_fwd_one_operand_residual"] = median_ms(lambda: capi.dense_layer_fwd(X1, None, W, R, n, ld, False, Y), reps, warmup)
    out["dense_layer_dpre_relu"] = median_ms(lambda: capi.dense_layer_dpre_relu(dY, Y, n, ld, g2), reps, warmup)
    out["dense_layer_bwd_two_operands"] = median_ms(lambda: capi.dense_layer_bwd(dY, X1, X2, W, n, ld, g1, g2, gW, ws), reps, warmup)
    out["dense_layer_bwd_one_operand"] = median_ms(lambda: capi.dense_layer_bwd(dY, X1, None, W, n, ld, g1, None, gW, ws), reps, warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default=None, help="with --steps: run a plain loop of this model's steps (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--shape", default="yelp2018")
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()
    capi.init(0)
    if a.steps:
        tr, (u, i, j), s = make(a.model, a.shape)
        for _ in range(a.steps):
            tr.train_step_async(u, i, j, s["B"])
        print(json.dumps(dict(model=a.model, shape=a.shape, steps=a.steps, loss=tr.loss())))
        return
    res = dict(device=capi.device_info().get("arch"), timer="device events around one call; median of reps after warm-up", shapes={})
    for shape in SHAPES:
        row = dict(SHAPES[shape], kernels=kernel_times(shape, a.reps, a.warmup))
        for model in ("DiffNet", "DHCF", "NGCF"):
            tr, (u, i, j), s = make(model, shape)
            row[f"{model}_step"] = median_ms(lambda: tr.train_step_async(u, i, j, s["B"]), a.reps, a.warmup)
            assert np.isfinite(tr.loss())
        res["shapes"][shape] = row
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
