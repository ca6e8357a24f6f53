"""Bits and device time of the order-exact walkers (sgd_walkers.hip, social.hip, bpr_levels_kernel of bpr_exact.hip), for
comparing two builds of libqrec_hip.so: every walker is deterministic, so a build reproduces another bit for bit or differs.

    python tools/walker_bits.py bits LABEL [--lib PATH] [--out profiles/refactor_walkers_bits.json]
    python tools/walker_bits.py time LABEL [--lib PATH] [--out profiles/refactor_walkers_speed.json]

``bits``: seeded inputs at d = 10, 64, 65, 128, 129, 200 (LOCABAL: up to 128), both dtypes where the entry point has two,
through the seven *_sgd_ordered entry points, qrec_bpr_sgd_scheduled, qrec_social_user_pass in its three modes and
qrec_sorec_relation_pass; one SHA-256 per leg over every output table (pad columns included) and the loss.
``time``: device time per call (events, median of 20 after 3 warm-up calls) at about 35,000 steps, the size these passes run at.
The result goes under LABEL into the JSON file, next to what other runs left there; ``--lib`` loads another build of the
library in the place of the tree's own.  Only calls that every build since the social models has are used."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (10, 64, 65, 128, 129, 200)
LR, REG_U, REG_I = 0.02, 0.01, 0.02


def problem(seed, U, I, n, n_rel):
    """index streams first, tables later: the streams of a leg are the same at every width"""
    rng = np.random.default_rng(seed)
    p = dict(U=U, I=I, n=n, rng=rng)
    p["u"] = np.sort(rng.integers(0, U, n)).astype(np.int32)             # user-major, as the reference walks
    p["i"], p["b"] = (rng.integers(0, I, n, dtype=np.int32) for _ in range(2))      # b: TBPR's second item, b == i happens
    p["j"] = ((p["i"] + rng.integers(1, I, n)) % I).astype(np.int32)                 # a negative is never the positive
    p["r"] = rng.integers(1, 11, n) / 2.0
    a, b = rng.integers(0, U, n_rel), rng.integers(0, U, n_rel)
    keep = a != b
    p["rel"] = (a[keep].astype(np.int32), b[keep].astype(np.int32), rng.random(int(keep.sum())) * 0.9 + 0.1)
    k = np.where(rng.random(n) < 0.4, -1, rng.integers(0, I, n))
    jj = np.where((k >= 0) & (rng.random(n) < 0.2), k, p["j"])
    rows = np.stack([p["u"], p["i"], k, jj, np.where(k >= 0, rng.integers(1, 5, n), 0)], axis=1)
    rows[rng.random(n) < 0.02, 1:] = (-1, -1, -1, 0)                     # bare visits
    p["sbpr_rows"] = np.ascontiguousarray(rows, dtype=np.int32)
    return p


def legs(p, d, dtype, which):
    """(name, launch, outputs) per requested leg: launch() enqueues the pass once more on the same tables"""
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer as DB
    from qrec_amd.engine import DeviceTables, SocialHSgd, SocialSgd
    from qrec_amd.interactions import user_item_csr
    from qrec_amd.social import synthetic_graph_steps
    U, I, n, rng = p["U"], p["I"], p["n"], p["rng"]
    tab = lambda rows, scale=3.0: rng.random((rows, d)) / scale
    dev = DB.from_numpy
    d_u, d_i, d_j, d_b, d_r = dev(p["u"]), dev(p["i"]), dev(p["j"]), dev(p["b"]), dev(p["r"])
    f64 = dtype == np.float64

    def tables():
        return DeviceTables(tab(U), tab(I), dtype)

    def sums_of(t):
        """{sum P^2, sum Q^2} of the uploaded tables, summed on the host: one fixed order (qrec_sumsq adds block sums atomically)"""
        return dev(np.array([float((x.numpy().astype(np.float64) ** 2).sum()) for x in (t.P, t.Q)]))

    for name in which:
        if name == "bpr":
            t, loss = tables(), DB.zeros(1, np.float64)
            yield name, (lambda t=t, loss=loss: capi.bpr_sgd_ordered(t.P, t.Q, t.code, d, t.ld, d_u, d_i, d_j, n, LR, REG_U, REG_I, loss)), (t.P, t.Q, loss)
        elif name == "tbpr":
            t, loss = tables(), DB.zeros(2, np.float64)
            sums = sums_of(t)
            yield name, (lambda t=t, loss=loss, sums=sums: capi.tbpr_sgd_ordered(t.P, t.Q, t.code, d, t.ld, d_u, d_i, d_b, n, LR, REG_U, REG_I, sums,
                                                                                 loss)), (t.P, t.Q, loss)
        elif name == "sbpr":
            t, loss = tables(), DB.zeros(2, np.float64)
            bias = rng.random(I)
            sums, d_b, d_rows = sums_of(t), dev(bias.astype(dtype)), dev(p["sbpr_rows"])
            yield name, (lambda t=t, loss=loss, sums=sums, d_b=d_b, d_rows=d_rows, bb=float(bias.dot(bias)):
                         capi.sbpr_sgd_ordered(t.P, t.Q, d_b, t.code, d, t.ld, d_rows, n, LR, REG_U, REG_I, bb, sums, loss)), (t.P, t.Q, loss)
        elif name.startswith("mf"):
            variant = int(name[2:])
            t, loss = tables(), DB.zeros(1, np.float64)
            Bu, Bi = dev((rng.random(U) / 5).astype(dtype)), dev((rng.random(I) / 5).astype(dtype))
            yield name, (lambda t=t, loss=loss, Bu=Bu, Bi=Bi, variant=variant:
                         capi.mf_sgd_ordered(t.P, t.Q, t.code, d, t.ld, d_u, d_i, d_r, n, 0.01, loss, None, variant, REG_U, REG_I, Bu, Bi, 0.05, 3.0)), \
                (t.P, t.Q, Bu, Bi, loss)
        elif name == "svdpp":
            t, loss = tables(), DB.zeros(1, np.float64)
            rated = user_item_csr(p["u"], p["i"], p["r"], U, I)
            Yp = np.zeros((I, t.ld), dtype); Yp[:, :d] = tab(I)
            Y, Bu, Bi = dev(Yp), dev((rng.random(U) / 5).astype(dtype)), dev((rng.random(I) / 5).astype(dtype))
            ptr, items = dev(rated.indptr.astype(np.int64)), dev(rated.indices.astype(np.int32))
            yield name, (lambda t=t, loss=loss, Y=Y, Bu=Bu, Bi=Bi, ptr=ptr, items=items:
                         capi.svdpp_sgd_ordered(t.P, t.Q, Y, Bu, Bi, t.code, d, t.ld, ptr, items, d_u, d_i, d_r, n, 0.01, REG_U, REG_I, 0.05, 0.03, 3.0,
                                                loss)), (t.P, t.Q, Y, Bu, Bi, loss)
        elif name == "scheduled":
            t, loss = tables(), DB.zeros(1, np.float64)
            width = min(8, capi.bpr_exact_width(t.code, d))
            entries, off = capi.bpr_exact_schedule(p["u"], p["i"], p["j"], U, I, width)
            d_e, d_off = dev(entries), dev(off)
            xlog, scratch = DB(n + capi.EXACT_XLOG_PAD, dtype), DB.zeros(capi.EXACT_SCRATCH_WORDS, np.float64)
            yield name, (lambda t=t, loss=loss, d_e=d_e, d_off=d_off, steps=int(off.size - 1), width=width, xlog=xlog, scratch=scratch:
                         capi.bpr_sgd_scheduled(t.P, t.Q, t.code, d, t.ld, d_e, d_off, steps, width, n, LR, REG_U, REG_I, xlog, scratch, loss)), \
                (t.P, t.Q, loss)
        elif not f64:
            continue                                                     # the social passes are fp64 only
        elif name == "rste":
            t = tables()
            s = SocialSgd(t, n, "RSTE", synthetic_graph_steps("RSTE", U, *p["rel"]))
            s.d_u.upload(p["u"]); s.d_i.upload(p["i"]); s.d_r.upload(p["r"])
            yield name, (lambda t=t, s=s: capi.rste_sgd_ordered(t.P, t.Q, d, t.ld, s.d_fe_ptr, s.d_fe_ids, s.d_fe_w, s.d_den, s.d_u, s.d_i, s.d_r, n,
                                                                LR, 0.6, REG_U, REG_I, s.d_stats)), (t.P, t.Q, s.d_stats)
        elif name == "locabal":
            if d > capi.SOCIAL_H_MAX_D:
                continue
            t = tables()
            edges, W = synthetic_graph_steps("LOCABAL", U, *p["rel"])
            s = SocialHSgd(t, n, "LOCABAL", edges, rng.random((d, d)) / d, W=W)
            s.d_u.upload(p["u"]); s.d_i.upload(p["i"]); s.d_r.upload(p["r"] / 5)
            yield name, (lambda t=t, s=s: capi.locabal_sgd_ordered(t.P, t.Q, d, t.ld, s.d_W, s.d_u, s.d_i, s.d_r, n, LR, REG_U, REG_I, s.d_stats)), \
                (t.P, t.Q, s.d_stats)
        else:                                                            # the level-scheduled social passes, through the engine
            kind = {"user_socialmf": "SocialMF", "user_soreg": "SoReg", "user_sree": "SREE", "sorec": "SoRec"}[name]
            t = tables()
            s = SocialSgd(t, 1, kind, synthetic_graph_steps(kind, U, *p["rel"]), Z=tab(U, 10.0), Bu=rng.random(U) / 10, Bi=rng.random(I) / 10)
            outs = (t.P, s.d_Z, s.d_stats) if kind == "SoRec" else (t.P, s.d_stats)      # d_stats: the slots folded in walk order
            yield name, (lambda s=s: s.social_pass(0.05, 0.3, 0.1)), outs


BITS_LEGS = ("bpr", "tbpr", "sbpr", "mf0", "mf1", "mf2", "mf3", "mf4", "svdpp", "scheduled", "rste", "locabal", "user_socialmf", "user_soreg",
             "user_sree", "sorec")
TIME_LEGS = (("bpr", 64), ("mf1", 10), ("svdpp", 10), ("tbpr", 20), ("sbpr", 20), ("rste", 10), ("scheduled", 64))


def run_bits():
    from qrec_amd import capi
    out = {}
    for d in DIMS:
        for dtype in (np.float64, np.float32):
            p = problem(1000 + d, U=60, I=50, n=700, n_rel=300)
            for name, launch, outputs in legs(p, d, dtype, BITS_LEGS):
                launch()
                capi.device_sync()
                h = hashlib.sha256()
                for buf in outputs:
                    h.update(buf.numpy().tobytes())
                out[f"{name}/d{d}/{np.dtype(dtype).name}"] = h.hexdigest()
    return out


def run_time(repeats=20, warmup=3):
    from qrec_amd import capi
    out = {}
    for name, d in TIME_LEGS:
        p = problem(7, U=1500, I=2000, n=35_000, n_rel=1800)
        for _, launch, _ in legs(p, d, np.float64, (name,)):
            for _ in range(warmup):
                launch()
            ms = []
            for _ in range(repeats):
                e0, e1 = capi.Event(), capi.Event()
                e0.record(); launch(); e1.record(); e1.sync()
                ms.append(e1.elapsed_ms_since(e0))
            out[f"{name}/d{d}"] = dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("bits", "time"))
    ap.add_argument("label")
    ap.add_argument("--lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    from qrec_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    capi.init(0)
    res = run_bits() if a.mode == "bits" else run_time()
    path = a.out or os.path.join(ROOT, "profiles", "refactor_walkers_bits.json" if a.mode == "bits" else "refactor_walkers_speed.json")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc["device"] = capi.device_info()["arch"]
    if a.mode == "bits":
        doc.setdefault("runs", {})[a.label] = res
        runs = list(doc["runs"].values())
        doc["legs"] = len(res)
        doc["unequal_legs"] = sorted(k for k in runs[0] if any(r.get(k) != runs[0][k] for r in runs[1:]))
    else:
        doc.setdefault("runs", {}).setdefault(a.label, []).append(res)      # one entry per process
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(a.mode, a.label, len(res), "legs ->", path, flush=True)


if __name__ == "__main__":
    main()
