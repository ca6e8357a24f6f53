"""SoRec / SoReg / SocialMF / RSTE / SREE timing on the MI355X (engine.SocialSgd, social.hip, mf_ordered_kernel).

    python tools/bench_social.py [out.json]          # default out: profiles/social_bench.json

Two workloads, d = 10: FilmTrust (tests/golden/social_*_filmtrust.npz: the training rows and the kept relation list) and an
Epinions-like shape (40,000 users, 140,000 items, 660,000 ratings, 490,000 trust edges; synth.gen_edges, seeded).  Per
model and epoch: the rating pass and the social pass (each call ends in a device synchronisation), the social pass'
level count and mean width; the social pass again at width 1 (social.sequential_schedule) on the same tables; and at
FilmTrust the one-core numpy host mirror (tests/social_mirror.py) of both passes.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODELS = ("SoRec", "SoReg", "SocialMF", "RSTE", "SREE")
EPOCHS = 3


def filmtrust():
    z = np.load(os.path.join(ROOT, "tests", "golden", "social_sorec_filmtrust.npz"))
    u, i, r = z["order0_u"].astype(np.int32), z["order0_i"].astype(np.int32), z["order0_r"]
    keep = (z["raw_follower"] >= 0) & (z["raw_followee"] >= 0)
    return dict(U=int(z["P"].shape[0]), I=int(z["Q"].shape[0]), u=u, i=i, r=r, a=z["raw_follower"][keep], b=z["raw_followee"][keep],
                w=z["raw_weight"][keep], raw=(z["raw_follower"].tolist(), z["raw_followee"].tolist(), z["raw_weight"].tolist()))


def epinions_like(seed=11, U=40_000, I=140_000, n_ratings=660_000, n_edges=490_000):
    from qrec_amd.synth import gen_edges
    rng = np.random.default_rng(seed)
    u, i = gen_edges(U, I, n_ratings, seed)
    perm = rng.permutation(u.size)
    a, b = gen_edges(U, U, n_edges, seed + 1)
    return dict(U=U, I=I, u=u[perm].astype(np.int32), i=i[perm].astype(np.int32), r=rng.integers(1, 11, u.size) / 2.0,
                a=a.astype(np.int32), b=b.astype(np.int32), w=np.ones(a.size))


def bench_model(kind, wl, d=10, seed=0):
    from qrec_amd.engine import DeviceTables, SocialSgd
    from qrec_amd.social import sequential_schedule, synthetic_graph_steps
    rng = np.random.default_rng(seed)
    U, I = wl["U"], wl["I"]
    t0 = time.perf_counter()
    steps = synthetic_graph_steps(kind, U, wl["a"], wl["b"], wl["w"])
    host_steps_s = time.perf_counter() - t0
    t = DeviceTables(rng.random((U, d)) / 3, rng.random((I, d)) / 3, np.float64)
    t0 = time.perf_counter()
    s = SocialSgd(t, wl["u"].size, kind, steps, Z=rng.random((U, d)) / 10, Bu=rng.random(U) / 10, Bi=rng.random(I) / 10)
    setup_s = time.perf_counter() - t0
    out = dict(model=kind, host_steps_s=round(host_steps_s, 3), setup_incl_schedule_s=round(setup_s, 3), epochs=[])
    lr, coef = 0.005, 0.1
    if kind != "RSTE":
        out.update(n_steps=s.n_steps, n_levels=s.schedule.n_levels, mean_width=round(s.n_steps / max(s.schedule.n_levels, 1), 2),
                   max_width=s.schedule.max_width, n_waves=s.n_waves)
    for ep in range(EPOCHS):
        t0 = time.perf_counter()
        s.rating_pass(wl["u"], wl["i"], wl["r"], lr, 0.01, 0.01, 0.01, 3.0, alpha=0.5)
        t1 = time.perf_counter()
        rec = dict(rating_pass_ms=round(1e3 * (t1 - t0), 3))
        if kind != "RSTE":
            s.social_pass(lr, coef, 0.1)
            rec["social_pass_ms"] = round(1e3 * (time.perf_counter() - t1), 3)
        out["epochs"].append(rec)
    if kind != "RSTE":
        level = s.schedule
        s.set_schedule(sequential_schedule(s.n_steps))
        w1 = []
        for _ in range(EPOCHS):
            t0 = time.perf_counter()
            s.social_pass(lr, coef, 0.1)
            w1.append(round(1e3 * (time.perf_counter() - t0), 3))
        s.set_schedule(level)
        out["social_pass_width1_ms"] = w1
    P, Q = t.download()
    out["finite"] = bool(np.isfinite(P).all() and np.isfinite(Q).all())
    return out


def mirror_filmtrust(kind, wl, d=10, seed=0):
    """one epoch of the one-core numpy host mirror at FilmTrust: (rating pass s, social pass s)"""
    import social_mirror as M
    rng = np.random.default_rng(seed)
    U, I = wl["U"], wl["I"]
    P, Q, Z = rng.random((U, d)) / 3, rng.random((I, d)) / 3, rng.random((U, d)) / 10
    Bu, Bi = rng.random(U) / 10, rng.random(I) / 10
    g = M.Graph(*wl["raw"])
    rows = list(zip(wl["u"].tolist(), wl["i"].tolist(), wl["r"].tolist()))
    t0 = time.perf_counter()
    if kind == "RSTE":
        M.rating_rste(P, Q, g, rows, 0.005, 0.5, 0.01, 0.01)
    elif kind == "SREE":
        M.rating_ee(P, Q, Bu, Bi, rows, 0.005, 0.01, 0.01, 0.01, 3.0)
    else:
        M.rating_pmf(P, Q, rows, 0.005, 0.01, 0.01, copies=kind == "SocialMF")
    t1 = time.perf_counter()
    if kind == "RSTE":
        return t1 - t0, None
    if kind == "SoRec":
        sp = M.RelationPass(g, U); slots = np.zeros(sp.n_slots)
        for k in range(sp.n_steps):
            sp.step(P, Z, k, 0.005, 0.1, 0.1, slots)
    else:
        sim = None
        if kind == "SoReg":
            sim = {}
            for u in range(U):
                for f, w in g.fe(u).items():
                    sim.setdefault(u, {})[f] = w; sim.setdefault(f, {})[u] = w
        sp = M.UserPass(kind, g, sim); slots = np.zeros(sp.n_slots)
        for k in range(sp.n_steps):
            sp.step(P, k, 0.005, 0.1, slots)
    return t1 - t0, time.perf_counter() - t1


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "social_bench.json")
    from qrec_amd import capi
    capi.init(0)
    res = dict(device=capi.device_info()["arch"], d=10, epochs_timed=EPOCHS, workloads={})
    for name, wl in (("filmtrust", filmtrust()), ("epinions_like", epinions_like())):
        rows = []
        for kind in MODELS:
            r = bench_model(kind, wl)
            if name == "filmtrust":
                rs, ss = mirror_filmtrust(kind, wl)
                r["host_mirror_rating_pass_ms"] = round(1e3 * rs, 1)
                if ss is not None:
                    r["host_mirror_social_pass_ms"] = round(1e3 * ss, 1)
            rows.append(r)
            print(name, json.dumps(r), flush=True)
        res["workloads"][name] = dict(n_users=wl["U"], n_items=wl["I"], n_ratings=int(wl["u"].size), n_relations=int(wl["a"].size),
                                      models=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
