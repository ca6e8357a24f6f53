"""SoRec / SoReg / SocialMF / RSTE / SREE timing on the MI355X (engine.SocialSgd, social.hip, mf_ordered_kernel of sgd_walkers.hip).

    python tools/bench_social.py [out.json]          # default out: profiles/social_bench.json

Two workloads, d = 10: FilmTrust (tests/golden/social_*_filmtrust.npz: the training rows and the kept relation list) and an
Epinions-like shape (40,000 users, 140,000 items, 660,000 ratings, 490,000 trust edges; synth.gen_edges, seeded).  Per
model and epoch: the rating pass and the social pass (each call ends in a device synchronisation), the social pass'
level count and mean width; the social pass again at width 1 (social.sequential_schedule) on the same tables; and at
FilmTrust the one-core numpy host mirror (tests/social_mirror.py) of both passes.

    python tools/bench_social.py --locabal-fd [out.json]      # default out: profiles/locabal_fd_bench.json

LOCABAL and SocialFD (engine.SocialHSgd; their passes carry a d x d matrix, one workgroup walks them step by step) at the
same two workloads, d = 10 and d = 64: the rating pass and the social pass per epoch as the median of the same repeat
count, microseconds per step (a rating; a similarity edge or followee edge), and beside them the one-core numpy mirror
(tests/locabal_fd_mirror.py) in microseconds per step over the first MIRROR_STEPS steps of each pass; then, at FilmTrust and
d = 10, 64, 128, the same passes with 1, 2, 4, 8 and 16 wavefronts in the workgroup (the results do not depend on it).
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


H_MODELS = ("LOCABAL", "SocialFD")
H_DIMS = (10, 64)
MIRROR_STEPS = 20_000
SWEEP_DIMS = (10, 64, 128)
SWEEP_WAVES = (1, 2, 4, 8, 16)


def h_inputs(kind, wl, d, seed=0):
    """tables scaled so that a whole pass at either shape stays finite: ratings in (0, 1], distances under H around 1"""
    rng = np.random.default_rng(seed)
    U, I = wl["U"], wl["I"]
    r = wl["r"] / wl["r"].max()
    P, Q = rng.random((U, d)) / 3, rng.random((I, d)) / 3
    if kind == "SocialFD":
        return dict(r=r, P=P / 10, Q=Q / 10, H=rng.random((d, d)) * 2 / d, Bu=rng.random(U) / 5, Bi=rng.random(I) / 5)
    return dict(r=r, P=P, Q=Q, H=rng.random((d, d)) / d)


def bench_h_model(kind, wl, d, n_waves=0):
    from qrec_amd.engine import DeviceTables, SocialHSgd
    from qrec_amd.social import synthetic_graph_steps
    x = h_inputs(kind, wl, d)
    t0 = time.perf_counter()
    steps = synthetic_graph_steps(kind, wl["U"], wl["a"], wl["b"], wl["w"])
    host_steps_s = time.perf_counter() - t0
    t = DeviceTables(x["P"], x["Q"], np.float64)
    if kind == "LOCABAL":
        edges, W = steps
        s = SocialHSgd(t, wl["u"].size, kind, edges, x["H"], W=W, n_waves=n_waves)
    else:
        s = SocialHSgd(t, wl["u"].size, kind, steps, x["H"], Bu=x["Bu"], Bi=x["Bi"], n_waves=n_waves)
    lr = 0.001
    rating, social = [], []
    for _ in range(EPOCHS):
        t0 = time.perf_counter()
        s.rating_pass(wl["u"], wl["i"], x["r"], lr, 0.01, 0.01, 0.1, 0.3, 0.5)
        t1 = time.perf_counter()
        s.social_pass(lr, alpha=0.4, regS=0.01, eta=0.1, beta=0.1)
        t2 = time.perf_counter()
        rating.append(t1 - t0); social.append(t2 - t1)
    P, Q = t.download()
    rm, sm = float(np.median(rating)), float(np.median(social))
    return dict(model=kind, d=d, host_steps_s=round(host_steps_s, 3), n_ratings=int(wl["u"].size), n_social_edges=int(s.n_slots),
                rating_pass_ms=round(1e3 * rm, 3), social_pass_ms=round(1e3 * sm, 3),
                rating_us_per_step=round(1e6 * rm / max(wl["u"].size, 1), 3), social_us_per_step=round(1e6 * sm / max(s.n_slots, 1), 3),
                rating_pass_ms_all=[round(1e3 * v, 3) for v in rating], social_pass_ms_all=[round(1e3 * v, 3) for v in social],
                finite=bool(np.isfinite(P).all() and np.isfinite(Q).all() and np.isfinite(s.H()).all()))


def mirror_h_model(kind, wl, d):
    """the one-core numpy mirror over the first MIRROR_STEPS steps of each pass: (rating us / step, social us / step)"""
    import locabal_fd_mirror as L
    from qrec_amd.social import synthetic_graph_steps
    x = h_inputs(kind, wl, d)
    P, Q, H = x["P"].copy(), x["Q"].copy(), x["H"].copy()
    n = min(MIRROR_STEPS, wl["u"].size)
    rows = list(zip(wl["u"][:n].tolist(), wl["i"][:n].tolist(), x["r"][:n].tolist()))
    steps = synthetic_graph_steps(kind, wl["U"], wl["a"], wl["b"], wl["w"])
    if kind == "LOCABAL":
        edges, W = steps
        walk = list(zip(edges.u[:MIRROR_STEPS].tolist(), edges.k[:MIRROR_STEPS].tolist(), edges.sim[:MIRROR_STEPS].tolist()))
        t0 = time.perf_counter()
        L.rating_locabal(P, Q, W, rows, 0.001, 0.01, 0.01)
        t1 = time.perf_counter()
        L.social_locabal(P, H, walk, 0.001, 0.4, 0.01, np.zeros(len(walk)))
        m = len(walk)
    else:
        walk, m = [], 0
        for k, u in enumerate(steps.user.tolist()):
            fol = steps.fe_ids[steps.fe_ptr[k]:steps.fe_ptr[k + 1]].tolist()[:MIRROR_STEPS - m]
            walk.append((u, fol)); m += len(fol)
            if m >= MIRROR_STEPS:
                break
        Bu, Bi = x["Bu"].copy(), x["Bi"].copy()
        t0 = time.perf_counter()
        L.rating_socialfd(P, Q, Bu, Bi, H, rows, 0.001, 0.01, 0.01, 0.1, 0.3, 0.5)
        t1 = time.perf_counter()
        L.social_socialfd(P, H, walk, 0.001, 0.1, 0.1, np.zeros(m))
    t2 = time.perf_counter()
    return 1e6 * (t1 - t0) / max(n, 1), 1e6 * (t2 - t1) / max(m, 1)


def main_locabal_fd(out_path):
    from qrec_amd import capi
    capi.init(0)
    res = dict(device=capi.device_info()["arch"], repeats=EPOCHS, mirror_steps_timed=MIRROR_STEPS, workloads={})
    for name, wl in (("filmtrust", filmtrust()), ("epinions_like", epinions_like())):
        rows = []
        for kind in H_MODELS:
            for d in H_DIMS:
                r = bench_h_model(kind, wl, d)
                mr, ms = mirror_h_model(kind, wl, d)
                r["host_mirror_rating_us_per_step"], r["host_mirror_social_us_per_step"] = round(mr, 2), round(ms, 2)
                rows.append(r)
                print(name, json.dumps(r), flush=True)
        res["workloads"][name] = dict(n_users=wl["U"], n_items=wl["I"], n_ratings=int(wl["u"].size), n_relations=int(wl["a"].size),
                                      models=rows)
    # the same passes at FilmTrust under every workgroup size (a workgroup never has fewer than ceil(d / 64) wavefronts)
    wl, sweep = filmtrust(), []
    for kind in H_MODELS:
        for d in SWEEP_DIMS:
            for nw in SWEEP_WAVES:
                r = bench_h_model(kind, wl, d, nw)
                row = dict(model=kind, d=d, n_waves=max(nw, (d + 63) // 64), social_us_per_step=r["social_us_per_step"])
                if kind == "SocialFD":
                    row["rating_us_per_step"] = r["rating_us_per_step"]
                sweep.append(row)
                print("wave_sweep", json.dumps(row), flush=True)
    res["wave_sweep_filmtrust"] = sweep
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--locabal-fd":
        return main_locabal_fd(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "locabal_fd_bench.json"))
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
