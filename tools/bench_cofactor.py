"""CoFactor timing on the MI355X (engine.CoOccurrence / engine.CoFactorSolver, cofactor.hip).

    python tools/bench_cofactor.py [out.json]            # device: FilmTrust and the Yelp2018 shape, d = 64
    python tools/bench_cofactor.py --host [out.json]     # the one-core CPU baselines of the same cases (no GPU needed)

Per device case, one JSON line: ms of the SPPMI build split into the count pass, the fill pass and the host part (logarithms,
neighbour order), the kept directed pairs, the level schedule's depth and width, and ms per epoch (median of the timed epochs)
split into the user half and the item half.  ``-filter`` of the Yelp2018 shape is the smallest of FILTERS whose kept pairs fit
CAPACITY directed entries (found with the count pass alone, recorded in the output).
Per host case: a scipy.sparse product B^T B with the thresholds applied (the honest CPU way to the counts), the same host
SPPMI part, and one epoch of the numpy host mirror of tests/test_cofactor_cpu.py, all on one core.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

D, NEG, LAM, GAMMA = 64, 5, 1.0, 0.01
FILTERS = (2, 5, 10, 20, 40, 80)
CAPACITY = 2_000_000


def filmtrust_graph():
    import numpy as np
    from test_wrmf_cpu import train_pairs
    z = np.load(os.path.join(ROOT, "tests", "golden", "cofactor_filmtrust.npz"))
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_cofactor_meta.json")))["cofactor_filmtrust"]
    u, i, r = train_pairs(z, meta["n_items"])
    return meta["n_users"], meta["n_items"], u, i, r


def yelp_graph():
    import numpy as np
    from qrec_amd.synth import make_dataset
    g = make_dataset("yelp2018")
    u, i = g["train_u"].astype(np.int64), g["train_i"].astype(np.int64)
    return g["n_users"], g["n_items"], u, i, np.ones(u.size)


def start(U, I):
    import numpy as np
    rng = np.random.default_rng(1)
    return (rng.random((U, D)) / 3 * 10, rng.random((I, D)) / 3 * 10, rng.random((I, D)) / 10, rng.random(I) / 10, rng.random(I) / 10)


def device_case(name, U, I, u, i, r, filters, epochs):
    import numpy as np
    from qrec_amd import capi
    from qrec_amd.engine import CoFactorSolver, CoOccurrence
    CoOccurrence(u, i, U, I, filters[-1]).counts()                  # warm-up: code objects
    for filt in filters:
        co = CoOccurrence(u, i, U, I, filt)
        views = (co.d_i_indptr, co.d_i_users, I, co.nnz, co.d_u_indptr, co.d_u_items, U, co.nnz, filt)
        if capi.cooc_count(*views, co.d_ws, co.ws_bytes) <= CAPACITY:
            break
    co.capacity = CAPACITY
    sppmi = co.sppmi(NEG)
    X, Y, G, w, c = start(U, I)
    t0 = time.perf_counter()
    s = CoFactorSolver(X, Y, G, w, c, u, i, r, sppmi, LAM, GAMMA)
    setup_ms = (time.perf_counter() - t0) * 1e3
    s.epoch()                                                       # warm-up
    rows = []
    for _ in range(epochs):
        t0 = time.perf_counter(); s.epoch(); rows.append(((time.perf_counter() - t0) * 1e3, s.timings["user_half_ms"], s.timings["item_half_ms"]))
    capi.device_sync()
    med = np.median(np.array(rows), axis=0)
    return dict(case=name, users=U, items=I, nnz=int(u.size), d=D, filter=filt, k=NEG, capacity=CAPACITY, kept_pairs=int(co.kept),
                sppmi_count_ms=round(co.timings["count_ms"], 3), sppmi_fill_ms=round(co.timings["fill_ms"], 3),
                sppmi_host_ms=round(co.timings["host_ms"], 3), solver_setup_ms=round(setup_ms, 3), schedule=s.schedule,
                epochs_timed=epochs, ms_per_epoch=round(float(med[0]), 3), user_half_ms=round(float(med[1]), 3),
                item_half_ms=round(float(med[2]), 3), item_workspace_bytes=int(s.item_ws_bytes))


def host_case(name, U, I, u, i, r, filt):
    import numpy as np
    from qrec_amd.engine import sppmi_from_counts
    from test_cofactor_cpu import item_sweep, product_counts
    from test_wrmf_cpu import csr, half_sweep
    t0 = time.perf_counter()
    counts = product_counts(u, i, U, I, filt)
    t1 = time.perf_counter()
    sppmi = sppmi_from_counts(*counts, NEG)
    t2 = time.perf_counter()
    X, Y, G, w, c = start(U, I)
    conf = 10.0 * r
    half_sweep(Y, X, *csr(u, i, conf, U), LAM, True)
    t3 = time.perf_counter()
    item_sweep(X, Y, G, w, c, csr(i, u, conf, I), sppmi, LAM, GAMMA)
    t4 = time.perf_counter()
    return dict(case=name + "_host_one_core", users=U, items=I, nnz=int(u.size), d=D, filter=filt, k=NEG, kept_pairs=int(counts[1].size),
                scipy_product_ms=round((t1 - t0) * 1e3, 3), sppmi_host_ms=round((t2 - t1) * 1e3, 3),
                mirror_user_half_ms=round((t3 - t2) * 1e3, 3), mirror_item_half_ms=round((t4 - t3) * 1e3, 3))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    if "--host" in sys.argv:
        if os.environ.get("OMP_NUM_THREADS") != "1":       # one core: a fresh interpreter with the BLAS pools at one thread
            env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            return subprocess.call([sys.executable] + sys.argv, env=env)
        yelp_filter = int(os.environ.get("QREC_BENCH_YELP_FILTER", FILTERS[0]))     # the filter the device run settled on
        res = [host_case("filmtrust_d64", *filmtrust_graph(), 2), host_case("yelp2018_d64", *yelp_graph(), yelp_filter)]
    else:
        res = [device_case("filmtrust_d64", *filmtrust_graph(), (2,), 10), device_case("yelp2018_d64", *yelp_graph(), FILTERS, 5)]
    for x in res:
        print(json.dumps(x), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
