"""WRMF / ALS epoch timing on the MI355X (engine.AlsSolver, als.hip).

    python tools/bench_wrmf.py [out.json]            # device: Yelp2018 shape (d = 64) and lastfm at the stock WRMF.conf
    python tools/bench_wrmf.py --host [out.json]     # the numpy host mirror (tests/test_wrmf_cpu.py) on ONE core, Yelp2018 shape

Prints one JSON line per case: ms per epoch (median of the timed epochs; an epoch ends in the loss read-back, so the host
clock around it measures the device work), the fp64 operations the epoch executes, counted from the CSR and the shapes:
  Gram     2 ld^2 per row of the table multiplied (the kernel runs the whole padded ld x ld block)
  accum    2 ld^2 + 2 ld per CSR entry (the padded rank-1 update and b); the symmetric half alone is d (d + 1) per entry
  solve    d^3 / 3 (Cholesky) + 2 d^2 (the two triangular solves) per row
and the achieved rate.  The kernel split comes from a run of this script under rocprofv3 --kernel-trace --stats.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def yelp_graph():
    import numpy as np
    from qrec_amd.synth import make_dataset
    g = make_dataset("yelp2018")
    u, i = g["train_u"].astype(np.int64), g["train_i"].astype(np.int64)
    return g["n_users"], g["n_items"], u, i, np.ones(u.size)


def lastfm_graph():
    import numpy as np
    from test_wrmf_cpu import train_pairs
    z = np.load(os.path.join(ROOT, "tests", "golden", "wrmf_lastfm.npz"))
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_wrmf_meta.json")))["wrmf_lastfm"]
    u, i, r = train_pairs(z, meta["n_items"])
    return meta["n_users"], meta["n_items"], u, i, r


def flops(U, I, nnz, d, ld):
    gram = 2 * ld * ld * (I + U)
    accum = 2 * nnz * (2 * ld * ld + 2 * ld)
    sym = 2 * nnz * d * (d + 1)
    solve = (U + I) * (d ** 3 / 3 + 2 * d * d)
    return dict(gram=gram, accum_executed=accum, accum_symmetric=sym, solve=solve, total_executed=gram + accum + solve)


def device_case(name, U, I, u, i, r, d, lam, epochs):
    import numpy as np
    from qrec_amd import capi
    from qrec_amd.engine import AlsSolver, padded_ld
    rng = np.random.default_rng(1)
    X0, Y0 = rng.random((U, d)) / 3 * 10, rng.random((I, d)) / 3 * 10
    s = AlsSolver(X0, Y0, u, i, r, lam)
    s.epoch()                                      # warm-up: code objects, first touches
    times = []
    for _ in range(epochs):
        t0 = time.perf_counter(); s.epoch(); times.append((time.perf_counter() - t0) * 1e3)
    capi.device_sync()
    ms = float(np.median(times))
    f = flops(U, I, u.size, d, padded_ld(d, np.float64))
    deg_i = np.bincount(i, minlength=I)
    deg_u = np.bincount(u, minlength=U)
    from qrec_amd.capi import load
    return dict(case=name, users=U, items=I, nnz=int(u.size), d=d, epochs_timed=epochs, ms_per_epoch=round(ms, 4),
                ms_min=round(min(times), 4), ms_max=round(max(times), 4), flop=f,
                tflops_executed=round(f["total_executed"] / ms * 1e-9, 3),
                max_item_degree=int(deg_i.max()), max_user_degree=int(deg_u.max()),
                split_rows=int((deg_i > 512).sum() + (deg_u > 512).sum()))


def host_case(U, I, u, i, r, d, lam):
    import numpy as np
    from test_wrmf_cpu import csr, half_sweep
    rng = np.random.default_rng(1)
    X, Y = rng.random((U, d)) / 3 * 10, rng.random((I, d)) / 3 * 10
    c = 10.0 * r
    t0 = time.perf_counter()
    half_sweep(Y, X, *csr(u, i, c, U), lam, True)
    half_sweep(X, Y, *csr(i, u, c, I), lam, False)
    return dict(case="host_mirror_yelp2018_one_core", users=U, items=I, nnz=int(u.size), d=d,
                s_per_epoch=round(time.perf_counter() - t0, 3))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    if "--host" in sys.argv:
        if os.environ.get("OMP_NUM_THREADS") != "1":       # one core: a fresh interpreter with the BLAS pools at one thread
            env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            return subprocess.call([sys.executable] + sys.argv, env=env)
        res = [host_case(*yelp_graph(), 64, 1.0)]
    else:
        res = [device_case("yelp2018_d64", *yelp_graph(), 64, 1.0, 10),
               device_case("lastfm_wrmf_conf_d20", *lastfm_graph(), 20, 1.0, 10)]
    for x in res:
        print(json.dumps(x))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
