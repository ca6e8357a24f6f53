"""ExpoMF / SERec epoch timing on the MI355X (engine.ExposureSolver, exposure.hip).

    python tools/bench_expo.py [out.json]            # device: lastfm at the stock ExpoMF.conf (d = 50), the Yelp2018 shape
                                                     # (d = 64), SERec on lastfm with its trust graph (d = 20)
    python tools/bench_expo.py --host [out.json]     # the numpy host mirror (tests/test_expo_cpu.py) on ONE core, on a row
                                                     # subsample of the Yelp2018 shape, extrapolated to a whole epoch

Prints one JSON line per case: ms per epoch (median of the timed epochs; every call of an epoch ends in a status read-back,
so the host clock around it measures the device work) and the fp64 operations the epoch executes, counted from the shapes:
  gram     2 * 16^2 * 4 per MFMA, NT = T (T + 1) / 2 lower-triangle 16 x 16 tiles (T = ld / 16) per row, one k-step per 4
           columns (the dense pass over every column, both halves) and per 4 observed entries (the correction)
  post     2 d per (row, column) pair for x_r . f_c: both halves and the prior pass
  solve    d^3 / 3 + 2 d^2 per row
with the fraction of the measured f64 MFMA rate (profiles/wrmf_fp64_rate.json, 73.0 TFLOP/s) the Gram reaches.  The kernel
split comes from a run of this script under rocprofv3 --kernel-trace --stats.
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MFMA_TFLOPS = 73.0          # profiles/wrmf_fp64_rate.json


def yelp_graph():
    import numpy as np
    from qrec_amd.synth import make_dataset
    g = make_dataset("yelp2018")
    key = np.unique(g["train_u"].astype(np.int64) * g["n_items"] + g["train_i"].astype(np.int64))
    return g["n_users"], g["n_items"], key // g["n_items"], key % g["n_items"], None


def fixture_graph(name):
    import numpy as np
    from test_expo_cpu import load_expo, train_pairs
    meta, z = load_expo(name)
    u, i = train_pairs(z, meta["n_items"])
    return meta["n_users"], meta["n_items"], u, i, (z["t"] if "t" in z.files else None)


def flops(U, I, nnz, d, ld):
    T = ld // 16
    nt = T * (T + 1) // 2
    steps = U * ((I + 63) // 64 * 16) + I * ((U + 63) // 64 * 16)       # 16 k-steps per 64-column chunk, every row
    gram = 2 * 16 * 16 * 4 * nt * (steps + 2 * (nnz + 3) // 4)
    post = 2 * d * (3 * U * I + 2 * nnz)
    solve = (U + I) * (d ** 3 / 3 + 2 * d * d)
    return dict(gram_executed=gram, gram_symmetric_exact=U * I * d * (d + 1) * 2, posterior=post, solve=solve,
                total_executed=gram + post + solve)


def device_case(name, U, I, u, i, t, d, lam_y, epochs):
    import numpy as np
    from qrec_amd import capi
    from qrec_amd.engine import ExposureSolver, padded_ld
    rng = np.random.default_rng(1)
    std = 0.5 if t is not None else 0.01
    th0, be0 = std * rng.standard_normal((U, d)), std * rng.standard_normal((I, d))
    s = ExposureSolver(th0, be0, u, i, 1e-5 / lam_y, lam_y, t=t)
    s.epoch()                                      # warm-up: code objects, first touches
    times, halves = [], []
    for _ in range(epochs):
        t0 = time.perf_counter(); s.half(0); t1 = time.perf_counter(); s.half(1); t2 = time.perf_counter(); s.update_prior()
        t3 = time.perf_counter()
        times.append((t3 - t0) * 1e3); halves.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    capi.device_sync()
    ms = float(np.median(times))
    h = np.median(np.array(halves), axis=0)
    f = flops(U, I, int(u.size), d, padded_ld(d, np.float64))
    gram_ms = float(h[0] + h[1])
    return dict(case=name, users=U, items=I, nnz=int(u.size), d=d, social=t is not None, epochs_timed=epochs,
                ms_per_epoch=round(ms, 3), ms_min=round(min(times), 3), ms_max=round(max(times), 3),
                ms_user_half=round(float(h[0]), 3), ms_item_half=round(float(h[1]), 3), ms_prior=round(float(h[2]), 3), flop=f,
                tflops_executed=round(f["total_executed"] / ms * 1e-9, 3),
                gram_tflops_in_halves=round(f["gram_executed"] / gram_ms * 1e-9, 3),
                fraction_of_f64_mfma_rate=round(f["gram_executed"] / gram_ms * 1e-9 / MFMA_TFLOPS, 3))


def host_case(U, I, u, i, d, rows):
    """one user half of the mirror on ``rows`` users, extrapolated to both halves of an epoch (items take the same work per
    (row, column) pair) -- an estimate, labelled as such"""
    import numpy as np
    from test_expo_cpu import csr, solve_half
    rng = np.random.default_rng(1)
    th, be = 0.01 * rng.standard_normal((U, d)), 0.01 * rng.standard_normal((I, d))
    indptr, cols = csr(u, i, U)
    sub = np.arange(rows)
    mu = np.full(I, float(np.float32(0.01)))
    t0 = time.perf_counter()
    solve_half(be, th[sub], indptr[:rows + 1], cols, lambda r: mu[None, :], 1e-5, 1.0)
    dt = time.perf_counter() - t0
    return dict(case="host_mirror_yelp2018_one_core", users=U, items=I, d=d, rows_timed=rows, s_rows_timed=round(dt, 3),
                s_per_epoch_extrapolated=round(dt / rows * 2 * U, 1),
                note="extrapolated: one user half on a row subsample, scaled to U + I rows of the same pair count")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = args[0] if args else None
    if "--host" in sys.argv:
        if os.environ.get("OMP_NUM_THREADS") != "1":       # one core: a fresh interpreter with the BLAS pools at one thread
            env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            return subprocess.call([sys.executable] + sys.argv, env=env)
        U, I, u, i, _ = yelp_graph()
        res = [host_case(U, I, u, i, 64, 64)]
    else:
        cases = [lambda: device_case("expomf_lastfm_conf_d50", *fixture_graph("expo_expomf_lastfm")[:4], None, 50, 1.0, 5),
                 lambda: device_case("expomf_yelp2018_d64", *yelp_graph(), 64, 1.0, 3),
                 lambda: device_case("serec_lastfm_trusts_d20", *fixture_graph("expo_serec_lastfm"), 20, 0.01, 5)]
        res = []
        for c in cases:
            res.append(c())
            print(json.dumps(res[-1]), flush=True)
    if "--host" in sys.argv:
        print(json.dumps(res[0]))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
