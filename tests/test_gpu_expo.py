"""GPU tests of the exposure-weighted ALS kernels (exposure.hip) and the drop-in ExpoMF and SERec classes: the row solves and
the prior pass against the numpy mirror of tests/test_expo_cpu.py on random inputs, their error paths, bit-reproducibility,
and the classes end to end against the unmodified reference's runs (tests/golden/gen_golden_expo.py)."""
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.engine import ExposureSolver, padded_ld

from helpers import check, conf_from_text, pad_cols, rows_from_golden, same_bits
from test_expo_cpu import (A_PRIOR, B_PRIOR, load_expo, mu_of_epoch, prior_a_sum, rel_max, serec_mu, solve_half,
                           train_pairs)

pytestmark = pytest.mark.gpu

MODES = ("col", "row", "social_t_row", "social_t_col")
ERR_INVALID = -1          # QREC_ERR_INVALID (include/qrec_hip.h)


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    assert capi.device_info()["arch"].startswith("gfx950")
    yield


def random_csr(rng, n_rows, n_cols, mean_deg):
    """observed columns per row (unique, ascending); row 0 has none, row 1 has every column"""
    rows, cols = [], []
    for r in range(n_rows):
        if r == 0:
            c = np.zeros(0, np.int64)
        elif r == 1:
            c = np.arange(n_cols)
        else:
            c = np.sort(rng.choice(n_cols, min(n_cols, int(rng.integers(1, 2 * mean_deg + 1))), replace=False))
        rows.append(np.full(c.size, r)); cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
    return indptr, cols.astype(np.int32)


class Problem:
    def __init__(self, rng, d, n_rows, n_cols, mode, lam_y=1.0, n_users=None, mean_deg=12):
        self.d, self.ld, self.mode, self.lam_y = d, padded_ld(d, np.float64), mode, lam_y
        self.F = rng.standard_normal((n_cols, d)) * (2.0 / np.sqrt(d))
        self.X0 = rng.standard_normal((n_rows, d)) * (2.0 / np.sqrt(d))
        self.indptr, self.cols = random_csr(rng, n_rows, n_cols, mean_deg)
        self.n_users = n_users or n_rows
        self.v = rng.uniform(0.002, 0.3, max(n_rows, n_cols))
        self.t = rng.integers(0, 12, max(n_rows, n_cols)).astype(np.float64)
        self.a_sum = rng.uniform(0.0, 40.0, max(n_rows, n_cols))
        self.d_F = DB.from_numpy(pad_cols(self.F, self.ld)) if n_cols else DB((1, self.ld), np.float64)
        self.d_X = DB.from_numpy(pad_cols(self.X0, self.ld))
        self.d_indptr, self.d_cols = DB.from_numpy(self.indptr), DB.from_numpy(self.cols)
        self.d_v, self.d_t, self.d_a = DB.from_numpy(self.v), DB.from_numpy(self.t), DB.from_numpy(self.a_sum)
        self.ws = capi.expo_solve_workspace_bytes(n_rows, self.ld)
        self.d_ws = DB((self.ws,), np.uint8)

    def prior(self):
        return capi.expo_prior_desc(MODES.index(self.mode), self.lam_y, v=self.d_v, t=self.d_t, a_sum=self.d_a, s=2.2,
                                    n_users=self.n_users)

    def mu_of(self):
        v, t, a, n = self.v, self.t, self.a_sum, self.n_users
        return {"col": lambda rows: v[None, :self.F.shape[0]],
                "row": lambda rows: v[rows, None],
                "social_t_row": lambda rows: serec_mu(t[rows], a[:self.F.shape[0]], n, 2.2),
                "social_t_col": lambda rows: serec_mu(t[:self.F.shape[0]], a[rows], n, 2.2).T}[self.mode]

    def solve(self, lam, **over):
        a = dict(d_F=self.d_F, n_cols=self.F.shape[0], d_X=self.d_X, n_rows=self.X0.shape[0], d=self.d, ld=self.ld,
                 d_indptr=self.d_indptr, d_indices=self.d_cols, prior=self.prior(), lam=lam, d_ws=self.d_ws, ws_bytes=self.ws)
        a.update(over)
        capi.expo_solve_rows(**a)
        return self.d_X.numpy()


@pytest.mark.parametrize("d", [8, 20, 50, 64, 128])
@pytest.mark.parametrize("mode", MODES)
def test_row_solve_matches_numpy(d, mode):
    rng = np.random.default_rng(100 * d + MODES.index(mode))
    n_rows, n_cols = 203, 1000 + 37                 # neither a multiple of a block's rows nor of the 64-column chunk
    p = Problem(rng, d, n_rows, n_cols, mode)
    X = p.solve(0.1)
    want = solve_half(p.F, p.X0, p.indptr, p.cols, p.mu_of(), 0.1, p.lam_y)
    check(f"expo row solve d={d} {mode}: max |X - X_np| / max |X_np|", rel_max(X[:, :d], want), 1e-10)
    assert (X[:, d:] == 0).all()                    # padded ld: the pad columns stay zero


def test_row_solve_tiny_and_wide_shapes():
    rng = np.random.default_rng(7)
    for d, n_rows, n_cols in ((8, 2, 5), (20, 9, 63), (50, 130, 65), (128, 5, 3000)):
        p = Problem(rng, d, n_rows, n_cols, "col", mean_deg=3)
        X = p.solve(0.5)
        want = solve_half(p.F, p.X0, p.indptr, p.cols, p.mu_of(), 0.5, p.lam_y)
        check(f"expo row solve d={d} rows={n_rows} cols={n_cols}", rel_max(X[:, :d], want), 1e-10)


@pytest.mark.parametrize("d", [20, 64])
@pytest.mark.parametrize("mode", ["col", "social_t_row"])
def test_prior_pass_matches_numpy(d, mode):
    rng = np.random.default_rng(d)
    U, I = 4100, 777                                # users over two fixed segments of the prior's partition
    p = Problem(rng, d, U, I, mode, lam_y=0.5, n_users=U, mean_deg=6)
    by_user = (p.indptr, p.cols.astype(np.int64))
    want = prior_a_sum(p.X0, p.F, by_user, p.mu_of(), p.lam_y)
    order = np.lexsort((np.repeat(np.arange(U), np.diff(p.indptr)), p.cols))
    col_indptr = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(p.cols, minlength=I), out=col_indptr[1:])
    col_rows = np.repeat(np.arange(U), np.diff(p.indptr))[order].astype(np.int32)
    ws = capi.expo_prior_workspace_bytes(U, I)
    d_a, d_mu = DB.zeros((I,), np.float64), DB.zeros((I,), np.float64)
    capi.expo_prior(p.d_X, U, p.d_F, I, d, p.ld, DB.from_numpy(col_indptr), DB.from_numpy(col_rows), p.prior(), d_a, d_mu,
                    DB((ws,), np.uint8), ws)
    got = d_a.numpy()
    check(f"expo prior pass d={d} {mode}: max |A_sum - numpy| / max", rel_max(got, want), 1e-12)
    mu = (A_PRIOR + want - 1) / (A_PRIOR + B_PRIOR + U - 2)
    check(f"expo prior pass d={d} {mode}: ExpoMF mu", rel_max(d_mu.numpy(), mu), 1e-12)


def test_errors_write_nothing():
    rng = np.random.default_rng(5)
    p = Problem(rng, 20, 40, 300, "col")
    X0p = pad_cols(p.X0, p.ld)

    def unchanged():
        assert np.array_equal(p.d_X.numpy(), X0p)

    with pytest.raises(capi.QRecError) as e:
        p.solve(0.1, d=129, ld=128)
    assert e.value.code == capi.ERR_UNSUPPORTED
    unchanged()
    bad_cols = p.cols.copy(); bad_cols[p.indptr[7]] = 300
    with pytest.raises(capi.QRecError) as e:
        p.solve(0.1, d_indices=DB.from_numpy(bad_cols))
    assert e.value.code == ERR_INVALID
    unchanged()
    with pytest.raises(capi.QRecError) as e:               # lambda = 0 against a zero table: B = 0
        p.solve(0.0, d_F=DB.zeros((300, p.ld), np.float64))
    assert e.value.code == capi.ERR_NOT_SPD
    unchanged()
    for over in (dict(d=0), dict(ld=48), dict(lam=-1.0), dict(lam=float("nan")), dict(d_X=None), dict(d_indptr=None),
                 dict(ws_bytes=16), dict(prior=capi.expo_prior_desc(9, 1.0))):
        with pytest.raises(capi.QRecError) as e:
            p.solve(over.pop("lam", 0.1), **over)
        assert e.value.code == ERR_INVALID
        unchanged()
    X = p.solve(0.1)                                         # and the call still works afterwards
    assert np.isfinite(X).all()


def test_solver_is_bit_reproducible():
    rng = np.random.default_rng(11)
    U, I, d = 700, 1900, 50
    deg = rng.integers(1, 40, U)
    u = np.repeat(np.arange(U), deg)
    i = np.concatenate([rng.choice(I, k, replace=False) for k in deg])
    th0, be0 = rng.standard_normal((U, d)) * 0.5, rng.standard_normal((I, d)) * 0.5
    t = rng.integers(0, 9, U).astype(np.float64)

    def run(social):
        s = ExposureSolver(th0, be0, u, i, 1e-3, 0.01, t=t if social else None)
        for _ in range(2):
            s.epoch()
        th, be, prior = s.download()
        return dict(theta=th, beta=be, prior=prior[1] if social else prior)

    same_bits("ExposureSolver (ExpoMF prior), two epochs", run(False), run(False))
    same_bits("ExposureSolver (SERec prior), two epochs", run(True), run(True))


def synthetic_relation(t):
    """follower -> followee pairs with t[a] followees for user a (the prior depends on the graph only through t)"""
    U = t.size
    return [[f"u{a}", f"u{(a + 1 + k) % U}", 1.0] for a in range(U) for k in range(int(t[a]))]


def _run_class(name):
    meta, z = load_expo(name)
    train, test = rows_from_golden(z)
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    if "-ap" in meta["conf"]:          # the reference's -ap split drew one random() per loaded row (util/dataSplit.py:9-26)
        for _ in range(meta["n_train"] + meta["n_test"]):
            random.random()
    captured = []
    buf = io.StringIO()
    with redirect_stdout(buf):
        if meta["model"] == "ExpoMF":
            from qrec_amd.model.ranking.ExpoMF import ExpoMF
            m = ExpoMF(conf_from_text(meta["conf"]), train, test)
        else:
            from qrec_amd.model.ranking.SERec import SERec
            m = SERec(conf_from_text(meta["conf"]), train, test, synthetic_relation(z["t"]))
        import qrec_amd.engine as eng
        orig = eng.ExposureSolver.update_prior

        def spy(self, stream=None):
            orig(self, stream)
            th, be, prior = self.download()
            captured.append((th, be, prior[1] if self.social else prior))
        eng.ExposureSolver.update_prior = spy
        try:
            measure = m.execute()
        finally:
            eng.ExposureSolver.update_prior = orig
    return meta, z, m, captured, measure, buf.getvalue()


@pytest.mark.parametrize("name", ["expo_expomf_filmtrust", "expo_expomf_lastfm", "expo_serec_filmtrust", "expo_serec_lastfm"])
def test_model_end_to_end_reproduces_reference_runs(name):
    meta, z, m, captured, measure, out = _run_class(name)
    assert len(captured) == meta["maxEpoch"]
    if meta["model"] == "SERec":
        assert np.array_equal(m.t, z["t"])
    s = meta["row_stride"]
    for k in meta["kept_epochs"]:
        th, be, prior = captured[k - 1]
        dist = meta["distance_ref32_ref64"][k - 1]
        for key, got in (("theta", th[::s]), ("beta", be[::s]), ("mu", mu_of_epoch(meta, z, prior))):
            ref64, ref32 = z["ref64_%s%d" % (key, k)], z["ref32_%s%d" % (key, k)]
            check(f"{name} epoch {k}: {key} vs ref64 (max-normalised)", rel_max(got, ref64), 1e-10)
            check(f"{name} epoch {k}: {key} vs ref32, 2.5x |ref32 - ref64| = {2.5 * dist[key]:.2e}", rel_max(got, ref32),
                  2.5 * dist[key], kind="floor")
    # the printed training lines: the same sequence, the prior's own lines aside (its numbers are checked above)
    lines = out[out.index("training..."):].splitlines()
    marks = lambda ls: [ln for ln in ls if ln.startswith("epoch #") or ln == "\tUpdating exposure prior..." or ln == "training..."]
    assert marks(lines)[:len(marks(meta["printed"]["ref64"]))] == marks(meta["printed"]["ref64"])
    assert np.array_equal(capi.state_from_python(random.getstate()), z["py_state"])
    assert len(measure) == len(meta["measure"]["ref64"])
    for g, w in zip(measure, meta["measure"]["ref64"]):
        if ":" in w:
            check(f"{name}: {w.split(':')[0]} vs ref64 (relative)", abs(float(g.split(":")[1]) / float(w.split(":")[1]) - 1), 1e-9)
        else:
            assert g == w
    # the recommendation lists: the ref64 run's, except where two swapped items' ref64 scores tie to 1e-9
    N = z["ref64_rec_ids"].shape[1]
    rl = m.rank_all_test_users(N)
    keys = [f"u{u}" if u >= 0 else f"xu{n}" for u, n in zip(z["rec_users"].tolist(), z["rec_user_names"].tolist())]
    assert list(rl) == keys
    ids = np.array([[m.data.item[it] for it, _ in rl[k]] for k in keys], dtype=np.int32)
    want = z["ref64_rec_ids"]
    th, be = m.theta, m.beta
    for row in np.nonzero((ids != want).any(axis=1))[0]:
        uid = int(z["rec_users"][row])
        assert uid >= 0
        sc = be.dot(th[uid])
        for a, b in zip(ids[row], want[row]):
            if a != b:
                assert abs(sc[a] - sc[b]) <= 1e-9 * max(abs(sc[a]), abs(sc[b])), (row, a, b)


@pytest.mark.parametrize("name", ["expo_expomf_filmtrust", "expo_serec_filmtrust"])
def test_conf_runs_through_main(name, tmp_path, monkeypatch):
    """`python -m qrec_amd.main <conf>` with model.name=ExpoMF / SERec: the FilmTrust fixture's rows written out as files"""
    from qrec_amd.main import main
    meta, z = load_expo(name)
    train, test = rows_from_golden(z)
    rows = train + test
    (tmp_path / "ratings.txt").write_text("".join(f"{a} {b} {r}\n" for a, b, r in rows))
    (tmp_path / "train.txt").write_text("".join(f"{a} {b} {r}\n" for a, b, r in train))
    (tmp_path / "test.txt").write_text("".join(f"{a} {b} {r}\n" for a, b, r in test))
    conf = meta["conf"].replace("./dataset/FilmTrust/trainset.txt", str(tmp_path / "train.txt")) \
                       .replace("./dataset/FilmTrust/testset.txt", str(tmp_path / "test.txt"))
    if meta["model"] == "SERec":
        (tmp_path / "trust.txt").write_text("".join(f"{a} {b} {w}\n" for a, b, w in synthetic_relation(z["t"])))
        conf = conf.replace("./dataset/FilmTrust/trust.txt", str(tmp_path / "trust.txt"))
    (tmp_path / "m.conf").write_text(conf)
    monkeypatch.chdir(tmp_path)
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert main([str(tmp_path / "m.conf")]) == 0
    out = buf.getvalue()
    assert out.count("epoch #") == meta["maxEpoch"] and out.count("Updating exposure prior") == meta["maxEpoch"]
    result = out[out.index("The result of"):].splitlines()[1:]
    assert any(ln.startswith("Recall") for ln in result)
