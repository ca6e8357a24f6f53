"""GPU tests of the fp64 ALS kernels (als.hip) and the drop-in WRMF class: the Gram and row-solve kernels against numpy
and the host mirror of tests/test_wrmf_cpu.py, their error paths, and the class end to end against the unmodified
reference's runs (tests/golden/gen_golden_wrmf.py)."""
import io
import os
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.engine import AlsSolver, padded_ld

from helpers import check, conf_from_text, pad_cols, rows_from_golden, same_bits
from test_wrmf_cpu import half_sweep, load_wrmf, rel_max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    assert capi.device_info()["arch"].startswith("gfx950")
    yield


def gram(F, d):
    ld = padded_ld(d, np.float64)
    rows = F.shape[0]
    d_F = DB.from_numpy(pad_cols(F, ld)) if rows else DB((1, ld), np.float64)
    ws = capi.als_gram_workspace_bytes(rows, ld)
    d_ws, d_G = DB((ws,), np.uint8), DB((ld, ld), np.float64)
    d_G.fill_bytes(0xFF)
    capi.als_gram(d_F, rows, d, ld, d_G, d_ws, ws)
    return d_G.numpy()


@pytest.mark.parametrize("d", [1, 16, 20, 50, 64, 128])
def test_gram_matches_numpy(d):
    rng = np.random.default_rng(d)
    for rows in (0, 1, 1000, 40000):
        F = rng.random((rows, d)) - 0.3
        G = gram(F, d)
        want = F.T.dot(F)
        check(f"Gram d={d} rows={rows}: max |G - F^T F| / max |F^T F|", rel_max(G[:d, :d], want) if rows else np.abs(G).max(), 1e-12,
              inclusive=True)
        assert (G[d:, :] == 0).all() and (G[:, d:] == 0).all()       # the pad block is exactly zero
        assert np.array_equal(G, G.T)


class Problem:
    """a row-solve problem on the device: the rows of F, a CSR over them with confidences, the table X being solved"""

    def __init__(self, F, X0, indptr, cols, c, d):
        self.d, self.ld = d, padded_ld(d, np.float64)
        self.F, self.X0, self.indptr, self.cols, self.c = F, X0, indptr, cols, c
        self.d_F = DB.from_numpy(pad_cols(F, self.ld))
        self.d_X = DB.from_numpy(pad_cols(X0, self.ld))
        self.d_indptr = DB.from_numpy(indptr)
        self.d_cols = DB.from_numpy(cols.astype(np.int32))
        self.d_c = DB.from_numpy(c)
        gws = capi.als_gram_workspace_bytes(F.shape[0], self.ld)
        self.d_G = DB((self.ld, self.ld), np.float64)
        capi.als_gram(self.d_F, F.shape[0], d, self.ld, self.d_G, DB((gws,), np.uint8), gws)
        self.ws = capi.als_solve_workspace_bytes(indptr, self.ld)
        self.d_ws = DB((max(self.ws, 256),), np.uint8)
        self.d_loss = DB.from_numpy(np.array([-7.0]))

    def solve(self, lam, **over):
        a = dict(d_F=self.d_F, f_rows=self.F.shape[0], d_G=self.d_G, d_X=self.d_X, n_rows=self.X0.shape[0], d=self.d, ld=self.ld,
                 d_indptr=self.d_indptr, d_indices=self.d_cols, d_c=self.d_c, lam=lam, d_loss=self.d_loss, d_ws=self.d_ws,
                 ws_bytes=self.ws)
        a.update(over)
        capi.als_solve_rows(**a)
        return self.d_X.numpy(), float(self.d_loss.numpy()[0])


def random_problem(rng, d, n_rows=300, f_rows=12000, heavy=12000):
    deg = rng.integers(0, 40, n_rows)
    deg[0] = 0                        # b = 0: x = 0
    deg[1] = heavy                    # split into segments (>= 10k neighbours)
    deg[2], deg[3] = 513, 512         # just above / at the split threshold
    indptr = np.zeros(n_rows + 1, np.int64); np.cumsum(deg, out=indptr[1:])
    cols = np.concatenate([rng.choice(f_rows, k, replace=False) for k in deg]).astype(np.int64)
    c = rng.random(cols.size) * 50
    F = rng.random((f_rows, d)) - 0.5
    X0 = rng.random((n_rows, d)) * 0.5
    return Problem(F, X0, indptr, cols, c, d)


@pytest.mark.parametrize("d,lam", [(20, 1.0), (64, 0.5), (50, 0.0), (128, 2.0)])
def test_row_solve_matches_host_mirror(d, lam):
    rng = np.random.default_rng(d)
    p = random_problem(rng, d)
    X, loss = p.solve(lam)
    Xh = p.X0.copy()
    lh = half_sweep(p.F, Xh, p.indptr, p.cols, p.c, lam, True)
    check(f"row solve d={d} lam={lam}: max |X - X_host| / max |X_host|", rel_max(X[:, :d], Xh), 1e-10)
    check(f"row solve d={d} lam={lam}: loss", abs(loss - lh) / lh, 1e-12)
    assert (X[0] == 0).all()                                 # zero-degree row, b = 0
    assert (X[:, d:] == 0).all()                             # pad columns stay zero
    # without the loss pointer: the same solutions, the loss word untouched
    p.d_X.upload(pad_cols(p.X0, p.ld)); p.d_loss.upload(np.array([-7.0]))
    X2, l2 = p.solve(lam, d_loss=None)
    assert np.array_equal(X2, X) and l2 == -7.0


def test_row_solve_errors_write_nothing():
    rng = np.random.default_rng(3)
    p = random_problem(rng, 20, n_rows=40, f_rows=600, heavy=600)
    X0p = pad_cols(p.X0, p.ld)

    def unchanged():
        X, loss = p.d_X.numpy(), float(p.d_loss.numpy()[0])
        assert np.array_equal(X, X0p) and loss == -7.0

    # an indefinite system: one strongly negative confidence
    c_bad = p.c.copy(); c_bad[p.indptr[5]] = -1e6
    with pytest.raises(capi.QRecError) as e:
        p.solve(1.0, d_c=DB.from_numpy(c_bad))
    assert e.value.code == capi.ERR_NOT_SPD and "row 5" in str(e.value)
    unchanged()
    # a singular one: G = 0 (zero table), lambda = 0
    with pytest.raises(capi.QRecError) as e:
        p.solve(0.0, d_G=DB.zeros((p.ld, p.ld), np.float64), d_c=DB.zeros((p.c.size,), np.float64))
    assert e.value.code == capi.ERR_NOT_SPD
    unchanged()
    # bad arguments
    bad = [dict(d=0), dict(d=129), dict(d=40), dict(ld=48), dict(lam=-1.0), dict(lam=float("nan")), dict(n_rows=-1),
           dict(d_G=None), dict(d_X=None), dict(d_indptr=None), dict(d_indices=None), dict(d_c=None), dict(d_ws=None),
           dict(ws_bytes=16), dict(f_rows=100)]                      # f_rows=100: column indices past the table's end
    for over in bad:
        with pytest.raises(capi.QRecError):
            p.solve(**{"lam": 1.0, **over})
        unchanged()
    # a workspace sized for another CSR (no split rows) is refused on the device, nothing written
    small = capi.als_solve_workspace_bytes(np.zeros(p.X0.shape[0] + 1, np.int64), p.ld)
    with pytest.raises(capi.QRecError, match="workspace"):
        p.solve(1.0, ws_bytes=small)
    unchanged()
    with pytest.raises(capi.QRecError):
        capi.als_gram(p.d_F, 600, 20, 48, p.d_G, p.d_ws, p.ws)
    with pytest.raises(capi.QRecError):
        capi.als_gram(p.d_F, 600, 20, 32, p.d_G, p.d_ws, 8)
    # and the call still works afterwards
    X, _ = p.solve(1.0)
    assert np.isfinite(X).all()


def test_solver_is_bit_reproducible():
    rng = np.random.default_rng(11)
    U, I, d = 500, 3000, 64
    deg = rng.integers(1, 30, U); deg[7] = 2500              # a split user row; item 0 gets every user (split item row)
    u = np.repeat(np.arange(U), deg)
    i = np.concatenate([np.concatenate([[0], rng.choice(np.arange(1, I), k - 1, replace=False)]) for k in deg])
    r = rng.integers(1, 6, u.size).astype(np.float64)
    X0, Y0 = rng.random((U, d)) / 3 * 10, rng.random((I, d)) / 3 * 10

    def run():
        s = AlsSolver(X0, Y0, u, i, r, 1.0)
        losses = np.array([s.epoch() for _ in range(2)])
        X, Y = s.download()
        return dict(X=X, Y=Y, loss=losses)

    same_bits("AlsSolver, two epochs", run(), run())


def _run_class(name):
    from qrec_amd.model.ranking.WRMF import WRMF
    meta, z = load_wrmf(name)
    train, test = rows_from_golden(z)
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    if "-ap" in meta["conf"]:          # the reference's -ap split drew one random() per loaded row (util/dataSplit.py:9-26)
        for _ in range(meta["n_train"] + meta["n_test"]):
            random.random()
    captured = {}
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = WRMF(conf_from_text(meta["conf"]), train, test)
        orig = m.isConverged

        def spy(epoch):
            st = meta["row_stride"]              # the fixture keeps every st-th row of the tables
            captured[epoch] = (float(m.loss), m.X[::st].copy(), m.Y[::st].copy()) if ("X%d" % epoch) in z else (float(m.loss), None, None)
            return orig(epoch)
        m.isConverged = spy
        measure = m.execute()
    return meta, z, m, captured, measure, buf.getvalue()


@pytest.mark.parametrize("name", ["wrmf_filmtrust", "wrmf_lastfm"])
def test_wrmf_model_end_to_end_reproduces_reference_run(name):
    meta, z, m, captured, measure, out = _run_class(name)
    assert sorted(captured) == [e["epoch"] for e in meta["epochs"]]
    for e in meta["epochs"]:
        loss, X, Y = captured[e["epoch"]]
        check(f"{name} epoch {e['epoch']}: loss", abs(loss - e["loss"]) / e["loss"], 1e-12)
        if X is not None:
            check(f"{name} epoch {e['epoch']}: max |X - X_ref| / max |X_ref|", rel_max(X, z["X%d" % e["epoch"]]), 1e-9)
            check(f"{name} epoch {e['epoch']}: max |Y - Y_ref| / max |Y_ref|", rel_max(Y, z["Y%d" % e["epoch"]]), 1e-9)
    printed = [ln for ln in out.splitlines() if ln.startswith("epoch:")]
    assert [ln.split()[:3] for ln in printed] == [ln.split()[:3] for ln in meta["printed"]]
    assert np.array_equal(capi.state_from_python(random.getstate()), z["py_state"])
    for g, w in zip(measure, meta["measure"]):
        if ":" in w:
            assert float(g.split(":")[1]) == pytest.approx(float(w.split(":")[1]), rel=1e-9), (g, w)
        else:
            assert g == w
    assert len(measure) == len(meta["measure"])
    # the recommendation lists: same items in the same order for every test user
    N = z["rec_ids"].shape[1]
    rl = m.rank_all_test_users(N)
    keys = [f"u{u}" if u >= 0 else f"xu{n}" for u, n in zip(z["rec_users"].tolist(), z["rec_user_names"].tolist())]
    assert list(rl) == keys                                  # testSet_u order
    ids = np.array([[m.data.item[it] for it, _ in rl[k]] for k in keys], dtype=np.int32)
    assert np.array_equal(ids, z["rec_ids"])


def test_wrmf_conf_runs_through_main(tmp_path, monkeypatch):
    """`python -m qrec_amd.main <conf>` with model.name=WRMF: the FilmTrust fixture's rows written out as rating files"""
    from qrec_amd.main import main
    meta, z = load_wrmf("wrmf_filmtrust")
    train, test = rows_from_golden(z)
    (tmp_path / "train.txt").write_text("".join(f"{a} {b} {r}\n" for a, b, r in train))
    (tmp_path / "test.txt").write_text("".join(f"{a} {b} {r}\n" for a, b, r in test))
    conf = meta["conf"].replace("./dataset/FilmTrust/trainset.txt", str(tmp_path / "train.txt")) \
                       .replace("./dataset/FilmTrust/testset.txt", str(tmp_path / "test.txt"))
    (tmp_path / "WRMF.conf").write_text(conf)
    monkeypatch.chdir(tmp_path)
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert main([str(tmp_path / "WRMF.conf")]) == 0
    out = buf.getvalue()
    assert out.count("epoch:") >= len(meta["epochs"])
    result = out[out.index("The result of"):].splitlines()[1:]
    for g, w in zip(result, meta["measure"]):
        if ":" in w:
            assert g.split(":")[0] == w.split(":")[0] and float(g.split(":")[1]) == pytest.approx(float(w.split(":")[1]), rel=1e-9), (g, w)
        else:
            assert g == w.strip()
