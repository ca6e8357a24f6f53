"""GPU tests of the CoFactor kernels (cofactor.hip) and the drop-in CoFactor class: the co-occurrence counts against a
scipy.sparse product (exact), the SPPMI against the fixtures (bit for bit, neighbour order included), the item-step kernel
against the host mirror of tests/test_cofactor_cpu.py, the error paths, and the class end to end against the unmodified
reference's runs (tests/golden/gen_golden_cofactor.py).

Bounds.  Losses 1e-12 relative and measures rel=1e-9, as for WRMF.  Every table (X, Y, G, w, c) of every kept epoch is held to
the reference within max(1e-9, 4 x d) of the table's largest magnitude, d = the distance of the fp64 host mirror (independent
test code, Cholesky) from the same recorded run, measured in this process: the kernel differs from the mirror only in how its
sums are partitioned.  A recommendation list is left out only when the reference's own gap at the cut is positive and below
that bound (an exact tie is decided by the selection rule and is compared)."""
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.engine import CoFactorSolver, CoOccurrence, cofactor_schedule, padded_ld

from helpers import check, conf_from_text, pad_cols, rows_from_golden, same_bits
from test_cofactor_cpu import (CASES, TABLES, counts_by_product, distances, item_sweep, load_cofactor, mirror_distances, product_counts,
                               record_parity)
from test_wrmf_cpu import csr, rel_max, train_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    assert capi.device_info()["arch"].startswith("gfx950")
    yield


def same_csr(what, got, want):
    for g, w, part in zip(got, want, ("indptr", "cols", "counts")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, part)


@pytest.mark.parametrize("name", CASES)
def test_cooccurrence_and_sppmi_match_fixture(name):
    meta, z, (ptr, idx, val) = load_cofactor(name)
    u, i, _ = train_pairs(z, meta["n_items"])
    co = CoOccurrence(u, i, meta["n_users"], meta["n_items"], meta["filter"])
    same_csr(name, co.counts(), counts_by_product(z, meta["n_users"], meta["n_items"], meta["filter"]))
    got = co.sppmi(meta["negCount"])
    assert np.array_equal(got[0], ptr) and np.array_equal(got[1], idx)
    assert np.array_equal(got[2].view(np.uint64), val.view(np.uint64))


def random_pairs(rng, U, I, density):
    m = rng.random((U, I)) < density
    return np.nonzero(m)


def test_cooccurrence_thresholds_and_shapes():
    rng = np.random.default_rng(5)
    F = 3
    # items 0, 1: exactly F raters each, the same ones (kept as items, their pair has F common raters: dropped);
    # items 2, 3: F + 1 common raters (kept); item 4: F - 1 raters (does not qualify)
    u = np.concatenate([[0, 1, 2], [0, 1, 2], [3, 4, 5, 6], [3, 4, 5, 6, 7], [0, 1]])
    i = np.concatenate([[0] * 3, [1] * 3, [2] * 4, [3] * 5, [4] * 2])
    ru, ri = random_pairs(rng, 60, 40, 0.15)
    u, i = np.concatenate([u, ru + 8]), np.concatenate([i, ri + 5])
    U, I = 68, 45
    for filt in (F, 0, 1, 100):                 # 100: no qualifying item
        want = product_counts(u, i, U, I, filt)
        got = CoOccurrence(u, i, U, I, filt).counts()
        same_csr(f"filter {filt}", got, want)
        if filt == F:
            row = lambda a: got[1][got[0][a]:got[0][a + 1]].tolist()
            assert 1 not in row(0) and 0 not in row(1) and 3 in row(2) and 2 in row(3)
        if filt == 100:
            assert got[1].size == 0
    # more items than one tile of counters, an item with more raters than a tile has counters, duplicated pairs
    U, I = 9000, capi.COOC_TILE + 900
    ru, ri = random_pairs(rng, 300, 400, 0.05)
    u = np.concatenate([np.arange(U), ru * 29, ru[:50] * 29, np.arange(0, U, 3)])
    i = np.concatenate([np.full(U, I - 2), ri * 23, ri[:50] * 23, np.full(len(range(0, U, 3)), 7)])
    for filt in (0, 2):
        same_csr(f"two tiles, filter {filt}", CoOccurrence(u, i, U, I, filt).counts(), product_counts(*np.divmod(np.unique(u * I + i), I), U, I, filt))


def test_cooccurrence_errors_write_nothing():
    rng = np.random.default_rng(9)
    u, i = random_pairs(rng, 50, 30, 0.3)
    co = CoOccurrence(u, i, 50, 30, 1)
    views = (co.d_i_indptr, co.d_i_users, 30, co.nnz, co.d_u_indptr, co.d_u_items, 50, co.nnz)
    kept = capi.cooc_count(*views, 1, co.d_ws, co.ws_bytes)
    assert kept > 0
    d_ptr, d_cols, d_cnt = DB((31,), np.int64), DB((kept,), np.int32), DB((kept,), np.int32)
    for b in (d_ptr, d_cols, d_cnt):
        b.fill_bytes(0xFF)
    with pytest.raises(capi.QRecError, match="kept pairs"):
        capi.cooc_fill(*views, 1, d_ptr, d_cols, d_cnt, kept - 1, co.d_ws, co.ws_bytes)
    assert (d_ptr.numpy() == -1).all() and (d_cols.numpy() == -1).all() and (d_cnt.numpy() == -1).all()
    with pytest.raises(capi.QRecError):
        CoOccurrence(u, i, 50, 30, 1, capacity=kept - 2).counts()
    for bad in (dict(filt=-1), dict(ws_bytes=64), dict(n_items=0)):
        a = dict(n_items=30, filt=1, ws_bytes=co.ws_bytes); a.update(bad)
        with pytest.raises(capi.QRecError):
            capi.cooc_count(co.d_i_indptr, co.d_i_users, a["n_items"], co.nnz, co.d_u_indptr, co.d_u_items, 50, co.nnz, a["filt"], co.d_ws, a["ws_bytes"])
    with pytest.raises(capi.QRecError):               # a user index past the table
        capi.cooc_count(*views[:6], 20, co.nnz, 1, co.d_ws, co.ws_bytes)
    # and the calls still work afterwards
    capi.cooc_count(*views, 1, co.d_ws, co.ws_bytes)
    capi.cooc_fill(*views, 1, d_ptr, d_cols, d_cnt, kept, co.d_ws, co.ws_bytes)
    same_csr("after errors", (d_ptr.numpy(), d_cols.numpy(), d_cnt.numpy()), product_counts(u, i, 50, 30, 1))


class ItemProblem:
    """a random item half: X, ratings by item, a symmetric context graph with values, the tables it sweeps"""

    def __init__(self, rng, d, U=400, I=700, hub=320):
        self.d, self.ld, self.U, self.I = d, padded_ld(d, np.float64), U, I
        deg = rng.integers(0, 30, I); deg[5] = 0; deg[6] = U
        self.r_indptr = np.zeros(I + 1, np.int64); np.cumsum(deg, out=self.r_indptr[1:])
        self.r_users = np.concatenate([rng.choice(U, k, replace=False) for k in deg]).astype(np.int32)
        self.r_conf = rng.random(self.r_users.size) * 20
        # contexts: a hub (item 300) with several hundred, item 0 whose every context follows it, item I - 1 whose every context
        # precedes it, a sparse random rest; items >= 600 (but the last) have none
        edges = {(min(300, j), max(300, j)) for j in rng.choice(600, hub, replace=False).tolist() if j != 300}
        edges |= {(0, j) for j in (3, 17, 300, 450)} | {(j, I - 1) for j in (2, 17, 299, 300, 599)}
        a, b = rng.integers(1, 600, 2500), rng.integers(1, 600, 2500)
        edges |= {(min(x, y), max(x, y)) for x, y in zip(a.tolist(), b.tolist()) if x != y}
        e = np.array(sorted(edges)); v = rng.random(e.shape[0])
        x, y, val = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]), np.concatenate([v, v])
        order = np.lexsort((rng.random(x.size), x))              # any neighbour order inside a row
        self.s_ptr = np.zeros(I + 1, np.int64); np.cumsum(np.bincount(x, minlength=I), out=self.s_ptr[1:])
        self.s_idx, self.s_val = y[order].astype(np.int32), val[order]
        self.X = rng.random((U, d)) - 0.3
        self.Y, self.G = rng.random((I, d)) - 0.4, rng.random((I, d)) - 0.5
        self.w, self.c = rng.random(I) / 10, rng.random(I) / 10
        self.order, self.level_ptr = cofactor_schedule(self.s_ptr, self.s_idx)
        self.solo = np.flatnonzero(np.diff(self.s_ptr) == 0).astype(np.int32)
        self.d_X = DB.from_numpy(pad_cols(self.X, self.ld))
        self.d_XtX = DB((self.ld, self.ld), np.float64)
        gws = capi.als_gram_workspace_bytes(U, self.ld)
        capi.als_gram(self.d_X, U, d, self.ld, self.d_XtX, DB((gws,), np.uint8), gws)
        self.dev = dict(Y=DB.from_numpy(pad_cols(self.Y, self.ld)), G=DB.from_numpy(pad_cols(self.G, self.ld)), w=DB.from_numpy(self.w),
                        c=DB.from_numpy(self.c))
        self.ws = capi.cofactor_item_workspace_bytes(I, self.order.size, self.ld)
        self.args = dict(d_X=self.d_X, n_users=U, d_XtX=self.d_XtX, d_Y=self.dev["Y"], d_G=self.dev["G"], d_w=self.dev["w"], d_c=self.dev["c"],
                         n_items=I, d=d, ld=self.ld, d_r_indptr=DB.from_numpy(self.r_indptr), d_r_users=DB.from_numpy(self.r_users),
                         d_r_conf=DB.from_numpy(self.r_conf), r_nnz=self.r_users.size, d_s_indptr=DB.from_numpy(self.s_ptr),
                         d_s_items=DB.from_numpy(self.s_idx), d_s_vals=DB.from_numpy(self.s_val), s_nnz=self.s_idx.size,
                         d_order=DB.from_numpy(self.order), level_ptr=self.level_ptr, d_solo=DB.from_numpy(self.solo), n_solo=self.solo.size,
                         lam=1.0, gamma=0.5, d_ws=DB((self.ws,), np.uint8), ws_bytes=self.ws)

    def run(self, **over):
        capi.cofactor_item_rows(**{**self.args, **over})
        return self.tables()

    def tables(self):
        return {k: v.numpy() for k, v in self.dev.items()}


@pytest.mark.parametrize("d", [20, 50, 64, 128])
def test_item_step_matches_host_mirror(d):
    p = ItemProblem(np.random.default_rng(d), d)
    assert np.diff(p.s_ptr).max() >= 300 and p.level_ptr.size > 3
    got = p.run()
    Y, G, w, c = p.Y.copy(), p.G.copy(), p.w.copy(), p.c.copy()
    item_sweep(p.X, Y, G, w, c, (p.r_indptr, p.r_users, p.r_conf), (p.s_ptr, p.s_idx, p.s_val), 1.0, 0.5)
    # fp64 on both sides, the same formulas and orders up to how a sum is partitioned: rounding, amplified by the systems'
    # condition (gamma = 0.5 against Grams of a few contexts) and carried along the sweep -- the project's 1e-9 table bound
    for t, want in (("Y", Y), ("G", G)):
        check(f"item step d={d}: max |{t} - {t}_host| / max |{t}_host|", rel_max(got[t][:, :d], want), 1e-9)
        assert (got[t][:, d:] == 0).all()
    for t, want in (("w", w), ("c", c)):
        check(f"item step d={d}: max |{t} - {t}_host| / max |{t}_host|", rel_max(got[t], want), 1e-9)
    untouched = np.setdiff1d(np.arange(p.I), p.order)
    assert np.array_equal(got["G"][untouched, :d], p.G[untouched]) and np.array_equal(got["w"][untouched], p.w[untouched])


def test_item_step_errors_write_nothing():
    p = ItemProblem(np.random.default_rng(3), 20, U=120, I=700, hub=300)
    before = p.tables()

    def unchanged():
        now = p.tables()
        assert all(np.array_equal(now[k], before[k]) for k in before)

    rated_solo = int(next(s for s in p.solo if p.r_indptr[s + 1] > p.r_indptr[s]))
    for item in (rated_solo, 300):                # an indefinite system in an item without contexts, and in the hub of the schedule
        bad = p.r_conf.copy(); bad[p.r_indptr[item]] = -1e7
        assert p.r_indptr[item + 1] > p.r_indptr[item]
        with pytest.raises(capi.QRecError) as e:
            p.run(d_r_conf=DB.from_numpy(bad))
        assert e.value.code == capi.ERR_NOT_SPD and f"item {item} " in str(e.value)
        unchanged()
    bad_args = [dict(d=0), dict(d=129), dict(d=40), dict(ld=48), dict(lam=-1.0), dict(gamma=float("nan")), dict(n_items=-1), dict(d_XtX=None),
                dict(d_Y=None), dict(d_G=None), dict(d_w=None), dict(d_c=None), dict(d_r_indptr=None), dict(d_s_indptr=None), dict(d_ws=None),
                dict(ws_bytes=256), dict(n_users=50), dict(n_items=500), dict(r_nnz=10), dict(s_nnz=10), dict(n_solo=p.I),
                dict(level_ptr=np.array([1, 2], np.int32)), dict(level_ptr=np.array([0, 5, 3], np.int32))]
    for over in bad_args:
        with pytest.raises(capi.QRecError):
            p.run(**over)
        unchanged()
    got = p.run()
    assert all(np.isfinite(v).all() for v in got.values()) and not np.array_equal(got["Y"], before["Y"])


def test_solver_is_bit_reproducible():
    rng = np.random.default_rng(11)
    p = ItemProblem(rng, 64, U=300, I=700)
    u = p.r_users.astype(np.int64); i = np.repeat(np.arange(p.I), np.diff(p.r_indptr))
    r = rng.integers(1, 3, u.size).astype(np.float64)
    X0 = rng.random((p.U, 64)) / 3 * 10

    def run():
        s = CoFactorSolver(X0, p.Y * 3, p.G, p.w, p.c, u, i, r, (p.s_ptr, p.s_idx, p.s_val), 1.0, 0.01)
        losses = np.array([s.epoch() for _ in range(2)])
        return dict(zip(TABLES, s.download()), loss=losses)

    same_bits("CoFactorSolver, two epochs", run(), run())


def _run_class(name):
    import qrec_amd.model.ranking.CoFactor as mod
    meta, z, sppmi = load_cofactor(name)
    train, test = rows_from_golden(z)
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    if "-ap" in meta["conf"]:          # the reference's -ap split drew one random() per loaded row (util/dataSplit.py:9-26)
        for _ in range(meta["n_train"] + meta["n_test"]):
            random.random()
    captured = {}
    buf = io.StringIO()

    def spy(*args, **kw):               # the class has no per-epoch hook, as the reference has none: watch its epoch line
        if len(args) == 4 and args[0] == "epoch:":
            captured[int(args[1])] = (float(args[3]), {t: getattr(m, t).copy() for t in TABLES})
        print(*args, **kw)
    mod.print = spy
    try:
        with redirect_stdout(buf):
            m = mod.CoFactor(conf_from_text(meta["conf"]), train, test)
            measure = m.execute()
    finally:
        del mod.print
    return meta, z, sppmi, m, captured, measure, buf.getvalue()


@pytest.mark.parametrize("name", CASES)
def test_cofactor_model_end_to_end_reproduces_reference_run(name):
    meta, z, sppmi, m, captured, measure, out = _run_class(name)
    assert np.array_equal(m.SPPMI[1], sppmi[1]) and np.array_equal(m.SPPMI[2].view(np.uint64), sppmi[2].view(np.uint64))
    assert sorted(captured) == [e["epoch"] for e in meta["epochs"]]
    mirror = mirror_distances(name)
    worst, gpu = 1e-9, {}
    for e in meta["epochs"]:
        k = e["epoch"]
        loss, tables = captured[k]
        check(f"{name} epoch {k}: loss", abs(loss - e["loss"]) / e["loss"], 1e-12)
        if k in meta["kept_epochs"]:
            gpu[str(k)] = dist = distances(meta, z, sppmi, tables, k)
            for t in TABLES:
                bound = max(1e-9, 4 * mirror[k][t])
                worst = max(worst, bound) if t == "Y" or t == "X" else worst
                print(f"{name} epoch {k}: {t} device-reference {dist[t]:.3e}  mirror-reference {mirror[k][t]:.3e}  bound {bound:.1e}")
                check(f"{name} epoch {k}: max |{t} - {t}_ref| / max |{t}_ref|", dist[t], bound)
    record_parity("host_mirror_vs_reference", name, {str(k): v for k, v in mirror.items()})
    record_parity("device_vs_reference", name, gpu)
    record_parity("schedule", name, m.solver.schedule)
    assert "Constructing SPPMI matrix..." in out and "training..." in out
    printed = [ln for ln in out.splitlines() if ln.startswith("epoch:")]
    assert [ln.split()[:3] for ln in printed] == [ln.split()[:3] for ln in meta["printed"]]
    assert np.array_equal(capi.state_from_python(random.getstate()), z["py_state"])       # training leaves Python's generator alone
    for g, w in zip(measure, meta["measure"]):
        if ":" in w:
            assert float(g.split(":")[1]) == pytest.approx(float(w.split(":")[1]), rel=1e-9), (g, w)
        else:
            assert g == w
    assert len(measure) == len(meta["measure"])
    # the recommendation lists: same items in the same order for every test user the reference separates at the cut
    N = z["rec_ids"].shape[1]
    rl = m.rank_all_test_users(N)
    keys = [f"u{u}" if u >= 0 else f"xu{n}" for u, n in zip(z["rec_users"].tolist(), z["rec_user_names"].tolist())]
    assert list(rl) == keys                                  # testSet_u order
    ids = np.array([[m.data.item[it] for it, _ in rl[k]] for k in keys], dtype=np.int32)
    left_out = (z["rec_gap"] > 0) & (z["rec_gap"] < worst * meta["y_max"])
    print(f"{name}: {int(left_out.sum())} of {len(keys)} test users left out of the list comparison (gap at the cut below {worst:.1e} of max |Y|)")
    assert left_out.sum() <= 0.01 * len(keys)
    assert np.array_equal(ids[~left_out], z["rec_ids"][~left_out])


def test_cofactor_conf_runs_through_main(tmp_path, monkeypatch):
    """`python -m qrec_amd.main <conf>` with model.name=CoFactor: the FilmTrust fixture's rows written out as rating files"""
    from qrec_amd.main import main
    meta, z, _ = load_cofactor("cofactor_filmtrust")
    train, test = rows_from_golden(z)
    (tmp_path / "train.txt").write_text("".join(f"{a} {b} {r}\n" for a, b, r in train))
    (tmp_path / "test.txt").write_text("".join(f"{a} {b} {r}\n" for a, b, r in test))
    conf = meta["conf"].replace("./dataset/FilmTrust/trainset.txt", str(tmp_path / "train.txt")) \
                       .replace("./dataset/FilmTrust/testset.txt", str(tmp_path / "test.txt"))
    (tmp_path / "CoFactor.conf").write_text(conf)
    monkeypatch.chdir(tmp_path)
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert main([str(tmp_path / "CoFactor.conf")]) == 0
    out = buf.getvalue()
    assert out.count("epoch:") >= len(meta["epochs"])
    result = out[out.index("The result of"):].splitlines()[1:]
    for g, w in zip(result, meta["measure"]):
        if ":" in w:
            assert g.split(":")[0] == w.split(":")[0] and float(g.split(":")[1]) == pytest.approx(float(w.split(":")[1]), rel=1e-9), (g, w)
        else:
            assert g == w.strip()
