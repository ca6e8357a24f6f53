"""CoFactor without a GPU: the model is provided; the host SPPMI builder gives the reference's neighbour sequences and values;
the formulation the kernels implement -- the sparse form of model/ranking/CoFactor.py:84-162 solved by Cholesky, in the
reference's orders -- reproduces the unmodified reference's runs (tests/golden/gen_golden_cofactor.py) in fp64; and the sweep
run by levels is the sequential sweep.

The distance of this mirror from the recorded runs is the yardstick of the GPU test (test_gpu_cofactor.py holds the device to the
reference within max(1e-9, 4 x that distance) per table and epoch): it is printed here, and written as JSON when
QREC_PARITY_JSON names a file (profiles/cofactor_parity.json is such a run)."""
import hashlib
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.linalg import cho_factor, cho_solve

from helpers import GOLDEN
from test_wrmf_cpu import csr, half_sweep, rel_max, train_pairs

CASES = ["cofactor_filmtrust", "cofactor_filmtrust_b", "cofactor_lastfm"]
TABLES = ("X", "Y", "G", "w", "c")


def load_cofactor(name):
    """meta, the fixture, and the SPPMI (ptr, idx, val) with the value of every directed entry restored from its pair's"""
    meta = json.load(open(os.path.join(GOLDEN, "golden_cofactor_meta.json")))[name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    s = np.load(os.path.join(GOLDEN, name + "_sppmi.npz"))
    ptr, idx, up = s["sppmi_ptr"], s["sppmi_idx"], s["sppmi_val_upper"]
    I = ptr.size - 1
    row = np.repeat(np.arange(I, dtype=np.int64), np.diff(ptr))
    key = np.minimum(row, idx) * I + np.maximum(row, idx)
    upper = idx > row
    srt = np.argsort(key[upper], kind="stable")
    val = up[srt][np.searchsorted(key[upper][srt], key)]
    return meta, z, (ptr, idx, val)


def start_tables(meta):
    """the base class's draws and trainModel's (CoFactor.py:85-89) from the legacy numpy stream"""
    U, I, d = meta["n_users"], meta["n_items"], meta["emb_size"]
    np.random.seed(meta["seed"])
    X0 = np.random.rand(U, d) / 3 * 10
    Y0 = np.random.rand(I, d) / 3 * 10
    w0 = np.random.rand(I) / 10
    c0 = np.random.rand(I) / 10
    G0 = np.random.rand(I, d) / 10
    return X0, Y0, G0, w0, c0


def item_step(i, X, XtX, Y, G, w, c, ratings, sppmi, lam, gamma):
    """CoFactor.py:117-159 for item i, in place"""
    indptr, users, conf = ratings
    ptr, idx, val = sppmi
    d = X.shape[1]
    k = slice(indptr[i], indptr[i + 1])
    Xi, ci = X[users[k]], conf[k]
    A = XtX + (Xi.T * ci).dot(Xi) + lam * np.eye(d)
    b = (Xi.T * (1.0 + ci)).sum(axis=1)
    n = ptr[i + 1] - ptr[i]
    if n == 0:
        Y[i] = cho_solve(cho_factor(A, lower=True), b)
        return
    nb, s = idx[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]
    Gn, Yn = G[nb], Y[nb]
    A = A + Gn.T.dot(Gn)
    b = b + ((s - w[i]) - c[nb]).dot(Gn)
    uw = float(((s - Gn.dot(Y[i])) - c[nb]).sum())
    uc = float(((s - Yn.dot(G[i])) - w[nb]).sum())
    g = cho_solve(cho_factor(Yn.T.dot(Yn) + gamma * np.eye(d), lower=True), ((s - w[nb]) - c[i]).dot(Yn))
    Y[i] = cho_solve(cho_factor(A, lower=True), b)
    G[i] = g
    w[i] = uw / n
    c[i] = uc / n


def item_sweep(X, Y, G, w, c, ratings, sppmi, lam, gamma, order=None):
    XtX = X.T.dot(X)
    for i in (range(Y.shape[0]) if order is None else order):
        item_step(int(i), X, XtX, Y, G, w, c, ratings, sppmi, lam, gamma)


def levels_of(sppmi):
    """(order, level_ptr): level(i) = 1 + max level(context before i), items ascending inside a level -- written out here, apart
    from the product's schedule builder"""
    ptr, idx, _ = sppmi
    level = np.full(ptr.size - 1, -1, dtype=np.int64)
    for i in np.flatnonzero(np.diff(ptr) > 0):
        nb = idx[ptr[i]:ptr[i + 1]]
        prev = level[nb[nb < i]]
        level[i] = prev.max() + 1 if prev.size else 0
    ctx = np.flatnonzero(level >= 0)
    order = ctx[np.argsort(level[ctx], kind="stable")]
    lp = np.zeros(level.max() + 2 if ctx.size else 1, dtype=np.int64)
    if ctx.size:
        np.cumsum(np.bincount(level[ctx]), out=lp[1:])
    return order, lp


def host_mirror(meta, z, sppmi, epochs=None, by_levels=False):
    X, Y, G, w, c = start_tables(meta)
    U, I = meta["n_users"], meta["n_items"]
    u, i, r = train_pairs(z, I)
    conf = 10.0 * r
    users, items = csr(u, i, conf, U), csr(i, u, conf, I)
    order = None
    if by_levels:
        lv_order, _ = levels_of(sppmi)
        order = np.concatenate([np.flatnonzero(np.diff(sppmi[0]) == 0), lv_order])      # items without contexts in any place
    for _ in range(epochs or len(meta["epochs"])):
        loss = half_sweep(Y, X, *users, meta["regU"], True)
        item_sweep(X, Y, G, w, c, items, sppmi, meta["regU"], meta["regR"], order)
        yield loss, dict(X=X, Y=Y, G=G, w=w, c=c)


def fixture_rows(meta, sppmi, t, a):
    """the part of table ``t`` the fixture keeps"""
    s, ctx = meta["row_stride"], np.flatnonzero(np.diff(sppmi[0]) > 0)
    return a[::s] if t in "XY" else a[ctx][::s] if t == "G" else a[ctx]


def distances(meta, z, sppmi, tables, k):
    """per table: max |got - ref| / max |ref| over the fixture's rows of epoch k"""
    return {t: rel_max(fixture_rows(meta, sppmi, t, tables[t]), z["%s%d" % (t, k)]) for t in TABLES}


def record_parity(section, name, value):
    path = os.environ.get("QREC_PARITY_JSON")
    if not path:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.setdefault(section, {})[name] = value
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


_mirror_cache = {}


def mirror_distances(name):
    """{epoch: {table: distance of the host mirror from the reference's recorded run}, 'loss': {epoch: relative}} -- computed once"""
    if name not in _mirror_cache:
        meta, z, sppmi = load_cofactor(name)
        out, kept = {"loss": {}}, set(meta["kept_epochs"])
        for k, (loss, tables) in enumerate(host_mirror(meta, z, sppmi), 1):
            out["loss"][k] = abs(loss - meta["epochs"][k - 1]["loss"]) / meta["epochs"][k - 1]["loss"]
            if k in kept:
                out[k] = distances(meta, z, sppmi, tables, k)
        _mirror_cache[name] = out
    return _mirror_cache[name]


def test_resolve_model_provides_cofactor():
    from qrec_amd.QRec import resolve_model
    from qrec_amd.model.ranking.CoFactor import CoFactor
    assert resolve_model("CoFactor") is CoFactor
    with pytest.raises(ImportError, match="CoFactor"):
        resolve_model("NoSuchModel")


def test_conf_parsing():
    from qrec_amd.model.ranking.CoFactor import CoFactor
    from helpers import conf_from_text
    meta, _, _ = load_cofactor("cofactor_filmtrust")
    for text, want in ((meta["conf"], (5, 0.01, 2)), (meta["conf"].replace("-k 5", "-k 0").replace("-filter 2", "-filter 7"), (1, 0.01, 7))):
        m = CoFactor(conf_from_text(text), [["u0", "i0", 1.0]], [["u0", "i0", 1.0]])
        m.readConfiguration()
        assert (m.negCount, m.regR, m.filter) == want
        assert m.regU == 1.0


def product_counts(u, i, n_users, n_items, filt):
    """B^T B with the two thresholds of CoFactor.py:44-55 applied: CSR (indptr, cols, counts), columns ascending"""
    B = sp.csr_matrix((np.ones(u.size, dtype=np.int64), (u, i)), shape=(n_users, n_items))
    C = (B.T @ B).tocoo()
    deg = np.asarray(B.sum(axis=0)).ravel()
    keep = (C.row != C.col) & (C.data > filt) & (deg[C.row] >= filt) & (deg[C.col] >= filt)
    order = np.lexsort((C.col[keep], C.row[keep]))
    rows, cols, cnt = C.row[keep][order], C.col[keep][order], C.data[keep][order]
    indptr = np.zeros(n_items + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_items), out=indptr[1:])
    return indptr, cols.astype(np.int32), cnt.astype(np.int32)


def counts_by_product(z, n_users, n_items, filt):
    u, i, _ = train_pairs(z, n_items)
    return product_counts(u, i, n_users, n_items, filt)


@pytest.mark.parametrize("name", CASES)
def test_host_sppmi_builder_gives_the_reference_sequences_and_bits(name):
    from qrec_amd.engine import sppmi_from_counts
    meta, z, (ptr, idx, val) = load_cofactor(name)
    assert (meta["sppmi_rows"], meta["sppmi_entries"]) == (int((np.diff(ptr) > 0).sum()), idx.size)
    got = sppmi_from_counts(*counts_by_product(z, meta["n_users"], meta["n_items"], meta["filter"]), meta["negCount"])
    assert np.array_equal(got[0], ptr)
    assert np.array_equal(got[1], idx)                                  # the neighbour sequences, in order
    assert np.array_equal(got[2].view(np.uint64), val.view(np.uint64))  # bit for bit


def test_sppmi_builder_without_kept_pairs():
    from qrec_amd.engine import sppmi_from_counts
    ptr, idx, val = sppmi_from_counts(np.zeros(6, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), 5)
    assert ptr.tolist() == [0] * 6 and idx.size == 0 and val.size == 0
    # one pair whose PMI is not positive: log(3 * 6 / (3 * 3)) - log(5) < 0
    ptr, idx, val = sppmi_from_counts(np.array([0, 1, 2], dtype=np.int64), np.array([1, 0], dtype=np.int32), np.array([3, 3], dtype=np.int32), 5)
    assert ptr.tolist() == [0, 0, 0] and idx.size == 0


@pytest.mark.parametrize("name", CASES)
def test_level_schedule_has_no_edge_inside_a_level(name):
    from qrec_amd.engine import cofactor_schedule
    _, _, sppmi = load_cofactor(name)
    ptr, idx, _ = sppmi
    order, lp = cofactor_schedule(ptr, idx)
    want_order, want_lp = levels_of(sppmi)
    assert np.array_equal(order, want_order) and np.array_equal(lp, want_lp)
    level = np.full(ptr.size - 1, -1)
    for l in range(lp.size - 1):
        level[order[lp[l]:lp[l + 1]]] = l
    row = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    assert (level[row] != level[idx]).all()                       # no SPPMI edge joins two items of one level
    assert (level[row] >= 0).all() and (level[idx] >= 0).all()
    earlier = idx < row
    assert (level[idx[earlier]] < level[row[earlier]]).all()      # an earlier context runs in an earlier level
    print(f"{name}: schedule depth {lp.size - 1}, widest level {int(np.diff(lp).max())}, {order.size} items")


@pytest.mark.parametrize("name", ["cofactor_filmtrust", "cofactor_filmtrust_b"])
def test_mirror_by_levels_is_the_sequential_mirror(name):
    meta, z, sppmi = load_cofactor(name)
    (l1, seq), = list(host_mirror(meta, z, sppmi, epochs=1))
    (l2, lev), = list(host_mirror(meta, z, sppmi, epochs=1, by_levels=True))
    assert l1 == l2
    for t in TABLES:
        assert np.array_equal(seq[t].view(np.uint64), lev[t].view(np.uint64)), t


@pytest.mark.parametrize("name", CASES)
def test_host_mirror_reproduces_reference_run(name):
    meta, z, sppmi = load_cofactor(name)
    X0, Y0, G0, w0, c0 = start_tables(meta)
    assert hashlib.sha256(X0.tobytes()).hexdigest() == meta["X0_sha256"]
    assert hashlib.sha256(Y0.tobytes()).hexdigest() == meta["Y0_sha256"]
    # w and c outside the items with contexts stay the draws: with the fixture's entries the whole tables are the reference's
    ctx = np.flatnonzero(np.diff(sppmi[0]) > 0)
    for k in meta["kept_epochs"]:
        for t, a0 in (("w", w0), ("c", c0)):
            full = a0.copy(); full[ctx] = z["%s%d" % (t, k)]
            assert hashlib.sha256(full.tobytes()).hexdigest() == meta["table_sha256"]["%s%d" % (t, k)]
    dist = mirror_distances(name)
    for k in sorted(dist["loss"]):
        print(f"{name} epoch {k}: mirror loss rel {dist['loss'][k]:.3e}" + ("  " + "  ".join(f"{t} {dist[k][t]:.3e}" for t in TABLES) if k in dist else ""))
    record_parity("host_mirror_vs_reference", name, {str(k): v for k, v in dist.items()})
    # the targets of the issue for the well-conditioned quantities; G, w, c are measured, not assumed
    for k in sorted(dist["loss"]):
        assert dist["loss"][k] < 1e-10, k
        if k in dist:
            assert dist[k]["X"] < 1e-9 and dist[k]["Y"] < 1e-9, (k, dist[k])
            assert all(np.isfinite(v) for v in dist[k].values())
