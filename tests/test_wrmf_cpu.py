"""WRMF without a GPU: the model is provided, and the formulation the ALS kernel implements -- the sparse form of
model/ranking/WRMF.py:17-67 solved by Cholesky -- reproduces the unmodified reference's runs
(tests/golden/gen_golden_wrmf.py) in fp64."""
import hashlib
import json
import os

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from helpers import GOLDEN


def load_wrmf(name):
    meta = json.load(open(os.path.join(GOLDEN, "golden_wrmf_meta.json")))[name]
    return meta, np.load(os.path.join(GOLDEN, name + ".npz"))


def csr(rows, cols, vals, n_rows):
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
    return indptr, cols[order], vals[order]


def train_pairs(z, n_items):
    """trainSet_u semantics: a duplicated (user, item) pair keeps its last rating"""
    u, i, r = z["train_uid"].astype(np.int64), z["train_iid"].astype(np.int64), z["train_r"]
    key = u * n_items + i
    _, last_rev = np.unique(key[::-1], return_index=True)
    keep = np.sort(key.size - 1 - last_rev)
    return u[keep], i[keep], r[keep]


def half_sweep(F, X, indptr, cols, c, lam, with_loss):
    """every row of X: (F^T F + sum c f f^T + lam I) x = sum (1 + c) f; loss from the rows before their update"""
    d = F.shape[1]
    G = F.T.dot(F) + lam * np.eye(d)
    loss = 0.0
    for r in range(indptr.size - 1):
        k = slice(indptr[r], indptr[r + 1])
        Fr, cr = F[cols[k]], c[k]
        if with_loss:
            loss += float(((1.0 - Fr.dot(X[r])) ** 2).sum())
        A = G + (Fr.T * cr).dot(Fr)
        X[r] = cho_solve(cho_factor(A, lower=True), (Fr.T * (1.0 + cr)).sum(axis=1))
    return loss


def host_mirror(X0, Y0, u, i, r, lam, epochs):
    X, Y = X0.copy(), Y0.copy()
    c = 10.0 * r
    users = csr(u, i, c, X.shape[0])
    items = csr(i, u, c, Y.shape[0])
    for _ in range(epochs):
        loss = half_sweep(Y, X, *users, lam, True)
        half_sweep(X, Y, *items, lam, False)
        yield loss, X, Y


def rel_max(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_resolve_model_provides_wrmf():
    from qrec_amd.QRec import resolve_model
    from qrec_amd.model.ranking.WRMF import WRMF
    assert resolve_model("WRMF") is WRMF


def test_resolve_model_error_lists_wrmf():
    from qrec_amd.QRec import resolve_model
    with pytest.raises(ImportError, match="WRMF"):
        resolve_model("NoSuchModel")


@pytest.mark.parametrize("name", ["wrmf_filmtrust", "wrmf_lastfm"])
def test_host_mirror_reproduces_reference_run(name):
    meta, z = load_wrmf(name)
    U, I, d = meta["n_users"], meta["n_items"], meta["emb_size"]
    np.random.seed(meta["seed"])     # base initModel's draws (np.random legacy stream), times 10 (WRMF.py:14-15)
    X0 = np.random.rand(U, d) / 3 * 10
    Y0 = np.random.rand(I, d) / 3 * 10
    assert hashlib.sha256(X0.tobytes()).hexdigest() == meta["X0_sha256"]
    assert hashlib.sha256(Y0.tobytes()).hexdigest() == meta["Y0_sha256"]
    u, i, r = train_pairs(z, I)
    kept, s = set(meta["kept_epochs"]), meta["row_stride"]     # the fixture keeps every s-th row of the tables
    for k, (loss, X, Y) in enumerate(host_mirror(X0, Y0, u, i, r, meta["regU"], len(meta["epochs"])), 1):
        assert loss == pytest.approx(meta["epochs"][k - 1]["loss"], rel=1e-10)
        assert loss == pytest.approx(float(z["loss"][k - 1]), rel=1e-10)
        if k in kept:
            assert rel_max(X[::s], z["X%d" % k]) < 1e-10, k
            assert rel_max(Y[::s], z["Y%d" % k]) < 1e-10, k
