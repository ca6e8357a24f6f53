"""float64 numpy restatement of the reference's DiffNet (model/ranking/DiffNet.py:22-65) and DHCF (model/ranking/DHCF.py:16-113),
written from the maths: forward, loss, analytic gradients, TF-1.14 Adam.  The checker of tests/test_diffusion_cpu.py (against
the reference's own recorded runs) and tests/test_gpu_diffusion.py (against the HIP trainers)."""
import numpy as np
import scipy.sparse as sp


# ---- the dense layer on its own (csrc/dense_layer.hip) ------------------------------------------------------------------------
def layer_fwd(X1, X2, W, R=None, relu=False):
    """Y = [X1 | X2] W (+ R); W: [d, d] or (with X2) [2d, d]"""
    X = X1 if X2 is None else np.concatenate([X1, X2], 1)
    Y = X @ W
    if R is not None:
        Y = Y + R
    return np.maximum(Y, 0.0) if relu else Y


def layer_bwd(dpre, X1, X2, W):
    """(dX1, dX2 or None, dW); the residual's gradient is dpre itself"""
    d = X1.shape[1]
    X = X1 if X2 is None else np.concatenate([X1, X2], 1)
    dX = dpre @ W.T
    return dX[:, :d], (None if X2 is None else dX[:, d:]), X.T @ dpre


def ngcf_fwd(E, S, W1, W2):
    """NGCF's propagation layer before its activation: pre = (S + E) W1 + (E * S) W2"""
    return (S + E) @ W1 + (E * S) @ W2


def ngcf_bwd(dpre, E, S, W1, W2):
    """(dside, dE, gW1, gW2) of ngcf_fwd; dE without the sparse product's share (A^T dside)"""
    dA1, dA2 = dpre @ W1.T, dpre @ W2.T
    return dA1 + dA2 * E, dA1 + dA2 * S, (S + E).T @ dpre, (E * S).T @ dpre


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
def social_matrix(n_users, follower, followee):
    """DiffNet.py:22-29: entry 1 / |followees(follower)| per relation row, duplicates summed (coo -> TF's sparse product)"""
    follower = np.asarray(follower, np.int64); followee = np.asarray(followee, np.int64)
    distinct = sp.coo_matrix((np.ones(follower.size), (follower, followee)), shape=(n_users, n_users)).tocsr()
    n_fe = np.diff(distinct.indptr).astype(np.float64)                     # len(self.social.followees[u]): distinct followees
    vals = (1.0 / n_fe[follower]).astype(np.float32).astype(np.float64)      # the reference's coo_matrix is float32
    return sp.coo_matrix((vals, (follower, followee)), shape=(n_users, n_users)).tocsr()


def rating_matrix(n_users, n_items, uid, iid):
    """base/graphRecommender.py:41-51: entry 1 / |items(u)| per training row"""
    uid = np.asarray(uid, np.int64); iid = np.asarray(iid, np.int64)
    distinct = sp.coo_matrix((np.ones(uid.size), (uid, iid)), shape=(n_users, n_items)).tocsr()
    n_it = np.diff(distinct.indptr).astype(np.float64)
    vals = (1.0 / n_it[uid]).astype(np.float32).astype(np.float64)
    return sp.coo_matrix((vals, (uid, iid)), shape=(n_users, n_items)).tocsr()


def dhcf_operators(n_users, n_items, uid, iid):
    """DHCF.py:29-50, formed as the reference forms them: A_u = D_v^-1/2 A D_e^-1 A^T D_v^-1/2 and the same over A^T"""
    A = sp.coo_matrix((np.ones(len(uid)), (np.asarray(uid, np.int64), np.asarray(iid, np.int64))), shape=(n_users, n_items)).tocsr()

    def formed(H):
        dv = np.asarray(H.sum(1)).ravel(); de = np.asarray(H.sum(0)).ravel()
        with np.errstate(divide="ignore"):
            M = sp.diags(np.sqrt(1.0 / dv)) @ H
            return (M @ sp.diags(1.0 / de) @ M.T).tocsr()
    return formed(A), formed(A.T.tocsr())


def dhcf_factors(n_users, n_items, uid, iid):
    """the same two operators in factored form over the joint [users; items] row space: H = P Q with
    Q = [[0, D_u^-1 A D_i^-1/2], [D_i^-1 A^T D_u^-1/2, 0]] and P = [[0, D_u^-1/2 A], [D_i^-1/2 A^T, 0]] (never multiplied out)"""
    A = sp.coo_matrix((np.ones(len(uid)), (np.asarray(uid, np.int64), np.asarray(iid, np.int64))), shape=(n_users, n_items)).tocsr()
    du = np.asarray(A.sum(1)).ravel(); di = np.asarray(A.sum(0)).ravel()
    with np.errstate(divide="ignore"):
        su, si, iu, ii = np.sqrt(1.0 / du), np.sqrt(1.0 / di), 1.0 / du, 1.0 / di
    for v in (su, si, iu, ii):
        v[~np.isfinite(v)] = 0.0
    Q = sp.bmat([[None, sp.diags(iu) @ A @ sp.diags(si)], [sp.diags(ii) @ A.T @ sp.diags(su), None]]).tocsr()
    P = sp.bmat([[None, sp.diags(su) @ A], [sp.diags(si) @ A.T, None]]).tocsr()
    return P, Q


# ---- loss head shared by both (DiffNet.py:59-63, DHCF.py:105-111): no epsilon inside the log ------------------------------------
def _bpr_head(Fu, Fv, u, i, j, reg):
    """loss and the gradients w.r.t. the user table Fu and the item table Fv"""
    eu, ei, ej = Fu[u], Fv[i], Fv[j]
    y = (eu * ei).sum(1) - (eu * ej).sum(1)
    sig = 1.0 / (1.0 + np.exp(-y))
    loss = -np.log(sig).sum() + reg * 0.5 * ((eu ** 2).sum() + (ei ** 2).sum() + (ej ** 2).sum())
    c = -(1.0 - sig)[:, None]
    dFu = np.zeros_like(Fu); dFv = np.zeros_like(Fv)
    np.add.at(dFu, u, c * (ei - ej) + reg * eu)
    np.add.at(dFv, i, c * eu + reg * ei)
    np.add.at(dFv, j, -c * eu + reg * ej)
    return loss, dFu, dFv


def diffnet_loss_grads(U, V, Ws, S, A, u, i, j, reg):
    """(loss, dU, dV, [dW_k]) of DiffNet.py:45-63; Ws: list of (2d x d)"""
    hs, us = [], [U]
    for W in Ws:
        h = S @ us[-1]
        hs.append(h); us.append(layer_fwd(h, us[-1], W, relu=True))
    F = us[-1] + A @ V
    loss, dF, dV = _bpr_head(F, V, u, i, j, reg)
    dV = dV + A.T @ dF
    du, dWs = dF, [None] * len(Ws)
    for k in range(len(Ws) - 1, -1, -1):
        dpre = du * (us[k + 1] > 0)
        dh, dx, dWs[k] = layer_bwd(dpre, hs[k], us[k], Ws[k])
        du = dx + S.T @ dh
    return loss, du, dV, dWs


def diffnet_final(U, V, Ws, S, A):
    u = U
    for W in Ws:
        u = layer_fwd(S @ u, u, W, relu=True)
    return u + A @ V


def _dhcf_forward(E0, Ws, H, masks, keep):
    side = H @ E0
    z, cache, blocks = E0, [], [E0]
    for k, W in enumerate(Ws):
        pre = side @ W + z
        act = np.where(pre > 0, pre, 0.2 * pre)
        fac = np.ones_like(pre) if masks is None else masks[k] / keep
        nxt = act * fac
        inv = 1.0 / np.sqrt(np.maximum((nxt ** 2).sum(1, keepdims=True), 1e-12))
        cache.append((fac * np.where(pre > 0, 1.0, 0.2), inv))
        z = nxt * inv
        blocks.append(z)
    return side, blocks, cache


def dhcf_loss_grads(U, V, Ws, H, u, i, j, reg, masks=None, keep=0.9):
    """(loss, dU, dV, [dW_k]) of DHCF.py:62-111.  H: the block-diagonal operator diag(A_u, A_i) over [users; items] (symmetric);
    masks[k]: 0/1 keep decisions of layer k over the joint rows (None: the inference graph).  Both layers propagate the LAYER-0
    tables (:75-76), share W_k between users and items, carry the normalised rows as the residual; reg * l2_loss(W_k) is in."""
    nu = U.shape[0]
    E0 = np.concatenate([U, V])
    side, blocks, cache = _dhcf_forward(E0, Ws, H, masks, keep)
    All = np.concatenate(blocks, 1)
    loss, dFu, dFv = _bpr_head(All[:nu], All[nu:], u, i, j, reg)
    loss += sum(reg * 0.5 * (W ** 2).sum() for W in Ws)
    dAll = np.concatenate([dFu, dFv])
    d = U.shape[1]
    dside = np.zeros_like(E0); dWs = [None] * len(Ws); dz_next = 0.0
    for k in range(len(Ws) - 1, -1, -1):
        gate, inv = cache[k]
        z = blocks[k + 1]
        dz = dAll[:, (k + 1) * d:(k + 2) * d] + dz_next
        dpre = (dz - z * (z * dz).sum(1, keepdims=True)) * inv * gate
        dside += dpre @ Ws[k].T
        dWs[k] = side.T @ dpre + reg * Ws[k]
        dz_next = dpre
    dE0 = dAll[:, :d] + dz_next + H.T @ dside
    return loss, dE0[:nu], dE0[nu:], dWs


def dhcf_inference(U, V, Ws, H):
    """the 3d-wide tables of the inference graph (isTraining = 0, DHCF.py:123-127)"""
    _, blocks, _ = _dhcf_forward(np.concatenate([U, V]), Ws, H, None, 1.0)
    All = np.concatenate(blocks, 1)
    return All[:U.shape[0]], All[U.shape[0]:]


class Adam:
    """tf.train.AdamOptimizer (TF 1.14 ApplyAdam) in float64"""

    def __init__(self, params, lr):
        self.p = [np.array(x, np.float64) for x in params]
        self.m = [np.zeros_like(x) for x in self.p]; self.v = [np.zeros_like(x) for x in self.p]
        self.lr, self.t = lr, 0

    def step(self, grads):
        self.t += 1
        alpha = self.lr * np.sqrt(1 - 0.999 ** self.t) / (1 - 0.9 ** self.t)
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            m += (g - m) * (1 - 0.9); v += (g * g - v) * (1 - 0.999)
            p -= m * alpha / (np.sqrt(v) + 1e-8)
