"""DiffNet and DHCF on the device: sparse products (qrec_spmm_csr) around the dense layer of csrc/dense_layer.hip, the batch
BPR loss with its ordered scatter, TF-1.14 Adam.  Reached as ``qrec_amd.graph.DiffNetTrainer`` / ``DHCFTrainer``."""
from __future__ import annotations

import numpy as np

from . import capi
from . import graph as _g
from .capi import DeviceBuffer, DeviceSlice
from .engine import padded_ld
from .optim import Adam


def _csr(M):
    """(indptr int64, indices int32, values float32) of a scipy matrix, duplicates summed, columns ascending"""
    M = M.tocsr(); M.sum_duplicates(); M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(np.float32)


def social_csr(n_users: int, follower, followee):
    """S of model/ranking/DiffNet.py:22-29 as a scipy CSR: row = follower, entry 1 / |followees(follower)| (float32) per
    relation row; a pair listed twice adds up, as TF's sparse product adds duplicate indices"""
    import scipy.sparse as sp
    follower = np.asarray(follower, np.int64); followee = np.asarray(followee, np.int64)
    distinct = sp.coo_matrix((np.ones(follower.size, np.float32), (follower, followee)), shape=(n_users, n_users)).tocsr()
    n_fe = np.diff(distinct.indptr)                                  # len(self.social.followees[u])
    vals = (1.0 / n_fe[follower]).astype(np.float32) if follower.size else np.zeros(0, np.float32)
    return sp.coo_matrix((vals, (follower, followee)), shape=(n_users, n_users)).tocsr()


def rating_mean_csr(n_users: int, n_items: int, uid, iid):
    """create_sparse_rating_matrix (base/graphRecommender.py:41-51): entry 1 / |items(u)| (float32) per training row"""
    import scipy.sparse as sp
    uid = np.asarray(uid, np.int64); iid = np.asarray(iid, np.int64)
    distinct = sp.coo_matrix((np.ones(uid.size, np.float32), (uid, iid)), shape=(n_users, n_items)).tocsr()
    n_it = np.diff(distinct.indptr)
    vals = (1.0 / n_it[uid]).astype(np.float32) if uid.size else np.zeros(0, np.float32)
    return sp.coo_matrix((vals, (uid, iid)), shape=(n_users, n_items)).tocsr()


def dhcf_factor_graphs(n_users: int, n_items: int, uid, iid):
    """The hypergraph operators of model/ranking/DHCF.py:29-50, A_u = D_v^-1/2 A D_e^-1 A^T D_v^-1/2 over the users and the same
    construction over A^T for the items, as TWO sparse factors over the joint [users; items] row space with the rating
    graph's own sparsity -- diag(A_u, A_i) = P Q with
        Q = [[0, D_u^-1 A D_i^-1/2], [D_i^-1 A^T D_u^-1/2, 0]],   P = [[0, D_u^-1/2 A], [D_i^-1/2 A^T, 0]]
    (D_u, D_i: user and item degrees; float64 scalings rounded to float32 once).  The product A A^T is never formed: at the
    Yelp2018 shape it is close to dense.  Returns (P, Q) as scipy CSR."""
    import scipy.sparse as sp
    A = sp.coo_matrix((np.ones(len(uid)), (np.asarray(uid, np.int64), np.asarray(iid, np.int64))), shape=(n_users, n_items)).tocsr()
    du = np.asarray(A.sum(1)).ravel(); di = np.asarray(A.sum(0)).ravel()
    with np.errstate(divide="ignore"):
        su, si, iu, ii = np.sqrt(1.0 / du), np.sqrt(1.0 / di), 1.0 / du, 1.0 / di
    for v in (su, si, iu, ii):
        v[~np.isfinite(v)] = 0.0                                     # a node without ratings: an all-zero row
    Q = sp.bmat([[None, sp.diags(iu) @ A @ sp.diags(si)], [sp.diags(ii) @ A.T @ sp.diags(su), None]], format="csr")
    P = sp.bmat([[None, sp.diags(su) @ A], [sp.diags(si) @ A.T, None]], format="csr")
    return P.astype(np.float32), Q.astype(np.float32)


LOSS_SLOTS = 256


def _ordered_loss_slots(ows):
    """parity mode: the loss is read from per-block partial sums written in a fixed order (qrec_bpr_batch_loss_slots) -- the gradient
    kernel's own loss is added up with fp64 atomics, whose order changes the last bits from launch to launch"""
    return DeviceBuffer.zeros(LOSS_SLOTS, np.float64) if ows is not None else None


def _read_loss(d_loss, slots, stream):
    if slots is None:
        return float(d_loss.numpy(stream)[0])
    total = 0.0
    for x in slots.numpy(stream).tolist():      # in slot order
        total += x
    return total


class DiffNetTrainer:
    """model/ranking/DiffNet.py:38-73 on the device.  Per layer  h = S u;  u <- relu([h | u] W_k)  (W_k: 2d x d, its two halves
    the two blocks of the dense layer -- the concat is never materialised), then  u_final = u + A V  and the batch BPR loss
    -sum log sigmoid(y) (no epsilon, :61) + regU * l2 of the three batch rows; the user row is the diffused one, so the L2 term
    flows back through every layer; the weights are not regularised.  Adam on [U; V] (one launch) and on all W_k (one launch)."""

    def __init__(self, U0, V0, W, S_csr, A_csr, lr: float, reg: float, n_layers: int):
        self.ows = _g._ordered_ws()
        self.nu, self.ni, self.d = U0.shape[0], V0.shape[0], U0.shape[1]
        self.n, self.L = self.nu + self.ni, int(n_layers)
        if len(W) != self.L:
            raise ValueError("DiffNetTrainer: one (2d x d) weight per layer")
        self.ld = ld = padded_ld(self.d, np.float32)
        if ld > 128:
            raise ValueError("DiffNet on the device supports embedding sizes up to 128")
        self.lr, self.reg = lr, reg
        nu, ni, d = self.nu, self.ni, self.d
        self.plan_S = _g.SpmmPlan(*_csr(S_csr), ld); self.plan_St = _g.SpmmPlan(*_csr(S_csr.T), ld)
        self.plan_A = _g.SpmmPlan(*_csr(A_csr), ld); self.plan_At = _g.SpmmPlan(*_csr(A_csr.T), ld)
        self.E = DeviceBuffer.from_numpy(_g.pack_joint(U0, V0, ld))   # [U; V], the parameters
        self.Eu, self.Ev = DeviceSlice(self.E, 0, (nu, ld)), DeviceSlice(self.E, nu * ld, (ni, ld))
        zu = lambda: DeviceBuffer.zeros((nu, ld), np.float32)
        self.u = [self.Eu] + [zu() for _ in range(self.L)]         # u_0 (= U), u_1 .. u_L
        self.h = [zu() for _ in range(self.L)]
        self.F = DeviceBuffer.zeros((self.n, ld), np.float32)      # [u_final; V]: what the batch looks up
        self.dF = DeviceBuffer.zeros((self.n, ld), np.float32)
        self.Fu, self.Fv = DeviceSlice(self.F, 0, (nu, ld)), DeviceSlice(self.F, nu * ld, (ni, ld))
        self.dFu, self.dFv = DeviceSlice(self.dF, 0, (nu, ld)), DeviceSlice(self.dF, nu * ld, (ni, ld))
        self.g = DeviceBuffer.zeros((self.n, ld), np.float32)      # gradient of [U; V]
        self.gu, self.gv = DeviceSlice(self.g, 0, (nu, ld)), DeviceSlice(self.g, nu * ld, (ni, ld))
        self.dpre, self.dh, self.dx, self.du = zu(), zu(), zu(), zu()
        Wp = np.zeros((self.L, 2, ld, ld), np.float32)
        for k, w in enumerate(W):
            w = np.asarray(w, np.float32)
            Wp[k, 0, :d, :d] = w[:d]; Wp[k, 1, :d, :d] = w[d:]
        self.W_all = DeviceBuffer.from_numpy(Wp)
        self.gW_all = DeviceBuffer.zeros(Wp.shape, np.float32)
        ll = 2 * ld * ld
        self.W = [DeviceSlice(self.W_all, k * ll, (2, ld, ld)) for k in range(self.L)]
        self.gW = [DeviceSlice(self.gW_all, k * ll, (2, ld, ld)) for k in range(self.L)]
        self.ws = DeviceBuffer(capi.dense_layer_ws_bytes(nu, ld, 2), np.uint8)
        self.optE = Adam(self.E, lr)
        self.optW = Adam(self.W_all, lr) if self.L else None
        self.d_loss = DeviceBuffer.zeros(1, np.float64)
        self.loss_slots = _ordered_loss_slots(self.ows)

    def forward(self, stream=None):
        """fills h_k, u_k and F = [u_L + A V; V]"""
        nu, ld = self.nu, self.ld
        for k in range(self.L):
            capi.spmm_csr(self.plan_S, self.u[k], self.h[k], ld, stream=stream)
            capi.dense_layer_fwd(self.h[k], self.u[k], self.W[k], None, nu, ld, True, self.u[k + 1], stream)
        capi.spmm_csr(self.plan_A, self.Ev, self.Fu, ld, d_addend=self.u[self.L], addend_scale=1.0, stream=stream)
        self.Fv.copy_from(self.Ev, stream)

    def train_step_async(self, d_u, d_i, d_j, B: int, stream=None):
        nu, ld = self.nu, self.ld
        self.forward(stream)
        self.dF.fill_bytes(0, stream); self.d_loss.fill_bytes(0, stream)
        if B:
            capi.bpr_batch_loss_grad(self.F, 1.0, nu, self.n, ld, d_u, d_i, d_j, B, 0.0, self.reg, self.dF, self.d_loss, stream,
                                     ordered=self.ows)
        if self.loss_slots is not None:
            capi.bpr_batch_loss_slots(self.F, 1.0, nu, ld, d_u, d_i, d_j, B, 0.0, self.reg, self.loss_slots, stream)
        capi.spmm_csr(self.plan_At, self.dFu, self.gv, ld, d_addend=self.dFv, addend_scale=1.0, stream=stream)     # dV = dF_v + A^T dF_u
        du = self.dFu
        for k in range(self.L - 1, -1, -1):
            capi.dense_layer_dpre_relu(du, self.u[k + 1], nu, ld, self.dpre, stream)
            capi.dense_layer_bwd(self.dpre, self.h[k], self.u[k], self.W[k], nu, ld, self.dh, self.dx, self.gW[k], self.ws, stream=stream)
            out = self.gu if k == 0 else self.du             # the incoming du was consumed by dpre above
            capi.spmm_csr(self.plan_St, self.dh, out, ld, d_addend=self.dx, addend_scale=1.0, stream=stream)      # du_k = dx + S^T dh
            du = out
        if self.L == 0:
            self.gu.copy_from(self.dFu, stream)
        self.optE.step(self.g, stream=stream)
        if self.L:
            self.optW.step(self.gW_all, stream=stream)

    def loss(self, stream=None) -> float:
        return _read_loss(self.d_loss, self.loss_slots, stream)

    def _weights(self, buf):
        a, d = buf.numpy(), self.d
        return [np.concatenate([a[k, 0, :d, :d], a[k, 1, :d, :d]]) for k in range(self.L)]

    def parameters(self):
        """(U, V, [W_k (2d x d)])"""
        return (*_g.split_joint(self.E.numpy(), self.nu, self.d), self._weights(self.W_all))

    def gradients(self):
        """(dU, dV, [dW_k]) of the last step, before Adam"""
        return (*_g.split_joint(self.optE.applied_gradient(), self.nu, self.d), self._weights(self.gW_all))

    def inference_embeddings(self):
        """(u_final, V): the tables DiffNet.py:57 scores with"""
        self.forward()
        return _g.split_joint(self.F.numpy(), self.nu, self.d)


class DHCFTrainer:
    """model/ranking/DHCF.py:26-121 on the device, its quirks kept:
      * both layers propagate the LAYER-0 tables (``self.user_embeddings``, :75-76), so H_u U_0 and H_i V_0 are formed once per step;
      * users and items share one W_k per layer (:78-79);
      * the residual of layer k is layer k-1's OUTPUT, i.e. the dropped-out, l2-normalised rows (:78, :86-87);
      * the output is the 3d-wide concat [E_0 | z_1 | z_2] (:95-96);
      * regU * l2_loss(W_k) is part of the loss (:109-110) -- folded into Adam's gradient as TF's minimize() sees it;
      * no epsilon inside the log (:111).
    The operators A_u, A_i are applied in factored form (``dhcf_factor_graphs``): two sparse products over the rating graph, both
    ways (diag(A_u, A_i) is symmetric).  Dropout (rate 0.1, :72): Philox on the device, or ``masks=`` (0/1 keep decisions per
    layer over the joint rows) for parity runs."""

    KEEP = 0.9
    N_LAYERS = 2

    def __init__(self, U0, V0, W, uid, iid, lr: float, reg: float, seed: int = 0):
        self.ows = _g._ordered_ws()
        self.nu, self.ni, self.d = U0.shape[0], V0.shape[0], U0.shape[1]
        self.n = n = self.nu + self.ni
        self.ld = ld = padded_ld(self.d, np.float32)
        if ld > 128 or 3 * self.d > 256:
            raise ValueError("DHCF on the device supports embedding sizes up to 85 (3d <= 256)")
        self.wide_d, self.wide_ld = 3 * self.d, padded_ld(3 * self.d, np.float32)
        self.lr, self.reg, self.seed = lr, reg, seed
        P, Q = dhcf_factor_graphs(self.nu, self.ni, uid, iid)
        self.plan_P = _g.SpmmPlan(*_csr(P), ld, split_row=self.nu); self.plan_Q = _g.SpmmPlan(*_csr(Q), ld, split_row=self.nu)
        z = lambda: DeviceBuffer.zeros((n, ld), np.float32)
        self.Z = [DeviceBuffer.from_numpy(_g.pack_joint(U0, V0, ld)), z(), z()]          # E_0 (parameters), z_1, z_2: each layer's residual input / output
        self.T, self.side, self.nxt = z(), z(), z()
        self.gate = [z(), z()]
        self.inv = [DeviceBuffer.zeros(n, np.float32), DeviceBuffer.zeros(n, np.float32)]
        self.dpre = [z(), z()]; self.dside, self.gE = z(), z()
        self.All = DeviceBuffer.zeros((n, self.wide_ld), np.float32)
        self.dAll = DeviceBuffer.zeros((n, self.wide_ld), np.float32)
        pad = lambda w: np.pad(np.asarray(w, np.float32), ((0, ld - self.d), (0, ld - self.d)))
        self.W_all = DeviceBuffer.from_numpy(np.stack([pad(w) for w in W]))
        self.W_prev = DeviceBuffer.zeros((2, ld, ld), np.float32)  # the weights a step started from: its L2 gradient is reg * these
        self.gW_all = DeviceBuffer.zeros((2, ld, ld), np.float32)
        self.W = [DeviceSlice(self.W_all, k * ld * ld, (ld, ld)) for k in range(2)]
        self.gW = [DeviceSlice(self.gW_all, k * ld * ld, (ld, ld)) for k in range(2)]
        self.ws = DeviceBuffer(capi.dense_layer_ws_bytes(n, ld, 1), np.uint8)
        self.optE = Adam(self.Z[0], lr)
        self.optW = Adam(self.W_all, lr)
        self.d_loss = DeviceBuffer.zeros(1, np.float64)
        self.loss_slots = _ordered_loss_slots(self.ows)
        self.step_no = 0

    def _propagate(self, x, y, stream, addend=None):
        """y = diag(A_u, A_i) x (+ addend): Q first, then P"""
        capi.spmm_csr(self.plan_Q, x, self.T, self.ld, stream=stream)
        capi.spmm_csr(self.plan_P, self.T, y, self.ld, d_addend=addend, addend_scale=1.0 if addend is not None else 0.0, stream=stream)

    def forward(self, training: bool, masks=None, stream=None):
        """fills side = H E_0, gate, inv, z_1, z_2 and the wide table All = [E_0 | z_1 | z_2]"""
        n, d, ld = self.n, self.d, self.ld
        capi.copy_cols(self.All, self.wide_ld, self.Z[0], ld, 0, n, d, False, stream)
        self._propagate(self.Z[0], self.side, stream)
        for k in range(self.N_LAYERS):
            capi.dense_layer_fwd(self.side, None, self.W[k], self.Z[k], n, ld, False, self.gate[k], stream)
            # LeakyReLU(0.2) -> dropout -> l2_normalize: NGCF's activation step; its un-normalised output is not carried on here
            capi.ngcf_activate(self.gate[k], n, d, ld, self.KEEP if training else 1.0, None if masks is None else masks[k],
                               self.seed, self.step_no * 8 + k, self.nxt, self.All, self.wide_ld, (k + 1) * d, self.inv[k], stream)
            capi.copy_cols(self.Z[k + 1], ld, self.All, self.wide_ld, (k + 1) * d, n, d, False, stream)

    def train_step_async(self, d_u, d_i, d_j, B: int, masks=None, stream=None):
        n, d, ld = self.n, self.d, self.ld
        self.forward(True, masks, stream)
        self.dAll.fill_bytes(0, stream); self.d_loss.fill_bytes(0, stream)
        if B:
            capi.bpr_batch_loss_grad(self.All, 1.0, self.nu, n, self.wide_ld, d_u, d_i, d_j, B, 0.0, self.reg, self.dAll, self.d_loss,
                                     stream, ordered=self.ows)
        if self.loss_slots is not None:
            capi.bpr_batch_loss_slots(self.All, 1.0, self.nu, self.wide_ld, d_u, d_i, d_j, B, 0.0, self.reg, self.loss_slots, stream)
        for k in (1, 0):
            capi.dense_layer_dpre_norm(self.dAll, self.All, self.wide_ld, (k + 1) * d, self.dpre[1] if k == 0 else None, self.inv[k],
                                       self.gate[k], n, d, ld, self.dpre[k], stream)
            capi.dense_layer_bwd(self.dpre[k], self.side, None, self.W[k], n, ld, self.dside, None, self.gW[k], self.ws,
                                 accumulate_dX1=(k == 0), stream=stream)
        # dE_0 = ego block of the concat + the first layer's residual + H^T dside (H symmetric)
        capi.copy_cols(self.dpre[0], ld, self.dAll, self.wide_ld, 0, n, d, True, stream)
        self._propagate(self.dside, self.gE, stream, addend=self.dpre[0])
        self.W_prev.copy_from(self.W_all, stream)
        self.optE.step(self.gE, stream=stream)
        self.optW.step(self.gW_all, stream=stream, grad_l2=self.reg)
        self.step_no += 1

    def loss(self, stream=None) -> float:
        """the batch loss incl. the weights' L2 term (the weights the step started from)"""
        w = self.W_prev.numpy(stream).astype(np.float64)
        return _read_loss(self.d_loss, self.loss_slots, stream) + self.reg * 0.5 * float((w * w).sum())

    def parameters(self):
        """(U, V, [W_1, W_2])"""
        return (*_g.split_joint(self.Z[0].numpy(), self.nu, self.d), [w.numpy()[:self.d, :self.d].copy() for w in self.W])

    def gradients(self):
        """(dU, dV, [dW_1, dW_2]) of the last step as minimize() applied them, before Adam"""
        gw = self.optW.applied_gradient(self.W_prev.numpy())
        return (*_g.split_joint(self.optE.applied_gradient(), self.nu, self.d), [gw[k, :self.d, :self.d] for k in range(2)])

    def inference_embeddings(self):
        """3d-wide (U, V) of the inference graph (isTraining = 0, DHCF.py:123-127)"""
        self.forward(False)
        return _g.split_joint(self.All.numpy(), self.nu, self.wide_d)
