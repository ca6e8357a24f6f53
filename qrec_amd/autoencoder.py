"""CDAE on the device (model/ranking/CDAE.py): the batch lists the kernels of csrc/autoencoder.hip consume, and the trainer.

The reference feeds four dense batch x n_items arrays per step.  What moves numbers is the kept inputs (rated and mask = 1) and the
live loss positions ((rated or sampled negative) and mask = 1): everywhere else it multiplies by an exact 0.  ``BatchLists`` holds
exactly those, row-major (CSR over the batch rows, item ids ascending) and item-major (CSC, batch rows ascending; a live entry carries
the index of its CSR slot), so that both the forward pass and the transposed weight-gradient passes walk contiguous lists."""
from __future__ import annotations

import numpy as np

from . import capi
from .capi import DeviceBuffer, DeviceSlice
from .engine import padded_ld
from .optim import Adam, AdamClock

NEGATIVES_PER_RATED = 5          # CDAE.py:53


class BatchLists:
    """one batch in list form, host (numpy) or device (DeviceBuffer / DeviceSlice) arrays under the same names:
    users [B]; in_ptr [B+1], in_item, in_val; in_cptr [n_items+1], in_crow, in_cval; lv_ptr [B+1], lv_item, lv_label;
    lv_cptr [n_items+1], lv_crow, lv_cslot.  int32 everywhere but the float32 values."""
    INT = ("users", "in_ptr", "in_item", "in_cptr", "in_crow", "lv_ptr", "lv_item", "lv_label", "lv_cptr", "lv_crow", "lv_cslot")
    FLOAT = ("in_val", "in_cval")
    NAMES = INT + FLOAT

    def __init__(self, B: int, n_items: int, **arrays):
        self.B, self.n_items = int(B), int(n_items)
        for k in self.NAMES:
            setattr(self, k, arrays[k])
        self.on_device = isinstance(self.users, DeviceBuffer)

    @property
    def n_in(self) -> int:
        return self._n[0] if hasattr(self, "_n") else int(self.in_item.shape[0])

    @property
    def n_live(self) -> int:
        return self._n[1] if hasattr(self, "_n") else int(self.lv_item.shape[0])

    def host(self) -> "BatchLists":
        if not self.on_device:
            return self
        a = {k: getattr(self, k).numpy().ravel() for k in self.NAMES}       # entry arrays may be capacities: cut to the counts
        B, ni, n_in, n_lv = self.B, self.n_items, int(a["in_ptr"][self.B]), int(a["lv_ptr"][self.B])
        size = dict(users=B, in_ptr=B + 1, lv_ptr=B + 1, in_cptr=ni + 1, lv_cptr=ni + 1, in_item=n_in, in_val=n_in, in_crow=n_in, in_cval=n_in)
        return BatchLists(B, ni, **{k: v[:size.get(k, n_lv)].copy() for k, v in a.items()})

    def device_copy(self) -> "BatchLists":
        """the same lists in device buffers of their own (a trainer takes either form)"""
        if self.on_device:
            return self
        self.validate()
        up = lambda a, t: DeviceBuffer.from_numpy(np.ascontiguousarray(a, t) if a.size else np.zeros(1, t))
        out = BatchLists(self.B, self.n_items, **{k: up(getattr(self, k), np.float32 if k in self.FLOAT else np.int32) for k in self.NAMES})
        out._n = (self.n_in, self.n_live)
        return out

    def validate(self):
        """host lists only: every index inside its table, rows ascending -- the kernels skip bad ids, this names them"""
        B, ni = self.B, self.n_items
        for ptr, item, n in ((self.in_ptr, self.in_item, self.n_in), (self.lv_ptr, self.lv_item, self.n_live)):
            if ptr.size != B + 1 or ptr[0] != 0 or ptr[-1] != n or (np.diff(ptr) < 0).any():
                raise ValueError("BatchLists: bad row pointer")
            if n and (item.min() < 0 or item.max() >= ni):
                raise ValueError("BatchLists: item id out of range")
        for ptr, row, n in ((self.in_cptr, self.in_crow, self.n_in), (self.lv_cptr, self.lv_crow, self.n_live)):
            if ptr.size != ni + 1 or ptr[0] != 0 or ptr[-1] != n or (np.diff(ptr) < 0).any():
                raise ValueError("BatchLists: bad item pointer")
            if n and (row.min() < 0 or row.max() >= B):
                raise ValueError("BatchLists: batch row out of range")
        if self.n_live and (self.lv_cslot.min() < 0 or self.lv_cslot.max() >= self.n_live):
            raise ValueError("BatchLists: slot index out of range")


def _csr_csc(B, n_items, rows, items):
    """entries (rows, items), distinct pairs -> (order into the entries giving the CSR, ptr, cptr, csc order into the CSR)"""
    order = np.argsort(rows.astype(np.int64) * n_items + items, kind="stable")
    r, i = rows[order], items[order]
    ptr = np.zeros(B + 1, np.int32); np.cumsum(np.bincount(r, minlength=B), out=ptr[1:])
    cptr = np.zeros(n_items + 1, np.int32); np.cumsum(np.bincount(i, minlength=n_items), out=cptr[1:])
    corder = np.argsort(i, kind="stable")          # stable: batch rows stay ascending inside an item
    return order, ptr, cptr, corder.astype(np.int32)


def lists_from_entries(users, n_items: int, pos_rows, pos_items, pos_vals, neg_rows, neg_items, keep) -> BatchLists:
    """``pos_*``: the rated items of every batch row with their ratings; ``neg_*``: the sampled negatives (duplicates allowed, they are a
    set per row); ``keep(rows, items) -> bool array``: the corruption mask at those positions"""
    users = np.ascontiguousarray(users, np.int32)
    B = users.size
    pos_rows = np.asarray(pos_rows, np.int32); pos_items = np.asarray(pos_items, np.int32); pos_vals = np.asarray(pos_vals, np.float32)
    nkey = np.unique(np.asarray(neg_rows, np.int64) * n_items + np.asarray(neg_items, np.int64))
    neg_rows, neg_items = (nkey // n_items).astype(np.int32), (nkey % n_items).astype(np.int32)
    kp = keep(pos_rows, pos_items)
    pr, pi, pv = pos_rows[kp], pos_items[kp], pos_vals[kp]
    o, in_ptr, in_cptr, co = _csr_csc(B, n_items, pr, pi)
    in_item, in_val = pi[o], pv[o]
    kn = keep(neg_rows, neg_items)
    lr = np.concatenate([pr, neg_rows[kn]]); li = np.concatenate([pi, neg_items[kn]])
    ll = np.concatenate([np.ones(pr.size, np.int32), np.zeros(int(kn.sum()), np.int32)])
    o2, lv_ptr, lv_cptr, co2 = _csr_csc(B, n_items, lr, li)
    lv_row = lr[o2]
    c = np.ascontiguousarray
    return BatchLists(B, n_items, users=users, in_ptr=in_ptr, in_item=c(in_item), in_val=c(in_val), in_cptr=in_cptr,
                      in_crow=c(pr[o][co]), in_cval=c(in_val[co]), lv_ptr=lv_ptr, lv_item=c(li[o2]), lv_label=c(ll[o2]),
                      lv_cptr=lv_cptr, lv_crow=c(lv_row[co2]), lv_cslot=c(co2))


def lists_from_dense(users, X, positive, negative, mask) -> BatchLists:
    """the reference's four dense feeds of one step (CDAE.py:89-92) in list form"""
    X = np.asarray(X); mask = np.asarray(mask)
    pr, pi = np.nonzero(np.asarray(positive))
    nr, ni = np.nonzero(np.asarray(negative))
    return lists_from_entries(users, X.shape[1], pr, pi, X[pr, pi], nr, ni, lambda r, i: mask[r, i] != 0)


def rated_rows(users, rated_indptr, rated_items, rated_vals):
    """(rows, items, values) of the rated items of the batch's users, from the rated CSR over all users"""
    users = np.asarray(users, np.int64)
    cnt = (rated_indptr[users + 1] - rated_indptr[users]).astype(np.int64)
    rows = np.repeat(np.arange(users.size, dtype=np.int32), cnt)
    start = np.repeat(rated_indptr[users] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
    idx = start + np.arange(int(cnt.sum()), dtype=np.int64)
    return rows, rated_items[idx], rated_vals[idx]


class DeviceBatchStream:
    """the batch stream of throughput mode: users, negatives and keep decisions drawn on the device (Philox of seed, step and
    position; qrec_cdae_draw_batch) and the lists built there -- the reference's distribution, not its streams.  ``draw(step)``
    fills ONE set of list buffers, on the stream the training steps run on: the draw of step k + 1 is ordered behind the
    kernels of step k that read them.  The entry arrays are capacities (no count is read back): a row holds at most its
    user's rated items as inputs and (1 + per_rated) times as many live positions."""

    def __init__(self, rated_indptr, rated_items, rated_vals, n_items: int, batch: int, keep_prob: float, seed: int = 0,
                 per_rated: int = NEGATIVES_PER_RATED):
        indptr = np.ascontiguousarray(rated_indptr, np.int64)
        items = np.ascontiguousarray(rated_items, np.int32)
        self.nu, self.ni, self.B = indptr.size - 1, int(n_items), int(batch)
        if self.nu < 1 or self.B < 1 or indptr[0] != 0 or indptr[-1] != items.size or (np.diff(indptr) < 0).any():
            raise ValueError("DeviceBatchStream: bad rated CSR")
        if items.size and (items.min() < 0 or items.max() >= self.ni):
            raise ValueError("DeviceBatchStream: item id out of range")
        for u in range(self.nu):
            if (np.diff(items[indptr[u]:indptr[u + 1]]) <= 0).any():
                raise ValueError("DeviceBatchStream: the rated rows must be ascending")
        heaviest = int(np.diff(indptr).max())
        self.cap_in = max(1, self.B * heaviest)
        self.cap_live = max(1, self.B * min(self.ni, (1 + per_rated) * heaviest))
        if self.cap_live >= 2 ** 31:
            raise ValueError("DeviceBatchStream: the batch's lists would not fit int32 indices")
        self.keep_prob, self.seed, self.per_rated = float(keep_prob), int(seed), int(per_rated)
        nz = lambda a, t: DeviceBuffer.from_numpy(a if a.size else np.zeros(1, t))
        self.d_rated = (DeviceBuffer.from_numpy(indptr), nz(items, np.int32), nz(np.ascontiguousarray(rated_vals, np.float32), np.float32))
        self.ws = DeviceBuffer(max(capi.cdae_draw_workspace_bytes(self.B, self.ni), 4), np.uint8)
        self.cand_count = DeviceBuffer.zeros(self.B, np.int32)
        n = dict(users=self.B, in_ptr=self.B + 1, lv_ptr=self.B + 1, in_cptr=self.ni + 1, lv_cptr=self.ni + 1, in_item=self.cap_in,
                 in_val=self.cap_in, in_crow=self.cap_in, in_cval=self.cap_in)
        self.lists = BatchLists(self.B, self.ni, **{k: DeviceBuffer.zeros(n.get(k, self.cap_live), np.float32 if k in BatchLists.FLOAT else np.int32)
                                                    for k in BatchLists.NAMES})
        self.lists._n = (self.cap_in, self.cap_live)

    def draw(self, step: int, stream=None) -> BatchLists:
        capi.cdae_draw_batch(*self.d_rated, self.nu, self.ni, self.B, self.per_rated, self.keep_prob, self.seed, int(step), self.cap_in,
                             self.cap_live, self.ws, self.lists, self.cand_count, stream)
        return self.lists


class CdaeTrainer:
    """CDAE.py:51-93 on the device.  Variables as the reference shapes them: W_enc [n_items, nh], W_dec [nh, n_items], b_enc [nh],
    b_dec [n_items], V [n_users, nh]; on the device the decoder weight is item-major (transposed at this boundary).  The four weight
    variables sit in ONE buffer (one Adam launch, reg * theta folded in as grad_l2); V has its own, and its L2 term -- over the
    gathered rows, once per occurrence -- comes from the hidden-backward kernel.  TF's sparse Adam apply decays the slots of, and
    moves, every row of V each step, so the dense update over all of V is the reference's.
    No kernel here uses a float atomic in either mode: ``ordered_reductions`` has nothing to switch."""

    def __init__(self, W_enc, W_dec, b_enc, b_dec, V, lr: float, reg: float):
        W_enc, W_dec, V = (np.asarray(a, np.float32) for a in (W_enc, W_dec, V))
        self.ni, self.nh = W_enc.shape
        self.nu = V.shape[0]
        if W_dec.shape != (self.nh, self.ni) or V.shape[1] != self.nh or np.shape(b_enc) != (self.nh,) or np.shape(b_dec) != (self.ni,):
            raise ValueError("CdaeTrainer: W_enc [n_items, nh], W_dec [nh, n_items], b_enc [nh], b_dec [n_items], V [n_users, nh]")
        if self.nh > capi.CDAE_MAX_LD:
            raise ValueError(f"CDAE on the device supports hidden sizes up to {capi.CDAE_MAX_LD}")
        self.ld = ld = padded_ld(self.nh, np.float32)
        self.lr, self.reg = float(lr), float(reg)
        ni, nu, nh = self.ni, self.nu, self.nh
        self.n_theta = 2 * ni * ld + ld + -(-ni // 32) * 32          # b_dec zero-padded: qrec_adam_step takes multiples of 4 elements
        theta = np.zeros(self.n_theta, np.float32)
        theta[:ni * ld].reshape(ni, ld)[:, :nh] = W_enc
        theta[ni * ld:2 * ni * ld].reshape(ni, ld)[:, :nh] = W_dec.T
        theta[2 * ni * ld:2 * ni * ld + nh] = b_enc
        theta[2 * ni * ld + ld:2 * ni * ld + ld + ni] = b_dec
        self.theta = DeviceBuffer.from_numpy(theta)
        self.g_theta = DeviceBuffer.zeros(self.n_theta, np.float32)
        carve = lambda buf: (DeviceSlice(buf, 0, (ni, ld)), DeviceSlice(buf, ni * ld, (ni, ld)), DeviceSlice(buf, 2 * ni * ld, (ld,)),
                             DeviceSlice(buf, 2 * ni * ld + ld, (ni,)))
        self.W_enc, self.W_dec, self.b_enc, self.b_dec = carve(self.theta)
        self.gW_enc, self.gW_dec, self.gb_enc, self.gb_dec = carve(self.g_theta)
        Vp = np.zeros((nu, ld), np.float32); Vp[:, :nh] = V
        self.V = DeviceBuffer.from_numpy(Vp)
        self.gV = DeviceBuffer.zeros((nu, ld), np.float32)
        self.opt = Adam(self.theta, lr)
        self.optV = Adam(self.V, lr)
        self.d_loss = DeviceBuffer.zeros(1, np.float64)
        self._B = 0
        self._stage = None
        self._slots = 0

    # ---- buffers sized by the batch ---------------------------------------------------------------------------------------
    def _reserve(self, B: int, n_live: int):
        if B > self._B:
            self.h = DeviceBuffer.zeros((B, self.ld), np.float32); self.dz = DeviceBuffer.zeros((B, self.ld), np.float32)
            self.ws = DeviceBuffer(capi.cdae_workspace_bytes(B, self.ld), np.uint8)
            self._B = B
        if n_live > self._slots:
            self.g = DeviceBuffer.zeros(max(n_live, 1) * 5 // 4 + 64, np.float32)
            self._slots = self.g.shape[0]

    def to_device(self, L: BatchLists, stream=None) -> BatchLists:
        """one upload of all thirteen arrays into a staging buffer kept across steps (the copy is ordered on ``stream`` behind
        the kernels of the previous step that read it)"""
        if L.on_device:
            return L
        L.validate()
        parts = [np.ascontiguousarray(getattr(L, k), np.int32) for k in L.INT] + \
                [np.ascontiguousarray(getattr(L, k), np.float32).view(np.int32) for k in L.FLOAT]
        packed = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        if self._stage is None or self._stage.shape[0] < packed.size:
            self._stage = DeviceBuffer(max(packed.size, 1) * 5 // 4 + 1024, np.int32)
        self._stage.upload_head(packed, stream)
        views, off = {}, 0
        for k, p in zip(L.NAMES, parts):
            views[k] = DeviceSlice(self._stage, off, (p.size,), np.float32 if k in L.FLOAT else None); off += p.size
        return BatchLists(L.B, L.n_items, **views)

    # ---- the step -----------------------------------------------------------------------------------------------------------
    def _encode(self, L: BatchLists, stream):
        capi.cdae_encode(self.W_enc, self.b_enc, self.V, self.ni, self.nu, self.nh, self.ld, L.users, L.B, L.in_ptr, L.in_item, L.in_val,
                         self.h, stream)

    def forward_backward(self, lists: BatchLists, stream=None):
        """gradients and loss of one batch at the current variables (no update)"""
        if lists.n_items != self.ni:
            raise ValueError("CdaeTrainer: the lists are over another item count")
        self._reserve(lists.B, lists.n_live)
        L = self.to_device(lists, stream)
        B, ni, nh, ld = L.B, self.ni, self.nh, self.ld
        self._encode(L, stream)
        capi.cdae_decode(self.W_dec, self.b_dec, ni, nh, ld, self.h, B, L.lv_ptr, L.lv_item, L.lv_label, self.g, self.ws, stream)
        capi.cdae_hidden_bwd(self.h, self.V, self.nu, nh, ld, L.users, B, self.reg, self.ws, self.dz, self.gb_enc, self.gV, stream)
        capi.cdae_weight_grads(self.h, self.dz, self.g, ni, nh, ld, B, L.n_live, L.lv_cptr, L.lv_crow, L.lv_cslot, L.in_cptr, L.in_crow,
                               L.in_cval, self.gW_dec, self.gb_dec, self.gW_enc, stream)
        capi.cdae_loss(self.theta, self.n_theta, self.reg, B, ni, ld, self.ws, self.d_loss, stream)
        return L

    def train_step_async(self, lists: BatchLists, stream=None):
        self.forward_backward(lists, stream)
        self.opt.step(self.g_theta, stream=stream, grad_l2=self.reg)
        self.optV.step(self.gV, stream=stream)

    def loss(self, stream=None) -> float:
        """the loss the reference prints for the last step (CDAE.py:82), at the variables the step started from"""
        return float(self.d_loss.numpy(stream)[0])

    # ---- read-back ----------------------------------------------------------------------------------------------------------
    def _unpack(self, flat, Vp):
        ni, nh, ld = self.ni, self.nh, self.ld
        out = dict(W_enc=flat[:ni * ld].reshape(ni, ld)[:, :nh].copy(), W_dec=flat[ni * ld:2 * ni * ld].reshape(ni, ld)[:, :nh].T.copy(),
                   b_enc=flat[2 * ni * ld:2 * ni * ld + nh].copy(), b_dec=flat[2 * ni * ld + ld:2 * ni * ld + ld + ni].copy(), V=Vp[:, :nh].copy())
        return out

    def parameters(self) -> dict:
        """the five variables in the reference's shapes"""
        return self._unpack(self.theta.numpy(), self.V.numpy())

    def raw_gradients(self) -> dict:
        """the kernels' gradients of the last batch, without the reg * theta term of the four weight variables (V's is in)"""
        return self._unpack(self.g_theta.numpy(), self.gV.numpy())

    def padding_is_zero(self) -> bool:
        ni, nh, ld = self.ni, self.nh, self.ld
        t, gt = self.theta.numpy(), self.g_theta.numpy()
        tabs = [a[:2 * ni * ld].reshape(2 * ni, ld)[:, nh:] for a in (t, gt)] + [a[2 * ni * ld:2 * ni * ld + ld][nh:] for a in (t, gt)] + [a[2 * ni * ld + ld + ni:] for a in (t, gt)]
        tabs += [self.V.numpy()[:, nh:], self.gV.numpy()[:, nh:], self.h.numpy()[:, nh:], self.dz.numpy()[:, nh:]]
        return not any(x.any() for x in tabs)

    def hidden(self, users, rated_indptr, rated_items, rated_vals, stream=None) -> DeviceBuffer:
        """the encoder with an all-ones mask over the users' whole rated rows -- the inference graph of predictForRanking
        (CDAE.py:100-105).  Returns the device rows [len(users)][ld]."""
        users = np.ascontiguousarray(users, np.int32)
        rows, items, vals = rated_rows(users, rated_indptr, rated_items, rated_vals)
        order = np.argsort(rows.astype(np.int64) * self.ni + items, kind="stable")
        ptr = np.zeros(users.size + 1, np.int32); np.cumsum(np.bincount(rows, minlength=users.size), out=ptr[1:])
        if items.size and (items.min() < 0 or items.max() >= self.ni):
            raise ValueError("hidden: item id out of range")
        if users.size and (users.min() < 0 or users.max() >= self.nu):
            raise ValueError("hidden: user id out of range")
        out = DeviceBuffer.zeros((max(users.size, 1), self.ld), np.float32)
        d = lambda a, t: DeviceBuffer.from_numpy(np.ascontiguousarray(a, t) if a.size else np.zeros(1, t))
        capi.cdae_encode(self.W_enc, self.b_enc, self.V, self.ni, self.nu, self.nh, self.ld, d(users, np.int32), users.size, d(ptr, np.int32),
                         d(items[order], np.int32), d(vals[order], np.float32), out, stream)
        return out


# ---- CFGAN (model/ranking/CFGAN.py; csrc/cfgan.hip) ---------------------------------------------------------------------------------
def cfgan_lists(users, n_items: int, pos_rows, pos_items, pos_vals, mask_rows, mask_items, zr_rows, zr_items) -> BatchLists:
    """CFGAN's batch in CDAE's list form with everything kept: ``pos_*`` the rated entries of every batch row (the "in" lists, C[n,i]),
    ``mask_*`` the sampled negatives of ``mask`` (with the rated items they make the "live" lists), ``zr_*`` the sampled negatives of
    ``N_zr``.  ``lv_label`` of the result is the per-live-slot FLAG of N_zr and mask: the zero-reconstruction term lives only where
    the two independent draws coincide (CFGAN.py:107)."""
    L = lists_from_entries(users, n_items, pos_rows, pos_items, pos_vals, mask_rows, mask_items, lambda r, i: np.ones(len(r), bool))
    zr = np.unique(np.asarray(zr_rows, np.int64) * n_items + np.asarray(zr_items, np.int64))
    lv_row = np.repeat(np.arange(L.B, dtype=np.int64), np.diff(L.lv_ptr))
    L.lv_label = np.ascontiguousarray(np.isin(lv_row * n_items + L.lv_item, zr), np.int32)
    return L


def cfgan_lists_from_dense(users, C, mask, N_zr) -> BatchLists:
    """the reference's three dense feeds of one epoch (CFGAN.py:123) in list form"""
    C = np.asarray(C); mask = np.asarray(mask) != 0
    if (~mask & (C != 0)).any():
        raise ValueError("cfgan_lists_from_dense: the mask must hold every rated item")
    pr, pi = np.nonzero(C)
    mr, mi = np.nonzero(mask & (C == 0))
    zr, zi = np.nonzero(np.asarray(N_zr) != 0)
    return cfgan_lists(users, C.shape[1], pr, pi, C[pr, pi], mr, mi, zr, zi)


class CfganTrainer:
    """CFGAN.py:46-127 on the device.  Variables as the reference shapes them: G_W1 [n_items, n_items], G_b1 [n_items], D_W1
    [2 n_items, 1], D_b1 [1]; on the device G_W1 has row stride ld (n_items rounded up to 32, padding zero) and the discriminator's
    2 n_items + 1 values lie in one array.  One epoch is a discriminator step and three generator steps on one batch, each with the
    forward pass at the current variables; the two Adam optimizers keep separate beta powers.  The generator's step is one sweep over
    G_W1 and its two Adam slots (qrec_cfgan_gen_sweep): no [n_items, n_items] gradient exists unless ``keep_gradients`` asks for it.
    No kernel here uses a float atomic: ``ordered_reductions`` has nothing to switch."""

    def __init__(self, G_W1, G_b1, D_W1, D_b1, lr: float, alpha: float = 0.01, keep_gradients: bool = False):
        G_W1 = np.asarray(G_W1, np.float32)
        self.ni = ni = G_W1.shape[0]
        D_W1 = np.asarray(D_W1, np.float32).reshape(-1); D_b1 = np.asarray(D_b1, np.float32).reshape(-1)
        if G_W1.shape != (ni, ni) or np.shape(G_b1) != (ni,) or D_W1.size != 2 * ni or D_b1.size != 1:
            raise ValueError("CfganTrainer: G_W1 [n_items, n_items], G_b1 [n_items], D_W1 [2 n_items, 1], D_b1 [1]")
        if ni > capi.CFGAN_MAX_ITEMS:
            raise ValueError(f"CFGAN on the device supports up to {capi.CFGAN_MAX_ITEMS} items")
        self.ld = ld = -(-ni // 32) * 32
        self.n_d = -(-(2 * ni + 1) // 4) * 4
        self.lr, self.alpha = float(lr), float(alpha)
        W = np.zeros((ni, ld), np.float32); W[:, :ni] = G_W1
        b = np.zeros(ld, np.float32); b[:ni] = G_b1
        tD = np.zeros(self.n_d, np.float32); tD[:2 * ni] = D_W1; tD[2 * ni] = D_b1[0]
        self.W, self.b, self.thetaD = DeviceBuffer.from_numpy(W), DeviceBuffer.from_numpy(b), DeviceBuffer.from_numpy(tD)
        z = lambda a: DeviceBuffer.zeros(a.shape, np.float32)
        self.mW, self.vW, self.mb, self.vb, self.mD, self.vD = z(W), z(W), z(b), z(b), z(tD), z(tD)
        self.gW, self.gb, self.gD = (z(W), z(b), z(tD)) if keep_gradients else (None, None, None)
        self.optD, self.optG = AdamClock(lr), AdamClock(lr)      # the updates themselves run inside the step kernels
        self.losses = DeviceBuffer.zeros(8, np.float64)     # (D_loss, G_loss) of the forward pass of the D step and of the three G steps
        self._loss_at = [DeviceSlice(self.losses, 2 * k, (2,)) for k in range(4)]
        self._g_steps = 0
        self._B = self._slots = 0
        self._stage = None
        self.ws = None

    to_device = CdaeTrainer.to_device

    def _reserve(self, B: int, n_live: int):
        if B > self._B or n_live > self._slots:
            self._B, self._slots = max(B, self._B), max(max(n_live, 1) * 5 // 4 + 64, self._slots)
            self.ws = DeviceBuffer(capi.cfgan_workspace_bytes(self._B, self._slots), np.uint8)

    def _prepare(self, lists: BatchLists, stream) -> BatchLists:
        if lists.n_items != self.ni:
            raise ValueError("CfganTrainer: the lists are over another item count")
        if lists.B < 1:
            raise ValueError("CfganTrainer: an empty batch")
        self._reserve(lists.B, lists.n_live)
        return self.to_device(lists, stream)

    def forward(self, lists: BatchLists, stream=None, slot: int = 0) -> BatchLists:
        """r_hat and delta at the live slots, the row quantities and both losses at the current variables (no update)"""
        L = self._prepare(lists, stream)
        capi.cfgan_forward(self.W, self.b, self.thetaD, self.ni, self.ld, L, self.alpha, self.ws, self._loss_at[slot], stream)
        return L

    def dis_step_async(self, lists: BatchLists, stream=None) -> BatchLists:
        L = self.forward(lists, stream, 0)
        o = self.optD
        alpha = o.alpha(); o.advance()
        capi.cfgan_dis_step(self.thetaD, self.mD, self.vD, self.ni, L, self.ws, alpha, float(o.b1), float(o.b2), float(o.eps), self.gD, stream)
        self._g_steps = 0
        return L

    def gen_step_async(self, lists: BatchLists, stream=None) -> BatchLists:
        L = self.forward(lists, stream, 1 + self._g_steps % 3)
        o = self.optG
        alpha = o.alpha(); o.advance()
        capi.cfgan_gen_sweep(self.W, self.mW, self.vW, self.b, self.mb, self.vb, self.ni, self.ld, L, self.ws, alpha,
                             float(o.b1), float(o.b2), float(o.eps), self.gW, self.gb, stream)
        self._g_steps += 1
        return L

    def train_epoch_async(self, lists: BatchLists, stream=None):
        """CFGAN.py:120-125: D, G, G, G on one batch (uploaded once)"""
        L = self.dis_step_async(lists, stream)
        for _ in range(3):
            self.gen_step_async(L, stream)

    def d_loss(self, stream=None) -> float:
        """D_loss of the epoch's discriminator step, at the variables the step started from (what the reference prints)"""
        return float(self.losses.numpy(stream)[0])

    def g_losses(self, stream=None) -> np.ndarray:
        """G_loss of the generator steps since the last discriminator step (three after an epoch)"""
        return self.losses.numpy(stream)[3:3 + 2 * min(self._g_steps, 3):2].copy()

    def g_loss(self, stream=None) -> float:
        """G_loss of the last generator step (what the reference prints)"""
        return float(self.g_losses(stream)[-1])

    def slots(self, L: BatchLists) -> dict:
        """r_hat, delta per live slot and a_r, a_f per batch row of the last forward pass"""
        n, B = L.n_live, L.B
        out = dict(r=DeviceBuffer.zeros(max(n, 1), np.float32), delta=DeviceBuffer.zeros(max(n, 1), np.float32),
                   a_r=DeviceBuffer.zeros(B, np.float32), a_f=DeviceBuffer.zeros(B, np.float32))
        capi.cfgan_read_slots(self.ws, B, n, out["r"], out["delta"], out["a_r"], out["a_f"])
        return {k: v.numpy()[:n if k in ("r", "delta") else B] for k, v in out.items()}

    # ---- read-back ----------------------------------------------------------------------------------------------------------
    def parameters(self) -> dict:
        """the four variables in the reference's shapes"""
        ni = self.ni
        tD = self.thetaD.numpy()
        return dict(G_W1=self.W.numpy()[:, :ni].copy(), G_b1=self.b.numpy()[:ni].copy(), D_W1=tD[:2 * ni].reshape(2 * ni, 1).copy(),
                    D_b1=tD[2 * ni:2 * ni + 1].copy())

    def raw_gradients(self, which: str) -> dict:
        """``"D"``: the gradients the last discriminator step applied; ``"G"``: those of the last generator step"""
        if self.gW is None:
            raise RuntimeError("CfganTrainer: built without keep_gradients")
        ni = self.ni
        if which == "D":
            g = self.gD.numpy()
            return dict(D_W1=g[:2 * ni].reshape(2 * ni, 1).copy(), D_b1=g[2 * ni:2 * ni + 1].copy())
        if which == "G":
            return dict(G_W1=self.gW.numpy()[:, :ni].copy(), G_b1=self.gb.numpy()[:ni].copy())
        raise ValueError("raw_gradients: 'D' or 'G'")

    def padding_is_zero(self) -> bool:
        ni = self.ni
        tabs = [a.numpy()[:, ni:] for a in (self.W, self.mW, self.vW)] + [a.numpy()[ni:] for a in (self.b, self.mb, self.vb)]
        tabs += [a.numpy()[2 * ni + 1:] for a in (self.thetaD, self.mD, self.vD)]
        if self.gW is not None:
            tabs += [self.gW.numpy()[:, ni:], self.gb.numpy()[ni:]]
        return not any(x.any() for x in tabs)
