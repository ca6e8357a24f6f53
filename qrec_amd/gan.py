"""IRGAN on the device (model/ranking/IRGAN.py): two towers P[u] . Q[i] + b[i] (generator, discriminator), the per-user categorical
distributions over the whole item table with their draws, the policy-gradient step and the discriminator's batch step -- the
kernels of csrc/irgan.hip plus the existing ordered scatter and Adam.

An item table is kept as [Q | b] (the bias in column d of the row, see include/qrec_hip.h), so the row stride is that of d + 1
columns: d = 64 pays a stride of 128.  Nothing here reads the device back between steps; ``loss``, ``parameters`` and
``raw_gradients`` do, on request."""
from __future__ import annotations

import numpy as np

from . import capi
from .capi import DeviceBuffer, DeviceSlice
from .engine import padded_ld
from .optim import AdamClock

TEMPERATURE = 0.2          # IRGAN.py:88
SAMPLE_LAMBDA = 0.2        # IRGAN.py:143
NEG_PER_POS, GEN_PER_POS = 2, 3
ROW_SCRATCH_BYTES = 256 << 20      # get_data's block of users is sized so that its three [B][n_items] float rows stay below this


class _Tower:
    def __init__(self, P, Q, b, d: int, ld: int):
        nu, ni = P.shape[0], Q.shape[0]
        Pp = np.zeros((nu, ld), np.float32); Pp[:, :d] = P
        Qp = np.zeros((ni, ld), np.float32); Qp[:, :d] = Q; Qp[:, d] = b
        self.P, self.Q = DeviceBuffer.from_numpy(Pp), DeviceBuffer.from_numpy(Qp)
        self.mP, self.vP, self.gP = (DeviceBuffer.zeros((nu, ld), np.float32) for _ in range(3))
        self.mQ, self.vQ = (DeviceBuffer.zeros((ni, ld), np.float32) for _ in range(2))


class IrganTrainer:
    """``init``: the six variables g_P, g_Q, g_b, d_P, d_Q, d_b in the reference's shapes; ``pos_indptr`` / ``pos_items``: every
    user's rated items as a CSR over all users, item ids ascending inside a row.  ``keep_raw_gradients`` keeps the generator's
    [n_items][ld] gradient of the last step for ``raw_gradients`` (tests); a training run does not materialise it."""

    def __init__(self, init: dict, pos_indptr, pos_items, lr: float, reg: float, seed: int = 0, keep_raw_gradients: bool = False):
        a = {k: np.asarray(init[k], np.float32) for k in ("g_P", "g_Q", "g_b", "d_P", "d_Q", "d_b")}
        self.nu, self.d = a["g_P"].shape
        self.ni = a["g_Q"].shape[0]
        for t in "gd":
            if a[t + "_P"].shape != (self.nu, self.d) or a[t + "_Q"].shape != (self.ni, self.d) or a[t + "_b"].shape != (self.ni,):
                raise ValueError("IrganTrainer: P [n_users, d], Q [n_items, d], b [n_items] for both towers")
        if self.d + 1 > capi.IRGAN_MAX_LD:
            raise ValueError(f"IRGAN on the device supports embedding sizes up to {capi.IRGAN_MAX_LD - 1}")
        self.ld = padded_ld(self.d + 1, np.float32)
        indptr = np.ascontiguousarray(pos_indptr, np.int64); items = np.ascontiguousarray(pos_items, np.int32)
        if indptr.size != self.nu + 1 or indptr[0] != 0 or indptr[-1] != items.size or (np.diff(indptr) < 0).any():
            raise ValueError("IrganTrainer: bad positives CSR")
        if items.size and (items.min() < 0 or items.max() >= self.ni):
            raise ValueError("IrganTrainer: item id out of range")
        inner = np.ones(items.size, bool); inner[indptr[:-1][np.diff(indptr) > 0]] = False
        if (np.diff(items, prepend=-1)[inner] <= 0).any():
            raise ValueError("IrganTrainer: the positives of a user must be ascending")
        self.n_pos = np.diff(indptr)
        if (self.n_pos >= self.ni).any():
            raise ValueError("IRGAN: a user who rated every item has no negative to draw (the reference divides 0 by 0)")
        self.lr, self.reg, self.seed = float(lr), float(reg), int(seed)
        self.gen, self.dis = _Tower(a["g_P"], a["g_Q"], a["g_b"], self.d, self.ld), _Tower(a["d_P"], a["d_Q"], a["d_b"], self.d, self.ld)
        self.dis.gQ = DeviceBuffer.zeros((self.ni, self.ld), np.float32)
        self.gen_opt, self.dis_opt = AdamClock(lr), AdamClock(lr)
        self.d_pos = (DeviceBuffer.from_numpy(indptr), DeviceBuffer.from_numpy(items if items.size else np.zeros(1, np.int32)))
        self.d_user_ids = DeviceBuffer.from_numpy(np.arange(self.nu, dtype=np.int32))
        gen_ptr = np.zeros((self.nu, 2), np.int64); gen_ptr[:, 1] = GEN_PER_POS * self.n_pos
        self.d_gen_ptr = DeviceBuffer.from_numpy(gen_ptr)
        self.n_chunks = -(-self.ni // capi.IRGAN_CHUNK)
        self._rows = 0
        self._reserve_rows(1)
        k_max = max(1, GEN_PER_POS * int(self.n_pos.max()) if self.nu else 1)
        self.gen_ws = DeviceBuffer(capi.irgan_gen_workspace_bytes(self.ni, self.ld, k_max), np.uint8)
        self.d_samples = DeviceBuffer.zeros(k_max, np.int32)
        self.d_reward = DeviceBuffer.zeros(k_max, np.float32)
        self.d_uniforms = DeviceBuffer.zeros(k_max, np.float64)
        self.d_g = DeviceBuffer.zeros(self.ni, np.float32) if keep_raw_gradients else None
        self.d_gQ_raw = DeviceBuffer.zeros((self.ni, self.ld), np.float32) if keep_raw_gradients else None
        self.d_loss_g, self.d_loss_d = DeviceBuffer.zeros(1, np.float64), DeviceBuffer.zeros(1, np.float64)
        self.ordered = capi.OrderedScatter()
        self._dirty_row = None
        self._last = None
        self._last_K = 0
        self._slots = 0
        self.gen_steps = 0

    # ---- the per-user distributions ---------------------------------------------------------------------------------------------
    def _reserve_rows(self, B: int):
        if B > self._rows:
            capi.device_sync()
            self.z, self.w, self.p = (DeviceBuffer.zeros((B, self.ni), np.float32) for _ in range(3))
            self.csum = DeviceBuffer.zeros((B, self.n_chunks), np.float64)
            self.row_ws = DeviceBuffer(max(capi.irgan_row_workspace_bytes(B, self.ni), 4), np.uint8)
            self._rows = B

    def rows_per_block(self) -> int:
        return int(max(1, min(65535, ROW_SCRATCH_BYTES // (12 * self.ni))))

    def row_weights(self, tower: _Tower, d_users, B: int, mode: int, stream=None):
        """weights, p and the chunk prefix sums of the B users ``d_users`` (device int32) into self.w / self.p / self.csum"""
        self._reserve_rows(B)
        T, lam = (TEMPERATURE, 0.0) if mode == capi.IRGAN_NEGATIVES else (1.0, SAMPLE_LAMBDA)
        capi.irgan_row_weights(tower.P, tower.Q, self.nu, self.ni, self.d, self.ld, d_users, B, self.d_pos[0], self.d_pos[1], mode, T, lam,
                               self.z, self.w, self.p, self.csum, self.row_ws, stream)

    def _check_users(self, users):
        users = np.ascontiguousarray(users, np.int32)
        if users.size == 0 or users.min() < 0 or users.max() >= self.nu:
            raise ValueError("IrganTrainer: user id out of range")
        return users

    def draw_negatives(self, users, uniforms=None, step: int = 0, assemble: bool = False, stream=None):
        """get_data for ``users`` (IRGAN.py:81-101), in blocks of users sized to the scratch budget: 2 |pos| draws per user from the
        GENERATOR's tempered softmax with the positives removed.  ``uniforms``: one float64 per draw, in user order (the reference's
        np.random.random_sample inside np.random.choice); None draws them on the device (Philox of seed, step, row, index).
        Returns (draw_ptr int64 [len(users) + 1], d_samples device int32); with ``assemble`` also the rows on the device,
        (d_u, d_i, d_label, n_rows): per user the positives (ascending) with label 1, then the draws with label 0."""
        users = self._check_users(users)
        K = NEG_PER_POS * self.n_pos[users]
        ptr = np.zeros(users.size + 1, np.int64); np.cumsum(K, out=ptr[1:])
        total = int(ptr[-1])
        if uniforms is not None:
            uniforms = np.ascontiguousarray(uniforms, np.float64)
            if uniforms.size != total:
                raise ValueError(f"draw_negatives: {total} uniforms needed, {uniforms.size} given")
            d_x = DeviceBuffer.from_numpy(np.concatenate([uniforms, [0.0]]))      # one spare entry: an empty block's window stays inside
        d_samples = DeviceBuffer.zeros(total + 1, np.int32)
        d_users = DeviceBuffer.from_numpy(users)
        d_ptr = DeviceBuffer.from_numpy(ptr)
        rows = None
        if assemble:
            row_ptr = ptr + np.concatenate([[0], np.cumsum(self.n_pos[users])])
            n_rows = int(row_ptr[-1])
            d_row_ptr = DeviceBuffer.from_numpy(row_ptr)
            rows = (DeviceBuffer.zeros(n_rows + 1, np.int32), DeviceBuffer.zeros(n_rows + 1, np.int32), DeviceBuffer.zeros(n_rows + 1, np.float32), n_rows)
        per = self.rows_per_block()
        for b0 in range(0, users.size, per):
            B = min(per, users.size - b0)
            n = int(ptr[b0 + B] - ptr[b0])
            self.row_weights(self.gen, DeviceSlice(d_users, b0, (B,)), B, capi.IRGAN_NEGATIVES, stream)
            # the block's draw pointer is the global one from b0 on: the kernels take differences and offsets from its first entry
            blk_ptr = DeviceBuffer.from_numpy(ptr[b0:b0 + B + 1] - ptr[b0])
            out = DeviceSlice(d_samples, int(ptr[b0]), (max(n, 1),))
            capi.irgan_draw(self.w, self.csum, self.ni, B, blk_ptr, n, DeviceSlice(d_x, int(ptr[b0]), (max(n, 1),)) if uniforms is not None else None,
                            self.seed, (int(step) << 20) + b0, out, stream)
            if assemble:
                blk_rows = DeviceBuffer.from_numpy(row_ptr[b0:b0 + B + 1] - row_ptr[b0])
                r0, nr = int(row_ptr[b0]), int(row_ptr[b0 + B] - row_ptr[b0])
                capi.irgan_assemble_rows(DeviceSlice(d_users, b0, (B,)), self.nu, B, self.d_pos[0], self.d_pos[1], blk_ptr, out, blk_rows, nr,
                                         DeviceSlice(rows[0], r0, (max(nr, 1),)), DeviceSlice(rows[1], r0, (max(nr, 1),)),
                                         DeviceSlice(rows[2], r0, (max(nr, 1),)), stream)
            capi.device_sync()            # the block's small pointer buffers are released when this iteration ends
        return (ptr, d_samples) + ((rows,) if assemble else ())

    # ---- the discriminator's batch step -------------------------------------------------------------------------------------------
    def discriminator_step(self, u, i, label, apply: bool = True, stream=None):
        """one run of d_updates (IRGAN.py:134-136) on the batch (u, i, label): numpy arrays, or device int32 / int32 / float32"""
        if isinstance(u, DeviceBuffer):
            B, d_u, d_i, d_y = int(u.shape[0]), u, i, label
        else:
            u = np.ascontiguousarray(u, np.int32); B = u.size
            d_u, d_i = DeviceBuffer.from_numpy(u), DeviceBuffer.from_numpy(np.ascontiguousarray(i, np.int32))
            d_y = DeviceBuffer.from_numpy(np.ascontiguousarray(label, np.float32))
        if B < 1:
            raise ValueError("discriminator_step: empty batch")
        if B > self._slots:
            capi.device_sync()
            self.slotP, self.slotQ = DeviceBuffer.zeros((B, self.ld), np.float32), DeviceBuffer.zeros((B, self.ld), np.float32)
            self.keyP, self.keyQ = DeviceBuffer.zeros(B, np.int32), DeviceBuffer.zeros(B, np.int32)
            self.dz, self.terms = DeviceBuffer.zeros(B, np.float32), DeviceBuffer.zeros(B, np.float64)
            self._slots = B
        t = self.dis
        capi.irgan_dis_slots(t.P, t.Q, self.nu, self.ni, self.d, self.ld, d_u, d_i, d_y, B, self.reg, self.slotP, self.slotQ, self.keyP, self.keyQ,
                             self.dz, self.terms, self.d_loss_d, stream)
        t.gP.fill_bytes(0, stream); t.gQ.fill_bytes(0, stream)
        capi.scatter_add_rows_ordered(self.slotP, self.keyP, B, self.ld, t.gP, self.ordered, stream=stream)
        capi.scatter_add_rows_ordered(self.slotQ, self.keyQ, B, self.ld, t.gQ, self.ordered, stream=stream)
        if apply:
            o = self.dis_opt
            for theta, m, v, g in ((t.P, t.mP, t.vP, t.gP), (t.Q, t.mQ, t.vQ, t.gQ)):
                capi.adam_step(theta, m, v, g, int(np.prod(theta.shape)), 1.0, o.alpha(), float(o.b1), float(o.b2), float(o.eps), stream)
            o.advance()
        self._last, self._last_B = "dis", B
        if not isinstance(u, DeviceBuffer):
            capi.device_sync()            # the uploaded batch is released on return

    # ---- the generator's step for one user ------------------------------------------------------------------------------------------
    def generator_step(self, user: int, uniforms=None, samples=None, apply: bool = True, d_samples=None, stream=None):
        """IRGAN.py:143-168 for one user, asynchronous: the sampling distribution, K = 3 |pos| draws, their rewards from the
        discriminator, the policy gradient and Adam on the generator's three variables.  The draws use ``uniforms`` (float64 [K] on the host or the
        device: the reference's stream), or are ``samples`` (injected), or Philox uniforms of (seed, step count, index).  ``d_samples``: a device
        int32 window of K entries that receives the samples (the caller's log) instead of the trainer's own buffer."""
        user = int(user)
        if not 0 <= user < self.nu:
            raise ValueError("generator_step: user id out of range")
        K = GEN_PER_POS * int(self.n_pos[user])
        if K < 1:
            raise ValueError("generator_step: the user has no rated item")
        g = self.gen
        if self._dirty_row is not None:                  # the gradient buffer of the user table is zero except the last step's row
            capi.memset(DeviceSlice(g.gP, self._dirty_row * self.ld, (self.ld,)), 0, self.ld * 4, stream)
        d_user = DeviceSlice(self.d_user_ids, user, (1,))
        d_ptr = DeviceSlice(self.d_gen_ptr, 2 * user, (2,))
        self.row_weights(g, d_user, 1, capi.IRGAN_MIXTURE, stream)
        d_s = self.d_samples if d_samples is None else d_samples
        if samples is not None:
            samples = np.ascontiguousarray(samples, np.int32)
            if samples.size != K or samples.min() < 0 or samples.max() >= self.ni:
                raise ValueError(f"generator_step: {K} samples inside the item table needed")
            d_s.upload_head(samples, stream)
        else:
            d_x = None
            if isinstance(uniforms, DeviceBuffer):           # a window of a pass's uniforms, uploaded once by the caller
                if uniforms.dtype != np.float64 or int(np.prod(uniforms.shape)) != K:
                    raise ValueError(f"generator_step: {K} float64 uniforms needed")
                d_x = uniforms
            elif uniforms is not None:
                uniforms = np.ascontiguousarray(uniforms, np.float64)
                if uniforms.size != K:
                    raise ValueError(f"generator_step: {K} uniforms needed, {uniforms.size} given")
                self.d_uniforms.upload_head(uniforms, stream); d_x = self.d_uniforms
            capi.irgan_draw(self.w, self.csum, self.ni, 1, d_ptr, K, d_x, self.seed ^ 0x67656E, self.gen_steps, d_s, stream)
        capi.irgan_reward(self.dis.P, self.dis.Q, self.nu, self.ni, self.d, self.ld, d_user, 1, d_ptr, K, d_s, self.p, self.w, self.d_reward, stream)
        o = self.gen_opt
        capi.irgan_gen_step(g.P, g.Q, g.mQ, g.vQ, self.nu, self.ni, self.d, self.ld, user, d_s, self.d_reward, K, self.p, self.reg, apply,
                            o.alpha(), float(o.b1), float(o.b2), float(o.eps), g.gP, self.d_g, self.d_gQ_raw, self.d_loss_g, self.gen_ws, stream)
        if apply:
            capi.adam_step(g.P, g.mP, g.vP, g.gP, self.nu * self.ld, 1.0, o.alpha(), float(o.b1), float(o.b2), float(o.eps), stream)
            o.advance()
        self._dirty_row, self._last, self._last_K = user, "gen", K
        self.gen_steps += 1

    def step_uniforms(self, user: int) -> np.ndarray:
        """the Philox uniforms the NEXT generator_step(user) without uniforms or samples would draw with"""
        K = GEN_PER_POS * int(self.n_pos[user])
        out = DeviceBuffer.zeros(K, np.float64)
        capi.irgan_uniforms(1, DeviceSlice(self.d_gen_ptr, 2 * user, (2,)), K, self.seed ^ 0x67656E, self.gen_steps, out)
        return out.numpy()

    # ---- read-back ------------------------------------------------------------------------------------------------------------------
    def loss(self, stream=None) -> float:
        """the loss of the last step at the variables it started from: the generator's gan_loss, or the SUM of the discriminator's
        loss vector (what its minimize differentiates)"""
        return float((self.d_loss_g if self._last == "gen" else self.d_loss_d).numpy(stream)[0])

    def _tower_np(self, P, Q):
        d = self.d
        return P[:, :d].copy(), Q[:, :d].copy(), Q[:, d].copy()

    def parameters(self) -> dict:
        out = {}
        for name, t in (("g", self.gen), ("d", self.dis)):
            out[name + "_P"], out[name + "_Q"], out[name + "_b"] = self._tower_np(t.P.numpy(), t.Q.numpy())
        return out

    def last_samples(self) -> np.ndarray:
        return self.d_samples.numpy()[:self._last_K]

    def last_rewards(self) -> np.ndarray:
        return self.d_reward.numpy()[:self._last_K]

    def raw_gradients(self) -> dict:
        """the gradients the last step handed to Adam, in the reference's shapes (generator steps: needs ``keep_raw_gradients``;
        also ``g``, the policy gradient with respect to the logits)"""
        if self._last == "dis":
            P, Q, b = self._tower_np(self.dis.gP.numpy(), self.dis.gQ.numpy())
            return dict(d_P=P, d_Q=Q, d_b=b, dz=self.dz.numpy()[:self._last_B])
        if self.d_gQ_raw is None:
            raise RuntimeError("raw_gradients: construct the trainer with keep_raw_gradients=True")
        P, Q, b = self._tower_np(self.gen.gP.numpy(), self.d_gQ_raw.numpy())
        return dict(g_P=P, g_Q=Q, g_b=b, g=self.d_g.numpy())

    def padding_is_zero(self) -> bool:
        d = self.d
        tabs = []
        for t in (self.gen, self.dis):
            tabs += [x.numpy()[:, d:] for x in (t.P, t.mP, t.vP, t.gP)] + [x.numpy()[:, d + 1:] for x in (t.Q, t.mQ, t.vQ)]
        tabs.append(self.dis.gQ.numpy()[:, d + 1:])
        if self.d_gQ_raw is not None:
            tabs.append(self.d_gQ_raw.numpy()[:, d + 1:])
        return not any(x.any() for x in tabs)
