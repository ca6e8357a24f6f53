"""IRGAN behind the reference's class name and hooks (model/ranking/IRGAN.py:77-182): a generator and a discriminator, both
P[u] . Q[i] + b[i]; per epoch ``get_data`` draws 2 |pos| negatives per user from the generator's tempered softmax, the discriminator
takes one pass over the first ``train_size`` of those rows, and the generator takes five passes over the users, one policy-gradient
Adam step per user on 3 |pos| draws rewarded by the discriminator.  Items are scored with the discriminator.

Exact mode (the default) consumes ``np.random.random_sample(K)`` exactly where the reference calls ``np.random.choice(.., K, p=..)``
(choice draws its uniforms that way), so the global stream ends where the reference leaves it; the draws of every call are kept in
``self.draws``.  The chain of draws need not be the reference's: a uniform within rounding of a CDF boundary may select the
neighbouring item.  QREC_MODE=throughput draws the uniforms on the device instead (Philox, QREC_SEED), runs ``get_data`` for blocks
of users at once and assembles its rows there: the reference's distribution, not its stream, and ``np.random`` is not consumed."""
from __future__ import annotations

import os

import numpy as np

from ...base.deepRecommender import DeepRecommender
from ...capi import DeviceBuffer, DeviceSlice
from ...gan import GEN_PER_POS, NEG_PER_POS, IrganTrainer

GEN_PASSES = 5          # IRGAN.py:141


def _uniform(shape) -> np.ndarray:
    """tf.random_uniform(shape, -0.05, 0.05) (IRGAN.py:18-21), from numpy's global generator"""
    return np.random.uniform(-0.05, 0.05, shape).astype(np.float32)


class IRGAN(DeepRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def initModel(self):
        super().initModel()                      # the two tables of DeepRecommender.initModel: created first, never trained
        if self.data_parallel() is not None:
            raise RuntimeError("IRGAN runs on one GPU: start it without torch.distributed.run")
        nu, ni, d = self.num_users, self.num_items, self.emb_size
        self.variables = {}
        for t in "gd":                           # creation order of IRGAN.py:109-110
            self.variables[t + "_P"] = _uniform((nu, d)); self.variables[t + "_Q"] = _uniform((ni, d))
            self.variables[t + "_b"] = np.zeros(ni, np.float32)
        # trainSet_u order and the rated items in the reference's order (get_data's rows); the kernels take them ascending
        self.user_order = np.array([self.data.user[u] for u in self.data.trainSet_u if u in self.data.user], np.int32)
        self.pos = {int(self.data.user[u]): [self.data.item[i] for i in self.data.userRated(u)[0]]
                    for u in self.data.trainSet_u if u in self.data.user}
        if any(len(p) >= ni for p in self.pos.values()):
            raise ValueError("IRGAN: a user who rated every item has no negative to draw (the reference divides 0 by 0)")
        self.draws = []                          # exact mode: (user, samples) per np.random.choice call of the reference's loop

    def initial_variables(self) -> dict:
        return self.variables

    def _new_trainer(self):
        rated = self._rated_sorted()
        return self.build_trainer(IrganTrainer, self.variables, rated.indptr.astype(np.int64), rated.indices.astype(np.int32), self.lRate, self.regU,
                                  int(os.environ.get("QREC_SEED", "0")))

    # ---- exact mode: the reference's host stream ----------------------------------------------------------------------------------
    def get_data(self):
        """IRGAN.py:81-101: (users, items, labels) with the draws made on the device from np.random.random_sample's uniforms"""
        tr, order = self.trainer, self.user_order
        counts = [NEG_PER_POS * len(self.pos[int(u)]) for u in order]
        x = np.concatenate([np.random.random_sample(k) for k in counts])       # one call per user, as np.random.choice makes them
        ptr, d_samples = tr.draw_negatives(order, x)
        s = d_samples.numpy()
        us, it, lab = [], [], []
        for k, u in enumerate(order.tolist()):
            neg = s[ptr[k]:ptr[k + 1]]
            self.draws.append((u, neg.copy()))
            p = self.pos[u]
            us += [u] * (len(p) + neg.size); it += p + neg.tolist(); lab += [1.0] * len(p) + [0.0] * neg.size
        return np.array(us, np.int32), np.array(it, np.int32), np.array(lab, np.float32)

    def _generator_pass_exact(self):
        tr, order = self.trainer, self.user_order
        counts = np.array([GEN_PER_POS * len(self.pos[int(u)]) for u in order], np.int64)
        ptr = np.concatenate([[0], np.cumsum(counts)])
        x = np.concatenate([np.random.random_sample(int(k)) for k in counts])
        d_x, d_log = DeviceBuffer.from_numpy(x), DeviceBuffer.zeros(int(ptr[-1]), np.int32)      # one upload and one read-back per pass
        for k, u in enumerate(order.tolist()):
            n = int(counts[k])
            tr.generator_step(u, uniforms=DeviceSlice(d_x, int(ptr[k]), (n,)), d_samples=DeviceSlice(d_log, int(ptr[k]), (n,)))
        s = d_log.numpy()
        self.draws += [(u, s[ptr[k]:ptr[k + 1]].copy()) for k, u in enumerate(order.tolist())]

    def trainModel(self):
        quiet = os.environ.get("QREC_QUIET") == "1"
        tr = self.trainer = self._new_trainer()
        fast = self.throughput_mode()
        for epoch in range(self.maxEpoch):
            if not quiet:
                print("Update discriminator...")
            if fast:
                _, _, (d_u, d_i, d_y, n_rows) = tr.draw_negatives(self.user_order, None, step=epoch, assemble=True)
                take = lambda a, b: (DeviceSlice(d_u, a, (b - a,)), DeviceSlice(d_i, a, (b - a,)), DeviceSlice(d_y, a, (b - a,)))
            else:
                rows = self.get_data()
                take = lambda a, b: tuple(r[a:b] for r in rows)
            # only the first train_size rows are consumed (IRGAN.py:128), in batches of batch_size; the last holds the rest
            for a in range(0, self.train_size, self.batch_size):
                tr.discriminator_step(*take(a, min(a + self.batch_size, self.train_size)))
            if not quiet:
                print("epoch:", epoch + 1, "d_epoch:", 1, "loss=", "{:.6f}".format(tr.loss()))
                print("Update generator...")
            for g_epoch in range(GEN_PASSES):
                if fast:
                    for u in self.user_order.tolist():
                        tr.generator_step(u)
                else:
                    self._generator_pass_exact()
                if not quiet:
                    print("epoch:", epoch + 1, "g_epoch:", g_epoch + 1, "loss=", "{:.6f}".format(tr.loss()))
        self._refresh_scoring_tables()

    # ---- evaluation: the discriminator's P[u] . Q + b = [P | 1] . [Q | b] (IRGAN.py:172-182) ---------------------------------------
    def _refresh_scoring_tables(self):
        p = self.trainer.parameters()
        self.P_d, self.Q_d, self.b_d = p["d_P"], p["d_Q"], p["d_b"]

    def ranking_tables(self):
        return (np.ascontiguousarray(np.concatenate([self.P_d, np.ones((self.num_users, 1), np.float32)], axis=1)),
                np.ascontiguousarray(np.concatenate([self.Q_d, self.b_d[:, None]], axis=1)))

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            return self.Q_d.dot(self.P_d[self.data.getUserId(u)]) + self.b_d
        return [self.data.globalMean] * self.num_items
