"""CFGAN behind the reference's class name and hooks (model/ranking/CFGAN.py:9-136): a one-layer generator over the user's whole
rating row, r_hat = sigmoid(C G_W1 + G_b1) with G_W1 n_items x n_items, a one-layer discriminator over [r_hat * mask | C], Adam on
both; every ``num.max.epoch`` iteration draws one batch and runs one discriminator step and three generator steps on it.
``S_zr``, ``S_pm`` and ``alpha`` are instance attributes, as in the reference, not conf keys.

``next_batch`` consumes ``random`` as the reference's loop does -- per batch row ``choice(userList)``, then int(S_zr n_items)
negatives for N_zr and int(S_pm n_items) for the mask, each ``choice(itemList)`` redrawn while rated -- in plain Python; the lists
the kernels consume are then built on the host.  The variables are Xavier-initialised from numpy's global generator in the
reference's creation order.  There is one execution path, whose sums have a fixed order (two runs are bit-identical): ``QREC_MODE``
does not apply."""
from __future__ import annotations

import os
from random import choice

import numpy as np

from ...autoencoder import CfganTrainer, cfgan_lists, rated_rows
from ...base.deepRecommender import DeepRecommender


def _xavier(shape) -> np.ndarray:
    """tf.contrib.layers.xavier_initializer() on a rank-2 shape: U(+-sqrt(6 / (fan_in + fan_out))), from numpy's global generator"""
    lim = np.sqrt(6.0 / (shape[0] + shape[1]))
    return np.random.uniform(-lim, lim, shape).astype(np.float32)


class CFGAN(DeepRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)
        self.S_zr = 0.001            # CFGAN.py:14-16
        self.S_pm = 0.001
        self.alpha = 0.01

    def initModel(self):
        super().initModel()
        if self.data_parallel() is not None:
            raise RuntimeError("CFGAN runs on one GPU: start it without torch.distributed.run")
        ni = self.num_items
        self.G_W1 = _xavier((ni, ni))                                         # creation order of CFGAN.py:55-70
        self.G_b1 = np.zeros(ni, np.float32)
        self.D_W1 = _xavier((2 * ni, 1))
        self.D_b1 = np.zeros(1, np.float32)
        rated = self._rated_sorted()
        self._rated = (rated.indptr.astype(np.int64), rated.indices.astype(np.int32), rated.values.astype(np.float32))
        self.batches = []                  # the batches next_batch drew: (users, mask negatives (rows, items), N_zr negatives (rows, items))
        self.injected_lists = None         # a sequence of BatchLists, one per epoch: trainModel then draws nothing

    # ---- the batch stream -------------------------------------------------------------------------------------------------------
    def next_batch(self):
        """one epoch's draws in the reference's order (CFGAN.py:18-44).  Returns (users int32, BatchLists); the draw is kept in
        ``self.batches``."""
        B, ni = self.batch_size, self.num_items
        userList = list(self.data.user.keys())
        itemList = list(self.data.item.keys())
        item_id, train = self.data.item, self.data.trainSet_u
        n_zr, n_pm = int(self.S_zr * ni), int(self.S_pm * ni)
        users = np.empty(B, np.int32)
        zr, pm = ([], []), ([], [])
        for n in range(B):
            user = choice(userList)
            users[n] = self.data.user[user]
            rated = train[user]
            for count, (rows, items) in ((n_zr, zr), (n_pm, pm)):
                for _ in range(count):
                    ng = choice(itemList)
                    while ng in rated:
                        ng = choice(itemList)
                    rows.append(n); items.append(item_id[ng])
        draw = (users, tuple(np.array(a, np.int32) for a in pm), tuple(np.array(a, np.int32) for a in zr))
        self.batches.append(draw)
        return users, self._lists(draw)

    def _lists(self, draw):
        users, pm, zr = draw
        return cfgan_lists(users, self.num_items, *rated_rows(users, *self._rated), pm[0], pm[1], zr[0], zr[1])

    def recorded_lists(self, k: int):
        """the BatchLists of the k-th batch ``next_batch`` drew"""
        return self._lists(self.batches[k])

    def initial_variables(self) -> dict:
        return dict(G_W1=self.G_W1, G_b1=self.G_b1, D_W1=self.D_W1, D_b1=self.D_b1)

    def trainModel(self):
        quiet = os.environ.get("QREC_QUIET") == "1"
        tr = self.trainer = CfganTrainer(self.G_W1, self.G_b1, self.D_W1, self.D_b1, self.lRate, self.alpha)
        print("pretraining...")
        print("training...")
        for epoch in range(self.maxEpoch):
            lists = self.injected_lists[epoch] if self.injected_lists is not None else self.next_batch()[1]
            tr.train_epoch_async(lists)
            if not quiet:
                print("epoch:", epoch, "D_loss:", np.float32(tr.d_loss()), "G_loss", np.float32(tr.g_loss()))
        self._host_tables = None

    # ---- evaluation: sigmoid(C[u] G_W1 + G_b1) over the user's whole row (CFGAN.py:129-136) ------------------------------------------
    def ranking_tables(self):
        """row-count carriers for the evaluation's bookkeeping: the scores come from the trainer's device table, not from a product
        of two host tables"""
        return np.zeros((self.num_users, 1), np.float32), np.zeros((self.num_items, 1), np.float32)

    def _device_ranker(self, U, V):
        from ...ranking import SparseRowSigmoidRanker
        tr = self.trainer
        ranker = getattr(self, "_ranker", None)
        if ranker is None:
            ranker = self._ranker = SparseRowSigmoidRanker(tr.W, tr.b, self.num_users, self.num_items, tr.ld, self.data.rated_csr())
        else:
            ranker.update_tables(tr.W, tr.b)
        return ranker

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            if getattr(self, "_host_tables", None) is None:
                p = self.trainer.parameters()
                self._host_tables = (p["G_W1"], p["G_b1"])
            W, b = self._host_tables
            z = self.data.row(u).astype(np.float32).dot(W) + b
            return 1.0 / (1.0 + np.exp(-z))
        return [self.data.globalMean] * self.num_items
