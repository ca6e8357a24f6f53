"""CDAE behind the reference's class name and hooks (model/ranking/CDAE.py:8-107): a denoising auto-encoder over the whole user row --
``-co`` keep probability of the input mask, ``-nh`` hidden units with a per-user vector added, a sigmoid output over all items with
five sampled negatives per rated item, Adam; one batch per ``num.max.epoch``.

Exact mode (the default) consumes ``np.random`` and ``random`` as the reference's loop does: per step the mask by
``np.random.binomial(1, co, (batch, n_items))`` first, then the users and negatives of ``next_batch`` on the CPython stream (replayed
natively, csrc/mt_sampler.cpp); the lists the kernels consume are then built on the host.  QREC_MODE=throughput draws users,
negatives and keep decisions on the device instead (Philox, QREC_SEED) and builds the same lists there: the reference's
distribution, not its streams, and neither ``np.random`` nor ``random`` is consumed by the steps."""
from __future__ import annotations

import os
import random

import numpy as np

from ... import capi
from ...autoencoder import NEGATIVES_PER_RATED, CdaeTrainer, DeviceBatchStream, lists_from_entries, rated_rows
from ...base.deepRecommender import DeepRecommender
from ...util import config


def _xavier(shape) -> np.ndarray:
    """tf.contrib.layers.xavier_initializer(): U(+-sqrt(6 / (fan_in + fan_out))); on a rank-1 shape contrib takes
    fan_in = fan_out = n, i.e. U(+-sqrt(3 / n)).  From numpy's global generator."""
    lim = np.sqrt(6.0 / (shape[0] + shape[1])) if len(shape) == 2 else np.sqrt(3.0 / shape[0])
    return np.random.uniform(-lim, lim, shape).astype(np.float32)


class CDAE(DeepRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super().readConfiguration()
        args = config.OptionConf(self.config["CDAE"])
        self.corruption_level = float(args["-co"])
        self.n_hidden = int(args["-nh"])

    def initModel(self):
        super().initModel()
        if self.data_parallel() is not None:
            raise RuntimeError("CDAE runs on one GPU: start it without torch.distributed.run")
        self.negative_sp = NEGATIVES_PER_RATED
        nu, ni, nh = self.num_users, self.num_items, self.n_hidden
        self.V = _xavier((nu, nh))                                            # creation order of CDAE.py:58-67
        self.weights = {"encoder": _xavier((ni, nh)), "decoder": _xavier((nh, ni))}
        self.biases = {"encoder": _xavier((nh,)), "decoder": _xavier((ni,))}
        rated = self._rated_sorted()
        self._rated = (rated.indptr.astype(np.int64), rated.indices.astype(np.int32), rated.values.astype(np.float32))
        self.batches = []                                                     # the batch stream trainModel used (exact mode), see next_batch

    # ---- the batch stream -------------------------------------------------------------------------------------------------------
    def next_batch(self):
        """one step's draws in the reference's order (CDAE.py:89-90): the mask from numpy's global stream, then users and negatives
        from ``random``.  Returns (mask int [batch, n_items], users int32, BatchLists); the draw is kept in ``self.batches`` as
        (users, packed mask bits, negative indptr, negative items)."""
        B, ni = self.batch_size, self.num_items
        mask = np.random.binomial(1, self.corruption_level, (B, ni))
        indptr, items, vals = self._rated
        state = random.getstate()
        words = capi.state_from_python(state)
        users, neg_ptr, neg_items = capi.mt_cdae_sample_batch(words, indptr, items, ni, B, self.negative_sp)
        random.setstate(capi.state_to_python(words, state[2]))
        pr, pi, pv = rated_rows(users, indptr, items, vals)
        nr = np.repeat(np.arange(B, dtype=np.int32), np.diff(neg_ptr))
        lists = lists_from_entries(users, ni, pr, pi, pv, nr, neg_items, lambda r, i: mask[r, i] != 0)
        self.batches.append((users, np.packbits(mask.astype(bool), axis=None), neg_ptr, neg_items))
        return mask, users, lists

    def recorded_lists(self, k: int):
        """the BatchLists of the k-th batch ``trainModel`` used, rebuilt from ``self.batches``"""
        users, bits, neg_ptr, neg_items = self.batches[k]
        B, ni = users.size, self.num_items
        mask = np.unpackbits(bits)[:B * ni].reshape(B, ni)
        pr, pi, pv = rated_rows(users, *self._rated)
        nr = np.repeat(np.arange(B, dtype=np.int32), np.diff(neg_ptr))
        return lists_from_entries(users, ni, pr, pi, pv, nr, neg_items, lambda r, i: mask[r, i] != 0)

    def initial_variables(self) -> dict:
        return dict(W_enc=self.weights["encoder"], W_dec=self.weights["decoder"], b_enc=self.biases["encoder"],
                    b_dec=self.biases["decoder"], V=self.V)

    def trainModel(self):
        quiet = os.environ.get("QREC_QUIET") == "1"
        # nothing between here and the first step's draws touches np.random or random
        tr = self.trainer = self.build_trainer(CdaeTrainer, self.weights["encoder"], self.weights["decoder"], self.biases["encoder"],
                                               self.biases["decoder"], self.V, self.lRate, self.regU)
        stream = None
        if self.throughput_mode():
            stream = self.device_stream = DeviceBatchStream(*self._rated, self.num_items, self.batch_size, self.corruption_level,
                                                            int(os.environ.get("QREC_SEED", "0")), self.negative_sp)
        for epoch in range(self.maxEpoch):
            tr.train_step_async(stream.draw(epoch) if stream else self.next_batch()[2])
            if not quiet:
                print(self.foldInfo, "Epoch:", "%04d" % (epoch + 1), "loss=", "{:.9f}".format(tr.loss()))
        print("Optimization Finished!")
        self._refresh_scoring_tables()

    # ---- evaluation: sigmoid(h_u W_dec + b_dec), h_u from the whole rated row (CDAE.py:100-105) ------------------------------------
    def _refresh_scoring_tables(self):
        tr = self.trainer
        indptr, items, vals = self._rated
        self._d_hidden = tr.hidden(np.arange(self.num_users, dtype=np.int32), indptr, items, vals)
        p = tr.parameters()
        self.U = self._d_hidden.numpy()[:self.num_users, :self.n_hidden].copy()        # hidden rows of all users
        self.Vt = np.ascontiguousarray(p["W_dec"].T)                                    # item-major decoder weight
        self.b_dec = p["b_dec"]

    def ranking_tables(self):
        return self.U, self.Vt

    def _device_ranker(self, U, V):
        from ...ranking import SigmoidBiasRanker
        tr = self.trainer
        ranker = getattr(self, "_ranker", None)
        if ranker is None:
            ranker = self._ranker = SigmoidBiasRanker(self._d_hidden, tr.W_dec, tr.b_dec, self.num_users, self.num_items, self.n_hidden,
                                                      tr.ld, self.data.rated_csr())
        else:
            ranker.update_tables(self._d_hidden, tr.W_dec, tr.b_dec)
        return ranker

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            s = self.Vt.dot(self.U[self.data.getUserId(u)]) + self.b_dec
            return 1.0 / (1.0 + np.exp(-s))
        return [self.data.globalMean] * self.num_items
