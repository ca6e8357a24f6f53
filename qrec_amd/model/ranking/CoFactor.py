"""CoFactor (Liang et al., *Factorization Meets the Item Embedding: Regularizing Matrix Factorization with Item
Co-occurrence*, RecSys 2016) behind the reference's class name and hooks (model/ranking/CoFactor.py), trained on the MI355X in
fp64 (engine.CoOccurrence / engine.CoFactorSolver, cofactor.hip, als.hip).

What the reference computes, and so what this class computes:
  * ``CoFactor=-k K -gamma R -filter F`` (K < 1 becomes 1); ``reg.lambda -u`` regularises both halves, ``-i`` is never read,
    R only the context solve;
  * ``initModel``: the co-occurrence counts of the items with >= F raters, pairs kept when they share > F raters (:36-56),
    then the shifted positive PMI ``max(log(count D / (f_i f_j)) - log K, 0) / max`` (:58-81).  The counts come from the
    device; the logarithms are the C library's, taken on the host, and the neighbour order of every SPPMI row -- the order the
    item step sums in -- is the reference's dict order (engine.sppmi_from_counts).  The reference's ``i/num_items`` progress
    lines of its pair loop have no counterpart here and are not printed;
  * ``trainModel``: ``X = P * 10``, ``Y = Q * 10``, then w, c, G drawn from ``np.random`` in that order (:85-89); per epoch
    WRMF's user half with the loss ``sum (1 - x_u . y_i)^2`` (x_u before its update), then the Gauss-Seidel item sweep in
    ``data.item`` order with the context terms, the second solve for G[i] and the two biases (:116-159), run by levels that
    keep the sweep's read-after-write order;
  * ``epoch: k loss: ...`` and nothing else per epoch: no ``isConverged``, so no learning-rate bookkeeping, no shuffle, no
    early stop;
  * ranking scores ``Y.dot(X[u])``.
There is one execution path; ``QREC_MODE`` does not apply.
"""
from __future__ import annotations

import numpy as np

from ...base.iterativeRecommender import IterativeRecommender
from ...engine import CoFactorSolver, CoOccurrence
from ...util import config

CONFIDENCE = 10.0        # CoFactor.py:104-107,124-127: c_ui = 10 * r_ui


class CoFactor(IterativeRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super().readConfiguration()
        extra = config.OptionConf(self.config["CoFactor"])
        self.negCount = int(extra["-k"])       # the number of negative samples
        if self.negCount < 1:
            self.negCount = 1
        self.regR = float(extra["-gamma"])
        self.filter = int(extra["-filter"])

    def printAlgorConfig(self):
        super().printAlgorConfig()
        print("Specified Arguments of", self.config["model.name"] + ":")
        print("k: %d" % self.negCount)
        print("regR: %.5f" % self.regR)
        print("filter: %d" % self.filter)
        print("=" * 80)

    def initModel(self):
        super().initModel()
        print("Constructing SPPMI matrix...")
        rated = self.data.rated_csr()
        self.cooccurrence = CoOccurrence(rated.row_ids(), rated.indices, self.num_users, self.num_items, self.filter)
        self.SPPMI = self.cooccurrence.sppmi(self.negCount)        # (ptr, idx, val): row i = the reference's SPPMI[i], in its order

    def trainModel(self):
        self.X = self.P * 10     # Theta
        self.Y = self.Q * 10     # Beta
        self.w = np.random.rand(self.num_items) / 10     # bias value of item
        self.c = np.random.rand(self.num_items) / 10     # bias value of context
        self.G = np.random.rand(self.num_items, self.emb_size) / 10     # context embedding
        print("training...")
        rated = self.data.rated_csr()         # trainSet_u: a duplicated (user, item) pair keeps its last rating
        self.solver = solver = CoFactorSolver(self.X, self.Y, self.G, self.w, self.c, rated.row_ids(), rated.indices, rated.values,
                                              self.SPPMI, self.regU, self.regR, CONFIDENCE)
        epoch = 0
        while epoch < self.maxEpoch:
            self.loss = solver.epoch()
            self.X, self.Y, self.G, self.w, self.c = solver.download()
            epoch += 1
            print("epoch:", epoch, "loss:", self.loss)

    def ranking_tables(self):
        return self.X, self.Y

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            return self.Y.dot(self.X[self.data.getUserId(u)])
        return [self.data.globalMean] * self.num_items
