"""WRMF (Hu, Koren & Volinsky, *Collaborative Filtering for Implicit Feedback Datasets*) behind the reference's class name
and hooks (model/ranking/WRMF.py:9-74), trained on the MI355X by alternating least squares in fp64 (engine.AlsSolver,
als.hip).

What the reference computes, and so what this class computes:
  * ``X = P * 10``, ``Y = Q * 10`` from the base class's tables (:12-15);
  * per epoch, every user's row of X solved against Y, then every item's row of Y against X, with confidence
    ``c = 10 * r`` and ``lambda = reg.lambda -u`` -- the 10 is hard-coded and the conf's ``WRMF=-alpha .. -lamba ..`` is
    never read (:31-34,56-60);
  * the loss is the user half's ``sum (1 - x_u . y_i)^2`` over the training pairs, with x_u before its update (:37-38);
  * ``epoch: k loss: ...``, then ``isConverged`` (its print, the learning-rate bookkeeping, the shuffle of trainingData);
  * ranking scores ``Y.dot(X[u])`` (:69-74).
There is one execution path: the solves are independent within a half, so the parallel kernel is the reference's
algorithm, and its sums have a fixed order (two runs are bit-identical).  ``QREC_MODE`` does not apply.
"""
from __future__ import annotations

import numpy as np

from ...base.iterativeRecommender import IterativeRecommender
from ...engine import AlsSolver

CONFIDENCE = 10.0        # WRMF.py:31-34,56-60: c_ui = 10 * r_ui, whatever the conf says


class WRMF(IterativeRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def initModel(self):
        super().initModel()
        self.X = self.P * 10
        self.Y = self.Q * 10

    def trainModel(self):
        print("training...")
        rated = self.data.rated_csr()         # trainSet_u: a duplicated (user, item) pair keeps its last rating
        solver = AlsSolver(self.X, self.Y, rated.row_ids(), rated.indices, rated.values, self.regU, CONFIDENCE)
        epoch = 0
        while epoch < self.maxEpoch:
            self.loss = solver.epoch()
            epoch += 1
            print("epoch:", epoch, "loss:", self.loss)
            self.X, self.Y = solver.download()     # live tables at isConverged, as the reference's in-place updates are
            if self.isConverged(epoch):
                break

    def ranking_tables(self):
        return self.X, self.Y

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            return self.Y.dot(self.X[self.data.getUserId(u)])
        return [self.data.globalMean] * self.num_items
