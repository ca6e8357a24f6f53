"""ExpoMF (Liang, Charlin, McInerney & Blei, *Modeling User Exposure in Recommendation*) behind the reference's class name and
hooks (model/ranking/ExpoMF.py), trained on the MI355X by exposure-weighted ALS in fp64 (engine.ExposureSolver, exposure.hip).

What the reference computes, and so what this class computes:
  * after the base class's P and Q, ``theta = init_std * randn(U, d).astype(float32)`` and then ``beta`` likewise, on numpy's
    global stream; the prior starts at float32(0.01) per item (:16-31);
  * per epoch (:42-46): every user's row solved with the posterior from its old row and mu per item, every item's row against
    the new theta with mu of that item, then ``\\tUpdating exposure prior...``, the old mu printed, and
    ``mu_i = (a + sum_u A_ui - 1) / (a + b + U - 2)`` with the new tables and the old mu (:61-73);
  * observed pairs are the training pairs with value 1, whatever the rating; the ridge is lam_theta / lam_y = 1e-5, the
    conf's ``reg.lambda`` is never read; ``n_jobs`` and ``batch_size`` only chunk the work;
  * no ``isConverged``: no per-epoch measure, no shuffle, Python's ``random`` untouched by training;
  * ranking scores ``beta.dot(theta[u])``.
The reference forms the posterior and the Gram in float32 and stores float32 rows; this class computes and stores in fp64 (its
run is the reference's with the tables cast to float64, tests/test_gpu_expo.py).  With as many users as items the reference's
item half reads mu by user index (its size test, :104); the solver does the same.
"""
from __future__ import annotations

import numpy as np

from ...base.iterativeRecommender import IterativeRecommender
from ...engine import ExposureSolver


class ExpoMF(IterativeRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def initModel(self):
        super().initModel()
        self.lam_theta = 1e-5
        self.lam_beta = 1e-5
        self.lam_y = 1.0
        self.init_mu = 0.01
        self.a = 1.0
        self.b = 99.0
        self.init_std = 0.01
        self.theta = self.init_std * np.random.randn(self.num_users, self.emb_size).astype(np.float32)
        self.beta = self.init_std * np.random.randn(self.num_items, self.emb_size).astype(np.float32)
        self.mu = self.init_mu * np.ones(self.num_items, dtype=np.float32)

    def trainModel(self):
        print("training...")
        rated = self.data.rated_csr()                 # trainSet_u's pairs, value 1
        solver = ExposureSolver(self.theta, self.beta, rated.row_ids(), rated.indices, self.lam_theta / self.lam_y, self.lam_y,
                                mu0=float(self.mu[0]) if self.mu.size else self.init_mu, a=self.a, b=self.b)
        for i in range(self.maxEpoch):
            print("epoch #%d" % i)
            solver.half(0)
            solver.half(1)
            print("\tUpdating exposure prior...")
            print(solver.prior_state())               # the old mu, as _update_expo prints it
            solver.update_prior()
        self.theta, self.beta, self.mu = solver.download()

    def ranking_tables(self):
        return self.theta, self.beta

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            return self.beta.dot(self.theta[self.data.getUserId(u)])
        return [self.data.globalMean] * self.num_items
