"""SERec (Wang et al., *Collaborative Filtering with Social Exposure: A Modular Approach to Social Recommendation*, the boosting
variant) behind the reference's class name and hooks (model/ranking/SERec.py), trained on the MI355X by exposure-weighted ALS in
fp64 (engine.ExposureSolver, exposure.hip).

It is ExpoMF's algorithm (see ExpoMF.py) with lam_y = 0.01, init_std = 0.5, s = 2.2 and a prior per (user, item): it starts
at float32(0.01) and is then
    mu[u, i] = (a + A_i + (s - 1) t_u A_i - 1) / (a + b + (s - 1) t_u A_i + U - 2),   A_i = sum_u A_ui,
where t_u is the number of the user's followees that survive the social base class's filtering: the reference's
``T.dot(tile(A_sum))`` (:92-94) has t_u A_i in every entry.  The solver keeps (t, A_sum) and forms mu inside the kernels, so no
users x items array exists; ``self.mu`` after training is therefore not materialised -- ``mu_rows(users)`` builds the rows
asked for, and ``self.t`` / ``self.A_sum`` hold the state (``A_sum`` is None while the prior is still the constant).
Per epoch the reference prints ``epoch #k``, then the old mu (a users x items array), then ``\\tUpdating exposure prior...``
(:70-75); this class prints the same lines, mu summarised as numpy summarises an array of that shape (its corner entries,
built from (t, A_sum)).  With as many users as items the reference's item half reads mu transposed (its size test, :141); the
solver does the same.
"""
from __future__ import annotations

import numpy as np

from ...base.socialRecommender import SocialRecommender
from ...engine import ExposureSolver, serec_mu


class SERec(SocialRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, relation=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, relation if relation is not None else [], fold)

    def initModel(self):
        super().initModel()
        self.lam_theta = 1e-5
        self.lam_beta = 1e-5
        self.lam_y = 0.01
        self.init_mu = 0.01
        self.a = 1.0
        self.b = 99.0
        self.s = 2.2
        self.init_std = 0.5
        self.theta = self.init_std * np.random.randn(self.num_users, self.emb_size).astype(np.float32)
        self.beta = self.init_std * np.random.randn(self.num_items, self.emb_size).astype(np.float32)
        self.mu0 = float(np.float32(self.init_mu))
        t = np.zeros(self.num_users, dtype=np.float64)     # row sums of the followee matrix T (SERec.py:43-51)
        for user in self.social.followees:
            t[self.data.user[user]] += len(self.social.followees[user])
        self.t, self.A_sum = t, None

    def mu_rows(self, users) -> np.ndarray:
        """mu[users, :] of the current prior (float64)"""
        users = np.asarray(users, dtype=np.int64)
        if self.A_sum is None:
            return np.full((users.size, self.num_items), self.mu0)
        return serec_mu(self.t[users], self.A_sum, self.num_users, self.a, self.b, self.s)

    @property
    def mu(self) -> np.ndarray:
        """the whole users x items prior, built on request (the solver never forms it)"""
        return self.mu_rows(np.arange(self.num_users))

    def _mu_summary(self) -> str:
        """str(mu) of the U x I array from its corner rows and columns: numpy summarises an array above 1000 entries by its
        3 edge items per axis and formats only what it shows, so a 7 x 7 array with those corners prints the same text"""
        U, I = self.num_users, self.num_items
        if U * I <= 1000 or U < 7 or I < 7:
            return str(self.mu)
        corner = self.mu_rows([0, 1, 2, U - 3, U - 2, U - 1])[:, [0, 1, 2, I - 3, I - 2, I - 1]]
        stand = np.zeros((7, 7))
        stand[np.ix_([0, 1, 2, 4, 5, 6], [0, 1, 2, 4, 5, 6])] = corner
        with np.printoptions(threshold=6, edgeitems=3):
            return str(stand)

    def trainModel(self):
        print("training...")
        rated = self.data.rated_csr()
        solver = ExposureSolver(self.theta, self.beta, rated.row_ids(), rated.indices, self.lam_theta / self.lam_y, self.lam_y,
                                mu0=self.mu0, a=self.a, b=self.b, s=self.s, t=self.t)
        for i in range(self.maxEpoch):
            print("epoch #%d" % i)
            solver.half(0)
            solver.half(1)
            print(self._mu_summary())
            print("\tUpdating exposure prior...")
            solver.update_prior()
            self.A_sum = solver.prior_state()[1]
        self.theta, self.beta, _ = solver.download()

    def ranking_tables(self):
        return self.theta, self.beta

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            return self.beta.dot(self.theta[self.data.getUserId(u)])
        return [self.data.globalMean] * self.num_items
