"""SocialMF behind the reference's class name, numpy path (model/rating/SocialMF.py:11-47): PMF's arithmetic on copies of
P[u], Q[i] for the ratings, then every training user of ``social.user`` is moved towards the weighted mean of its
followees.  Both passes are order-exact device kernels (fp64); the per-user pass runs a level schedule built once per
instance (qrec_amd/social.py).  The TF path (trainModel_tf) is not provided."""
from __future__ import annotations

import numpy as np

from ...base.socialRecommender import SocialRecommender
from ...engine import DeviceTables, SocialSgd
from ...social import user_steps


class SocialMF(SocialRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, relation=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, relation, fold)

    def rating_evaluator(self):
        return getattr(self, "_rating_eval", None)      # bound in trainModel to the tables the SGD object holds

    def trainModel(self):
        tables = DeviceTables(self.P, self.Q, np.float64)
        sgd = SocialSgd(tables, self.data.elemCount(), "SocialMF", user_steps(self))
        self.bind_rating_evaluator("DOT", tables)
        epoch = 0
        while epoch < self.maxEpoch:
            u, i, r = self.data.training_arrays()
            sgd.rating_pass(u, i, r, self.lRate, self.regU, self.regI)
            self.loss = sgd.social_pass(self.lRate, self.regS)
            sp, sq, _, _, _ = sgd.sumsq_terms()
            self.loss += self.regU * sp + self.regI * sq                      # SocialMF.py:42
            epoch += 1
            self.P, self.Q = tables.download(np.float64)
            if self.isConverged(epoch):
                break
