"""SREE behind the reference's class name (model/rating/SREE.py:11-81): EE's rating pass and bias term, line for line,
then every training user of ``social.user`` is pulled towards each followee in turn.  Both passes are order-exact device
kernels (fp64); the per-user pass runs a level schedule built once per instance (qrec_amd/social.py).  Like EE, the
reference ignores the convergence test (SREE.py:66)."""
from __future__ import annotations

import numpy as np

from ...base.socialRecommender import SocialRecommender
from ...engine import DeviceTables, SocialSgd
from ...social import user_steps
from ...util import config


class SREE(SocialRecommender):
    ranking_form = "EUCLID"      # predictForRanking on the device: ranking.FormRanker

    def __init__(self, conf, trainingSet=None, testSet=None, relation=list(), fold="[1]"):
        super().__init__(conf, trainingSet, testSet, relation, fold)

    def readConfiguration(self):
        super().readConfiguration()
        self.alpha = float(config.OptionConf(self.config["SREE"])["-alpha"])

    def initModel(self):
        super().initModel()
        self.Bu = np.random.rand(self.data.trainingSize()[0]) / 10      # SREE.py:22-23
        self.Bi = np.random.rand(self.data.trainingSize()[1]) / 10

    def rating_evaluator(self):
        return getattr(self, "_rating_eval", None)      # bound in trainModel to the tables the SGD object holds

    def trainModel(self):
        tables = DeviceTables(self.P, self.Q, np.float64)
        sgd = SocialSgd(tables, self.data.elemCount(), "SREE", user_steps(self), Bu=self.Bu, Bi=self.Bi)
        self.bind_rating_evaluator("EUCLID", tables, Bu=sgd.mf.d_Bu, Bi=sgd.mf.d_Bi)
        self.bind_form_ranker("EUCLID", tables, Bu=sgd.mf.d_Bu, Bi=sgd.mf.d_Bi, sign=1.0)      # predictForRanking ADDS the distance
        epoch = 0
        while epoch < self.maxEpoch:
            u, i, r = self.data.training_arrays()
            self.loss = sgd.rating_pass(u, i, r, self.lRate, self.regU, self.regI, self.regB, self.data.globalMean)
            _, _, _, sbu, sbi = sgd.sumsq_terms()
            self.loss += self.regB * sbu + self.regB * sbi                  # SREE.py:47
            self.loss = sgd.social_pass(self.lRate, self.alpha, start=self.loss)   # SREE.py:49-63, after the bias term
            epoch += 1
            self.P, self.Q = tables.download(np.float64)
            self.Bu, self.Bi = sgd.biases()
            self.isConverged(epoch)                                        # result ignored, as in the reference

    def predictForRating(self, u, i):
        if self.data.containsUser(u) and self.data.containsItem(i):
            u, i = self.data.user[u], self.data.item[i]
            diff = self.P[u] - self.Q[i]
            return self.data.globalMean + self.Bi[i] + self.Bu[u] - diff.dot(diff)
        return self.data.globalMean

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            u = self.data.user[u]
            return ((self.Q - self.P[u]) * (self.Q - self.P[u])).sum(axis=1) + self.Bi + self.Bu[u] + self.data.globalMean
        return [self.data.globalMean] * len(self.data.item)
