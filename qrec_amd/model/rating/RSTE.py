"""RSTE behind the reference's class name (model/rating/RSTE.py:4-82): the prediction blends the user's own P[u].Q[i]
(weight alpha) with its followees' weighted mean P[f].Q[i]; per-rating SGD in ``trainingData`` order through an
order-exact device kernel (fp64).  Like SVD, the reference ignores the convergence test (RSTE.py:40)."""
from __future__ import annotations

import numpy as np

from ...base.socialRecommender import SocialRecommender
from ...engine import DeviceTables, SocialSgd
from ...social import followee_csr_by_user
from ...util import config


class RSTE(SocialRecommender):
    ranking_form = "RSTE"        # predictForRanking on the device: ranking.FormRanker

    def __init__(self, conf, trainingSet=None, testSet=None, relation=list(), fold="[1]"):
        super().__init__(conf, trainingSet, testSet, relation, fold)

    def readConfiguration(self):
        super().readConfiguration()
        self.alpha = float(config.OptionConf(self.config["RSTE"])["-alpha"])

    def printAlgorConfig(self):
        super().printAlgorConfig()
        print("Specified Arguments of", self.config["model.name"] + ":")
        print("alpha: %.3f" % self.alpha)
        print("=" * 80)

    def rating_evaluator(self):
        return getattr(self, "_rating_eval", None)      # bound in trainModel to the tables the SGD object holds

    def trainModel(self):
        tables = DeviceTables(self.P, self.Q, np.float64)
        sgd = SocialSgd(tables, self.data.elemCount(), "RSTE", followee_csr_by_user(self))
        self.bind_rating_evaluator("RSTE", tables, followees=(sgd.d_fe_ptr, sgd.d_fe_ids, sgd.d_fe_w, sgd.d_den), alpha=self.alpha)
        self.bind_form_ranker("RSTE", tables, followees=(sgd.d_fe_ptr, sgd.d_fe_ids, sgd.d_fe_w, sgd.d_den), alpha=self.alpha)
        epoch = 0
        while epoch < self.maxEpoch:
            u, i, r = self.data.training_arrays()
            self.loss = sgd.rating_pass(u, i, r, self.lRate, self.regU, self.regI, alpha=self.alpha)
            sp, sq, _, _, _ = sgd.sumsq_terms()
            self.loss += self.regU * sp + self.regI * sq                      # RSTE.py:38
            epoch += 1
            self.P, self.Q = tables.download(np.float64)
            self.isConverged(epoch)                                        # result ignored, as in the reference

    def predictForRating(self, u, i):
        if self.data.containsUser(u) and self.data.containsItem(i):
            i = self.data.item[i]
            relations = self.social.getFollowees(u)
            indexes = [self.data.user[f] for f in relations if self.data.containsUser(f)]
            weights = np.array([relations[f] for f in relations if self.data.containsUser(f)])
            indexes = np.array(indexes)
            denom = weights.sum()
            u = self.data.user[u]
            if denom != 0:
                fPred = 0 + weights.dot(self.P[indexes].dot(self.Q[i]))
                return self.alpha * self.P[u].dot(self.Q[i]) + (1 - self.alpha) * fPred / denom
            return self.P[u].dot(self.Q[i])
        return self.data.globalMean

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            fPred, denom = 0, 0
            relations = self.social.getFollowees(u)
            for f in relations:
                if self.data.containsUser(f):
                    fPred += relations[f] * self.Q.dot(self.P[self.data.user[f]])
                    denom += relations[f]
            u = self.data.user[u]
            if denom != 0:
                return self.alpha * self.Q.dot(self.P[u]) + (1 - self.alpha) * fPred / denom
            return self.Q.dot(self.P[u])
        return [self.data.globalMean] * len(self.data.item)
