"""SocialFD behind the reference's class name (model/rating/SocialFD.py:5-114): ratings are predicted from the distance
(x - y) H H^T (x - y)^T between a user and an item under the learned metric H; the rating pass treats high (r > 0.7), low
(r <= 0.5, two branches on the distance) and medium ratings differently, the social pass pulls every user towards its
followees under the same metric.  x = P[u], y = Q[i] are views in the reference and stay so here.  Both passes are
order-exact device kernels (fp64); the d x d matrix H stays in LDS for a whole pass (social.hip), which bounds
num.factors by 128.  A ranking score is a quadratic form in x - y: a squared distance of the rows projected by H, which is how the
device ranks it (ranking.FormRanker, form METRIC)."""
from __future__ import annotations

import numpy as np

from ... import capi
from ...base.socialRecommender import SocialRecommender
from ...engine import DeviceTables, SocialHSgd
from ...social import socialfd_steps
from ...util import config


class SocialFD(SocialRecommender):
    ranking_form = "METRIC"      # predictForRanking on the device: ranking.FormRanker

    def __init__(self, conf, trainingSet=None, testSet=None, relation=list(), fold="[1]"):
        super().__init__(conf, trainingSet, testSet, relation, fold)

    def initModel(self):
        super().initModel()
        if self.emb_size > capi.SOCIAL_H_MAX_D:
            raise ValueError(f"SocialFD supports num.factors <= {capi.SOCIAL_H_MAX_D} (the d x d matrix H stays in LDS), got {self.emb_size}")
        self.Bu = np.random.rand(self.data.trainingSize()[0]) / 5          # SocialFD.py:11-15, in this order
        self.Bi = np.random.rand(self.data.trainingSize()[1]) / 5
        self.H = np.random.rand(self.emb_size, self.emb_size) / 5
        self.P /= 10
        self.Q /= 10

    def readConfiguration(self):
        super().readConfiguration()
        eps = config.OptionConf(self.config["SocialFD"])
        self.alpha = float(eps["-alpha"])
        self.eta = float(eps["-eta"])
        self.beta = float(eps["-beta"])

    def rating_evaluator(self):
        return getattr(self, "_rating_eval", None)      # bound in trainModel to the tables the SGD object holds

    def trainModel(self):
        tables = DeviceTables(self.P, self.Q, np.float64)
        sgd = SocialHSgd(tables, self.data.elemCount(), "SocialFD", socialfd_steps(self), self.H, Bu=self.Bu, Bi=self.Bi)
        self.bind_rating_evaluator("METRIC", tables, Bu=sgd.d_Bu, Bi=sgd.d_Bi, H=sgd.d_H)
        self.bind_form_ranker("METRIC", tables, Bu=sgd.d_Bu, Bi=sgd.d_Bi, H=sgd.d_H, sign=-1.0)
        epoch = 0
        while epoch < self.maxEpoch:
            u, i, r = self.data.training_arrays()
            sgd.rating_pass(u, i, r, self.lRate, self.regU, self.regI, self.eta, self.alpha, self.data.globalMean)
            self.loss = sgd.social_pass(self.lRate, eta=self.eta, beta=self.beta)
            epoch += 1
            self.P, self.Q = tables.download(np.float64)
            self.H = sgd.H()
            self.Bu, self.Bi = sgd.biases()
            self.loss += self.regU * self.Bu.dot(self.Bu) + self.regI * self.Bi.dot(self.Bi)      # SocialFD.py:88
            if self.isConverged(epoch):
                break

    def predictForRating(self, u, i):
        if self.data.containsUser(u) and self.data.containsItem(i):
            u, i = self.data.user[u], self.data.item[i]
            diff = self.P[u] - self.Q[i]
            return self.Bi[i] + self.Bu[u] + self.data.globalMean - diff.dot(self.H).dot(self.H.T).dot(diff.T)
        return self.data.globalMean

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            u = self.data.user[u]
            diff = self.P[u] - self.Q
            A = self.H.dot(self.H.T)
            return self.Bi + self.Bu[u] + self.data.globalMean - (diff.dot(A) * diff).sum(axis=1)
        return np.array([self.data.globalMean] * len(self.data.item))
