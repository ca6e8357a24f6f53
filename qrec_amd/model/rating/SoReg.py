"""SoReg behind the reference's class name (model/rating/SoReg.py:6-77): PMF's rating pass, then every training user of
``social.user`` is pulled towards its followees and followers, weighted by Sim = (pearson_sp of the two users' ratings +
trust weight) / 2.  Both passes are order-exact device kernels (fp64); the per-user pass runs a level schedule built once
per instance (qrec_amd/social.py)."""
from __future__ import annotations

from collections import defaultdict

import numpy as np

from ...base.socialRecommender import SocialRecommender
from ...engine import DeviceTables, SocialSgd
from ...social import user_steps
from ...util import config, qmath


class SoReg(SocialRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, relation=list(), fold="[1]"):
        super().__init__(conf, trainingSet, testSet, relation, fold)

    def readConfiguration(self):
        super().readConfiguration()
        self.alpha = float(config.OptionConf(self.config["SoReg"])["-alpha"])

    def printAlgorConfig(self):
        super().printAlgorConfig()
        print("Specified Arguments of", self.config["model.name"] + ":")
        print("alpha: %.3f" % self.alpha)
        print("=" * 80)

    def initModel(self):
        super().initModel()
        # SoReg.py:24-33: Sim[u][f] is set with Sim[f][u] by whichever direction is met first, in data.user order
        self.Sim = defaultdict(dict)
        print("constructing similarity matrix...")
        for user in self.data.user:
            for f in self.social.getFollowees(user):
                if not (user in self.Sim and f in self.Sim[user]):
                    self.Sim[user][f] = self.sim(user, f)
                    self.Sim[f][user] = self.Sim[user][f]

    def sim(self, u, v):
        return (qmath.pearson_sp(self.data.sRow(u), self.data.sRow(v)) + self.social.weight(u, v)) / 2.0

    def rating_evaluator(self):
        return getattr(self, "_rating_eval", None)      # bound in trainModel to the tables the SGD object holds

    def trainModel(self):
        tables = DeviceTables(self.P, self.Q, np.float64)
        steps = user_steps(self, weight=lambda u, v: self.Sim[u][v], followers=True)
        sgd = SocialSgd(tables, self.data.elemCount(), "SoReg", steps)
        self.bind_rating_evaluator("DOT", tables)
        epoch = 0
        while epoch < self.maxEpoch:
            u, i, r = self.data.training_arrays()
            sgd.rating_pass(u, i, r, self.lRate, self.regU, self.regI)
            self.loss = sgd.social_pass(self.lRate, self.alpha)
            sp, sq, _, _, _ = sgd.sumsq_terms()
            self.loss += self.regU * sp + self.regI * sq                      # SoReg.py:73
            epoch += 1
            self.P, self.Q = tables.download(np.float64)
            if self.isConverged(epoch):
                break
