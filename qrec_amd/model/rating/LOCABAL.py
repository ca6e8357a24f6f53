"""LOCABAL behind the reference's class name (model/rating/LOCABAL.py:8-83): a rating pass whose error is weighted by the
user's PageRank rank in the trust graph (W = 1 / (1 + log(rank)); a user with a weight gets the weighted update and then
the plain one, the reference's ``else`` being commented out), then a pass over the cosine similarities S of the kept
relations that fits p^T H q to them and moves H, P[u] and P[k].  Both passes are order-exact device kernels (fp64); the
d x d matrix H stays in LDS for a whole pass (social.hip), which bounds num.factors by 128.  The ranks come from
qrec_amd.social.pagerank_ranks (no networkx in the product).  The reference ignores the convergence test (LOCABAL.py:83)."""
from __future__ import annotations

import numpy as np

from ... import capi
from ...base.socialRecommender import SocialRecommender
from ...engine import DeviceTables, SocialHSgd
from ...social import locabal_edges, locabal_weights
from ...util import config


class LOCABAL(SocialRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, relation=list(), fold="[1]"):
        super().__init__(conf, trainingSet, testSet, relation, fold)

    def readConfiguration(self):
        super().readConfiguration()
        self.alpha = float(config.OptionConf(self.config["LOCABAL"])["-alpha"])

    def printAlgorConfig(self):
        super().printAlgorConfig()
        print("Specified Arguments of", self.config["model.name"] + ":")
        print("alpha: %.3f" % self.alpha)
        print("=" * 80)

    def initModel(self):
        super().initModel()
        if self.emb_size > capi.SOCIAL_H_MAX_D:
            raise ValueError(f"LOCABAL supports num.factors <= {capi.SOCIAL_H_MAX_D} (the d x d matrix H stays in LDS), got {self.emb_size}")
        self.H = np.random.rand(self.emb_size, self.emb_size)              # LOCABAL.py:25, before the derived data
        self.W = locabal_weights(self)                                     # :26-34, 0 = the user is in no relation
        self.S = locabal_edges(self)                                       # :35-44 in the walk order of :68-69

    def rating_evaluator(self):
        return getattr(self, "_rating_eval", None)      # bound in trainModel to the tables the SGD object holds

    def trainModel(self):
        tables = DeviceTables(self.P, self.Q, np.float64)
        sgd = SocialHSgd(tables, self.data.elemCount(), "LOCABAL", self.S, self.H, W=self.W)
        self.bind_rating_evaluator("DOT", tables)
        epoch = 0
        while epoch < self.maxEpoch:
            u, i, r = self.data.training_arrays()
            sgd.rating_pass(u, i, r, self.lRate, self.regU, self.regI)
            self.loss = sgd.social_pass(self.lRate, alpha=self.alpha, regS=self.regS)
            sp, sq, sh, _, _ = sgd.sumsq_terms()
            self.loss += self.regU * sp + self.regI * sq + self.regS * sh   # LOCABAL.py:81
            epoch += 1
            self.P, self.Q = tables.download(np.float64)
            self.H = sgd.H()
            self.isConverged(epoch)                                        # result ignored, as in the reference
