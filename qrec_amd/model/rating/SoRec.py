"""SoRec behind the reference's class name (model/rating/SoRec.py:6-65): PMF's rating pass, then a pass over the pruned
``social.relation`` list that factorises the weighted trust values through P and a social table Z.  Both passes are
order-exact device kernels (fp64); the relation pass runs a level schedule built once per instance (qrec_amd/social.py)."""
from __future__ import annotations

import numpy as np

from ...base.socialRecommender import SocialRecommender
from ...engine import DeviceTables, SocialSgd
from ...social import sorec_relations
from ...util import config


class SoRec(SocialRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, relation=list(), fold="[1]"):
        super().__init__(conf, trainingSet, testSet, relation, fold)

    def readConfiguration(self):
        super().readConfiguration()
        self.regZ = float(config.OptionConf(self.config["SoRec"])["-z"])

    def initModel(self):
        super().initModel()
        self.Z = np.random.rand(self.data.trainingSize()[0], self.emb_size) / 10      # SoRec.py:17

    def printAlgorConfig(self):
        super().printAlgorConfig()
        print("Specified Arguments of", self.config["model.name"] + ":")
        print("regZ: %.3f" % self.regZ)
        print("=" * 80)

    def rating_evaluator(self):
        return getattr(self, "_rating_eval", None)      # bound in trainModel to the tables the SGD object holds

    def trainModel(self):
        tables = DeviceTables(self.P, self.Q, np.float64)
        sgd = SocialSgd(tables, self.data.elemCount(), "SoRec", sorec_relations(self), Z=self.Z)
        self.bind_rating_evaluator("DOT", tables)
        epoch = 0
        while epoch < self.maxEpoch:
            u, i, r = self.data.training_arrays()
            sgd.rating_pass(u, i, r, self.lRate, self.regU, self.regI)
            self.loss = sgd.social_pass(self.lRate, self.regS, self.regZ)
            sp, sq, sz, _, _ = sgd.sumsq_terms()
            self.loss += self.regU * sp + self.regI * sq + self.regZ * sz     # SoRec.py:60
            epoch += 1
            self.P, self.Q = tables.download(np.float64)
            self.Z = sgd.Z()
            if self.isConverged(epoch):
                break
