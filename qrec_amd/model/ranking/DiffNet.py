"""DiffNet behind the reference's class name and hooks (model/ranking/DiffNet.py:12-81): ``-n_layer`` rounds of social
diffusion  u <- relu([S u | u] W_k)  over the follow graph, the user's mean rated-item vector added on top, batch BPR loss +
batch L2, Adam.  Needs the ``social`` file (``social.setup``).  Scores come from the diffused user table and the item table."""
from __future__ import annotations

import os

import numpy as np

from ...base.graphRecommender import GraphRecommender
from ...base.socialRecommender import SocialRecommender
from ...diffusion import rating_mean_csr, social_csr
from ...graph import DiffNetTrainer
from ...util import config


def _xavier(shape) -> np.ndarray:
    """tf.contrib.layers.xavier_initializer(): U(+-sqrt(6 / (fan_in + fan_out))), from numpy's global generator"""
    lim = np.sqrt(6.0 / (shape[0] + shape[1]))
    return np.random.uniform(-lim, lim, shape).astype(np.float32)


class DiffNet(SocialRecommender, GraphRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, relation=None, fold="[1]"):
        SocialRecommender.__init__(self, conf, trainingSet, testSet, relation if relation is not None else [], fold)

    def readConfiguration(self):
        super().readConfiguration()
        args = config.OptionConf(self.config["DiffNet"])
        self.n_layers = int(args["-n_layer"])

    def buildSparseRelationMatrix(self):
        """S (DiffNet.py:22-29): row = follower, 1 / |followees| per follow edge"""
        fo, fe = self.relation_ids()
        return social_csr(self.num_users, fo, fe)

    def initModel(self):
        super().initModel()
        if self.data_parallel() is not None:
            raise RuntimeError("DiffNet runs on one GPU: start it without torch.distributed.run")
        uid, iid, _ = self.data.training_arrays()
        d = self.emb_size
        self.weights = [_xavier((2 * d, d)) for _ in range(self.n_layers)]          # weights%d, fan-in 2d (DiffNet.py:41-43)
        self.trainer = self.build_trainer(DiffNetTrainer, self.user_embeddings, self.item_embeddings, self.weights,
                                          self.buildSparseRelationMatrix(), rating_mean_csr(self.num_users, self.num_items, uid, iid),
                                          self.lRate, self.regU, self.n_layers)

    def trainModel(self):
        quiet = os.environ.get("QREC_QUIET") == "1"
        tr = self.trainer
        for epoch, (n_rows, d_u, d_i, d_j) in enumerate(self.iter_epoch_device_samples(self.maxEpoch)):     # base/deepRecommender.py:29-52
            for n, s in enumerate(range(0, n_rows, self.batch_size)):
                tr.train_step_async(d_u.ptr + 4 * s, d_i.ptr + 4 * s, d_j.ptr + 4 * s, min(self.batch_size, n_rows - s))
                if not quiet:
                    print("training:", epoch + 1, "batch", n, "loss:", tr.loss())
        # the reference scores one user per sess.run(self.test) (DiffNet.py:75-79); here both tables are materialised once
        self.U, self.V = tr.inference_embeddings()

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            return self.V.dot(self.U[self.data.getUserId(u)])
        return [self.data.globalMean] * self.num_items
