"""DHCF behind the reference's class name and hooks (model/ranking/DHCF.py:12-129): two hypergraph-convolution layers over
the 1-hop user and item hypergraphs with one shared d x d weight per layer, LeakyReLU(0.2), message dropout 0.1 while
training, L2-normalised layer outputs concatenated with the ego embeddings (3d wide), batch BPR loss + batch L2 + L2 of the
weights, Adam.  Test-time scores come from the inference graph (no dropout)."""
from __future__ import annotations

import os

from ...base.deepRecommender import DeepRecommender
from ...graph import DHCFTrainer
from .SimGCL import xavier_uniform


class DHCF(DeepRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def initModel(self):
        super().initModel()
        if self.data_parallel() is not None:
            raise RuntimeError("DHCF runs on one GPU: start it without torch.distributed.run")
        d = self.emb_size
        self.n_layer = 2                                                               # DHCF.py:57
        self.weights = [xavier_uniform((d, d)) for _ in range(self.n_layer)]           # JU_1, JU_2
        uid, iid, _ = self.data.training_arrays()
        self.trainer = self.build_trainer(DHCFTrainer, self.user_embeddings, self.item_embeddings, self.weights, uid, iid,
                                          self.lRate, self.regU, seed=int(os.environ.get("QREC_SEED", "0")))

    def trainModel(self):
        quiet = os.environ.get("QREC_QUIET") == "1"
        tr = self.trainer
        for epoch, (n_rows, d_u, d_i, d_j) in enumerate(self.iter_epoch_device_samples(self.maxEpoch)):     # base/deepRecommender.py:29-52
            for n, s in enumerate(range(0, n_rows, self.batch_size)):
                tr.train_step_async(d_u.ptr + 4 * s, d_i.ptr + 4 * s, d_j.ptr + 4 * s, min(self.batch_size, n_rows - s))
                if not quiet:
                    print("training:", epoch + 1, "batch", n, "loss:", tr.loss())
        # the reference scores with sess.run(self.test, isTraining=0) per user (DHCF.py:123-127); here the inference-graph
        # tables are materialised once and ranked in one batch
        self.U, self.V = tr.inference_embeddings()

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            return self.V.dot(self.U[self.data.getUserId(u)])
        return [self.data.globalMean] * self.num_items
