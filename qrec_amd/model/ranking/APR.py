"""APR (Adversarial Personalized Ranking) behind the reference's class name and hooks (model/ranking/APR.py:8-130): ``-eps`` the
length of a row's perturbation, ``-regA`` the weight of the adversarial term, ``-advEpoch`` read and unused, as in the file.
``num.max.epoch // 2`` epochs of pretraining on softplus(-x) + the batch L2 of the looked-up user and positive rows, then as many
adversarial epochs: per batch the perturbation update first, then the step on both objectives, one Adam across both phases.

Which rows the perturbation update is fed, conf key ``qrec.apr.perturb``, else env ``QREC_APR_PERTURB``:

``reference`` (default)
    (u, j, j): what the file feeds (APR.py:116-117, the negatives as ``v_idx`` too).  The perturbed positive and negative rows are
    then one tensor, every contribution to the perturbations' gradient meets its exact negation, and both perturbation tables stay
    exactly zero: the file as it stands trains BPR with the softplus term weighted 1 + regA.
``paper``
    (u, i, j): the batch's positives, the update the paper describes.

Both go through the same kernels (csrc/apr.hip).  Exact mode (the default) replays the CPython stream of ``next_batch_pairwise`` and
adds the step's gradients in the reference's CPU order; ``QREC_MODE=throughput`` draws the epochs on the device and adds them with
float atomics.  The perturbation pass is the same in both."""
from __future__ import annotations

import os

from ...base.deepRecommender import DeepRecommender
from ...graph import AprTrainer
from ...util import config

PERTURB_FEEDS = ("reference", "paper")


class APR(DeepRecommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super().readConfiguration()
        args = config.OptionConf(self.config["APR"])
        self.eps = float(args["-eps"])
        self.regAdv = float(args["-regA"])
        self.advEpoch = int(args["-advEpoch"])
        feed = self.config["qrec.apr.perturb"] if self.config.contains("qrec.apr.perturb") else os.environ.get("QREC_APR_PERTURB", "reference")
        if feed not in PERTURB_FEEDS:
            raise ValueError(f"qrec.apr.perturb / QREC_APR_PERTURB must be one of {', '.join(PERTURB_FEEDS)} (got {feed!r})")
        self.perturb_feed = feed

    def initModel(self):
        super().initModel()
        if self.data_parallel() is not None:
            raise RuntimeError("APR runs on one GPU: start it without torch.distributed.run")

    def perturb_feeds(self, u, i, j):
        """(u, v, n) of the perturbation update for a batch (u, i, j)"""
        return (u, j, j) if self.perturb_feed == "reference" else (u, i, j)

    def trainModel(self):
        quiet = os.environ.get("QREC_QUIET") == "1"
        tr = self.trainer = self.build_trainer(AprTrainer, self.user_embeddings, self.item_embeddings, self.lRate, self.regU, self.regAdv,
                                               self.eps, self.batch_size)
        half = self.maxEpoch // 2
        print("pretraining...")
        # one stream of epochs for both phases (base/deepRecommender.py:29-52): the device-drawn one numbers its epochs from the start
        for k, (n_rows, d_u, d_i, d_j) in enumerate(self.iter_epoch_device_samples(2 * half)):
            if k == half:
                print("adversarial training...")
            for n, s in enumerate(range(0, n_rows, self.batch_size)):
                B = min(self.batch_size, n_rows - s)
                u, i, j = d_u.ptr + 4 * s, d_i.ptr + 4 * s, d_j.ptr + 4 * s
                if k < half:
                    tr.pretrain_step_async(u, i, j, B)
                    continue
                tr.perturb_async(*self.perturb_feeds(u, i, j), B)
                tr.adversarial_step_async(u, i, j, B)
                if not quiet:                                        # the reference prints every adversarial batch
                    print(self.foldInfo, "training:", k - half + 1, "batch", n, "loss:", tr.loss())
            if k >= half:                                            # APR.py:120-121: after every adversarial epoch
                self.P, self.Q = tr.tables()
        if half == 0:
            print("adversarial training...")

    def predictForRanking(self, u):
        if self.data.containsUser(u):
            return self.Q.dot(self.P[self.data.getUserId(u)])
        return [self.data.globalMean] * self.num_items
