"""Shared body of UserKNN and ItemKNN (model/rating/{UserKNN,ItemKNN}.py): the device neighbourhood and the host paths
that serve it."""
from __future__ import annotations

import numpy as np

from ... import capi
from ...base.recommender import Recommender
from ...engine import CoRatingKnn

MEASURES = {"pcc": capi.KNN_PCC, "euclidean": capi.KNN_EUCLIDEAN}     # util/qmath.py:108-114: anything else is cosine


class KnnRatingModel(Recommender):
    side = "user"

    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super().readConfiguration()
        self.sim = self.config["similarity"]
        self.neighbors = int(self.config["num.neighbors"])

    def printAlgorConfig(self):
        super().printAlgorConfig()
        print("Specified Arguments of", self.config["model.name"] + ":")
        print("num.neighbors:", self.config["num.neighbors"])
        print("similarity:", self.config["similarity"])
        print("=" * 80)

    def initModel(self):
        if self.side == "user":
            self.topUsers = {}
        else:
            self.topItems = {}
        self.computeSimilarities()

    def _sides(self):
        d = self.data
        if self.side == "user":
            return d.testSet_u, d.user, d.id2user, d.userMeans, d.rated_csr(), len(d.item)
        return d.testSet_i, d.item, d.id2item, d.itemMeans, d.item_rated_csr(), len(d.user)

    def computeSimilarities(self):
        tests, ids, id2name, means, rows, n_keys = self._sides()
        print("Computing %s similarities..." % self.side)
        names = list(tests)
        query_ids = np.array([ids.get(q, -1) for q in names], dtype=np.int64)
        mean_arr = np.array([means[id2name[c]] for c in range(len(ids))], dtype=np.float64)
        self.knn = CoRatingKnn(MEASURES.get(self.sim, capi.KNN_COS), rows, n_keys, mean_arr, query_ids, self.neighbors)
        self.knn.run()
        nb_ids, nb_vals, counts = self.knn.neighbours()
        top = self.topUsers if self.side == "user" else self.topItems
        for idx, q in enumerate(names):
            top[q] = [(id2name[c] if c >= 0 else names[-1 - c], s) for c, s in
                      zip(nb_ids[idx, :counts[idx]].tolist(), nb_vals[idx, :counts[idx]].tolist())]
            if idx % 100 == 0:
                print("progress:", idx, "/", len(names))
        print("The %s similarities have been calculated." % self.side)
        self._predict_test_rows(names, mean_arr)

    def _predict_test_rows(self, names, mean_arr):
        d = self.data
        tpos = {q: k for k, q in enumerate(names)}
        rows = d.testData
        if self.side == "user":
            query = [tpos[u] for u, _, _ in rows]
            other = [d.item.get(i, -1) for _, i, _ in rows]
            base = [d.userMeans[u] if u in d.user else d.globalMean for u, _, _ in rows]
        else:
            query = [tpos[i] for _, i, _ in rows]
            other = [d.user.get(u, -1) for u, _, _ in rows]
            base = [d.itemMeans[i] if i in d.item else d.globalMean for _, i, _ in rows]
        pred, status = self.knn.predict(0 if self.side == "user" else 1, np.array(query), np.array(other), np.array(base),
                                        d.rated_csr().sorted_rows(), mean_arr)
        self._test_pred = {(r[0], r[1]): (p, s) for r, p, s in zip(rows, pred.tolist(), status.tolist())}

    def predictForRating(self, u, i):
        hit = self._test_pred.get((u, i))
        if hit is not None:
            if hit[1] == capi.KNN_ZERO_DIVISION:
                raise ZeroDivisionError("float division by zero")
            return hit[0]
        return self._host_predict(u, i)

    def _host_predict(self, u, i):
        """the reference's predictForRating over the downloaded neighbour lists"""
        d = self.data
        if self.side == "user":
            top, means, own, fallback_known = self.topUsers[u], d.userMeans, u, d.containsUser(u)
        else:
            top, means, own, fallback_known = self.topItems[i], d.itemMeans, i, d.containsItem(i)
        total, denom = 0, 0
        for name, s in top[:self.neighbors]:
            r = d.rating(name, i) if self.side == "user" else (d.rating(u, name) if d.contains(u, name) else -1)
            if r != -1:
                total += s * (r - means[name])
                denom += s
        if total == 0:
            return means[own] if fallback_known else d.globalMean
        return means[own] + total / float(denom)

    def predictForRanking(self, u):
        print("Using Memory based algorithms to rank items is extremely time-consuming. So ranking for all items in %s is not available."
              % type(self).__name__)
        exit(0)
