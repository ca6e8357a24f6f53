"""SlopeOne behind the reference's class name and printed lines (model/rating/SlopeOne.py), on the MI355X in fp64
(engine.SlopeOneSolver, knn.hip).

What the reference computes, and so what this class computes: for every test item i and every training item j (j == i
included), ``diffAverage[i][j] = sum (x1[u] - x2[u]) / count`` over the users of ``sCol(i)`` in its dict order that also rated
j (0 when none) and ``freq[i][j] = count``; a training user's prediction walks the user's row in dict order,
``sum (r + diffAverage) * freq / sum freq``, or ``userMeans[u]`` when the frequencies sum to 0; an unknown user gets
``itemMeans[i]`` or ``globalMean``.  Departure: ``diffAverage`` / ``freq`` are not materialised -- the test items are swept in
batches whose deviation rows live on the device only while that batch's test rows are predicted; another (user, item)
pair of a test item is predicted on the host.  ``QREC_MODE`` does not apply.
"""
from __future__ import annotations

import numpy as np

from ...base.recommender import Recommender
from ...engine import SlopeOneSolver


class SlopeOne(Recommender):
    def __init__(self, conf, trainingSet=None, testSet=None, fold="[1]"):
        super().__init__(conf, trainingSet, testSet, fold)

    def initModel(self):
        self.computeAverage()

    def computeAverage(self):
        d = self.data
        names = list(d.testSet_i)
        self.solver = SlopeOneSolver(d.item_rated_csr(), d.rated_csr(), np.array([d.item.get(i, -1) for i in names], dtype=np.int64))
        tpos = {i: k for k, i in enumerate(names)}
        rows = d.testData
        query = np.array([tpos[i] for _, i, _ in rows], dtype=np.int32)
        user = np.array([d.user.get(u, -1) for u, _, _ in rows], dtype=np.int32)
        base = np.array([d.userMeans[u] if u in d.user else (d.itemMeans[i] if i in d.item else d.globalMean) for u, i, _ in rows])
        pred, _ = self.solver.predict(query, user, base)
        self._test_pred = {(r[0], r[1]): p for r, p in zip(rows, pred.tolist())}
        for item in names:
            print("item " + item + " finished.")

    def predictForRating(self, u, i):
        hit = self._test_pred.get((u, i))
        if hit is not None:
            return hit
        return self._host_predict(u, i)

    def _host_predict(self, u, i):
        """the reference's predictForRating for one pair, its deviations taken on the host"""
        d = self.data
        if d.containsUser(u):
            x1 = d.sCol(i) if d.containsItem(i) else {}
            total, freqSum = 0, 0
            for item, rating in zip(*d.userRated(u)):
                x2 = d.sCol(item)
                diff, count = 0.0, 0
                for key in x1:
                    if key in x2:
                        diff += x1[key] - x2[key]
                        count += 1
                total += (rating + (diff / count if count else 0)) * count
                freqSum += count
            try:
                return float(total) / freqSum
            except ZeroDivisionError:
                return d.userMeans[u]
        if d.containsItem(i):
            return d.itemMeans[i]
        return d.globalMean
