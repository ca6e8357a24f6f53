"""UserKNN behind the reference's class name, conf keys and printed lines (model/rating/UserKNN.py), with the co-rating
sweep, the neighbour selection and the predictions on the MI355X in fp64 (engine.CoRatingKnn, knn.hip).

What the reference computes, and so what this class computes:
  * ``qmath.similarity(sRow(x1), sRow(x2), similarity)`` -- ``pcc``, ``euclidean``, anything else cosine -- summed over x1's
    keys in dict order, every product and sum rounded on its own;
  * ``topUsers[q]``: the stable sort (descending) of q's row of the reference's ``SymmetricMatrix`` -- the earlier test users
    first (their value with the earlier user as x1), then the other training users in id order;
  * ``predictForRating``: the first ``num.neighbors`` neighbours that rated the item, ``userMeans[u] + sum / denom``, else
    ``userMeans[u]`` (or ``globalMean``); a zero ``denom`` with a non-zero sum raises ZeroDivisionError, as there.
Departures: ``topUsers[q]`` holds the first ``num.neighbors`` entries only (the rest are never read) and ``userSim`` is not
materialised (``self.knn.similarities()`` reads the rows).  The test rows' predictions are computed on the device in one
pass; another (user, item) pair of a test user is predicted on the host from ``topUsers``.  ``num.neighbors`` above
``capi.KNN_MAX_K`` raises ValueError.  ``QREC_MODE`` does not apply: the kernels are the reference's arithmetic.
"""
from __future__ import annotations

from ._knn import KnnRatingModel


class UserKNN(KnnRatingModel):
    side = "user"
