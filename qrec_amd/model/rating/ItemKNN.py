"""ItemKNN behind the reference's class name, conf keys and printed lines (model/rating/ItemKNN.py): UserKNN's contract on
the item side (``sCol``, ``testSet_i``, ``data.item``, ``itemMeans``; a neighbour item counts when the user rated it), on the
MI355X in fp64 (engine.CoRatingKnn, knn.hip).  Departures as UserKNN's: ``topItems[i]`` holds the first ``num.neighbors``
entries only, ``itemSim`` is not materialised.  ``QREC_MODE`` does not apply.
"""
from __future__ import annotations

from ._knn import KnnRatingModel


class ItemKNN(KnnRatingModel):
    side = "item"
