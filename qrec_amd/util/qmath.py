"""Host math helpers (util/qmath.py:19-32,58-76,127-146)."""
from __future__ import annotations

import heapq
from math import exp, sqrt


def sigmoid(val: float) -> float:
    return 1 / (1 + exp(-val))


def find_k_largest(K: int, candidates):
    """Top-K by the reference's procedure: a min-heap of ``(score, id)`` seeded with the
    first K entries, strict ``>`` replacement, then a stable descending sort by score
    (util/qmath.py:134-146).  Kept on the host for odd cases (ties at the cut, cold users);
    the batched device path is qrec_amd.ranking."""
    heap = [(score, iid) for iid, score in enumerate(candidates[:K])]
    heapq.heapify(heap)
    for iid in range(K, len(candidates)):
        score = candidates[iid]
        if score > heap[0][0]:
            heapq.heapreplace(heap, (score, iid))
    heap.sort(key=lambda pair: pair[0], reverse=True)
    return [iid for _, iid in heap], [score for score, _ in heap]


def pearson_sp(x1: dict, x2: dict) -> float:
    """Pearson correlation of two rating dicts over their common keys, each centred on its OWN full mean
    (util/qmath.py:58-76): summed in x1's key order, squares by Python's ``** 2``; a zero denominator gives 1 when the
    dicts overlap and 0 otherwise (so does an empty dict)."""
    total = denom1 = denom2 = 0
    overlapped = False
    try:
        mean1 = sum(x1.values()) / len(x1)
        mean2 = sum(x2.values()) / len(x2)
        for k in x1:
            if k in x2:
                a, b = x1[k] - mean1, x2[k] - mean2
                total += a * b
                denom1 += a ** 2
                denom2 += b ** 2
                overlapped = True
        return total / (sqrt(denom1) * sqrt(denom2))
    except ZeroDivisionError:
        return 1 if overlapped else 0


def cosine_sp(x1: dict, x2: dict) -> float:
    """Cosine of two rating dicts over their common keys only -- both norms run over the overlap, not over the whole
    dicts (util/qmath.py:19-32): summed in x1's key order, squares by Python's ``** 2``; no overlap gives 0."""
    total = denom1 = denom2 = 0
    try:
        for k in x1:
            if k in x2:
                total += x1[k] * x2[k]
                denom1 += x1[k] ** 2
                denom2 += x2[k] ** 2
        return total / (sqrt(denom1) * sqrt(denom2))
    except ZeroDivisionError:
        return 0
