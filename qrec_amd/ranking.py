"""Batched full-rank evaluation on the device (base/recommender.py:143-150,
util/qmath.py:134-146): scores by MFMA, rated items masked to 0, the reference's heap
top-N emulated lane-per-user.  ``DeviceRanker.topk`` returns ids/scores for many users at
once; nothing is computed on the host.  With ``set_test`` + ``cuts`` it also returns each user's hit count and
DCG sum (util/measure.py:15-21,70-82) from the lists while they are still on the device, so that the per-epoch
evaluation of the graph models never builds 31 k Python lists (0.8 s of host time per evaluation at the
Yelp2018 shape vs 10 ms of kernels)."""
from __future__ import annotations

import math

import numpy as np

from . import capi
from .capi import DeviceBuffer
from .interactions import CSR

_SCRATCH_BUDGET = 8 << 30   # bytes of transposed score block per batch (HBM is 288 GB)


class DeviceRanker:
    def __init__(self, U: np.ndarray, V: np.ndarray, rated: CSR | None = None):
        """U [users, d], V [items, d] host arrays of the same float dtype (fp64 for the
        numpy-path models, fp32 for the TF-path ones); ``rated`` = train items per user."""
        if U.dtype != V.dtype or U.dtype not in (np.float32, np.float64):
            raise TypeError("U and V must both be float32 or both float64")
        assert V.shape[1] == U.shape[1]
        slot = 16 if U.dtype == np.float64 else 32              # MFMA k-slot width of the scoring kernels
        self._init_state(U.dtype, U.shape[1], -(-U.shape[1] // slot) * slot, U.shape[0], V.shape[0], rated)
        self.dU = DeviceBuffer.from_numpy(self._pad(U))
        self.dV = DeviceBuffer.from_numpy(self._pad(V))

    def _init_state(self, dtype, d: int, ld: int, n_users: int, n_items: int, rated: CSR | None):
        """everything a ranker holds but its score tables (dU, dV); ``ld`` = zero-padded row stride (include/qrec_hip.h).
        Subclasses whose tables already sit on the device start here."""
        self.dtype = np.dtype(dtype)
        self.code = capi.F64 if self.dtype == np.float64 else capi.F32
        self.d, self.ld, self.n_users, self.n_items = d, ld, n_users, n_items
        self._scratch = self._d_ids = self._d_sc = None
        self._cap = (0, 0)
        self.rated = None
        self.test = None
        if rated is not None:
            rated = rated.sorted_rows()        # the fused route looks rated items up by bisection (include/qrec_hip.h)
            self.rated = (DeviceBuffer.from_numpy(rated.indptr.astype(np.int64)),
                          DeviceBuffer.from_numpy(rated.indices.astype(np.int32) if rated.indices.size else np.zeros(1, np.int32)))

    def _pad(self, a: np.ndarray) -> np.ndarray:
        if a.shape[1] == self.ld:
            return np.ascontiguousarray(a)
        out = np.zeros((a.shape[0], self.ld), dtype=self.dtype)
        out[:, :self.d] = a
        return out

    def update_tables(self, U: np.ndarray, V: np.ndarray):
        """New embeddings of the same shape/dtype (per-epoch evaluation): re-upload only."""
        if U.shape != (self.n_users, self.d) or V.shape != (self.n_items, self.d) or U.dtype != self.dtype or V.dtype != self.dtype:
            raise ValueError("update_tables: shape/dtype differ from the ranker's")
        self.dU.upload(self._pad(U)); self.dV.upload(self._pad(V))

    def set_test(self, test: CSR):
        """held-out items per user (CSR over ALL users of the table, ids ascending inside a row)"""
        srt = test.sorted_rows()
        if srt.indptr.size != self.n_users + 1:
            raise ValueError("set_test: the CSR must have one row per user of the table")
        self.test = (DeviceBuffer.from_numpy(srt.indptr.astype(np.int64)),
                     DeviceBuffer.from_numpy(srt.indices.astype(np.int32) if srt.indices.size else np.zeros(1, np.int32)))

    def _scratch_bytes(self, n_batch_users: int, N: int) -> int:
        return capi.score_topk_scratch_bytes(self.code, self.n_items, n_batch_users, self.ld, N)

    def _score_topk(self, d_users, n: int, N: int, scratch, d_ids, d_sc):
        capi.score_topk(self.dU, self.dV, self.code, self.d, self.ld, self.n_items, d_users, n,
                        self.rated[0] if self.rated else None, self.rated[1] if self.rated else None,
                        N, scratch, d_ids, d_sc)

    def topk(self, user_ids: np.ndarray, N: int, cuts=None, want_lists: bool = True):
        """(ids int32 [n, N], scores [n, N]) in the reference's order (descending score,
        heap order among ties).  With ``cuts`` (list of list lengths <= N; needs ``set_test``) a third
        value {cut: (hits int32 [n], dcg float64 [n])} comes back, computed from the device-resident lists;
        ``want_lists=False`` then skips the read-back of ids and scores."""
        user_ids = np.ascontiguousarray(user_ids, dtype=np.int32)
        n = user_ids.size
        ids = np.empty((n, N), dtype=np.int32) if want_lists else None
        scores = np.empty((n, N), dtype=self.dtype) if want_lists else None
        per_cut = None
        if cuts is not None:
            if self.test is None:
                raise RuntimeError("topk(cuts=...) needs set_test() first")
            if any(c < 1 or c > N for c in cuts):
                raise ValueError("cuts must lie in 1..N")
            per_cut = {c: (np.zeros(n, np.int32), np.zeros(n, np.float64)) for c in cuts}
            d_disc = DeviceBuffer.from_numpy(np.array([1.0 / math.log(pos + 2) for pos in range(N)], np.float64))
        if n == 0:
            return (ids, scores) if cuts is None else (ids, scores, per_cut)
        if user_ids.min() < 0 or user_ids.max() >= self.n_users:
            raise ValueError("user id out of range")
        # users per call: as many as the scratch budget allows (fused route: ~15 KB per user at the Yelp2018 shape,
        # block route: the whole score column, 150 KB)
        per_user = self._scratch_bytes(4096, N) // 4096
        batch = int(max(64, min(n, (_SCRATCH_BUDGET // max(per_user, 1)) // 64 * 64)))
        nb = min(batch, n)
        # kept across calls (per-epoch evaluation).  The byte count depends on the evaluation route the library picks from
        # QREC_EVAL_* at every call (bf16 copies, list capacity): it is asked again each time and the scratch re-made when the
        # cached one is too small for the route now in force
        need = self._scratch_bytes(nb, N)
        if self._cap[0] < nb or self._cap[1] != N or self._scratch.nbytes < need:
            self._scratch = DeviceBuffer(need, np.uint8)
            self._d_ids = DeviceBuffer((nb, N), np.int32); self._d_sc = DeviceBuffer((nb, N), self.dtype)
            self._cap = (nb, N)
        scratch, d_ids, d_sc = self._scratch, self._d_ids, self._d_sc
        if d_ids.shape[1] != N:                         # smaller N than the cached buffers: use exact-size views
            d_ids = DeviceBuffer((nb, N), np.int32); d_sc = DeviceBuffer((nb, N), self.dtype)
        for s in range(0, n, batch):
            chunk = user_ids[s:s + batch]
            d_users = DeviceBuffer.from_numpy(chunk)
            self._score_topk(d_users, chunk.size, N, scratch, d_ids, d_sc)
            if want_lists:
                ids[s:s + chunk.size] = d_ids.numpy()[:chunk.size]
                scores[s:s + chunk.size] = d_sc.numpy()[:chunk.size]
            if per_cut:
                d_hits, d_dcg = DeviceBuffer(chunk.size, np.int32), DeviceBuffer(chunk.size, np.float64)
                for c, (hits, dcg) in per_cut.items():
                    capi.rank_hits(d_ids, chunk.size, N, c, d_users, self.test[0], self.test[1], d_disc, d_hits, d_dcg)
                    hits[s:s + chunk.size] = d_hits.numpy(); dcg[s:s + chunk.size] = d_dcg.numpy()
        return (ids, scores) if cuts is None else (ids, scores, per_cut)


class SigmoidBiasRanker(DeviceRanker):
    """scores = sigmoid(V . U[user] + bias[item]), rated train items then set to 0 (CDAE.py:100-105 + base/recommender.py:147-149):
    the block route of the scoring with the element-wise pass in between (qrec_score_topk_sigmoid_bias).  The tables are the
    trainer's own device buffers -- hidden rows of ALL users [n_users][ld], the item-major decoder weight, the item bias; nothing
    is uploaded.  ``topk`` slices the users to the scratch budget as the base class does."""

    def __init__(self, d_U, d_V, d_bias, n_users: int, n_items: int, d: int, ld: int, rated: CSR | None = None):
        self._init_state(np.float32, d, ld, n_users, n_items, rated)
        self.dU, self.dV, self.d_bias = d_U, d_V, d_bias

    def update_tables(self, d_U, d_V, d_bias):
        self.dU, self.dV, self.d_bias = d_U, d_V, d_bias

    def _scratch_bytes(self, n_batch_users: int, N: int) -> int:
        return capi.score_topk_sigmoid_bias_scratch_bytes(self.n_items, n_batch_users)

    def _score_topk(self, d_users, n: int, N: int, scratch, d_ids, d_sc):
        capi.score_topk_sigmoid_bias(self.dU, self.dV, self.d_bias, self.d, self.ld, self.n_items, d_users, n,
                                     self.rated[0] if self.rated else None, self.rated[1] if self.rated else None, N, scratch, d_ids, d_sc)


class SparseRowSigmoidRanker(DeviceRanker):
    """scores = sigmoid(sum_i C[u,i] W[i] + bias) over the user's whole rating row, rated train items then set to 0 (CFGAN.py:129-134
    + base/recommender.py:147-149): the block route with its score block FILLED from the rated CSR with values
    (qrec_score_topk_sparse_row_sigmoid_bias) -- an SpMM against the trainer's own [n_items][ld] table; no users x items input is
    formed and nothing but the CSR is uploaded.  ``topk`` slices the users to the scratch budget as the base class does."""

    def __init__(self, d_W, d_bias, n_users: int, n_items: int, ld: int, rated: CSR):
        if rated is None or rated.values is None:
            raise ValueError("SparseRowSigmoidRanker: the rated CSR must carry the ratings")
        if rated.indptr.size != n_users + 1:
            raise ValueError("SparseRowSigmoidRanker: the CSR must have one row per user")
        self._init_state(np.float32, n_items, ld, n_users, n_items, rated)
        srt = rated.sorted_rows()
        self.d_vals = DeviceBuffer.from_numpy(srt.values.astype(np.float32) if srt.values.size else np.zeros(1, np.float32))
        self.dW, self.d_bias = d_W, d_bias

    def update_tables(self, d_W, d_bias):
        self.dW, self.d_bias = d_W, d_bias

    def _scratch_bytes(self, n_batch_users: int, N: int) -> int:
        return capi.score_topk_sparse_row_sigmoid_bias_scratch_bytes(self.n_items, n_batch_users)

    def _score_topk(self, d_users, n: int, N: int, scratch, d_ids, d_sc):
        capi.score_topk_sparse_row_sigmoid_bias(self.dW, self.d_bias, self.ld, self.n_items, d_users, n, self.rated[0], self.rated[1],
                                                self.d_vals, N, scratch, d_ids, d_sc)


class FormRanker(DeviceRanker):
    """The rating models whose ranking score is not one plain inner product -- SVD, SVDPlusPlus, EE, SREE, RSTE, SocialFD
    (their predictForRanking; include/qrec_hip.h, qrec_score_topk_form): the block route with the class's fp64 form as its scoring
    step, rated train items then set to 0 and the reference's heap top-N as everywhere else.

    ``form`` names the score (capi.RATING_*, or its name as engine.RatingEvaluator.FORMS spells it).  The ranker BINDS device
    buffers and copies none: ``tables`` (an engine.DeviceTables, fp64) and by keyword ``Bu`` / ``Bi`` (MfSgd.d_Bu / d_Bi), ``Y``
    with ``y_rated`` = (d_indptr, d_items) in userRated order (SvdppSgd), ``H`` (SocialHSgd.d_H), ``followees`` = (d_ptr, d_ids,
    d_w, d_den) with ``alpha`` (SocialSgd, RSTE); ``mu`` = the global mean, ``sign`` = +1 (EE, SREE rank by the distance itself)
    or -1 (SocialFD).  Its own buffer is the form's prepared item side (|Q[i]|^2, or Q.H and its norms), remade by
    ``update_tables`` -- call it whenever the bound tables have changed.  ``topk`` / ``set_test`` are the base class's."""
    FORMS = {"DOT": capi.RATING_DOT, "BIASED": capi.RATING_BIASED, "SVDPP": capi.RATING_SVDPP, "EUCLID": capi.RATING_EUCLID,
             "METRIC": capi.RATING_METRIC, "RSTE": capi.RATING_RSTE}

    def __init__(self, form, tables, rated: CSR | None = None, *, mu: float = 0.0, sign: float = 1.0, Bu=None, Bi=None, Y=None,
                 y_rated=None, H=None, followees=None, alpha: float = 0.0):
        self.form = self.FORMS[form] if isinstance(form, str) else int(form)
        if self.form not in self.FORMS.values():
            raise ValueError(f"unknown ranking form {form!r}")
        if tables.dtype != np.float64:
            raise ValueError("the form ranker runs on fp64 tables")
        if self.form == capi.RATING_METRIC and tables.d > capi.SOCIAL_H_MAX_D:
            raise ValueError(f"the METRIC form supports num.factors <= {capi.SOCIAL_H_MAX_D} (the d x d matrix H stays in LDS), got {tables.d}")
        if tables.ld % 16:
            raise ValueError(f"the form ranker needs a row stride that is a multiple of 16 doubles, got {tables.ld}")
        needs = {capi.RATING_BIASED: (Bu, Bi), capi.RATING_SVDPP: (Bu, Bi, Y, y_rated), capi.RATING_EUCLID: (Bu, Bi),
                 capi.RATING_METRIC: (Bu, Bi, H), capi.RATING_RSTE: (followees,)}.get(self.form, ())
        if any(x is None for x in needs):
            raise ValueError("the form's device buffers are missing (Bu/Bi, Y and y_rated, H or followees)")
        if self.form in (capi.RATING_EUCLID, capi.RATING_METRIC) and sign not in (1.0, -1.0):
            raise ValueError("sign must be +1 or -1")
        self._init_state(np.float64, tables.d, tables.ld, tables.n_users, tables.n_items, rated)
        self.t = tables
        self.mu, self.sign, self.alpha = float(mu), float(sign), float(alpha)
        self.d_Bu, self.d_Bi, self.d_Y, self.d_H = Bu, Bi, Y, H
        self.d_y = y_rated if y_rated is not None else (None, None)
        self.d_fe = followees if followees is not None else (None, None, None, None)
        self.prep_bytes = capi.rank_form_prepare_bytes(self.form, self.n_items, self.ld)
        self.d_prep = DeviceBuffer(self.prep_bytes, np.uint8) if self.prep_bytes else None
        self.update_tables()

    def update_tables(self, *_):
        """the bound tables have new values (an epoch ran): remake the prepared item side from them"""
        capi.rank_form_prepare(self.form, self.t.Q, self.d_H, self.d, self.ld, self.n_items, self.d_prep, self.prep_bytes)

    def _scratch_bytes(self, n_batch_users: int, N: int) -> int:
        return capi.score_topk_form_scratch_bytes(self.form, self.n_items, n_batch_users, self.ld, N)

    def _score_topk(self, d_users, n: int, N: int, scratch, d_ids, d_sc):
        capi.score_topk_form(self.form, self.sign, self.t.P, self.t.Q, self.d, self.ld, self.n_users, self.n_items, d_users, n,
                             self.rated[0] if self.rated else None, self.rated[1] if self.rated else None, N, scratch, scratch.nbytes,
                             d_ids, d_sc, mu=self.mu, d_Bu=self.d_Bu, d_Bi=self.d_Bi, d_Y=self.d_Y, d_y_indptr=self.d_y[0],
                             d_y_items=self.d_y[1], d_H=self.d_H, d_fe_indptr=self.d_fe[0], d_fe_ids=self.d_fe[1], d_fe_w=self.d_fe[2],
                             d_fe_den=self.d_fe[3], alpha=self.alpha, d_prep=self.d_prep, prep_bytes=self.prep_bytes)

    @classmethod
    def from_host(cls, form, P, Q, rated: CSR | None = None, *, mu: float = 0.0, sign: float = 1.0, Bu=None, Bi=None, Y=None,
                  y_rated: CSR | None = None, H=None, followees=None, alpha: float = 0.0):
        """the same ranker over host arrays, uploaded here (tests and tools); ``y_rated``: a CSR of every user's train items in
        userRated order, ``followees``: (ptr, ids, w, den) as social.followee_csr_by_user returns them"""
        from .engine import DeviceTables
        t = DeviceTables(np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64), np.float64)
        up = lambda a, dt: None if a is None else DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=dt) if np.size(a) else np.zeros(1, dt))
        kw = dict(mu=mu, sign=sign, alpha=alpha, Bu=up(Bu, np.float64), Bi=up(Bi, np.float64), H=up(H, np.float64))
        if Y is not None:
            kw["Y"] = DeviceBuffer.from_numpy(t._pad(np.asarray(Y, dtype=np.float64)))
            kw["y_rated"] = (up(y_rated.indptr, np.int64), up(y_rated.indices, np.int32))
        if followees is not None:
            ptr, ids, w, den = followees
            kw["followees"] = (up(ptr, np.int64), up(ids, np.int32), up(w, np.float64), up(den, np.float64))
        return cls(form, t, rated, **kw)


def ranking_measure_strings(test_lens, per_n: dict, Ns) -> list:
    """The strings of Measure.rankingMeasure (util/measure.py:24-49) from per-user hit counts and DCG sums:
    ``per_n[n] = (hits, dcg)`` sequences in testSet_u order, ``test_lens[k] = len(testSet_u[user_k])``.  Same
    operations in the same order as the reference: its ``sum()`` calls are left-to-right fp64 additions, which is what
    ``np.cumsum(...)[-1]`` computes (a scan, not numpy's pairwise ``sum``), so the digits are the same."""
    # (no interpreter-version guard here: the emulation is numpy's, its digits do not depend on what the running CPython's sum() does)
    out = []
    lens = np.asarray(test_lens, dtype=np.int64)
    n_users = lens.size
    for n in Ns:
        hits = np.asarray(per_n[n][0], dtype=np.int64); dcg = np.asarray(per_n[n][1], dtype=np.float64)
        prec = int(hits.sum()) / (n_users * n)                                   # exact integer sum
        rec = float(np.cumsum(hits / lens)[-1]) / n_users if n_users else 0.0
        f1 = 2 * prec * rec / (prec + rec) if (prec + rec) != 0 else 0
        prefix, acc = [0], 0
        for pos in range(n):
            acc += 1.0 / math.log(pos + 2)
            prefix.append(acc)
        idcg = np.asarray(prefix, dtype=np.float64)[np.minimum(lens, n)]
        ndcg = float(np.cumsum(dcg / idcg)[-1]) / n_users if n_users else 0.0
        out += ["Top " + str(n) + "\n", "Precision:" + str(prec) + "\n", "Recall:" + str(rec) + "\n",
                "F1:" + str(f1) + "\n", "NDCG:" + str(ndcg) + "\n"]
    return out
