"""The throughput mode's batch stream, stated from the oracle alone, and a way to make an EXACT-mode model train on it.

``QREC_MODE=throughput`` of the pairwise graph models draws every epoch on the device (DeepRecommender.iter_epoch_samples_device:
Philox permutation -> qrec_gather_pairs -> qrec_philox_bpr_sample; SGL / BUIR their sub-graphs too).  That stream is a pure function
of (QREC_SEED, epoch, stored rows), and the CPU oracle states each piece of it (oracle.c.philox_permutation, oracle.c.philox_bpr_sample,
oracle.tfmodels.philox_subgraph_rows).  ``predicted_epoch`` composes the pieces; ``replay_on_host`` feeds the composition to the exact
path (host upload per epoch, ordered reductions, host-built sub-graph CSR), so that the two modes can be compared on ONE stream."""
import contextlib
import sys

import numpy as np

from oracle import c as O
from oracle import tfmodels as T


def stored_rows(model):
    """(u0, i0): the training rows in stored order.  Exact mode shuffles ``trainingData`` in place every epoch, so the order is
    remembered the first time it is asked for -- ask before anything is drawn (the replay never shuffles)."""
    if not hasattr(model, "_stream_rows0"):
        u, i, _ = model.data.training_arrays()
        model._stream_rows0 = (np.ascontiguousarray(u, dtype=np.int32).copy(), np.ascontiguousarray(i, dtype=np.int32).copy())
    return model._stream_rows0


def predicted_epoch(model, seed: int, epoch: int):
    """(u, i, j) of epoch ``epoch`` as iter_epoch_samples_device draws it: rows in the order of permutation(n; seed, 2 epoch), one
    negative per row from stream 2 epoch + 1 (counter = position in the shuffled epoch)."""
    u0, i0 = stored_rows(model)
    perm = O.philox_permutation(u0.size, seed, 2 * epoch)
    u, i = np.ascontiguousarray(u0[perm]), np.ascontiguousarray(i0[perm])
    rated = model._rated_sorted()
    j = O.philox_bpr_sample(np.ascontiguousarray(rated.indptr, dtype=np.int64), np.ascontiguousarray(rated.indices, dtype=np.int32),
                            u, model.num_items, seed, 2 * epoch + 1)
    return u, i, j


def subgraph_stream_id(model, epoch: int, k: int) -> int:
    """the Philox stream id of the k-th sub-graph draw of an epoch (SGL._draw_subgraphs_device, BUIR._train_throughput)"""
    if hasattr(model, "SUBGRAPH_STREAM0"):                                   # SGL: node dropout takes two ids per draw
        n_draws = 2 if model.aug_type in (0, 1) else 2 * model.n_layers
        return model.SUBGRAPH_STREAM0 + 2 * n_draws * epoch + 2 * k
    return (1 << 32) + 2 * epoch + k                                         # BUIR: sub-graph O, T


def predicted_subgraph_rows(model, aug_type: int, drop_rate: float, seed: int, stream_id: int) -> np.ndarray:
    """the stored rows a device-drawn sub-graph keeps, ascending"""
    u0, i0 = stored_rows(model)
    return T.philox_subgraph_rows(model.num_users, model.num_items, u0, i0, aug_type, drop_rate, seed, stream_id)


@contextlib.contextmanager
def replay_on_host(model_cls, seed: int, epoch_shift: int = 0):
    """Inside the block an exact-mode ``model_cls`` instance consumes the device stream of ``seed`` instead of CPython's:
      * ``sample_epoch_pairwise`` returns ``predicted_epoch(self, seed, k)`` for its k-th call -- no shuffle of trainingData, no
        ``random`` draw;
      * the module's ``sample_subgraph_edges`` (SGL, BUIR) returns the rows the oracle keeps, the c-th call of the block with the
        c-th stream id the class uses in throughput mode;
      * the module's ``unique_first_appearance`` (SimGCL, SGL) returns ascending ids, the order qrec_unique_per_batch emits.
    Nothing else of the exact path changes.  One training run per block (the sub-graph draws are counted per block).
    ``epoch_shift`` is for showing that a paired test can fail: epoch k is fed epoch k + epoch_shift's stream."""
    mod = sys.modules[model_cls.__module__]
    calls = dict(sub=0)

    def sample_epoch_pairwise(self):
        stored_rows(self)
        k = self.__dict__.get("_replay_epoch", 0)
        self._replay_epoch = k + 1
        return predicted_epoch(self, seed, k + epoch_shift)

    def sample_subgraph_edges(state625, uid, iid, n_users, n_items, aug_type, drop_rate):
        if drop_rate <= 0:
            return uid, iid
        c = calls["sub"]; calls["sub"] = c + 1
        # SGL: SUBGRAPH_STREAM0 + 2 n_draws epoch + 2 k = SUBGRAPH_STREAM0 + 2 c;  BUIR: (1 << 32) + 2 epoch + k = (1 << 32) + c
        sid = model_cls.SUBGRAPH_STREAM0 + 2 * c if hasattr(model_cls, "SUBGRAPH_STREAM0") else (1 << 32) + c
        kept = T.philox_subgraph_rows(n_users, n_items, uid, iid, aug_type, drop_rate, seed, sid)
        return uid[kept], iid[kept]

    def unique_ascending(idx):
        return np.unique(idx)

    patches = [(model_cls, "sample_epoch_pairwise", sample_epoch_pairwise)]
    if hasattr(mod, "sample_subgraph_edges"):
        patches.append((mod, "sample_subgraph_edges", sample_subgraph_edges))
    if hasattr(mod, "unique_first_appearance"):
        patches.append((mod, "unique_first_appearance", unique_ascending))
    missing = object()
    saved = [(obj, name, obj.__dict__.get(name, missing)) for obj, name, _ in patches]
    for obj, name, new in patches:
        setattr(obj, name, new)
    try:
        yield calls
    finally:
        for obj, name, old in saved:
            if old is missing:
                delattr(obj, name)
            else:
                setattr(obj, name, old)


# ---- the two modes on one stream ---------------------------------------------------------------------------------------------------
PAIRED_BATCH = 2045          # FilmTrust golden rows: 32,736 = 16 x 2045 + 16 -- the 17th batch of an epoch has 16 rows, less than one workgroup


@contextlib.contextmanager
def _environ(**kv):
    import os
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def paired_conf(name: str, epochs: int, aug: int = 1):
    """the conf of test_throughput_mode_of_the_pairwise_models_draws_its_batches_on_the_device (FilmTrust golden rows, d = 16, lr 0.002,
    top-10) with a batch size that leaves a short last batch"""
    from helpers import conf_from_text, load_golden, rows_from_golden
    meta, _ = load_golden("pairwise_adj_filmtrust")
    train, test = rows_from_golden(load_golden("bpr_filmtrust")[1])
    conf = conf_from_text(meta["conf"]); conf["model.name"] = name; conf["num.max.epoch"] = str(epochs); conf["num.factors"] = "16"
    conf["item.ranking"] = "on -topN 10"; conf["learnRate"] = "-init 0.002 -max 1"; conf["batch_size"] = str(PAIRED_BATCH)
    conf["SimGCL"] = "-n_layer 2 -lambda 0.5 -eps 0.1"
    conf["SGL"] = f"-n_layer 2 -lambda 0.1 -droprate 0.1 -augtype {aug} -temp 0.2"
    conf["BUIR"] = "-n_layer 2 -tau 0.995 -drop_rate 0.5"
    assert len(train) % PAIRED_BATCH not in (0,) and len(train) % PAIRED_BATCH < 64
    return conf, train, test


def final_tables(m) -> dict:
    if hasattr(m, "ranking_tables") and hasattr(m, "q_user"):                # BUIR
        U, V = m.ranking_tables()
    elif hasattr(m, "bestU"):                                                # SimGCL, SGL: the best epoch's tables
        U, V = m.bestU, m.bestV
    else:
        U, V = m.U, m.V
    return dict(U=np.ascontiguousarray(U), V=np.ascontiguousarray(V))


def run_mode(name, conf, train, test, mode: str, seed: int, reductions=None, epoch_shift: int = 0) -> dict:
    """one training run of the drop-in class: ``throughput`` draws its stream on the device, ``exact`` replays the SAME stream on the host
    (replay_on_host).  QREC_SEED = seed in both (NGCF's dropout and SimGCL's noise take the trainer seed from it), numpy seed 3 for the
    initial tables.  ``reductions``: "ordered" / "atomic" (QREC_REDUCTIONS) or None = the mode's own choice.
    Returns the final tables, the measure strings and the four measures (Precision, Recall, F1, NDCG)."""
    import io
    import random
    from contextlib import redirect_stdout
    from qrec_amd.QRec import resolve_model
    cls = resolve_model(name)
    replay = replay_on_host(cls, seed, epoch_shift) if mode == "exact" else contextlib.nullcontext()
    with _environ(QREC_MODE=mode, QREC_SEED=seed, QREC_REDUCTIONS=reductions, QREC_QUIET=1), replay, redirect_stdout(io.StringIO()):
        state = random.getstate()
        np.random.seed(3)
        m = cls(conf, train, test)
        measure = m.execute()
        assert m.throughput_mode() == (mode == "throughput")
        assert random.getstate() == state                                    # neither run consumes CPython's generator
    out = final_tables(m)
    out["measure"] = np.frombuffer("\n".join(measure).encode(), dtype=np.uint8)
    return dict(arrays=out, values=[float(x.split(":")[1]) for x in measure if ":" in x])


def table_distance(a: dict, b: dict) -> float:
    """max |A - B| / max |B| over the final tables"""
    return max(float(np.max(np.abs(a[k].astype(np.float64) - b[k])) / max(float(np.max(np.abs(b[k]))), 1e-300)) for k in ("U", "V"))


def bytes_differing(a: dict, b: dict) -> int:
    return sum(int(np.count_nonzero(a[k].view(np.uint8) != b[k].view(np.uint8))) if a[k].shape == b[k].shape else max(a[k].nbytes, b[k].nbytes)
               for k in a)
