"""tests/device_stream.py without a GPU: the predicted throughput-mode stream has the properties a batch stream must have, and
``replay_on_host`` makes an exact-mode instance consume it -- and nothing else -- and takes itself back out."""
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

from device_stream import predicted_epoch, predicted_subgraph_rows, replay_on_host, stored_rows, subgraph_stream_id
from helpers import conf_from_text, load_golden, rows_from_golden
from oracle import c as O
from oracle import tfmodels as T


def _model(name, **extra):
    from qrec_amd.QRec import resolve_model
    meta, _ = load_golden("pairwise_adj_filmtrust")
    train, test = rows_from_golden(load_golden("bpr_filmtrust")[1])
    conf = conf_from_text(meta["conf"]); conf["model.name"] = name
    for k, v in extra.items():
        conf[k] = v
    cls = resolve_model(name)
    with redirect_stdout(io.StringIO()):
        m = cls(conf, train, test)
        m.readConfiguration()
    return cls, m


@pytest.mark.parametrize("seed", [0, 5, 2 ** 40 + 3])
def test_predicted_stream_is_a_shuffle_of_the_rows_with_unrated_negatives(seed):
    _, m = _model("LightGCN")
    random.seed(11)
    state = random.getstate()
    u0, i0 = stored_rows(m)
    want = np.sort(u0.astype(np.int64) * m.num_items + i0)
    rated = m.data.rated_csr()
    is_rated = np.zeros((m.num_users, m.num_items), bool); is_rated[rated.row_ids(), rated.indices] = True
    epochs = [predicted_epoch(m, seed, k) for k in (0, 1, 2, 2 ** 32 + 1)]
    for u, i, j in epochs:
        assert u.dtype == i.dtype == j.dtype == np.int32 and u.size == i.size == j.size == u0.size
        assert np.array_equal(np.sort(u.astype(np.int64) * m.num_items + i), want)            # a permutation of the training rows
        assert ((j >= 0) & (j < m.num_items)).all() and not is_rated[u, j].any()              # negatives exist and are unrated
        assert not np.array_equal(u, u0)                                                      # shuffled
    for a in range(len(epochs)):
        for b in range(a + 1, len(epochs)):
            assert not np.array_equal(epochs[a][0], epochs[b][0]) and not np.array_equal(epochs[a][2], epochs[b][2])
    again = predicted_epoch(m, seed, 1)
    assert all(np.array_equal(x, y) for x, y in zip(again, epochs[1]))                        # a function of (seed, epoch)
    other = predicted_epoch(m, seed + 1, 1)
    assert not np.array_equal(other[0], epochs[1][0])
    assert random.getstate() == state                                                         # CPython's generator is not consumed
    # the composition, spelled out once more from the pieces
    perm = O.philox_permutation(u0.size, seed, 4)
    assert np.array_equal(epochs[2][0], u0[perm]) and np.array_equal(epochs[2][1], i0[perm])
    rs = m._rated_sorted()
    assert np.array_equal(epochs[2][2], O.philox_bpr_sample(rs.indptr.astype(np.int64), rs.indices.astype(np.int32), np.ascontiguousarray(u0[perm]), m.num_items, seed, 5))


def test_replay_feeds_the_exact_path_the_predicted_stream_and_restores_what_it_patched():
    from qrec_amd.base.deepRecommender import DeepRecommender
    cls, m = _model("LightGCN")
    assert "sample_epoch_pairwise" not in cls.__dict__
    order0 = [tuple(r[:2]) for r in m.data.trainingData]
    random.seed(4)
    state = random.getstate()
    with replay_on_host(cls, 5):
        got = [m.sample_epoch_pairwise() for _ in range(3)]
        batches = list(m.next_batch_pairwise())                                               # the reference-shaped generator goes through it too (epoch 3)
    for k, g in enumerate(got):
        assert all(np.array_equal(x, y) for x, y in zip(g, predicted_epoch(m, 5, k)))
    assert np.array_equal(np.concatenate([b[0] for b in batches]), predicted_epoch(m, 5, 3)[0])
    assert random.getstate() == state                                                         # no shuffle, no choice()
    assert [tuple(r[:2]) for r in m.data.trainingData] == order0                              # trainingData keeps its stored order
    assert "sample_epoch_pairwise" not in cls.__dict__ and cls.sample_epoch_pairwise is DeepRecommender.sample_epoch_pairwise
    # a second instance starts at epoch 0 again; a shifted replay is a different stream
    _, m2 = _model("LightGCN")
    with replay_on_host(cls, 5, epoch_shift=1):
        shifted = m2.sample_epoch_pairwise()
    assert np.array_equal(shifted[0], got[1][0]) and not np.array_equal(shifted[0], got[0][0])


@pytest.mark.parametrize("name,extra,aug", [("SGL", {"SGL": "-n_layer 2 -lambda 0.1 -droprate 0.2 -augtype 0 -temp 0.2"}, 0),
                                            ("SGL", {"SGL": "-n_layer 2 -lambda 0.1 -droprate 0.2 -augtype 1 -temp 0.2"}, 1),
                                            ("SGL", {"SGL": "-n_layer 2 -lambda 0.1 -droprate 0.2 -augtype 2 -temp 0.2"}, 2),
                                            ("BUIR", {"BUIR": "-n_layer 2 -tau 0.995 -drop_rate 0.2"}, 1)])
def test_replay_draws_the_subgraphs_and_batch_uniques_the_device_would(name, extra, aug):
    import sys
    cls, m = _model(name, **extra)
    mod = sys.modules[cls.__module__]
    orig_sub, orig_unique = mod.sample_subgraph_edges, getattr(mod, "unique_first_appearance", None)
    u0, i0 = stored_rows(m)
    n_draws = 2 if name == "BUIR" or aug in (0, 1) else 2 * m.n_layers
    random.seed(9)
    state = random.getstate()
    with replay_on_host(cls, 7) as calls:
        for epoch in range(2):
            subs, rest = m._draw_epoch()
            pairs = rest if name == "BUIR" else rest[:3]
            assert all(np.array_equal(x, y) for x, y in zip(pairs, predicted_epoch(m, 7, epoch)))
            flat = list(subs) if not isinstance(subs[0], list) else [s for pair in zip(*subs) for s in pair]     # draw order: per layer view 1, view 2
            assert len(flat) == n_draws and calls["sub"] == n_draws * (epoch + 1)
            for k, adj in enumerate(flat):
                sid = subgraph_stream_id(m, epoch, k)
                kept = predicted_subgraph_rows(m, aug, 0.2, 7, sid)
                want = T.joint_norm_adjacency(m.num_users, m.num_items, u0[kept], i0[kept])
                want.sort_indices()
                assert np.array_equal(adj[0], want.indptr) and np.array_equal(adj[1], want.indices), (epoch, k)
                assert np.array_equal(np.asarray(adj[2]).view(np.uint32), want.data.view(np.uint32)), (epoch, k)
            if name == "SGL":
                u, i, _, starts, rows, off = rest
                step = m._step_rows()
                for b, s in enumerate(starts):
                    want_rows = np.concatenate([np.unique(u[s:s + step]), np.unique(i[s:s + step]) + m.num_users])
                    assert np.array_equal(rows[off[b]:off[b + 1]], want_rows)
    assert random.getstate() == state
    assert mod.sample_subgraph_edges is orig_sub and getattr(mod, "unique_first_appearance", None) is orig_unique
    # the stream ids of two epochs never collide with each other or with the batch stream's 2 * epoch (+ 1)
    ids = [subgraph_stream_id(m, e, k) + d for e in range(50) for k in range(n_draws) for d in ((0, 1) if aug == 0 else (0,))]
    assert len(set(ids)) == len(ids) and min(ids) >= 1 << 32
