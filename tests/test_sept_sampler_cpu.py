"""Host side of SEPT's device-drawn perturbed graph (qrec_amd.graph.SeptUnionStructure, the base of SeptGraphSampler): the fixed union
structure R + R^T + F every epoch's graph lives in, the positions the kernel scatters through, the transposition map the backward pass's
M^T comes from, the degree table and the keep-list sizes -- against the oracle's get_adj_mat (oracle.tfmodels.sept_sub_adjacency).  No
device is touched."""
import numpy as np
import pytest

from oracle import tfmodels as T

from sept_cases import CASES, case


@pytest.fixture(scope="module", params=sorted(CASES))
def problem(request):
    from qrec_amd.graph import SeptUnionStructure
    nu, ni, uid, iid, fo, fe = case(request.param)
    return nu, ni, uid, iid, fo, fe, SeptUnionStructure(nu, ni, uid, iid, fo, fe)


def _rows(indptr):
    return np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))


def test_case_a_has_the_edge_cases_it_is_there_for():
    nu, ni, uid, iid, fo, fe = case("A")
    pairs = list(zip(fo.tolist(), fe.tolist()))
    assert len(set(zip(uid.tolist(), iid.tolist()))) < uid.size and len(set(pairs)) < len(pairs)       # duplicated rows, duplicated pairs
    assert any(a == b for a, b in pairs)                                                                # a self-follow
    assert set(range(nu)) - set(fo.tolist())                                                            # users who follow nobody
    assert set(fe.tolist()) - set(fo.tolist())                                                          # users who are only followed


def test_union_structure_is_sorted_and_holds_every_position(problem):
    nu, ni, uid, iid, fo, fe, s = problem
    n = nu + ni
    assert (s.nu, s.ni, s.n, s.n_edges, s.n_pairs) == (nu, ni, n, uid.size, fo.size)
    assert s.indptr.dtype == np.int64 and s.indices.dtype == np.int32 and s.indptr.size == n + 1 and s.indptr[0] == 0 and s.indptr[-1] == s.nnz == s.indices.size
    r = _rows(s.indptr)
    keys = r * n + s.indices
    assert np.all(np.diff(keys) > 0)                                         # rows ascending, columns strictly ascending inside a row
    assert np.array_equal(s.row_of, r)
    # exactly the pattern of R + R^T + F
    want = np.unique(np.concatenate([uid.astype(np.int64) * n + nu + iid, (nu + iid.astype(np.int64)) * n + uid, fo.astype(np.int64) * n + fe]))
    assert np.array_equal(keys, want)
    # every row's two positions and every pair's one point at the right (row, col)
    assert np.array_equal(r[s.pos_ui], uid) and np.array_equal(s.indices[s.pos_ui], nu + iid)
    assert np.array_equal(r[s.pos_iu], nu + iid) and np.array_equal(s.indices[s.pos_iu], uid)
    assert np.array_equal(r[s.pos_f], fo) and np.array_equal(s.indices[s.pos_f], fe)
    assert s.pos_ui.dtype == s.pos_iu.dtype == s.pos_f.dtype == s.pos_t.dtype == np.int32


def test_transposition_map_is_a_bijection_onto_the_transposed_csr(problem):
    nu, ni, uid, iid, fo, fe, s = problem
    n = nu + ni
    assert np.array_equal(np.sort(s.pos_t), np.arange(s.nnz))
    rt = _rows(s.indptr_t)
    assert s.indptr_t[-1] == s.nnz and np.all(np.diff(rt * n + s.indices_t) > 0)                         # the transposed structure is sorted too
    # entry e = (r, c) lands at an entry (c, r) of the transposed CSR
    r = _rows(s.indptr)
    assert np.array_equal(rt[s.pos_t], s.indices) and np.array_equal(s.indices_t[s.pos_t], r)
    # and the transposed structure is scipy's transpose of the pattern
    import scipy.sparse as sp
    P = sp.csr_matrix((np.ones(s.nnz, np.float32), s.indices, s.indptr), shape=(n, n)).T.tocsr(); P.sort_indices()
    assert np.array_equal(P.indptr, s.indptr_t) and np.array_equal(P.indices, s.indices_t)


@pytest.mark.parametrize("rate", [0.3, 0.97])
def test_structure_contains_every_perturbed_graph_and_scattering_through_the_positions_rebuilds_it(problem, rate):
    """random keep lists: the oracle's matrix has no entry outside the structure, and the kernel's arithmetic carried out with numpy over
    the structure -- counts through the positions, weights squared in the user-user block, integer row sums, the float32 table -- gives the
    oracle's values bit for bit, the transposed array the oracle's transpose"""
    from sept_stream import values_on_structure
    nu, ni, uid, iid, fo, fe, s = problem
    rng = np.random.default_rng(int(rate * 100) + nu)
    k, sk = s.sizes(rate)
    assert (k, sk) == (int(uid.size * (1 - rate)), int(fo.size * (1 - rate)))                            # SEPT.py:85,91
    keep, skeep = rng.permutation(uid.size)[:k], rng.permutation(fo.size)[:sk]
    M = T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe, keep, skeep)
    want = values_on_structure(M, s.indptr, s.indices)                                                  # raises if M leaves the structure
    want_t = values_on_structure(M.T, s.indptr_t, s.indices_t)
    cnt = np.zeros(s.nnz, np.int64)
    np.add.at(cnt, s.pos_ui[keep], 1); np.add.at(cnt, s.pos_iu[keep], 1); np.add.at(cnt, s.pos_f[skeep], 1)
    r = _rows(s.indptr)
    a = np.where((r < nu) & (s.indices < nu), cnt * cnt, cnt)
    deg = np.bincount(r, weights=a, minlength=nu + ni).astype(np.int64)
    assert deg.max() <= s.max_deg
    got = ((s.dinv[deg[r]] * a.astype(np.float32)).astype(np.float32) * s.dinv[deg[s.indices]]).astype(np.float32)
    got[cnt == 0] = 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got_t = np.empty_like(got); got_t[s.pos_t] = got
    assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32))


def test_degree_table_reaches_the_full_graphs_largest_weighted_row_sum(problem):
    nu, ni, uid, iid, fo, fe, s = problem
    import scipy.sparse as sp
    n = nu + ni
    R = sp.csr_matrix((np.ones(uid.size), (uid, nu + iid)), shape=(n, n))
    F = sp.csr_matrix((np.ones(fo.size), (fo, fe)), shape=(n, n))
    full = R + R.T + F.multiply(F)                                           # every row and every pair kept
    assert s.max_deg == int(np.asarray(full.sum(1)).max())
    assert s.dinv.dtype == np.float32 and s.dinv.size == s.max_deg + 1 and s.dinv[0] == 0
    with np.errstate(divide="ignore"):
        assert np.array_equal(s.dinv[1:], np.power(np.arange(1, s.max_deg + 1, dtype=np.float32), -0.5))


def test_replay_feeds_the_exact_path_the_predicted_perturbed_graph_and_restores_what_it_patched(tmp_path):
    """tests/sept_stream.py without a GPU: inside replay_on_host an exact-mode SEPT's _draw_epoch returns the throughput mode's batch stream,
    ascending unique users and -- in the joint epochs -- the oracle's perturbed graph of that epoch's predicted keep lists; CPython's
    generator and the order of trainingData stay where they were."""
    import io
    import random
    import sys
    from contextlib import redirect_stdout
    import sept_stream as SS
    from device_stream import predicted_epoch, stored_rows
    from qrec_amd.model.ranking.SEPT import SEPT
    from qrec_amd.util.io import FileIO
    conf, train, test, trust = SS.social_problem("SEPT", tmp_path, epochs=6, extra="-n_layer 2 -ss_rate 0.005 -drop_rate 0.3 -ins_cnt 5")
    with redirect_stdout(io.StringIO()):
        m = SEPT(conf, train, test, FileIO.loadRelationship(conf, trust))
        m.readConfiguration()
    m._epochs_drawn = 0                                                      # initModel's (the trainer it builds needs the device)
    mod = sys.modules[SEPT.__module__]
    saved = (mod.sept_perturbed_adjacency, mod.unique_first_appearance, SEPT.get_adj_mat)
    u0, i0 = stored_rows(m)
    fo, fe = m.relation_ids()
    random.seed(9)
    state = random.getstate()
    with SS.replay_on_host(SEPT, 7) as calls:
        for epoch in range(6):
            sub, u, i, j, starts, uu, off = m._draw_epoch()
            assert all(np.array_equal(x, y) for x, y in zip((u, i, j), predicted_epoch(m, 7, epoch)))
            if epoch <= 6 / 3:
                assert sub is None and uu.size == 0
                continue
            keep, skeep = SS.predicted_keep_lists(m, 7, epoch)
            assert (keep.size, skeep.size) == (int(u0.size * 0.7), int(len(fo) * 0.7))
            assert np.array_equal(keep, SS.keep_lists(u0.size, len(fo), 0.3, 7, (1 << 32) + 2 * epoch)[0])
            want = T.sept_sub_adjacency(m.num_users, m.num_items, u0, i0, fo, fe, keep, skeep)
            assert (abs(sub - want)).nnz == 0 and sub.dtype == np.float32
            step = m._step_rows()
            for b, s in enumerate(starts):
                assert np.array_equal(uu[off[b]:off[b + 1]], np.unique(u[s:s + step]))
        assert calls["sub"] == 3
    assert random.getstate() == state
    assert (mod.sept_perturbed_adjacency, mod.unique_first_appearance, SEPT.get_adj_mat) == saved
    # two epochs' graphs differ, and a shifted replay draws the next epoch's
    a, b = SS.predicted_perturbed_adjacency(m, 7, 3), SS.predicted_perturbed_adjacency(m, 7, 4)
    assert (abs(a - b)).nnz > 0
    m._epochs_drawn = 3; m.__dict__.pop("_replay_epoch", None)
    with SS.replay_on_host(SEPT, 7, epoch_shift=1):
        assert (abs(m._draw_epoch()[0] - b)).nnz == 0


def test_sizes_are_the_references_truncations(problem):
    s = problem[-1]
    for rate in (0.3, 0.97, 0.1, 0.5, 0.7):
        assert s.sizes(rate) == (int(s.n_edges * (1 - rate)), int(s.n_pairs * (1 - rate)))
    assert s.sizes(0.0) == (s.n_edges, s.n_pairs)
