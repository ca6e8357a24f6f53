"""SEPT and MHCN in throughput mode (QREC_MODE=throughput): nothing of an epoch on the host.

SEPT's per-epoch perturbed joint graph (model/ranking/SEPT.py:84-111) is drawn on the device as two value arrays -- M and M^T -- over a
fixed union structure (csrc/augment.hip qrec_sept_perturbed_values, qrec_amd.graph.SeptGraphSampler).  The checker is the oracle:
oracle.c.philox_permutation for the keep lists, oracle.tfmodels.sept_sub_adjacency (bit-identical to the reference's own scipy arithmetic,
tests/test_oracle_golden.py) for the values; the device result is held to it BIT FOR BIT.  The classes are compared against their exact
mode fed the same stream (tests/sept_stream.py)."""
import numpy as np
import pytest

from oracle import tfmodels as T
from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.graph import SEPTTrainer, SeptGraphSampler, SpmmPlan, _View, ordered_reductions

import device_stream as DS
import sept_stream as SS
from helpers import check, check_rel, load_golden, pad_cols, rel_err, same_bits
from sept_cases import case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    yield


def _words_differ(a, b):
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)))


def _filmtrust():
    meta, z = load_golden("sept_graphs_filmtrust")
    return meta["n_users"], meta["n_items"], z["train_uid"], z["train_iid"], z["follower"], z["followee"]


_PROBLEMS = {}


def _problem(data):
    """(nu, ni, uid, iid, fo, fe, sampler, joint adjacency on the structure): built once per data set, left unchanged"""
    if data not in _PROBLEMS:
        nu, ni, uid, iid, fo, fe = _filmtrust() if data == "filmtrust" else case(data)
        smp = SeptGraphSampler(nu, ni, uid, iid, fo, fe)
        full = SS.values_on_structure(T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe), smp.indptr, smp.indices)
        _PROBLEMS[data] = (nu, ni, uid, iid, fo, fe, smp, full)
    return _PROBLEMS[data]


# ---- 1. value parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.0, 0.3, 0.97])
@pytest.mark.parametrize("data", ["A", "B", "filmtrust"])
def test_device_perturbed_values_equal_the_oracle_bit_for_bit(data, rate):
    nu, ni, uid, iid, fo, fe, smp, full = _problem(data)
    out, out_t = DB(max(smp.nnz, 1), np.float32), DB(max(smp.nnz, 1), np.float32)
    for seed, sid in ((7, (1 << 32) + 4), (2 ** 40 + 3, 11)):
        got, got_t = (b.numpy()[:smp.nnz].copy() for b in smp.draw(rate, seed, sid, out, out_t))
        what = f"device perturbed graph vs the oracle (rate {rate}, {data})"
        if rate > 0:
            keep, skeep = SS.keep_lists(uid.size, fo.size, rate, seed, sid)
            assert (keep.size, skeep.size) == smp.sizes(rate) == (int(uid.size * (1 - rate)), int(fo.size * (1 - rate)))    # SEPT.py:85,91
            assert np.array_equal(smp.d_keep.numpy()[:keep.size], keep) and np.array_equal(smp.d_skeep.numpy()[:skeep.size], skeep)
            M = T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe, keep, skeep)
        else:
            M = T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe)
        check(f"{what}: 32-bit words of M that differ", _words_differ(got, SS.values_on_structure(M, smp.indptr, smp.indices)), 0, inclusive=True)
        check(f"{what}: 32-bit words of M^T that differ", _words_differ(got_t, SS.values_on_structure(M.T, smp.indptr_t, smp.indices_t)), 0, inclusive=True)
        # a pure function of (seed, stream id): the same bytes again, other bytes for another stream id
        again, again_t = (b.numpy()[:smp.nnz] for b in smp.draw(rate, seed, sid))
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(again_t.view(np.uint32), got_t.view(np.uint32))
        if rate > 0:
            other = smp.draw(rate, seed, sid + 2)[0].numpy()[:smp.nnz]
            assert _words_differ(other, got) > 0
    if rate == 0.0:                                                                   # SEPT.py:98-103: the plain joint adjacency, no follow entries
        uu = (smp.row_of < nu) & (smp.indices < nu)
        assert not got[uu].any()
        check(f"rate 0 ({data}): words that differ from the joint adjacency's values", _words_differ(got, full), 0, inclusive=True)


# ---- 2. the ABI's argument checks --------------------------------------------------------------------------------------------------
def test_sept_perturbed_values_refuses_bad_arguments_and_handles_empty_graphs():
    nu, ni, uid, iid, fo, fe, smp, _ = _problem("A")
    lib = capi.load()
    out, out_t = DB(smp.nnz, np.float32), DB(smp.nnz, np.float32)
    out.upload(np.full(smp.nnz, 7, np.float32))
    smp.draw(0.3, 1, 2)                                                               # the keep lists hold a permutation's prefix

    def call(keep=smp.d_keep.ptr, n_keep=5, skeep=smp.d_skeep.ptr, n_skeep=5, nnz=smp.nnz, values=out.ptr, pos_t=smp.d_pos_t.ptr):
        return lib.qrec_sept_perturbed_values(smp.d_pos_ui.ptr, smp.d_pos_iu.ptr, smp.n_edges, smp.d_pos_f.ptr, smp.n_pairs, keep, n_keep, skeep, n_skeep,
                                              nu, ni, smp.d_indptr.ptr, smp.d_row_of.ptr, smp.d_indices.ptr, pos_t, nnz, smp.d_dinv.ptr, smp.max_deg,
                                              smp.d_cnt.ptr, smp.d_deg.ptr, values, out_t.ptr, None)

    msg = lambda: lib.qrec_last_error().decode()
    assert call(values=None) < 0 and "null" in msg() and len(msg()) > 20
    assert call(pos_t=None) < 0 and "null" in msg()
    assert call(n_keep=smp.n_edges + 1) < 0 and "keep" in msg()
    assert call(n_skeep=smp.n_pairs + 1) < 0 and "keep" in msg()
    assert call(skeep=None) < 0 and "keep" in msg()                                  # a count without its list
    assert call(n_keep=-1) < 0
    assert call(nnz=2 ** 31) < 0 and "2^31" in msg()
    capi.device_sync()
    assert np.all(out.numpy() == 7)                                                   # a refused call wrote nothing
    assert call() == 0
    # zero edges and zero pairs: an empty structure, nothing to write
    empty = SeptGraphSampler(5, 4, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert (empty.nnz, empty.max_deg, empty.sizes(0.3)) == (0, 0, (0, 0))
    for rate in (0.0, 0.3):
        empty.draw(rate, 1, 2)
    # pairs but no rows: only the user-user block
    none, pfo, pfe = np.zeros(0, np.int32), np.array([0, 1, 1, 4], np.int32), np.array([1, 0, 0, 4], np.int32)
    only = SeptGraphSampler(6, 3, none, none, pfo, pfe)
    got = only.draw(0.01, 3, 4)[0].numpy()[:only.nnz]
    keep, skeep = SS.keep_lists(0, 4, 0.01, 3, 4)
    assert (keep.size, skeep.size) == (0, 3)
    want = SS.values_on_structure(T.sept_sub_adjacency(6, 3, none, none, pfo, pfe, keep, skeep), only.indptr, only.indices)
    check("pairs without rows: words that differ", _words_differ(got, want), 0, inclusive=True)


# ---- 3. the view over (union plan + device values) vs over the host-built CSR ---------------------------------------------------------
def _sept_problem(rng, nu=300, ni=400, E=5000, R=1500):
    """test_gpu_graph.py's _sept_problem plus three hot users and three hot items: their rows hold more than the 128 entries of one SpMM
    segment, and the union structure splits them at other places than the compact CSR of the kept entries does"""
    uid = rng.integers(0, nu, E).astype(np.int32); iid = rng.integers(0, ni, E).astype(np.int32)
    uid[:900] = rng.integers(0, 3, 900); iid[900:1800] = rng.integers(0, 3, 900)
    fo = rng.integers(0, nu, R).astype(np.int32); fe = rng.integers(0, nu, R).astype(np.int32)
    assert min(np.unique(iid[uid == 0]).size, np.unique(uid[iid == 0]).size) > 128
    return nu, ni, uid, iid, fo, fe


@pytest.mark.parametrize("dim,ld", [(24, 32), (64, 64)])
def test_view_over_the_union_structure_equals_the_view_over_the_host_built_csr(dim, ld):
    """_View.forward / backward (two layers, l2-normalised) with plan = the union structure's plan + the device-drawn values and
    planT = the transposed structure's plan + the transposed values, against the exact path's plans of the same keep lists' scipy CSR.
    The value arrays add +0 terms and may split long rows differently: fp32 rounding, held to the project's 1e-5."""
    rng = np.random.default_rng(50 + dim)
    nu, ni, uid, iid, fo, fe = _sept_problem(rng)
    n, L, seed, sid = nu + ni, 2, 9, (1 << 32) + 6
    smp = SeptGraphSampler(nu, ni, uid, iid, fo, fe)
    vals, vals_t = smp.draw(0.3, seed, sid)
    M = T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe, *SS.keep_lists(uid.size, fo.size, 0.3, seed, sid)).astype(np.float32)
    dev, host = _View(n, ld, L), _View(n, ld, L)
    host.set_matrix(M, split_row=nu)
    assert host.planT is not host.plan
    dev.plan = SpmmPlan(smp.indptr, smp.indices, np.zeros(smp.nnz, np.float32), ld, split_row=nu, row_chunk=host.plan.row_chunk).with_values(vals)
    dev.planT = SpmmPlan(smp.indptr_t, smp.indices_t, np.zeros(smp.nnz, np.float32), ld, split_row=nu, row_chunk=host.plan.row_chunk).with_values(vals_t)
    X0 = DB.from_numpy(pad_cols((rng.standard_normal((n, dim)) * 0.1).astype(np.float32), ld))
    B = 256
    u, i, j = (DB.from_numpy(rng.integers(0, hi, B).astype(np.int32)) for hi in (nu, ni, ni))
    mask = DB.zeros((n + 31) // 32, np.uint32)
    capi.mark_batch_rows(u, i, j, B, nu, mask)
    bits = np.unpackbits(mask.numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
    assert 0 < bits.sum() < n
    for masked in (False, True):
        rows = bits if masked else np.ones(n, bool)
        dS = np.zeros((n, ld), np.float32); dS[rows, :dim] = rng.standard_normal((int(rows.sum()), dim)).astype(np.float32)
        res = []
        for v in (dev, host):
            v.forward(X0, last_rows=mask if masked else None)
            v.dS.upload(dS)
            d_total, T_, G = DB.zeros((n, ld), np.float32), DB.zeros((n, ld), np.float32), [DB.zeros((n, ld), np.float32), DB.zeros((n, ld), np.float32)]
            v.backward(T_, G, d_total, ds_rows=mask if masked else None)
            res.append((v.S.numpy()[rows, :dim], d_total.numpy()[:, :dim]))
        what = f"perturbed view, union structure + device values vs host-built CSR (d {dim}, {'batch-row masks' if masked else 'all rows'})"
        check(f"{what}: layer sum S, relative error", rel_err(res[0][0], res[1][0]), 1e-5, inclusive=True)
        check(f"{what}: gradient w.r.t. the input, relative error", rel_err(res[0][1], res[1][1]), 1e-5, inclusive=True)
        assert np.linalg.norm(res[1][1]) > 0


# ---- 4. trainer steps ----------------------------------------------------------------------------------------------------------------
def test_trainer_steps_on_device_drawn_values_follow_the_steps_on_the_host_built_graph():
    """two SEPTTrainers on identical inputs (ordered reductions), one with set_perturbed_graph(host CSR), the other with
    set_perturbed_values(device draw of the same keep lists): two recommendation steps, three joint steps.  The pseudo labels are a top-k
    over float32 softmax rows (discontinuous): agreement at 99.5 % as in test_sept_pseudo_labels_and_neighbour_discrimination_match_restatement;
    on the steps where every label agrees, losses and gradients to 1e-5."""
    rng = np.random.default_rng(61)
    nu, ni, uid, iid, fo, fe = _sept_problem(rng)
    dim, B, k, L, seed, sid = 24, 256, 5, 2, 4, (1 << 32) + 8
    adj = T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe).astype(np.float32)
    social, sharing = T.sept_social_views(nu, ni, uid, iid, fo, fe)
    U0 = (rng.standard_normal((nu, dim)) * 0.1).astype(np.float32); V0 = (rng.standard_normal((ni, dim)) * 0.1).astype(np.float32)
    with ordered_reductions():
        host, dev = (SEPTTrainer(U0, V0, adj, social, sharing, L, 0.002, 0.01, 0.05, k, max_unique=B) for _ in range(2))
    smp = SeptGraphSampler(nu, ni, uid, iid, fo, fe)
    with pytest.raises(RuntimeError):
        dev.set_perturbed_values(*smp.draw(0.3, seed, sid))                           # the structure first
    dev.set_perturbed_structure(smp.indptr, smp.indices, smp.indptr_t, smp.indices_t)
    plans = dev._aug_plans
    dev.set_perturbed_values(*smp.draw(0.3, seed, sid))
    assert dev._aug_plans is plans and dev.aug.plan.seg_row is plans[0].seg_row and dev.aug.planT.indices is plans[1].indices   # values swapped, nothing rebuilt
    host.set_perturbed_graph(T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe, *SS.keep_lists(uid.size, fo.size, 0.3, seed, sid)).astype(np.float32))
    compared = 0
    for step in range(5):
        u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, ni, B).astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
        joint = step >= 2
        uu = np.unique(u).astype(np.int32)
        got = []
        for tr in (dev, host):
            before = np.concatenate(tr.variables())
            tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, joint, DB.from_numpy(uu), uu.size, keep_labels=joint)
            got.append((tr.losses(), tr.gradients(before), tr.d_labels.numpy().reshape(-1, k) if joint else None))
        (la, ga, lab_a), (lb, gb, lab_b) = got
        if joint:
            agree = float(np.mean([np.array_equal(a, b) for a, b in zip(lab_a, lab_b)]))
            check(f"SEPT trainer, device-drawn vs host-built perturbed graph: share of pseudo-label rows that differ (step {step})", 1 - agree, 0.005,
                  inclusive=True, kind="discontinuity")
            if agree < 1.0:
                continue
        compared += 1
        check_rel(f"SEPT trainer, device-drawn vs host-built perturbed graph: rec loss (step {step})", la[0], lb[0], 1e-5)
        check_rel(f"... ssl loss (step {step})", la[1], lb[1], 1e-5, abs_tol=1e-9)
        check(f"... dU (step {step})", rel_err(ga[0], gb[0]), 1e-5, inclusive=True)
        check(f"... dV (step {step})", rel_err(ga[1], gb[1]), 1e-5, inclusive=True)
    assert compared >= 3                                                              # the two recommendation steps and a joint one at least


# ---- 5. - 7. the classes -------------------------------------------------------------------------------------------------------------
SEPT_EXTRA = "-n_layer 2 -ss_rate 0.005 -drop_rate 0.3 -ins_cnt 5"


def test_sept_class_in_throughput_mode_trains_without_touching_the_host_generators(tmp_path):
    problem = SS.social_problem("SEPT", tmp_path, epochs=6, batch=2000, extra=SEPT_EXTRA)
    a = SS.run_mode("SEPT", problem, "throughput", 4, "ordered")                      # asserts that random's state is unchanged over execute()
    m = a["model"]
    assert m.sampler is not None and m.trainer.ows is not None and (m.drop_rate, m.instance_cnt) == (0.3, 5)
    assert any(x.startswith("Recall") for x in a["measure"]) and a["values"][1] > 0
    assert m.U is m.bestU and m.U.shape == (m.num_users, 16) and m.trainer.opt[0].n and m.trainer.opt[1].b1p < m.trainer.opt[1].b1     # both optimizers stepped
    s = m.sampler
    want = SS.values_on_structure(SS.predicted_perturbed_adjacency(m, 4, 5), s.indptr, s.indices)
    check("SEPT class, throughput mode: the last epoch's perturbed graph vs the oracle, words that differ", _words_differ(m._perturbed[0].numpy()[:s.nnz], want), 0, inclusive=True)
    check("... its transpose", _words_differ(m._perturbed[1].numpy()[:s.nnz], SS.values_on_structure(SS.predicted_perturbed_adjacency(m, 4, 5).T, s.indptr_t, s.indices_t)),
          0, inclusive=True)
    assert m.trainer.aug.plan.values is m._perturbed[0] and m.trainer.aug.planT.values is m._perturbed[1]
    b = SS.run_mode("SEPT", problem, "throughput", 4, "ordered")
    same_bits("SEPT throughput mode, ordered reductions, two runs with the same seed", a["arrays"], b["arrays"])
    c = SS.run_mode("SEPT", problem, "throughput", 5, "ordered")
    assert DS.bytes_differing(a["arrays"], c["arrays"]) > 0
    d = SS.run_mode("SEPT", problem, "throughput", 4)                                  # as it ships: float atomics
    assert d["model"].trainer.ows is None and d["values"][1] > 0


def test_sept_class_in_throughput_mode_refuses_a_batch_with_fewer_users_than_ins_cnt(tmp_path):
    problem = SS.social_problem("SEPT", tmp_path, epochs=3, batch=2000, extra="-n_layer 1 -ss_rate 0.005 -drop_rate 0.3 -ins_cnt 1400")
    with pytest.raises(SystemExit) as e:
        SS.run_mode("SEPT", problem, "throughput", 1)
    assert e.value.code == -1


def test_mhcn_throughput_and_exact_mode_on_the_same_stream_are_bit_identical_with_ordered_reductions(tmp_path):
    problem = SS.social_problem("MHCN", tmp_path, epochs=3)
    a = SS.run_mode("MHCN", problem, "throughput", 7, "ordered")                      # asserts that the generator is untouched
    b = SS.run_mode("MHCN", problem, "exact", 7, "ordered")
    assert a["values"][1] > 0
    same_bits("MHCN throughput vs exact mode on the same stream", a["arrays"], b["arrays"])
    c = SS.run_mode("MHCN", problem, "exact", 7, "ordered", epoch_shift=1)            # the comparison can fail: another epoch's stream
    assert DS.bytes_differing(a["arrays"], c["arrays"]) > 0


@pytest.mark.parametrize("seed", [5, 11, 2 ** 40 + 3, 100])
def test_sept_throughput_and_exact_mode_on_the_same_stream(tmp_path, seed):
    """Run A: QREC_MODE=throughput; run B: exact mode fed the same batch stream, the same unique rows and the oracle's perturbed graph of the
    same keep lists (SS.replay_on_host); ordered reductions in both.  The recommendation-only epochs (0 .. maxEpoch / 3) do not involve the
    perturbed view: every batch loss bit-identical -- the stream, the hand-off and the trainer state.  In the joint epochs the value arrays
    add +0 terms, the union structure splits long rows differently, and the pseudo labels are a top-k (discontinuous): the distance is
    RECORDED (kind info), not bounded -- nobody has measured a bound yet (tools/bench_sept_epoch.py --paired runs the paired procedure)."""
    epochs = 6
    problem = SS.social_problem("SEPT", tmp_path, epochs=epochs, batch=2000, extra=SEPT_EXTRA)
    a = SS.run_mode("SEPT", problem, "throughput", seed, "ordered", quiet=False)
    b = SS.run_mode("SEPT", problem, "exact", seed, "ordered", quiet=False)
    n_batches = -(-len(problem[1]) // 2000)
    rec_only = (epochs // 3 + 1) * n_batches                                          # epochs with epoch <= maxEpoch / 3
    assert len(a["rec"]) == len(b["rec"]) == epochs * n_batches and len(a["con"]) == len(b["con"]) == epochs * n_batches - rec_only
    differ = sum(x != y for x, y in zip(a["rec"][:rec_only], b["rec"][:rec_only]))
    check(f"SEPT paired modes (seed {seed}): batch losses of the recommendation-only epochs that differ between throughput and exact mode on the same stream",
          differ, 0, inclusive=True)
    assert len(set(a["rec"][:rec_only])) > rec_only // 2                               # they are losses, not a constant
    what = f"SEPT paired modes (ordered / ordered, seed {seed})"
    check(f"{what}: max-normalised distance of the final tables", DS.table_distance(a["arrays"], b["arrays"]), 1e30, kind="info")
    check(f"{what}: |Recall@10(throughput) - Recall@10(exact on the same stream)|", abs(a["values"][1] - b["values"][1]), 1.0, inclusive=True, kind="info")
    check(f"{what}: |NDCG@10(throughput) - NDCG@10(exact on the same stream)|", abs(a["values"][3] - b["values"][3]), 1.0, inclusive=True, kind="info")
    rel = max(abs(float(x) - float(y)) / max(abs(float(y)), 1e-300) for x, y in zip(a["rec"][rec_only:], b["rec"][rec_only:]))
    check(f"{what}: worst relative difference of a joint epoch's batch rec loss", rel, 1e30, kind="info")
    print(what, "A", a["values"], "B", b["values"], "table distance", DS.table_distance(a["arrays"], b["arrays"]), "joint rec-loss rel diff", rel)
