"""GPU parity tests of the LightGCN-family kernels against the numpy/scipy restatement
(oracle/tfmodels.py): SpMM, batch BPR loss/grad, Adam, whole training steps, the drop-in class.
fp32 tolerance 1e-5 relative (north_star)."""
import io
import os
import random
from contextlib import redirect_stdout

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import tfmodels as T
from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.graph import LightGCNTrainer, SpmmPlan, joint_norm_adjacency, ordered_reductions
from qrec_amd.synth import make_dataset

from helpers import check, check_rel, conf_from_text, load_golden, pad_cols, rel_err, rows_from_golden

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    yield


@pytest.fixture(autouse=True)
def _parity_mode():
    """trainers these tests construct directly run with ordered reductions (csrc/ordered.hip: the parity mode, the exact mode of the
    drop-in classes); the drop-in classes choose for themselves (DeepRecommender.build_trainer), logical-rank threads keep the atomics"""
    with ordered_reductions():
        yield


def _graph(shape):
    d = make_dataset(shape)
    adj = joint_norm_adjacency(d["n_users"], d["n_items"], d["train_u"], d["train_i"])
    A = sp.csr_matrix((adj[2], adj[1], adj[0]), shape=(adj[0].size - 1,) * 2)
    return d, adj, A


@pytest.mark.parametrize("dim,ld", [(64, 64), (50, 64), (8, 32), (128, 128), (200, 256)])
@pytest.mark.parametrize("seg_len", [128, 7])
def test_spmm_matches_scipy(dim, ld, seg_len):
    d, adj, A = _graph("small")
    n = A.shape[0]
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((n, dim)).astype(np.float32); Z = rng.standard_normal((n, dim)).astype(np.float32)
    S0 = rng.standard_normal((n, dim)).astype(np.float32)
    plan = SpmmPlan(adj[0], adj[1], adj[2], ld, seg_len=seg_len)
    assert plan.n_long > 0 if seg_len == 7 else True
    dX, dY = DB.from_numpy(pad_cols(X, ld)), DB.zeros((n, ld), np.float32)
    capi.spmm_csr(plan, dX, dY, ld)
    ref = A.dot(X)
    got = dY.numpy()
    check("rel_err(got[:, :dim], ref)", rel_err(got[:, :dim], ref), TOL)
    assert (got[:, dim:] == 0).all()
    # rows that are not segmented accumulate in CSR order exactly like scipy: bit-identical
    whole = np.diff(adj[0]) <= seg_len
    assert np.array_equal(got[whole][:, :dim], ref[whole])
    # fused epilogues: Y = A X + 0.5 Z ; accum += Y
    dZ, dS = DB.from_numpy(pad_cols(Z, ld)), DB.from_numpy(pad_cols(S0, ld))
    capi.spmm_csr(plan, dX, dY, ld, d_addend=dZ, addend_scale=0.5, d_accum=dS)
    check("rel_err(dY.numpy()[:, :dim], ref + np.float32(0.5) * Z)", rel_err(dY.numpy()[:, :dim], ref + np.float32(0.5) * Z), TOL)
    check("rel_err(dS.numpy()[:, :dim], S0 + (ref + np.float32(0.5) * Z))", rel_err(dS.numpy()[:, :dim], S0 + (ref + np.float32(0.5) * Z)), TOL)
    # deterministic
    capi.spmm_csr(plan, dX, dY, ld); a = dY.numpy(); capi.spmm_csr(plan, dX, dY, ld); assert np.array_equal(a, dY.numpy())
    with pytest.raises(capi.QRecError):
        capi.spmm_csr(plan, dX, dX, ld)


@pytest.mark.parametrize("chunks", [2, 4])
@pytest.mark.parametrize("seg_len", [128, 7])
def test_spmm_row_chunks_do_not_change_a_bit(chunks, seg_len):
    """SpmmPlan(chunks=...) only reorders the segment list (rows of one spectral-key run on XCDs of their own): plain,
    with the fused epilogues, with the sparse-operand bitmap and with the wanted-rows bitmap the output is bit for bit
    the output of the plain order."""
    d, adj, A = _graph("small")
    n, ld = A.shape[0], 64
    rng = np.random.default_rng(chunks)
    X = rng.standard_normal((n, ld)).astype(np.float32); Z = rng.standard_normal((n, ld)).astype(np.float32)
    S0 = rng.standard_normal((n, ld)).astype(np.float32)
    xmask_rows = rng.random(n) < 0.2
    Xs = X * xmask_rows[:, None]
    bits = lambda rows: np.packbits(np.pad(rows, (0, (-n) % 32)).reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()
    ymask_rows = rng.random(n) < 0.3
    out = {}
    for c in (1, chunks):
        plan = SpmmPlan(adj[0], adj[1], adj[2], ld, seg_len=seg_len, split_row=d["n_users"], chunks=c)
        assert plan.chunks == c
        dX, dY = DB.from_numpy(X), DB.zeros((n, ld), np.float32)
        capi.spmm_csr(plan, dX, dY, ld); plain = dY.numpy()
        dZ, dS = DB.from_numpy(Z), DB.from_numpy(S0)
        capi.spmm_csr(plan, dX, dY, ld, d_addend=dZ, addend_scale=0.5, d_accum=dS); fused = (dY.numpy(), dS.numpy())
        capi.spmm_csr(plan, DB.from_numpy(Xs), dY, ld, d_x_row_mask=DB.from_numpy(bits(xmask_rows))); sparse = dY.numpy()
        dY2 = DB.from_numpy(np.full((n, ld), 7, np.float32))
        capi.spmm_csr(plan, dX, dY2, ld, d_y_row_mask=DB.from_numpy(bits(ymask_rows))); wanted = dY2.numpy()
        out[c] = (plain, fused[0], fused[1], sparse, wanted)
    for a, b in zip(out[1], out[chunks]):
        assert np.array_equal(a, b)
    check("rel_err(out[chunks][0], A.dot(X))", rel_err(out[chunks][0], A.dot(X)), TOL)
    assert (out[chunks][4][~ymask_rows] == 7).all() and np.array_equal(out[chunks][4][ymask_rows], out[chunks][0][ymask_rows])
    with pytest.raises(ValueError):
        SpmmPlan(adj[0], adj[1], adj[2], ld, chunks=2)          # chunks need the bipartite split


def test_spmm_empty_rows_and_heavy_row():
    # node 0 connected to everything (one very long row), nodes without edges (empty rows)
    n = 3000
    rows = np.concatenate([np.zeros(n - 10, np.int64), np.arange(10, n, dtype=np.int64)])
    cols = np.concatenate([np.arange(10, n, dtype=np.int64), np.zeros(n - 10, np.int64)])
    A = sp.csr_matrix((np.full(rows.size, 0.5, np.float32), (rows, cols)), shape=(n, n)); A.sort_indices()
    plan = SpmmPlan(A.indptr.astype(np.int64), A.indices, A.data, 64)
    X = np.random.default_rng(0).standard_normal((n, 64)).astype(np.float32)
    dX, dY = DB.from_numpy(X), DB.from_numpy(np.full((n, 64), 7, np.float32))
    capi.spmm_csr(plan, dX, dY, 64)
    got = dY.numpy()
    check("rel_err(got, A.dot(X))", rel_err(got, A.dot(X)), TOL)
    assert (got[1:10] == 0).all()


def test_batch_loss_grad_and_adam_match_restatement():
    rng = np.random.default_rng(1)
    nu, ni, dim, ld, B, L = 300, 200, 50, 64, 1000, 2
    S = rng.standard_normal((nu + ni, dim)).astype(np.float32)
    u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, ni, B).astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
    Ebar = (S / np.float32(L + 1)).astype(np.float32)
    loss, du, di, dj = T.bpr_batch_loss_and_grads(Ebar[u], Ebar[nu + i], Ebar[nu + j], 0.01)
    dref = np.zeros_like(Ebar); np.add.at(dref, u, du); np.add.at(dref, nu + i, di); np.add.at(dref, nu + j, dj)
    dS, dE, dl = DB.from_numpy(pad_cols(S, ld)), DB.zeros((nu + ni, ld), np.float32), DB.zeros(1, np.float64)
    capi.bpr_batch_loss_grad(dS, float(L + 1), nu, nu + ni, ld, DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, 1e-7, 0.01, dE, dl)
    got = dE.numpy()
    check("rel_err(got[:, :dim], dref)", rel_err(got[:, :dim], dref), TOL)
    assert (got[:, dim:] == 0).all()
    check("abs(dl.numpy()[0] - loss) / abs(loss)", abs(dl.numpy()[0] - loss) / abs(loss), TOL)
    # Adam, several steps
    theta = rng.standard_normal((nu + ni, ld)).astype(np.float32); ref = theta.copy()
    opt = T.AdamTF114(theta.shape, lr=0.01)
    dT, dM, dV = DB.from_numpy(theta), DB.zeros(theta.shape, np.float32), DB.zeros(theta.shape, np.float32)
    for t in range(1, 6):
        g = rng.standard_normal(theta.shape).astype(np.float32)
        alpha = float(opt.alpha())
        opt.step(ref, (np.float32(1 / 3) * g).astype(np.float32))
        capi.adam_step(dT, dM, dV, DB.from_numpy(g), theta.size, 1 / 3, alpha)
    check("rel_err(dT.numpy(), ref)", rel_err(dT.numpy(), ref), TOL)
    check("rel_err(dM.numpy(), opt.m)", rel_err(dM.numpy(), opt.m), TOL)
    check("rel_err(dV.numpy(), opt.v)", rel_err(dV.numpy(), opt.v), TOL)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_lightgcn_training_steps_match_restatement(L):
    d, adj, A = _graph("small")
    nu, ni, dim, B = d["n_users"], d["n_items"], 64, 2048
    rng = np.random.default_rng(L)
    U0 = (rng.standard_normal((nu, dim)) * 0.005).astype(np.float32); V0 = (rng.standard_normal((ni, dim)) * 0.005).astype(np.float32)
    ref = T.LightGCN(U0, V0, A, L, lr=0.001, reg=1e-4)
    tr = LightGCNTrainer(U0, V0, adj, L, lr=0.001, reg=1e-4)
    for step in range(8):
        sel = rng.integers(0, d["train_u"].size, B)
        u = d["train_u"][sel].astype(np.int32); i = d["train_i"][sel].astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
        lref = ref.train_step(u, i, j)
        tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B)
        check("abs(tr.loss() - lref) / abs(lref)", abs(tr.loss() - lref) / abs(lref), TOL)
    Ug, Vg = tr.ego_embeddings()
    # Adam normalises every coordinate's step to ~lr, so agreement is measured on the update
    check("rel_err(np.concatenate([Ug, Vg]) - np.concatenate([U0, V0]), ref.E - np.concatenate([U0, V0]))", rel_err(np.concatenate([Ug, Vg]) - np.concatenate([U0, V0]), ref.E - np.concatenate([U0, V0])), 1e-5)
    check("rel_err(np.concatenate([Ug, Vg]), ref.E)", rel_err(np.concatenate([Ug, Vg]), ref.E), TOL)
    Uf, Vf = tr.final_embeddings(); Ur, Vr = ref.final_embeddings()
    check("rel_err(Uf, Ur)", rel_err(Uf, Ur), 1e-5)
    check("rel_err(Vf, Vr)", rel_err(Vf, Vr), 1e-5)


def test_lightgcn_class_end_to_end_against_restatement_with_reference_sampler_stream():
    """The drop-in LightGCN class on the reference's FilmTrust rows: its batches are the
    reference's own next_batch_pairwise stream (golden), the training trajectory equals the
    restatement's from the same injected initial tables."""
    from qrec_amd.model.ranking.LightGCN import LightGCN
    meta, z = load_golden("pairwise_adj_filmtrust")
    gz = load_golden("bpr_filmtrust")[1]
    train, test = rows_from_golden(gz)
    conf = conf_from_text(meta["conf"]); conf["num.max.epoch"] = "2"
    rng = np.random.default_rng(0)
    U0 = (rng.standard_normal((meta["n_users"], 8)) * 0.005).astype(np.float32)
    V0 = (rng.standard_normal((meta["n_items"], 8)) * 0.005).astype(np.float32)
    random.seed(meta["seed"]); np.random.seed(meta["seed"])
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = LightGCN(conf, train, test)
        m.readConfiguration(); m.initializing_log = lambda: None
        m.initModel()
        m.trainer = type(m.trainer)(U0, V0, m.create_joint_sparse_adjaceny(), m.n_layers, m.lRate, m.regU)  # inject init
        m.trainModel()
    losses = [float(l.split("loss:")[1]) for l in buf.getvalue().splitlines() if "loss:" in l]
    # restatement fed with the reference's recorded stream (2 epochs were recorded)
    A = sp.csr_matrix((z["adj_data"], z["adj_indices"], z["adj_indptr"]), shape=(z["adj_indptr"].size - 1,) * 2)
    ref = T.LightGCN(U0, V0, A, 2, lr=float(conf["learnRate"].split()[1]), reg=1e-3)
    st, pos, ref_losses = z["stream"], 0, []
    for bs in z["batch_sizes"]:
        b = st[pos:pos + bs]; pos += bs
        ref_losses.append(ref.train_step(b[:, 0], b[:, 1], b[:, 2]))
    assert len(losses) == len(ref_losses)
    check_rel("class losses vs restatement on the reference stream", losses, ref_losses, 1e-5)
    Ur, Vr = ref.final_embeddings()
    check("rel_err(m.U, Ur)", rel_err(m.U, Ur), 1e-5)
    check("rel_err(m.V, Vr)", rel_err(m.V, Vr), 1e-5)
    assert np.array_equal(capi.state_from_python(random.getstate()), z["py_state"])   # sampler stayed in lock-step


@pytest.mark.parametrize("name", ["LightGCN", "NGCF", "SimGCL"])
def test_throughput_mode_of_the_pairwise_models_draws_its_batches_on_the_device(name, monkeypatch):
    """QREC_MODE=throughput (base/deepRecommender.py:29-52 on the device): every epoch is a uniform shuffle of the
    training rows with one negative per row that the user has not rated -- a permutation of the rows, valid negatives,
    reproducible per (seed, epoch), different from epoch to epoch -- Python's generator is left alone, and the class
    trains to the quality of the exact mode (same conf, same initial tables; measures within sampling noise)."""
    from qrec_amd.QRec import resolve_model
    meta, z = load_golden("pairwise_adj_filmtrust")
    gz = load_golden("bpr_filmtrust")[1]
    train, test = rows_from_golden(gz)
    conf = conf_from_text(meta["conf"]); conf["model.name"] = name; conf["num.max.epoch"] = os.environ.get("QREC_TEST_EPOCHS", "20"); conf["num.factors"] = "16"
    conf["item.ranking"] = "on -topN 10"; conf["learnRate"] = "-init 0.002 -max 1"
    if name == "SimGCL":
        conf["SimGCL"] = "-n_layer 2 -lambda 0.5 -eps 0.1"
    monkeypatch.setenv("QREC_QUIET", "1"); monkeypatch.setenv("QREC_SEED", "5")
    cls = resolve_model(name)

    def run(mode, stream_seed):
        """same conf, same initial tables (numpy's generator, seed 3); ``stream_seed`` moves the SAMPLING stream only: Python's generator
        in exact mode (the reference's next_batch_pairwise replayed), the device stream's seed in throughput mode"""
        monkeypatch.setenv("QREC_MODE", mode); monkeypatch.setenv("QREC_SEED", str(stream_seed))
        random.seed(stream_seed); np.random.seed(3)
        with redirect_stdout(io.StringIO()):
            m = cls(conf, train, test)
            measure = m.execute()
        return m, [float(x.split(":")[1]) for x in measure if ":" in x]
    # The two modes run the SAME training step (held to the reference at 1e-5 elsewhere); what differs is which uniform shuffle /
    # which unrated negatives an epoch sees.  So the statement is statistical: the difference of the two modes' MEAN measures over S
    # sampling streams per mode, inside a FLAT bound.  Round 5 ran three streams and allowed 0.002 + three standard errors, which
    # let 0.02-0.05 through for NGCF / SimGCL; measured since (tools/probe_mode_gap.py, 64 streams): one run's Recall@10 spreads 0.020-0.024
    # (sd) from stream to stream on this 1,500-user set in EITHER mode, NDCG 0.034, the reduction order (ordered / atomic) moves nothing.
    # A flat 0.005 needs the difference of the means known to ~0.0017 (3 sigma): streams are added in blocks of 32 per mode until the
    # standard error of the Recall difference is there (a run is 0.15 s; LightGCN stops at the first block, NGCF needs ~10).
    block, s_max = 32, int(os.environ.get("QREC_TEST_MAX_STREAMS", "512"))
    exact, thr, m = [], [], None
    while True:
        k0 = len(exact)
        exact += [run("exact", 3 + k)[1] for k in range(k0, k0 + block)]
        for k in range(k0, k0 + block):
            m, meas = run("throughput", 100003 + k)
            thr.append(meas)
        S = len(exact)
        e, t = np.array(exact), np.array(thr)
        se = np.sqrt(e.var(0, ddof=1) / S + t.var(0, ddof=1) / S)
        if se[1] <= 0.0017 or S >= s_max:
            break
    exact, thr = e, t
    assert m.throughput_mode()
    gap = np.abs(thr.mean(0) - exact.mean(0))
    print(name, "streams per mode", S, "exact mean", exact.mean(0), "sd", exact.std(0, ddof=1), "throughput mean", thr.mean(0), "sd", thr.std(0, ddof=1), "gap", gap, "se", se)
    for k, (what, bound) in enumerate((("Precision", 0.005), ("Recall", 0.005), ("F1", 0.005), ("NDCG", 0.01))):   # NDCG's own stream-to-stream sd is 1.7x Recall's
        check(f"{name} throughput-mode vs exact-mode {what}@10, |difference of the means over the sampling streams|", gap[k], bound, inclusive=True, kind="statistical", ctx=(S, se[k]))
    check(f"{name} Recall@10: standard error of that difference", se[1], 0.0025, inclusive=True, kind="statistical", ctx=S)
    assert thr[:, 1].min() > 0.05                                          # it learned something (Recall@10 on FilmTrust)
    # the stream itself
    u0, i0, _ = m.data.training_arrays()
    rated = m.data.rated_csr()
    want_pairs = np.sort(u0.astype(np.int64) * m.num_items + i0)
    state = random.getstate()
    epochs = [tuple(b.numpy() for b in bufs) for bufs in m.iter_epoch_samples_device(3)]
    assert random.getstate() == state                                      # no CPython draws
    again = [tuple(b.numpy() for b in bufs) for bufs in m.iter_epoch_samples_device(2)]
    for k, (u, i, j) in enumerate(epochs):
        assert np.array_equal(np.sort(u.astype(np.int64) * m.num_items + i), want_pairs)       # a permutation of the rows
        assert ((j >= 0) & (j < m.num_items)).all()
        is_rated = np.zeros((m.num_users, m.num_items), bool); is_rated[rated.row_ids(), rated.indices] = True
        assert not is_rated[u, j].any()                                                          # negatives are not rated
        if k < 2:
            assert all(np.array_equal(a, b) for a, b in zip(epochs[k], again[k]))                # reproducible
    assert not np.array_equal(epochs[0][0], epochs[1][0]) and not np.array_equal(epochs[0][2], epochs[1][2])
    assert not np.array_equal(epochs[0][0], u0)                                                  # and it is shuffled


# ---- the composed device stream, and the two modes on ONE stream (tests/device_stream.py) ------------------------------------------
import functools  # noqa: E402

import device_stream as DS  # noqa: E402
from helpers import same_bits  # noqa: E402


@functools.lru_cache(maxsize=None)
def _stream_model(rows):
    """a DeepRecommender over the named training rows (only its data, its rated CSR and its device generator are used)"""
    from qrec_amd.base.deepRecommender import DeepRecommender
    meta, _ = load_golden("pairwise_adj_filmtrust")
    if rows == "filmtrust":
        train, _ = rows_from_golden(load_golden("bpr_filmtrust")[1])                      # 32,736 rows = 127 x 256 + 224
    elif rows == "small":
        d = make_dataset("small")                                                         # 60,797 rows = 237 x 256 + 125
        train = [[f"u{u}", f"i{i}", 1.0] for u, i in zip(d["train_u"].tolist(), d["train_i"].tolist())]
    else:
        train = [["u0", "i0", 1.0], ["u1", "i1", 1.0], ["u0", "i2", 1.0]][:int(rows)]     # n = 1 (its only item is rated: j = -1), n = 3
    with redirect_stdout(io.StringIO()):
        return DeepRecommender(conf_from_text(meta["conf"]), train, [])


@functools.lru_cache(maxsize=None)
def _ballast():
    return DB(1 << 26, np.int32), DB(1 << 26, np.int32)                                   # 2 x 256 MiB


@pytest.mark.parametrize("own_stream", [False, True])
@pytest.mark.parametrize("seed", [0, 5, 2 ** 40 + 3])
@pytest.mark.parametrize("rows", ["filmtrust", "small", "1", "3"])
def test_device_batch_stream_equals_the_oracle_under_asynchronous_readers(rows, seed, own_stream, monkeypatch):
    """iter_epoch_samples_device read the way a trainer reads it: per epoch the readers of the three buffers are ENQUEUED on the caller's
    stream (copies into per-epoch snapshots, behind a few hundred MiB of copies so that they are still pending when the generator is
    advanced), the generator is advanced with no host synchronisation in between, and only after the last epoch the device is
    synchronised.  Six epochs: each of the two buffers is rewritten twice under pending readers.  Every snapshot equals the stream the
    oracle predicts (tests/device_stream.py), bit for bit -- the composition permutation -> qrec_gather_pairs -> qrec_philox_bpr_sample
    AND its hand-off (the caller's stream waits for the draw; the draw into a buffer waits for that buffer's readers).  Once on the null
    stream, once on a stream of the caller's."""
    monkeypatch.setenv("QREC_SEED", str(seed))
    m = _stream_model(rows)
    n = int(m.data.training_arrays()[0].size)
    assert n % 256 != 0
    E = 6
    stream = capi.Stream() if own_stream else None
    fill = np.full(n, -7, np.int32)
    snap = [[DB.from_numpy(fill) for _ in range(3)] for _ in range(E)]
    big_a, big_b = _ballast()
    capi.device_sync()
    state = random.getstate()
    seen = 0
    for k, bufs in enumerate(m.iter_epoch_samples_device(E, stream)):
        for _ in range(8):
            capi.memcpy_d2d(big_b, big_a, big_a.nbytes, stream)                           # work in front of the readers: they stay pending
        for dst, src in zip(snap[k], bufs):
            capi.memcpy_d2d(dst, src, 4 * n, stream)
        seen += 1
    capi.device_sync()
    assert seen == E and random.getstate() == state
    for k in range(E):
        want = DS.predicted_epoch(m, seed, k)
        for what, dst, w in zip("uij", snap[k], want):
            got = dst.numpy()
            assert np.array_equal(got, w), (rows, seed, own_stream, "epoch", k, what, int(np.count_nonzero(got != w)), "of", n, "rows differ")


PAIRED_EPOCHS = int(os.environ.get("QREC_TEST_PAIRED_EPOCHS", "20"))


@pytest.mark.parametrize("seed", [5, 11, 2 ** 40 + 3])
@pytest.mark.parametrize("name", ["LightGCN", "NGCF", "SimGCL"])
def test_throughput_and_exact_mode_on_the_same_stream_are_bit_identical_with_ordered_reductions(name, seed):
    """Run A: QREC_MODE=throughput (the stream drawn on the device, handed over with events, tf.unique on the device).  Run B:
    QREC_MODE=exact fed the SAME stream from the oracle (DS.replay_on_host: host arrays uploaded per epoch).  QREC_REDUCTIONS=ordered
    in both, same seed, same initial tables, a batch size that leaves a 16-row last batch.  Nothing differs between the two except where
    the stream was computed and how it reached the trainer: final tables and measure strings bit-identical."""
    assert PAIRED_EPOCHS >= 6
    conf, train, test = DS.paired_conf(name, PAIRED_EPOCHS)
    assert len(train) % DS.PAIRED_BATCH not in {0}
    a = DS.run_mode(name, conf, train, test, "throughput", seed, "ordered")
    b = DS.run_mode(name, conf, train, test, "exact", seed, "ordered")
    print(name, seed, "A", a["values"], "B", b["values"], "bytes differing", DS.bytes_differing(a["arrays"], b["arrays"]),
          "table distance", DS.table_distance(a["arrays"], b["arrays"]))
    check(f"{name} paired modes (ordered / ordered): Recall@10(throughput) - Recall@10(exact on the same stream)", abs(a["values"][1] - b["values"][1]), 1.0, kind="info")
    assert a["values"][1] > 0.05                                                          # it learned something
    same_bits(f"{name} throughput vs exact mode on the same stream", a["arrays"], b["arrays"])


@pytest.mark.parametrize("name,aug", [("LightGCN", 1), ("NGCF", 1), ("SimGCL", 1), ("SGL", 0), ("SGL", 1), ("SGL", 2), ("BUIR", 1)])
def test_throughput_and_exact_mode_on_the_same_stream_agree_on_the_measures(name, aug):
    """The two modes as they ship -- A: throughput, float atomics, sub-graphs as value arrays over the full graph's plan; B: exact, ordered
    reductions, host-built sub-graph CSR -- on the SAME stream (DS.replay_on_host).  The value arrays add +0 terms and split rows
    differently (test_gpu_augment.py), the atomics add in another order, so the tables differ in the last bits and the statement is on
    the measures, PAIRED: d_s = measure(A_s) - measure(B_s) over S seeds, |mean d| + 2 se(d) <= 0.002 for Recall@10 (the project's bar,
    README / DESIGN section 7) and <= 0.004 for NDCG@10 (the unpaired test's own 2 : 1).  S = 16, then blocks of 16 up to 64 while a bound is
    undecided (|mean| - 2 se <= bound < |mean| + 2 se); still undecided at 64 fails.  The max-normalised table distance is recorded."""
    conf, train, test = DS.paired_conf(name, PAIRED_EPOCHS, aug)
    bounds = ((1, "Recall", 0.002), (3, "NDCG", 0.004))
    d, dist, rec_a = [], [], 0.0
    while True:
        for s in range(len(d), len(d) + 16):
            a = DS.run_mode(name, conf, train, test, "throughput", 100 + s)
            b = DS.run_mode(name, conf, train, test, "exact", 100 + s)
            d.append(np.array(a["values"]) - np.array(b["values"]))
            dist.append(DS.table_distance(a["arrays"], b["arrays"])); rec_a += a["values"][1]
            assert a["values"][1] > 0 and b["values"][1] > 0, (a["values"], b["values"])             # the top-10 lists hit at all
        S = len(d)
        D = np.array(d)
        mean, se = D.mean(0), D.std(0, ddof=1) / np.sqrt(S)
        undecided = any(abs(mean[k]) - 2 * se[k] <= bound < abs(mean[k]) + 2 * se[k] for k, _, bound in bounds)
        if not undecided or S >= 64:
            break
    what = f"{name}{f' aug {aug}' if name == 'SGL' else ''} paired modes (atomic / ordered)"
    print(what, "S", S, "mean d", mean, "sd", D.std(0, ddof=1), "se", se, "table distance max", max(dist))
    check(f"{what}: mean of d = Recall@10(throughput) - Recall@10(exact on the same stream)", abs(mean[1]), 1.0, kind="info", ctx=S)
    check(f"{what}: sd of d (Recall@10)", D.std(0, ddof=1)[1], 1.0, kind="info", ctx=S)
    check(f"{what}: Recall@10 of the throughput runs, mean (what the gap is a gap of)", rec_a / S, 1.0, inclusive=True, kind="info", ctx=S)
    check(f"{what}: seeds", S, 64, inclusive=True, kind="info")
    check(f"{what}: max-normalised distance of the final tables, worst seed", max(dist), 1e30, kind="info", ctx=S)
    for k, measure, bound in bounds:
        check(f"{what}: |mean d| + 2 se(d), {measure}@10", abs(mean[k]) + 2 * se[k], bound, inclusive=True, kind="statistical", ctx=(S, mean[k], se[k]))


# ---------------------------------------------------------------------------------------------
# SimGCL
# ---------------------------------------------------------------------------------------------
from qrec_amd.graph import SimGCLTrainer, unique_first_appearance  # noqa: E402


@pytest.mark.parametrize("dim,ld", [(64, 64), (50, 64), (8, 32), (100, 128)])
def test_perturb_rows_matches_restatement_and_philox_is_uniform(dim, ld):
    rng = np.random.default_rng(dim)
    n = 1000
    emb = rng.standard_normal((n, dim)).astype(np.float32); emb[5, :3] = 0      # sign(0) = 0
    noise = rng.random((n, dim)).astype(np.float32)
    acc0 = rng.standard_normal((n, dim)).astype(np.float32)
    nz, _ = T.l2_normalize_rows(noise)
    want = (emb + (np.sign(emb) * nz) * np.float32(0.1)).astype(np.float32)
    dE, dN, dA = DB.from_numpy(pad_cols(emb, ld)), DB.from_numpy(pad_cols(noise, ld)), DB.from_numpy(pad_cols(acc0, ld))
    capi.perturb_rows(dE, n, dim, ld, 0.1, dN, d_accum=dA)
    got = dE.numpy()
    check("rel_err(got[:, :dim], want)", rel_err(got[:, :dim], want), TOL)
    assert (got[:, dim:] == 0).all()
    check("rel_err(dA.numpy()[:, :dim], acc0 + want)", rel_err(dA.numpy()[:, :dim], acc0 + want), TOL)
    # device-drawn noise: |delta| = eps * unit vector, all components same sign as emb, reproducible
    dE2 = DB.from_numpy(pad_cols(emb, ld)); capi.perturb_rows(dE2, n, dim, ld, 0.1, None, seed=3, stream_id=7)
    delta = dE2.numpy()[:, :dim] - emb
    np.testing.assert_allclose(np.linalg.norm(delta[np.abs(emb).min(1) > 0], axis=1), 0.1, rtol=1e-4)
    assert (delta * np.sign(emb) >= 0).all() and (dE2.numpy()[:, dim:] == 0).all()
    dE3 = DB.from_numpy(pad_cols(emb, ld)); capi.perturb_rows(dE3, n, dim, ld, 0.1, None, seed=3, stream_id=7)
    assert np.array_equal(dE2.numpy(), dE3.numpy())
    dE4 = DB.from_numpy(pad_cols(emb, ld)); capi.perturb_rows(dE4, n, dim, ld, 0.1, None, seed=3, stream_id=8)
    assert not np.array_equal(dE2.numpy(), dE4.numpy())
    # implied uniforms: delta/eps * |noise| ... check the direction's components are spread like U[0,1) draws
    u = np.abs(delta) / 0.1
    u = u / u.max(1, keepdims=True)
    assert 0.3 < u.mean() < 0.8


@pytest.mark.parametrize("n,dim,ld", [(1, 64, 64), (37, 50, 64), (300, 64, 64), (2048, 64, 64), (129, 8, 32), (200, 128, 128)])
def test_info_nce_matches_restatement(n, dim, ld):
    rng = np.random.default_rng(n + dim)
    N = max(3 * n, 10)
    S1 = rng.standard_normal((N, dim)).astype(np.float32); S2 = (S1 + 0.5 * rng.standard_normal((N, dim))).astype(np.float32)
    rows = rng.permutation(N)[:n].astype(np.int32)
    div = np.float32(2)
    loss, d1, d2 = T.info_nce_loss_and_grads((S1[rows] / div).astype(np.float32), (S2[rows] / div).astype(np.float32))
    base = rng.standard_normal((N, dim)).astype(np.float32)
    want = base.copy(); want[rows] += np.float32(0.5) * d1 + np.float32(0.5) * d2
    dOut, dl = DB.from_numpy(pad_cols(base, ld)), DB.zeros(1, np.float64)
    ws = DB(capi.info_nce_workspace_bytes(n, ld), np.uint8)
    capi.info_nce_loss_grad(DB.from_numpy(pad_cols(S1, ld)), DB.from_numpy(pad_cols(S2, ld)), 2.0, DB.from_numpy(rows), n, ld,
                            0.2, 0.5, ws, dOut, dl)
    got = dOut.numpy()
    check("InfoNCE loss vs restatement, relative", abs(dl.numpy()[0] - loss) / max(abs(loss), 1.0), TOL)
    check("InfoNCE gradient rows vs restatement", rel_err(got[:, :dim] - base, want - base), TOL)
    assert (got[:, dim:] == 0).all()
    untouched = np.ones(N, bool); untouched[rows] = False
    assert np.array_equal(got[untouched][:, :dim], base[untouched])


@pytest.mark.parametrize("L", [1, 2, 3])
def test_simgcl_training_steps_match_restatement(L):
    """Five steps, EVERY one from the restatement's state (table and Adam slots uploaded before the step): losses and the gradient
    minimize() applies at 1e-5, step by step -- the parity statement (Adam itself: test_adam_matches_restatement).  Not compared: a table after five
    FREE-running steps.  Adam divides by sqrt(v); on a coordinate whose gradient is cancellation noise of InfoNCE's softmax-weighted
    sums the step is ~lr in a direction the summation order decides, in any float32 implementation -- the reference's own float32 run
    sits 3e-5 from the same run in float64 after twelve steps (tests/golden/tf_f64_yardstick.npz; test_gpu_tf_golden.py holds the
    free-running HIP trainer to that measured floor).  The free-running distance is recorded (kind "info")."""
    d, adj, A = _graph("small")
    nu, ni, dim, B = d["n_users"], d["n_items"], 64, 1024
    N = nu + ni
    lim = np.sqrt(6.0 / (nu + dim))

    def run(forced):
        rng = np.random.default_rng(20 + L)
        U0 = rng.uniform(-lim, lim, (nu, dim)).astype(np.float32); V0 = rng.uniform(-lim, lim, (ni, dim)).astype(np.float32)
        ref = T.SimGCL(U0, V0, A, L, lr=0.001, reg=1e-4, cl_rate=0.5, eps=0.1)
        tr = SimGCLTrainer(U0, V0, adj, L, lr=0.001, reg=1e-4, cl_rate=0.5, eps=0.1, max_unique=B)
        for step in range(5):
            sel = rng.integers(0, d["train_u"].size, B)
            u = d["train_u"][sel].astype(np.int32); i = d["train_i"][sel].astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
            noises = [rng.random((N, dim)).astype(np.float32) for _ in range(2 * L)]
            if forced:
                tr.E.upload(pad_cols(ref.E, tr.ld)); tr.opt.m.upload(pad_cols(ref.opt.m, tr.ld)); tr.opt.v.upload(pad_cols(ref.opt.v, tr.ld))
                assert tr.opt.b1p == ref.opt.b1p and tr.opt.b2p == ref.opt.b2p
                _, _, _, g_ref = ref.loss_and_grad(u, i, j, noises)
            lref, rec_ref, cl_ref = ref.train_step(u, i, j, noises)
            uu = unique_first_appearance(u); vv = (unique_first_appearance(i) + nu).astype(np.int32)
            tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, DB.from_numpy(uu), uu.size,
                                DB.from_numpy(vv), vv.size, noises=[DB.from_numpy(x) for x in noises])
            tot, rec, cl = tr.losses()
            if forced:
                check("SimGCL rec loss, step from the restatement's state", abs(rec - rec_ref) / abs(rec_ref), 1e-5, ctx=step)
                check("SimGCL cl loss, step from the restatement's state", abs(cl - cl_ref) / abs(cl_ref), 1e-5, ctx=step)
                check("SimGCL gradient (before Adam), step from the restatement's state", rel_err(np.concatenate(tr.gradients()), g_ref), 1e-5, ctx=step)
                # (the table after the step is NOT a parity quantity: the first Adam step is -lr sign(g) exactly, and a coordinate whose gradient
                # is rounding noise takes the sign the summation order gives it -- recorded)
                check("SimGCL table after the step, from the restatement's state", rel_err(np.concatenate(tr.ego_embeddings()), ref.E), 1e-3, ctx=step, kind="info")
        return tr, ref, np.concatenate([U0, V0])
    tr, ref, E0 = run(forced=True)
    Um, Vm = tr.main_embeddings(); Ur, Vr = ref.final_embeddings()
    check("SimGCL main user embeddings after the forced steps", rel_err(Um, Ur), 1e-3, kind="info")
    check("SimGCL main item embeddings after the forced steps", rel_err(Vm, Vr), 1e-3, kind="info")
    tr, ref, E0 = run(forced=False)
    Eg = np.concatenate(tr.ego_embeddings())
    check("SimGCL, five free-running steps: table vs restatement (two float32 summation orders under Adam)", rel_err(Eg, ref.E), 1e-3, kind="info")
    check("SimGCL, five free-running steps: update vs restatement's update", rel_err(Eg - E0, ref.E - E0), 1e-2, kind="info")


def test_simgcl_class_runs_stock_conf_shape_and_keeps_best_epoch():
    """Drop-in SimGCL class on the FilmTrust rows with config/SimGCL.conf's hyper-parameters
    (smaller d / epochs): trains with device-drawn noise, evaluates every epoch, returns the
    best epoch's embeddings, loss decreases."""
    from qrec_amd.model.ranking.SimGCL import SimGCL
    meta, z = load_golden("bpr_filmtrust")
    train, test = rows_from_golden(z)
    conf = conf_from_text(meta["conf"])
    conf["model.name"] = "SimGCL"; conf["SimGCL"] = "-n_layer 2 -lambda 0.5 -eps 0.1"; conf["num.factors"] = "16"
    conf["num.max.epoch"] = "3"; conf["batch_size"] = "2048"; conf["learnRate"] = "-init 0.001 -max 1"
    conf["reg.lambda"] = "-u 0.0001 -i 0.0001 -b 0.2 -s 0.2"; conf["item.ranking"] = "on -topN 20"
    random.seed(1); np.random.seed(1)
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = SimGCL(conf, train, test)
        measure = m.execute()
    out = buf.getvalue()
    tot = [float(l.split("total_loss:")[1].split()[0]) for l in out.splitlines() if "total_loss:" in l]
    assert len(tot) == 3 * 16 and tot[-1] < tot[0] and np.isfinite(tot).all()
    assert out.count("Quick Ranking Performance") == 3 and m.bestPerformance[0] in (1, 2, 3)
    rec = [float(x.split(":")[1]) for x in measure if x.startswith("Recall")][0]
    assert 0.0 < rec <= 1.0
    assert m.U is m.bestU and m.U.shape == (meta["n_users"], 16)


def test_bpr_tf_variant_matches_restatement_and_runs_from_conf():
    """model/ranking/BPR.py:77-96 (the `-tf` path): per-step losses and tables vs the restatement,
    then the drop-in class with `-tf` in evaluation.setup."""
    from qrec_amd.graph import BprTfTrainer
    rng = np.random.default_rng(5)
    nu, ni, dim, B = 400, 300, 50, 512
    U0 = (rng.standard_normal((nu, dim)) * 0.005).astype(np.float32); V0 = (rng.standard_normal((ni, dim)) * 0.005).astype(np.float32)
    ref = T.BprTF(U0, V0, lr=0.01, reg=0.001); tr = BprTfTrainer(U0, V0, 0.01, 0.001)
    for step in range(6):
        u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, ni, B).astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
        lref = ref.train_step(u, i, j)
        tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B)
        check("abs(tr.loss() - lref) / abs(lref)", abs(tr.loss() - lref) / abs(lref), TOL)
    Ug, Vg = tr.tables()
    check("rel_err(np.concatenate([Ug, Vg]), ref.E)", rel_err(np.concatenate([Ug, Vg]), ref.E), 1e-5)
    # through the class: `-tf` selects trainModel_tf (base/recommender.py:194-201)
    from qrec_amd.model.ranking.BPR import BPR
    meta, z = load_golden("bpr_filmtrust")
    train, test = rows_from_golden(z)
    conf = conf_from_text(meta["conf"]); conf["evaluation.setup"] = conf["evaluation.setup"] + " -tf"
    conf["num.max.epoch"] = "2"; conf["batch_size"] = "4096"; conf["learnRate"] = "-init 0.01 -max 1"
    random.seed(2); np.random.seed(2)
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = BPR(conf, train, test); measure = m.execute()
    losses = [float(l.split("loss:")[1]) for l in buf.getvalue().splitlines() if l.startswith("training:")]
    assert len(losses) == 2 * 8 and losses[-1] < losses[0] and m.P.dtype == np.float32
    assert any(x.startswith("Recall") for x in measure)


# ---------------------------------------------------------------------------------------------
# NGCF
# ---------------------------------------------------------------------------------------------
from qrec_amd.graph import NGCFTrainer  # noqa: E402


def test_row_subset_helpers():
    """qrec_compact_marked_rows (bitmap -> ascending row list, capacity respected, bits past the last row ignored),
    qrec_zero_rows, and qrec_copy_cols with a source row mask."""
    rng = np.random.default_rng(5)
    for n in (1, 31, 32, 33, 1000, 69716):
        marked = rng.random(n) < (0.5 if n < 100 else 0.09)
        words = np.zeros((n + 31) // 32, np.uint32)
        idx = np.nonzero(marked)[0]
        np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
        if n % 32:
            words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(n % 32)           # garbage past the last row
        sub = capi.RowSubset(n).from_mask(DB.from_numpy(words), n, n)
        cnt = int(sub.count.numpy()[0])
        assert cnt == idx.size and np.array_equal(sub.rows.numpy()[:cnt], idx)
        small = capi.RowSubset(max(idx.size // 2, 1)).from_mask(DB.from_numpy(words), n, max(idx.size // 2, 1))
        c2 = int(small.count.numpy()[0])
        assert c2 == min(idx.size, small.capacity) and np.array_equal(small.rows.numpy()[:c2], idx[:c2])
        X = rng.standard_normal((n, 64)).astype(np.float32)
        dX = DB.from_numpy(X); capi.zero_rows(dX, 64, sub)
        want = X.copy(); want[idx] = 0
        assert np.array_equal(dX.numpy(), want)
        src = rng.standard_normal((n, 256)).astype(np.float32); dst = rng.standard_normal((n, 64)).astype(np.float32)
        dD = DB.from_numpy(dst)
        capi.copy_cols(dD, 64, DB.from_numpy(src), 256, 3, n, 50, True, rows=sub)
        want = dst.copy(); want[idx, :50] += src[idx, 3:53]
        assert np.array_equal(dD.numpy(), want)
        capi.copy_cols(dD, 64, DB.from_numpy(src), 256, 7, n, 50, False, rows=sub)
        want[idx, :50] = src[idx, 7:57]
        assert np.array_equal(dD.numpy(), want)
        # the fused form: bitmap + list from a batch's (u, i, j)
        nu = n // 2
        if nu >= 1 and n - nu >= 1:
            B = min(500, n)
            u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, n - nu, B).astype(np.int32); j = rng.integers(0, n - nu, B).astype(np.int32)
            dmask = DB.from_numpy(words)            # stale contents: the call clears it
            fused = capi.mark_compact_batch_rows(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, nu, n, dmask, capi.RowSubset(min(3 * B, n)), min(3 * B, n))
            touched = np.unique(np.concatenate([u, nu + i, nu + j]))
            c3 = int(fused.count.numpy()[0])
            assert c3 == touched.size and np.array_equal(fused.rows.numpy()[:c3], touched)
            wm = np.zeros_like(words); np.bitwise_or.at(wm, touched >> 5, (np.uint32(1) << (touched & 31).astype(np.uint32)))
            assert np.array_equal(dmask.numpy(), wm)


def test_unique_per_batch_matches_numpy():
    """qrec_unique_per_batch (tf.unique of every batch of an epoch's id stream, SimGCL.py:61-64, ascending): against
    np.unique per batch, ragged last batch, ids offset into the joint table"""
    rng = np.random.default_rng(9)
    for n, batch, id_range, off in ((10000, 2048, 31668, 0), (5000, 512, 700, 31668), (3, 2048, 10, 5), (4096, 4096, 100000, 1)):
        ids = rng.integers(0, id_range, n).astype(np.int32)
        nb = -(-n // batch)
        d_rows, d_cnt = DB.zeros(n, np.int32), DB.zeros(nb, np.int32)
        capi.unique_per_batch(DB.from_numpy(ids), n, batch, id_range, off, d_rows, d_cnt)
        rows, cnt = d_rows.numpy(), d_cnt.numpy()
        for b in range(nb):
            want = np.unique(ids[b * batch:(b + 1) * batch]) + off
            assert cnt[b] == want.size and np.array_equal(rows[b * batch:b * batch + cnt[b]], want)


@pytest.mark.parametrize("dim", [64, 50, 8, 70])
def test_ngcf_gradients_and_training_steps_match_restatement(dim):
    d, adj, A = _graph("small")
    nu, ni, B = d["n_users"], d["n_items"], 1024
    N = nu + ni
    rng = np.random.default_rng(dim)
    U0 = (rng.standard_normal((nu, dim)) * 0.1).astype(np.float32); V0 = (rng.standard_normal((ni, dim)) * 0.1).astype(np.float32)
    lim = np.sqrt(6.0 / (2 * dim))
    W = [[rng.uniform(-lim, lim, (dim, dim)).astype(np.float32) for _ in range(2)] for _ in range(2)]
    ref = T.NGCF(U0, V0, W, A, lr=0.002, reg=1e-3)
    tr = NGCFTrainer(U0, V0, W, adj, lr=0.002, reg=1e-3)
    ld = tr.ld
    for step in range(4):
        sel = rng.integers(0, d["train_u"].size, B)
        u = d["train_u"][sel].astype(np.int32); i = d["train_i"][sel].astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
        masks = [(rng.random((N, dim)) < 0.9).astype(np.float32) for _ in range(2)]
        if step == 0:   # gradients of the first step, before any update
            loss0, gE, gW = ref.loss_and_grads(u, i, j, masks)
        lref = ref.train_step(u, i, j, masks)
        tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, masks=[DB.from_numpy(pad_cols(m, ld)) for m in masks])
        check("abs(tr.loss() - lref) / abs(lref)", abs(tr.loss() - lref) / abs(lref), 1e-5)
        if step == 0:
            check("rel_err(tr.dEb.numpy()[:, :dim], gE)", rel_err(tr.dEb.numpy()[:, :dim], gE), 1e-5)
            for k in range(2):
                for t in range(2):
                    got = tr.gW[k][t].numpy()
                    check("rel_err(got[:dim, :dim], gW[k][t])", rel_err(got[:dim, :dim], gW[k][t]), 1e-5)
                    assert (got[dim:] == 0).all() and (got[:, dim:] == 0).all()
    Ug, Vg, Wg = tr.parameters()
    check("rel_err(np.concatenate([Ug, Vg]), ref.E)", rel_err(np.concatenate([Ug, Vg]), ref.E), TOL)
    for k in range(2):
        for t in range(2):
            check("rel_err(Wg[k][t], ref.W[k][t])", rel_err(Wg[k][t], ref.W[k][t]), TOL)
    Ui, Vi = tr.inference_embeddings(); Ur, Vr = ref.inference_embeddings()
    check("rel_err(Ui, Ur)", rel_err(Ui, Ur), TOL)
    check("rel_err(Vi, Vr)", rel_err(Vi, Vr), 1e-5)
    assert Ui.shape == (nu, 3 * dim)


def test_ngcf_class_trains_and_evaluates_with_device_dropout():
    from qrec_amd.model.ranking.NGCF import NGCF
    meta, z = load_golden("bpr_filmtrust")
    train, test = rows_from_golden(z)
    conf = conf_from_text(meta["conf"])
    conf["model.name"] = "NGCF"; conf["num.factors"] = "16"; conf["num.max.epoch"] = "3"; conf["batch_size"] = "1500"
    conf["learnRate"] = "-init 0.002 -max 1"; conf["reg.lambda"] = "-u 0.001 -i 0.001 -b 0.2 -s 0.2"; conf["item.ranking"] = "on -topN 5,10"
    random.seed(4); np.random.seed(4)
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = NGCF(conf, train, test); measure = m.execute()
    losses = [float(l.split("loss:")[1]) for l in buf.getvalue().splitlines() if l.startswith("training:")]
    assert len(losses) == 3 * 22 and np.isfinite(losses).all() and np.mean(losses[-22:]) < np.mean(losses[:22])
    assert m.U.shape == (meta["n_users"], 48) and m.V.shape == (meta["n_items"], 48)
    assert measure[0] == "Top 5\n" and any(x.startswith("Recall") for x in measure)
    # dropout really drops ~10% of the activations while training
    m.trainer.forward(True)
    E1 = m.trainer.E[1].numpy()[:, :16]
    assert 0.05 < (E1 == 0).mean() < 0.2


def test_spmm_sparse_operand_mask_is_bit_identical():
    d, adj, A = _graph("small")
    n = A.shape[0]
    rng = np.random.default_rng(9)
    X = np.zeros((n, 64), np.float32)
    nz = rng.permutation(n)[:n // 12]
    X[nz] = rng.standard_normal((nz.size, 64)).astype(np.float32)
    mask = np.zeros((n + 31) // 32, np.uint32)
    np.bitwise_or.at(mask, nz >> 5, (np.uint32(1) << (nz & 31).astype(np.uint32)))
    plan = SpmmPlan(adj[0], adj[1], adj[2], 64)
    dX, dY1, dY2 = DB.from_numpy(X), DB.zeros((n, 64), np.float32), DB.zeros((n, 64), np.float32)
    capi.spmm_csr(plan, dX, dY1, 64, d_addend=dX, addend_scale=1.0)
    capi.spmm_csr(plan, dX, dY2, 64, d_addend=dX, addend_scale=1.0, d_x_row_mask=DB.from_numpy(mask))
    assert np.array_equal(dY1.numpy(), dY2.numpy())
    check("rel_err(dY1.numpy(), A.dot(X) + X)", rel_err(dY1.numpy(), A.dot(X) + X), TOL)


# ---------------------------------------------------------------------------------------------
# SGL
# ---------------------------------------------------------------------------------------------
from qrec_amd.graph import SGLTrainer  # noqa: E402


@pytest.mark.parametrize("per_layer", [False, True])
def test_sgl_training_steps_match_restatement(per_layer):
    d, adj, A = _graph("small")
    nu, ni, dim, B, L = d["n_users"], d["n_items"], 64, 1024, 2
    rng = np.random.default_rng(31)
    E_n = d["train_u"].size
    def sub():
        keep = rng.permutation(E_n)[:int(E_n * 0.9)]
        a = joint_norm_adjacency(nu, ni, d["train_u"][keep], d["train_i"][keep])
        return a, sp.csr_matrix((a[2], a[1], a[0]), shape=(nu + ni,) * 2)
    s1 = [sub() for _ in range(L)] if per_layer else [sub()] * L
    s2 = [sub() for _ in range(L)] if per_layer else [sub()] * L
    U0 = (rng.standard_normal((nu, dim)) * 0.01).astype(np.float32); V0 = (rng.standard_normal((ni, dim)) * 0.01).astype(np.float32)
    ref = T.SGL(U0, V0, A, L, lr=0.001, reg=1e-3, ssl_reg=0.1, temp=0.2)
    tr = SGLTrainer(U0, V0, adj, L, lr=0.001, reg=1e-3, ssl_reg=0.1, temp=0.2, max_unique=2 * B)
    tr.set_subgraphs([x[0] for x in s1] if per_layer else s1[0][0], [x[0] for x in s2] if per_layer else s2[0][0])
    for step in range(5):
        sel = rng.integers(0, E_n, B)
        u = d["train_u"][sel].astype(np.int32); i = d["train_i"][sel].astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
        lref, rec_ref, ssl_ref = ref.train_step(u, i, j, [x[1] for x in s1], [x[1] for x in s2])
        rows = np.concatenate([unique_first_appearance(u), unique_first_appearance(i) + nu]).astype(np.int32)
        tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, DB.from_numpy(rows), rows.size)
        tot, rec, ssl = tr.losses()
        check("abs(rec - rec_ref) / abs(rec_ref)", abs(rec - rec_ref) / abs(rec_ref), 1e-5)
        check("abs(ssl - ssl_ref) / abs(ssl_ref)", abs(ssl - ssl_ref) / abs(ssl_ref), 1e-5)
    Ug, Vg = tr.ego_embeddings(); E0 = np.concatenate([U0, V0])
    check("SGL, five steps: update vs restatement's update (relative to the MOVEMENT, not the table)", rel_err(np.concatenate([Ug, Vg]) - E0, ref.E - E0), 0.0005, kind="info")
    check("rel_err(np.concatenate([Ug, Vg]), ref.E)", rel_err(np.concatenate([Ug, Vg]), ref.E), TOL)
    Um, Vm = tr.main_embeddings(); Ur, Vr = ref.final_embeddings()
    check("rel_err(Um, Ur)", rel_err(Um, Ur), TOL)
    check("rel_err(Vm, Vr)", rel_err(Vm, Vr), TOL)


@pytest.mark.parametrize("aug", [1, 0, 2])
def test_sgl_class_runs_and_stays_in_lock_step_with_the_generator(aug):
    """Drop-in SGL with config/SGL.conf's keys: per-epoch sub-graphs drawn from the CPython stream, then
    the batch stream -- the generator must end exactly where a pure-Python replay of the same draws ends."""
    from qrec_amd.model.ranking.SGL import SGL
    meta, z = load_golden("bpr_filmtrust")
    train, test = rows_from_golden(z)
    conf = conf_from_text(meta["conf"])
    conf["model.name"] = "SGL"; conf["SGL"] = f"-n_layer 2 -lambda 0.1 -droprate 0.1 -augtype {aug} -temp 0.2"
    conf["num.factors"] = "16"; conf["num.max.epoch"] = "2"; conf["batch_size"] = "2048"; conf["learnRate"] = "-init 0.001 -max 1"
    conf["reg.lambda"] = "-u 0.001 -i 0.001 -b 0.2 -s 0.2"; conf["item.ranking"] = "on -topN 20"
    random.seed(6); np.random.seed(6)
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = SGL(conf, train, test); measure = m.execute()
    out = buf.getvalue()
    rec = [float(l.split("rec_loss:")[1].split()[0]) for l in out.splitlines() if "rec_loss:" in l]
    assert len(rec) == 2 * 16 and np.isfinite(rec).all() and rec[-1] < rec[0]
    assert out.count("Quick Ranking Performance") == 2 and any(x.startswith("Recall") for x in measure)
    # pure-Python replay of the same random consumption (SGL.py:233-251 + deepRecommender.py:29-52)
    U, I, E = meta["n_users"], meta["n_items"], meta["n_train"]
    random.seed(6)
    rows = list(range(E)); item_of = z["train_iid"].tolist(); user_of = z["train_uid"].tolist()
    rated = {}
    for uu, ii in zip(user_of, item_of):
        rated.setdefault(uu, set()).add(ii)
    for ep in range(2):
        n_sub = 2 if aug in (0, 1) else 4
        for _ in range(n_sub):
            if aug == 0:
                random.sample(list(range(U)), int(U * 0.1)); random.sample(list(range(I)), int(I * 0.1))
            else:
                random.sample(list(range(E)), int(E * 0.9))
        random.shuffle(rows)
        for r in rows:
            neg = random.choice(range(I))
            while neg in rated[user_of[r]]:
                neg = random.choice(range(I))
    want = capi.state_from_python(random.getstate())
    random.seed(6); np.random.seed(6)
    with redirect_stdout(io.StringIO()):
        m2 = SGL(conf, train, test); m2.execute()
    assert np.array_equal(capi.state_from_python(random.getstate()), want)


# ---------------------------------------------------------------------------------------------
# BASELINE.json full size (config #3 / #5 shape: 31,668 x 38,048, nnz(adj) = 2.5 M, d = 64)
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yelp_graph():
    return _graph("yelp2018")


def test_spmm_yelp_shape_vs_scipy_and_operator_properties(yelp_graph):
    """The propagation operator at the bench shape: against scipy on the whole result, and through properties that
    do not need a reference at all -- linearity, symmetry of the normalised adjacency (<Ax, y> = <x, Ay>), and
    A 1 = row sums; rows that are not split are bit-identical to the sequential CSR sum."""
    d, adj, A = yelp_graph
    n = A.shape[0]
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, 64)).astype(np.float32); Y = rng.standard_normal((n, 64)).astype(np.float32)
    plan = SpmmPlan(adj[0], adj[1], adj[2], 64)
    dX, dY, dO, dO2 = DB.from_numpy(X), DB.from_numpy(Y), DB.zeros((n, 64), np.float32), DB.zeros((n, 64), np.float32)
    capi.spmm_csr(plan, dX, dO, 64); AX = dO.numpy()
    ref = A.dot(X)
    check("rel_err(AX, ref)", rel_err(AX, ref), TOL)
    whole = np.diff(adj[0]) <= 128
    assert whole.sum() > 0.95 * n and np.array_equal(AX[whole], ref[whole])
    capi.spmm_csr(plan, dY, dO2, 64); AY = dO2.numpy()
    dS = DB.from_numpy(X + Y); capi.spmm_csr(plan, dS, dO, 64)
    check("rel_err(dO.numpy(), AX + AY)", rel_err(dO.numpy(), AX + AY), 2e-6)                                   # linearity
    lhs = float((AX.astype(np.float64) * Y).sum()); rhs = float((X.astype(np.float64) * AY).sum())
    check("abs(lhs - rhs) / max(abs(lhs), 1.0)", abs(lhs - rhs) / max(abs(lhs), 1.0), 1e-5)                            # symmetry
    ones = DB.from_numpy(np.ones((n, 64), np.float32)); capi.spmm_csr(plan, ones, dO, 64)
    check_rel("A 1 vs row sums", dO.numpy()[:, 0], np.asarray(A.sum(axis=1)).ravel(), 2e-6)


def test_lightgcn_and_simgcl_steps_at_yelp_shape_match_restatement(yelp_graph):
    """One config-#3 LightGCN step (L=3, batch 2048) and one config-#5 SimGCL step (L=2, lambda 0.5, eps 0.1) at the
    full graph against the numpy/scipy restatement: losses to 2e-5, the Adam update direction on every coordinate
    whose gradient is not rounding noise."""
    d, adj, A = yelp_graph
    nu, ni, dim, B = d["n_users"], d["n_items"], 64, 2048
    N = nu + ni
    rng = np.random.default_rng(7)
    sel = rng.integers(0, d["train_u"].size, B)
    u = d["train_u"][sel].astype(np.int32); i = d["train_i"][sel].astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
    du, di, dj = DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j)
    U0 = (rng.standard_normal((nu, dim)) * 0.005).astype(np.float32); V0 = (rng.standard_normal((ni, dim)) * 0.005).astype(np.float32)
    E0 = np.concatenate([U0, V0])
    ref = T.LightGCN(U0, V0, A, 3, lr=0.001, reg=1e-4)
    tr = LightGCNTrainer(U0, V0, adj, 3, lr=0.001, reg=1e-4)
    lref = ref.train_step(u, i, j)
    tr.train_step_async(du, di, dj, B)
    check("abs(tr.loss() - lref) / abs(lref)", abs(tr.loss() - lref) / abs(lref), 1e-5)
    Eg = np.concatenate(tr.ego_embeddings())
    step_ref, step_gpu = ref.E - E0, Eg - E0
    solid = np.abs(ref.opt.m) > 1e-3 * np.abs(ref.opt.m).max()        # first Adam step = -lr*sign(g): compare where g is not noise
    assert solid.mean() > 0.2 and np.array_equal(np.sign(step_gpu[solid]), np.sign(step_ref[solid]))
    check("LightGCN first Adam step where the gradient is not rounding noise (|m| > 1e-3 max), norm-wise", rel_err(step_gpu[solid], step_ref[solid]), TOL)
    check_rel("... element by element", step_gpu[solid], step_ref[solid], 1e-4, kind="info")
    # SimGCL
    lim = np.sqrt(6.0 / (nu + dim))
    U1 = rng.uniform(-lim, lim, (nu, dim)).astype(np.float32); V1 = rng.uniform(-lim, lim, (ni, dim)).astype(np.float32)
    ref2 = T.SimGCL(U1, V1, A, 2, lr=0.001, reg=1e-4, cl_rate=0.5, eps=0.1)
    tr2 = SimGCLTrainer(U1, V1, adj, 2, lr=0.001, reg=1e-4, cl_rate=0.5, eps=0.1, max_unique=B)
    noises = [rng.random((N, dim)).astype(np.float32) for _ in range(4)]
    _, rec_ref, cl_ref = ref2.train_step(u, i, j, noises)
    uu = unique_first_appearance(u); vv = (unique_first_appearance(i) + nu).astype(np.int32)
    tr2.train_step_async(du, di, dj, B, DB.from_numpy(uu), uu.size, DB.from_numpy(vv), vv.size, noises=[DB.from_numpy(x) for x in noises])
    _, rec, cl = tr2.losses()
    check("abs(rec - rec_ref) / abs(rec_ref)", abs(rec - rec_ref) / abs(rec_ref), 1e-5)
    check("abs(cl - cl_ref) / abs(cl_ref)", abs(cl - cl_ref) / abs(cl_ref), 1e-5)


def test_ngcf_step_at_yelp_shape_matches_restatement(yelp_graph):
    """One config-#5 NGCF step (two layers, fixed by model/ranking/NGCF.py:19; batch 2048, d = 64, keep 0.9) at the FULL Yelp2018
    shape -- N = 69,716 rows through the dense MFMA kernels (ngcf.hip), the row-subset last layer and the weight-gradient partial
    sums, none of which the FilmTrust-sized golden run reaches at this size -- against the numpy/scipy restatement with the SAME
    injected dropout masks: loss, dU / dV / the four dW before Adam at 1e-5, and the first Adam step's direction and size on every
    coordinate whose gradient is not rounding noise (the first Adam step is -lr * g / (|g| + eps): a sign function of g)."""
    from helpers import pad_cols
    d, adj, A = yelp_graph
    nu, ni, dim, B = d["n_users"], d["n_items"], 64, 2048
    N = nu + ni
    rng = np.random.default_rng(17)
    sel = rng.integers(0, d["train_u"].size, B)
    u = d["train_u"][sel].astype(np.int32); i = d["train_i"][sel].astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
    U0 = (rng.standard_normal((nu, dim)) * 0.1).astype(np.float32); V0 = (rng.standard_normal((ni, dim)) * 0.1).astype(np.float32)
    lim = np.sqrt(6.0 / (2 * dim))
    W = [[rng.uniform(-lim, lim, (dim, dim)).astype(np.float32) for _ in range(2)] for _ in range(2)]
    masks = [(rng.random((N, dim)) < 0.9).astype(np.float32) for _ in range(2)]
    ref = T.NGCF(U0, V0, W, A, lr=0.002, reg=1e-3)
    tr = NGCFTrainer(U0, V0, W, adj, lr=0.002, reg=1e-3)
    lref, gE, gW = ref.loss_and_grads(u, i, j, masks)           # (20 s of numpy at this size: once; then train_step's own body)
    ref.optE.step(ref.E, gE)
    for k in range(2):
        for t in range(2):
            ref.optW[k][t].step(ref.W[k][t], gW[k][t])
    tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, masks=[DB.from_numpy(pad_cols(m, tr.ld)) for m in masks])
    check("NGCF loss at the Yelp2018 shape", abs(tr.loss() - lref) / abs(lref), 1e-5)
    gU, gV, gWg = tr.gradients()
    check("NGCF dU at the Yelp2018 shape", rel_err(gU, gE[:nu]), 1e-5)
    check("NGCF dV at the Yelp2018 shape", rel_err(gV, gE[nu:]), 1e-5)
    for k in range(2):
        for t in range(2):
            check(f"NGCF dW{t + 1} of layer {k} at the Yelp2018 shape", rel_err(gWg[k][t], gW[k][t]), 1e-5)
    Ug, Vg, Wg = tr.parameters()
    E0 = np.concatenate([U0, V0])
    step_ref, step_gpu = ref.E - E0, np.concatenate([Ug, Vg]) - E0
    solid = np.abs(gE) > 1e-3 * np.abs(gE).max()
    assert solid.mean() > 0.01 and np.array_equal(np.sign(step_gpu[solid]), np.sign(step_ref[solid]))
    check("NGCF first Adam step where the gradient is not rounding noise (tables), norm-wise", rel_err(step_gpu[solid], step_ref[solid]), TOL)
    check_rel("... element by element", step_gpu[solid], step_ref[solid], 1e-4, kind="info")
    for k in range(2):
        for t in range(2):
            sw = np.abs(gW[k][t]) > 1e-3 * np.abs(gW[k][t]).max()
            check(f"NGCF first Adam step where the gradient is not rounding noise (W{t + 1} of layer {k}), norm-wise", rel_err((Wg[k][t] - W[k][t])[sw], (ref.W[k][t] - W[k][t])[sw]), TOL)


@pytest.mark.parametrize("seg_len", [128, 7])
def test_spmm_output_row_mask_computes_exactly_the_marked_rows(seg_len):
    """d_y_row_mask: marked rows equal the unmasked product bit for bit (long rows included), all other rows of Y
    and of the accumulator keep what they held; qrec_mark_batch_rows marks {u, nu+i, nu+j}."""
    d, adj, A = _graph("small")
    n, nu, ni = A.shape[0], d["n_users"], d["n_items"]
    rng = np.random.default_rng(13)
    X = rng.standard_normal((n, 64)).astype(np.float32)
    B = 300
    u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, ni, B).astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
    heavy = int(np.argmax(np.diff(adj[0])[nu:]))              # make sure a multi-segment row is among the marked ones
    i[0] = heavy
    mask = DB.zeros((n + 31) // 32, np.uint32)
    capi.mark_batch_rows(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, nu, mask)
    rows = np.unique(np.concatenate([u, nu + i, nu + j]))
    bits = mask.numpy()
    want_bits = np.zeros_like(bits); np.bitwise_or.at(want_bits, rows >> 5, (np.uint32(1) << (rows & 31).astype(np.uint32)))
    assert np.array_equal(bits, want_bits)
    plan = SpmmPlan(adj[0], adj[1], adj[2], 64, seg_len=seg_len)
    dX, full = DB.from_numpy(X), DB.zeros((n, 64), np.float32)
    capi.spmm_csr(plan, dX, full, 64)
    Y0 = rng.standard_normal((n, 64)).astype(np.float32); S0 = rng.standard_normal((n, 64)).astype(np.float32)
    dY, dS = DB.from_numpy(Y0), DB.from_numpy(S0)
    capi.spmm_csr(plan, dX, dY, 64, d_accum=dS, d_y_row_mask=mask)
    Y, S, F = dY.numpy(), dS.numpy(), full.numpy()
    other = np.setdiff1d(np.arange(n), rows)
    assert np.array_equal(Y[rows], F[rows]) and np.array_equal(Y[other], Y0[other])
    assert np.array_equal(S[rows], S0[rows] + F[rows]) and np.array_equal(S[other], S0[other])


# ---------------------------------------------------------------------------------------------
# BUIR
# ---------------------------------------------------------------------------------------------
from qrec_amd.graph import BUIRTrainer  # noqa: E402


@pytest.mark.parametrize("L,dim", [(2, 50), (1, 64), (3, 20)])
def test_buir_training_steps_match_restatement(L, dim):
    """model/ranking/BUIR.py on the device vs the numpy restatement (oracle/tfmodels.py BUIR): losses, the online
    tables, the linear layer and the momentum tables over several steps on two different sub-graphs."""
    d, adj, A = _graph("small")
    nu, ni, B = d["n_users"], d["n_items"], 1024
    rng = np.random.default_rng(40 + L)
    n = d["train_u"].size
    def sub():
        keep = rng.permutation(n)[:n // 2]
        a = joint_norm_adjacency(nu, ni, d["train_u"][keep], d["train_i"][keep])
        return a, sp.csr_matrix((a[2], a[1], a[0]), shape=(nu + ni,) * 2)
    (ao, Ao), (at, At) = sub(), sub()
    lim = np.sqrt(6.0 / (nu + dim))
    U0 = rng.uniform(-lim, lim, (nu, dim)).astype(np.float32); V0 = rng.uniform(-lim, lim, (ni, dim)).astype(np.float32)
    W0 = rng.uniform(-0.3, 0.3, (dim, dim)).astype(np.float32); b0 = rng.uniform(-0.3, 0.3, (1, dim)).astype(np.float32)
    ref = T.BUIR(U0, V0, W0, b0, L, lr=0.001, tau=0.995)
    tr = BUIRTrainer(U0, V0, W0, b0, L, lr=0.001, tau=0.995)
    tr.set_subgraphs(ao, at)
    for step in range(6):
        sel = rng.integers(0, n, B)
        u = d["train_u"][sel].astype(np.int32); i = d["train_i"][sel].astype(np.int32)
        lref = ref.train_step(u, i, Ao, At)
        tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), B)
        check("abs(tr.loss() - lref) / abs(lref)", abs(tr.loss() - lref) / abs(lref), 1e-5)
    E0 = np.concatenate([U0, V0])
    Eg, Tg = tr.online_tables(), tr.target_tables()
    Wg, bg = tr.weights()
    check("BUIR, six steps: update vs restatement's update (relative to the MOVEMENT, not the table)", rel_err(Eg - E0, ref.E - E0), 5e-5, kind="info")
    check("rel_err(Eg, ref.E)", rel_err(Eg, ref.E), 1e-5)
    check("rel_err(Tg, ref.T)", rel_err(Tg, ref.T), 1e-5)
    check("rel_err(Wg, ref.W)", rel_err(Wg, ref.W), 1e-5)
    check("rel_err(bg, ref.b.ravel())", rel_err(bg, ref.b.ravel()), 1e-5)
    got, want = tr.final_tables(adj), ref.final_tables(A)
    for g, w in zip(got, want):
        check("rel_err(g, w)", rel_err(g, w), 1e-5)


def test_buir_class_runs_stock_conf_shape_and_replays_the_generator():
    """The drop-in BUIR class with the stock conf's options (-n_layer 2 -tau 0.995 -drop_rate 0.5): trains, ranks with
    the concatenated [o|q] tables, and leaves the CPython generator where the reference's draw sequence would
    (two random.sample sub-graphs, then shuffle + negatives, per epoch)."""
    from qrec_amd.model.ranking.BUIR import BUIR
    train, test = rows_from_golden(load_golden("bpr_filmtrust")[1])
    conf = conf_from_text("ratings=./x.txt\nratings.setup=-columns 0 1 2\nmodel.name=BUIR\nevaluation.setup=-testSet x -b 1\n"
                          "item.ranking=on -topN 10\nnum.factors=50\nnum.max.epoch=3\nbatch_size=2000\nlearnRate=-init 0.001 -max 1\n"
                          "BUIR=-n_layer 2 -tau 0.995 -drop_rate 0.5\nreg.lambda=-u 0.001 -i 0.001 -b 0.2 -s 0.2\noutput.setup=off -dir ./results/")
    random.seed(5); np.random.seed(5)
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = BUIR(conf, train, test)
        measure = m.execute()
    losses = [float(l.rsplit("loss:", 1)[1]) for l in buf.getvalue().splitlines() if "training:" in l]
    n_batches = -(-len(train) // 2000)
    assert len(losses) == 3 * n_batches and losses[-1] < losses[0] and all(np.isfinite(losses))
    assert any(x.startswith("Recall:") for x in measure)
    # replay of the host-side draws with Python's own generator
    random.seed(5)
    n = len(train)
    rated = {}
    for u, i, _ in train:
        rated.setdefault(u, set()).add(i)
    rows = [r[:] for r in train]
    items = list(dict.fromkeys(r[1] for r in train))
    for _ in range(3):
        random.sample(list(range(n)), int(n * 0.5)); random.sample(list(range(n)), int(n * 0.5))
        random.shuffle(rows)
        for u, _, _ in rows:
            neg = random.choice(items)
            while neg in rated[u]:
                neg = random.choice(items)
    want_state = random.getstate()
    assert np.array_equal(capi.state_from_python(want_state), capi.state_from_python(m._final_py_state))


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["LightGCN", "NGCF", "SimGCL", "SGL", "BUIR", "SEPT", "MHCN"])
def test_graph_models_data_parallel_two_ranks_equal_one_rank_with_double_batch(name, tmp_path):
    """one process per GPU, every step's rows split over the ranks, ONE all-reduce of the dense
    table gradient (+ NGCF's weight gradients) per step, test users sharded at evaluation.  Two real processes (both on
    device 0, gloo) with batch_size B must give what one process gives with batch_size 2B -- same batch stream, same
    initial tables, same dropout / noise streams -- up to fp32 summation order, and the replicas must stay IDENTICAL."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(root, "tests", "graph_dp_worker.py")
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir(); two.mkdir()
    env = dict(os.environ, QREC_SEED="11", QREC_DIST_TEST_ONE_DEVICE="1")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    r1 = subprocess.run([sys.executable, worker, name, "2048", str(one)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-3000:]
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", "29547", worker, name, "1024", str(two)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-3000:]
    a, b0, b1 = np.load(one / "rank0.npz"), np.load(two / "rank0.npz"), np.load(two / "rank1.npz")
    for k in ("U", "V", "E", "losses", "measure"):
        assert np.array_equal(b0[k], b1[k]), k                      # replicas bit-identical, same measures on both ranks
    assert a["losses"].size == b0["losses"].size > 0
    # SEPT's pseudo labels are discrete: a near-tie in the averaged softmax can resolve differently under another
    # summation order and move that row's positives, so its two runs agree to a looser bound (the replicas above do not)
    # (observed, profiles/r03_parity_errors.json: every model but SEPT <= 7e-8 on the losses and <= 6e-7 on the tables; SEPT
    # 2.3e-5 / 2.2e-3 -- a moved pseudo label is a different positive set for that row from then on)
    check_rel(f"{name}: two ranks (batch split) vs one rank (double batch), losses of the whole run", b0["losses"], a["losses"], 2e-4 if name == "SEPT" else TOL, kind="partition")
    tol = 2e-2 if name == "SEPT" else TOL
    check(f"{name}: two ranks vs one rank, ego table after the run", rel_err(b0["E"], a["E"]), tol, kind="partition")
    check(f"{name}: two ranks vs one rank, scoring users after the run", rel_err(b0["U"], a["U"]), tol, kind="partition")
    check(f"{name}: two ranks vs one rank, scoring items after the run", rel_err(b0["V"], a["V"]), tol, kind="partition")
    np.testing.assert_allclose(b0["measure"], a["measure"], atol=2e-3)
    assert len(os.listdir(two / "results")) == len(os.listdir(one / "results"))      # rank 0 alone wrote the result files


@pytest.mark.parametrize("model,port", [("LightGCN", 29553), ("NGCF", 29557), ("SimGCL", 29559)])
def test_graph_class_row_partitioned_two_ranks_equal_one_rank_at_the_same_batch_size(tmp_path, model, port):
    """QREC_GRAPH_DIST=rows: the drop-in LightGCN / NGCF / SimGCL class on two ranks with the node tables row-
    partitioned -- the reference's own batch size on every rank, each rank's SpMM (and, NGCF, dense layers) over its rows
    only, NGCF's weight gradients all-reduced -- must train what one rank trains with that batch size (not 2x the batch, as
    the batch-sharded scheme does): same losses, same final embeddings and measures up to fp32 summation order.  NGCF's
    device-drawn dropout is keyed by the table row, so both runs drop the same entries."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker = os.path.join(root, "tests", "graph_dp_worker.py")
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir(); two.mkdir()
    env = dict(os.environ, QREC_SEED="11", QREC_DIST_TEST_ONE_DEVICE="1", QREC_GRAPH_DIST="rows")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    r1 = subprocess.run([sys.executable, worker, model, "1024", str(one)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-3000:]
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", str(port), worker, model, "1024", str(two)], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-3000:]
    a, b0, b1 = np.load(one / "rank0.npz"), np.load(two / "rank0.npz"), np.load(two / "rank1.npz")
    for k in ("U", "V", "measure"):
        assert np.array_equal(b0[k], b1[k]), k                      # both ranks gathered the same tables, same measures
    check_rel("rank 0 vs rank 1 losses", b0["losses"], b1["losses"], 1e-6)   # every rank sums the batch loss itself (float atomics: own order)
    assert a["losses"].size == b0["losses"].size > 0
    check_rel(f"{model}: row-partitioned two ranks vs one rank, losses of the whole run", b0["losses"], a["losses"], 5e-4 if model == "NGCF" else TOL, kind="partition")
    # NGCF / SimGCL: ~70 Adam steps carry the summation-order differences of the float atomics along (coordinates with a
    # rounding-noise gradient move by +-alpha per step whatever the implementation; run-to-run 2e-4 .. 2e-3); the step-level
    # equivalence at 5e-5 is tests/test_gpu_dist.py::test_row_partitioned_{ngcf,simgcl}_step_equals_the_single_gpu_step
    tol = 1e-2 if model == "NGCF" else TOL      # observed: LightGCN 6e-8, SimGCL 9e-8, NGCF 5e-3 (see the note above)
    check(f"{model}: row-partitioned two ranks vs one rank, scoring users after ~70 Adam steps", rel_err(b0["U"], a["U"]), tol, kind="partition")
    check(f"{model}: row-partitioned two ranks vs one rank, scoring items after ~70 Adam steps", rel_err(b0["V"], a["V"]), tol, kind="partition")
    assert not np.array_equal(b0["E"], b1["E"]) and b0["E"].shape[0] + b1["E"].shape[0] >= a["E"].shape[0]   # each rank holds ITS rows
    np.testing.assert_allclose(b0["measure"], a["measure"], atol=1e-4 if model == "LightGCN" else 5e-3)


# ---------------------------------------------------------------------------------------------
# SEPT (model/ranking/SEPT.py)
# ---------------------------------------------------------------------------------------------
from qrec_amd.graph import SEPTTrainer  # noqa: E402


def _sept_problem(rng, nu=300, ni=400, E=5000, R=1500):
    uid = rng.integers(0, nu, E); iid = rng.integers(0, ni, E)
    fo = rng.integers(0, nu, R); fe = rng.integers(0, nu, R)
    social, sharing = T.sept_social_views(nu, ni, uid, iid, fo, fe)
    adj = T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe)
    sub = T.sept_sub_adjacency(nu, ni, uid, iid, fo, fe, rng.permutation(E)[:int(E * 0.7)], rng.permutation(R)[:int(R * 0.7)])
    return nu, ni, adj, social, sharing, sub


@pytest.mark.parametrize("dim,ld", [(16, 32), (50, 64), (64, 64)])
def test_l2norm_layer_kernels_match_restatement(dim, ld):
    """qrec_l2norm_rows_accum / _bwd / qrec_scale_copy: S += l2_normalize(x) with tf's 1e-12 clamp (all-zero rows
    included) and its gradient, vs the restatement."""
    rng = np.random.default_rng(3)
    n = 1000
    X = rng.standard_normal((n, dim)).astype(np.float32); X[5] = 0; X[77] *= 1e-4
    S0 = rng.standard_normal((n, dim)).astype(np.float32); dS = rng.standard_normal((n, dim)).astype(np.float32)
    z, inv = T.l2_normalize_rows(X)
    d_S, d_inv = DB.from_numpy(pad_cols(S0, ld)), DB.zeros(n, np.float32)
    d_X = DB.from_numpy(pad_cols(X, ld))
    capi.l2norm_rows_accum(d_X, n, ld, d_S, d_inv)
    check_rel("1/|row|", d_inv.numpy(), inv, 2e-6)
    check_rel("S0 + normalised rows", d_S.numpy()[:, :dim], S0 + z, 1e-5, abs_tol=1e-6)
    assert not d_S.numpy()[:, dim:].any() and d_inv.numpy()[5] == np.float32(1e6)
    d_out = DB.zeros((n, ld), np.float32)
    capi.l2norm_rows_bwd(d_X, d_inv, DB.from_numpy(pad_cols(dS, ld)), n, ld, d_out)
    want = T.l2_normalize_bwd(X, inv, dS)
    check("rel_err(d_out.numpy()[:, :dim], want)", rel_err(d_out.numpy()[:, :dim], want), 2e-6)
    np.testing.assert_array_equal(d_out.numpy()[5, :dim], dS[5] * np.float32(1e6))      # at the clamp: d * 1e6, like tf
    capi.scale_copy(d_out, d_X, n * ld, 0.5)
    np.testing.assert_array_equal(d_out.numpy()[:, :dim], X / np.float32(2))


@pytest.mark.parametrize("n,dim,ld,k", [(700, 50, 64, 10), (64, 16, 32, 3), (1999, 64, 64, 10), (4200, 16, 32, 4)])
def test_sept_pseudo_labels_and_neighbour_discrimination_match_restatement(n, dim, ld, k):
    """qrec_sept_ssl_loss_grad vs SEPT.py:214-262 restated: pseudo labels (top-k of the other two encoders' averaged
    softmax rows; a near-tie may legitimately resolve differently, so agreement is checked at 99.5 % and the loss /
    gradients with the device's own labels), the several-positives InfoNCE loss and the gradients of all four tables."""
    rng = np.random.default_rng(n)
    N = 6000
    tabs = [(rng.standard_normal((N, dim)) * rng.uniform(0.5, 2.0)).astype(np.float32) for _ in range(4)]
    tabs[3] = (0.6 * tabs[2] + 0.8 * tabs[3]).astype(np.float32)              # correlated views: informative predictions
    rows = rng.permutation(N)[:n].astype(np.int32)
    d_S = [DB.from_numpy(pad_cols(t, ld)) for t in tabs]
    d_dS = [DB.zeros((N, ld), np.float32) for _ in range(4)]
    ws = DB(capi.sept_ssl_workspace_bytes(n, ld, k), np.uint8)
    loss, labels = DB.zeros(1, np.float64), DB((3, n, k), np.int32)
    capi.sept_ssl_loss_grad(*d_S, DB.from_numpy(rows), n, ld, k, 0.25, ws, *d_dS, loss, labels)
    got_labels = labels.numpy()
    _, ref_labels, _ = T.sept_ssl_loss_and_grads(*(t[rows] for t in tabs), k)
    agree = np.mean([np.array_equal(a, b) for a, b in zip(got_labels.reshape(-1, k), np.asarray(ref_labels).reshape(-1, k))])
    assert agree > 0.995, agree
    assert all(len(set(r)) == k and min(r) >= 0 and max(r) < n for r in got_labels.reshape(-1, k).tolist())
    nd, _, dx = T.sept_ssl_loss_and_grads(*(t[rows] for t in tabs), k, labels=list(got_labels))
    check_rel("neighbour-discrimination loss", float(loss.numpy()[0]), nd, 1e-5)
    for d_d, g in zip(d_dS, dx):
        out = d_d.numpy()
        check("rel_err(out[rows, :dim], np.float32(0.25) * g)", rel_err(out[rows, :dim], np.float32(0.25) * g), 1e-5)
        rest = np.ones(N, bool); rest[rows] = False
        assert not out[rest].any() and not out[:, dim:].any()
    with pytest.raises(capi.QRecError, match="ins_cnt"):
        capi.sept_ssl_loss_grad(*d_S, DB.from_numpy(rows), 2, ld, 3, 0.25, ws, *d_dS, loss, None)


@pytest.mark.parametrize("L", [1, 2])
def test_sept_training_steps_match_restatement(L):
    """SEPTTrainer vs the restated model: recommendation-only steps (Adam #1), then joint steps on a perturbed graph
    (Adam #2; non-symmetric views -> transposed plans in the backward pass), losses and variables."""
    rng = np.random.default_rng(40 + L)
    nu, ni, adj, social, sharing, sub = _sept_problem(rng)
    dim, B, k = 24, 256, 5
    U0 = (rng.standard_normal((nu, dim)) * 0.1).astype(np.float32); V0 = (rng.standard_normal((ni, dim)) * 0.1).astype(np.float32)
    ref = T.SEPT(U0, V0, adj, social, sharing, L, lr=0.002, reg=0.01, ss_rate=0.05, ins_cnt=k)
    tr = SEPTTrainer(U0, V0, adj.astype(np.float32), social, sharing, L, 0.002, 0.01, 0.05, k, max_unique=B)
    tr.set_perturbed_graph(sub)
    assert tr.aug.planT is not tr.aug.plan and tr.friend.planT is not tr.friend.plan
    for step in range(6):
        u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, ni, B).astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
        joint = step >= 3
        uu = T.unique_first_appearance(u).astype(np.int32)
        tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, joint, DB.from_numpy(uu), uu.size, keep_labels=joint)
        got = tr.losses()
        want = ref.train_step(u, i, j, sub if joint else None, labels=list(tr.d_labels.numpy()) if joint else None)
        check_rel("SEPT rec loss", got[0], want[0], 1e-5); check_rel("SEPT ssl loss", got[1], want[1], 1e-5, abs_tol=1e-9)
        Ug, Vg = tr.variables()
        check("rel_err(np.concatenate([Ug, Vg]), ref.W)", rel_err(np.concatenate([Ug, Vg]), ref.W), 1e-5, ctx=step)
    assert ref.opt1.t == 3 and ref.opt2.t == 3
    Ur, Vr = ref.rec_embeddings(); Ud, Vd = tr.rec_embeddings()
    check("rel_err(Ud, Ur)", rel_err(Ud, Ur), 1e-5)
    check("rel_err(Vd, Vr)", rel_err(Vd, Vr), 1e-5)


def test_sept_class_runs_stock_conf_shape_with_social_data_and_replays_the_generator(tmp_path):
    """Drop-in SEPT with config/SEPT.conf's keys on FilmTrust + its trust file (the fixture's raw relation list):
    relation loader -> SocialRecommender pruning -> views -> first third of the epochs recommendation only, then joint
    training on a per-epoch perturbed graph; evaluated every epoch, best epoch kept; the CPython generator must end
    where a pure-Python replay of the reference's draws (SEPT.py:86,92 + deepRecommender.py:29-52) ends."""
    from qrec_amd.model.ranking.SEPT import SEPT
    from qrec_amd.util.io import FileIO
    meta, z = load_golden("sept_graphs_filmtrust")
    name = lambda c: f"u{c}" if c >= 0 else f"x{-1 - c}"
    path = tmp_path / "trust.txt"
    path.write_text("".join(f"{name(a)} {name(b)} {w:g}\n" for a, b, w in zip(z["raw_follower"].tolist(), z["raw_followee"].tolist(), z["raw_weight"].tolist())))
    conf = conf_from_text(meta["conf"])
    conf["num.factors"] = "16"; conf["num.max.epoch"] = "6"; conf["batch_size"] = "2000"; conf["learnRate"] = "-init 0.002 -max 1"
    conf["SEPT"] = "-n_layer 2 -ss_rate 0.005 -drop_rate 0.3 -ins_cnt 10"
    uid, iid = z["train_uid"].tolist(), z["train_iid"].tolist()
    train = [[f"u{u}", f"i{i}", 1.0] for u, i in zip(uid, iid)]
    test = [[f"u{u}", f"i{(i * 7 + 3) % meta['n_items']}", 1.0] for u, i in zip(uid[::19], iid[::19])]

    def run():
        random.seed(21); np.random.seed(21)
        buf = io.StringIO()
        with redirect_stdout(buf):
            m = SEPT(conf, [list(r) for r in train], [list(r) for r in test], FileIO.loadRelationship(conf, str(path)))
            measure = m.execute()
        return m, measure, buf.getvalue()
    m, measure, out = run()
    assert len(m.social.relation) == meta["relations_kept"]
    rec = [float(l.split("rec loss:")[1].split()[0]) for l in out.splitlines() if "rec loss:" in l]
    con = [float(l.split("con_loss:")[1]) for l in out.splitlines() if "con_loss:" in l]
    n_batches = -(-len(train) // 2000)
    assert len(rec) == 6 * n_batches and len(con) == 3 * n_batches             # epochs 0-2 alone, 3-5 joint (epoch > 6/3)
    assert np.isfinite(rec).all() and np.isfinite(con).all() and rec[-1] < rec[0] and all(c > 0 for c in con)
    assert out.count("Quick Ranking Performance") == 6 and any(x.startswith("Recall") for x in measure)
    assert m.U is m.bestU and m.U.shape == (meta["n_users"], 16) and m.trainer.opt[0].n and m.trainer.opt[1].b1p < m.trainer.opt[1].b1
    # replay of the random consumption
    E, R, I = len(train), meta["relations_kept"], meta["n_items"]
    random.seed(21)
    rows = list(range(E)); rated = {}
    for uu, ii in zip(uid, iid):
        rated.setdefault(uu, set()).add(ii)
    for ep in range(6):
        if ep > 6 / 3:
            random.sample(list(range(E)), int(E * 0.7)); random.sample(list(range(R)), int(R * 0.7))
        random.shuffle(rows)
        for r in rows:
            neg = random.choice(range(I))
            while neg in rated[uid[r]]:
                neg = random.choice(range(I))
    want = capi.state_from_python(random.getstate())
    run()
    assert np.array_equal(capi.state_from_python(random.getstate()), want)


# ---------------------------------------------------------------------------------------------
# MHCN (model/ranking/MHCN.py)
# ---------------------------------------------------------------------------------------------
from qrec_amd.graph import MHCNTrainer  # noqa: E402


def _mhcn_problem(rng, nu=300, ni=260, d=24, E=5000, Rn=1800):
    uid = rng.integers(0, nu, E); iid = rng.integers(0, ni, E)
    pairs = np.unique(np.stack([uid, iid], 1), axis=0); uid, iid = pairs[:, 0], pairs[:, 1]
    fo = rng.integers(0, nu, Rn); fe = rng.integers(0, nu, Rn)
    rel = np.unique(np.stack([fo[fo != fe], fe[fo != fe]], 1), axis=0)
    H = T.mhcn_motif_adjacencies(nu, ni, uid, iid, rel[:, 0], rel[:, 1])
    Rm = T.mhcn_joint_adjacency(nu, ni, uid, iid, np.ones(uid.size))
    lim = np.sqrt(6.0 / (2 * d))
    w = {}
    for k in (1, 2, 3, 4):
        for pre in ("gating", "sgating"):
            w[f"{pre}{k}"] = rng.uniform(-lim, lim, (d, d)).astype(np.float32)
            w[f"{pre}_bias{k}"] = rng.uniform(-0.5, 0.5, (1, d)).astype(np.float32)
    w["attention"] = rng.uniform(-0.5, 0.5, (1, d)).astype(np.float32); w["attention_mat"] = rng.uniform(-lim, lim, (d, d)).astype(np.float32)
    U0 = (rng.standard_normal((nu, d)) * 0.3).astype(np.float32); V0 = (rng.standard_normal((ni, d)) * 0.3).astype(np.float32)
    return nu, ni, d, H, Rm, w, U0, V0


def _perms(rng, nu, d):
    return [(rng.permutation(nu), rng.permutation(d), rng.permutation(nu), rng.permutation(d), rng.permutation(nu)) for _ in range(3)]


@pytest.mark.parametrize("dim,ld", [(24, 32), (50, 64), (64, 64)])
def test_mhcn_gate_attention_and_mim_kernels_match_restatement(dim, ld):
    """qrec_gate_fwd/_bwd (+ qrec_buir_wgrad for dW, db), qrec_channel_attention_fwd/_bwd and qrec_hss_loss_grad against
    the restated pieces of MHCN.py:109-121,184-206, one by one."""
    rng = np.random.default_rng(dim)
    nu, ni, d, H, Rm, w, U0, V0 = _mhcn_problem(rng, d=dim)
    m = T.MHCN(U0, V0, w, H, Rm, 1, lr=0.001, reg=0.01, ss_rate=0.05)
    pad2 = lambda a: pad_cols(np.pad(a, ((0, ld - dim), (0, 0))), ld)
    # --- gate
    W, b = w["gating2"], w["gating_bias2"]
    Y, bwd = m.gate(U0, W, b)
    dY = rng.standard_normal((nu, dim)).astype(np.float32)
    dX, dW, db = bwd(dY)
    d_X, d_W, d_b = DB.from_numpy(pad_cols(U0, ld)), DB.from_numpy(pad2(W)), DB.from_numpy(pad_cols(b, ld)[0])
    d_Y, d_S, d_Q, d_dX = (DB.zeros((nu, ld), np.float32) for _ in range(4))
    capi.gate_fwd(d_X, d_W, d_b, nu, ld, d_Y, d_S)
    check("rel_err(d_Y.numpy()[:, :dim], Y)", rel_err(d_Y.numpy()[:, :dim], Y), 2e-6)
    assert not d_Y.numpy()[:, dim:].any()
    prev = rng.standard_normal((nu, dim)).astype(np.float32); d_dX.upload(pad_cols(prev, ld))
    capi.gate_bwd(d_X, d_S, DB.from_numpy(pad_cols(dY, ld)), d_W, nu, dim, ld, d_Q, d_dX, True)
    check("rel_err(d_dX.numpy()[:, :dim], prev + dX)", rel_err(d_dX.numpy()[:, :dim], prev + dX), 5e-6)
    assert not d_dX.numpy()[:, dim:].any()
    gW, gb = DB.zeros((ld, ld), np.float32), DB.zeros(ld, np.float32)
    capi.buir_wgrad(d_X, d_Q, nu, ld, DB(capi.buir_wgrad_scratch_bytes(ld), np.uint8), gW, gb)
    check("rel_err(gW.numpy()[:dim, :dim], dW)", rel_err(gW.numpy()[:dim, :dim], dW), 1e-5)
    check("rel_err(gb.numpy()[:dim], db[0])", rel_err(gb.numpy()[:dim], db[0]), 1e-5)
    # --- channel attention
    es = [rng.standard_normal((nu, dim)).astype(np.float32) for _ in range(3)]
    half = rng.standard_normal((nu, dim)).astype(np.float32)
    out, score, abwd = m.attention(es)
    dOut = rng.standard_normal((nu, dim)).astype(np.float32)
    des, da, dM = abwd(dOut)
    d_e = [DB.from_numpy(pad_cols(e, ld)) for e in es]
    d_a, d_M = DB.from_numpy(pad_cols(w["attention"], ld)[0]), DB.from_numpy(pad2(w["attention_mat"]))
    d_v, d_dv, d_sc, d_out = DB.zeros(256, np.float32), DB.zeros(capi.channel_attention_scratch_floats(), np.float32), DB.zeros((nu, 4), np.float32), DB.zeros((nu, ld), np.float32)
    capi.channel_attention_fwd(d_e, d_a, d_M, DB.from_numpy(pad_cols(half, ld)), nu, ld, d_v, d_sc, d_out)
    check("rel_err(d_out.numpy()[:, :dim], out + half / 2)", rel_err(d_out.numpy()[:, :dim], out + half / 2), 5e-6)
    check("rel_err(d_sc.numpy()[:, :3], score)", rel_err(d_sc.numpy()[:, :3], score), 5e-6)
    d_de = [DB.zeros((nu, ld), np.float32) for _ in range(3)]
    d_dh = DB.from_numpy(pad_cols(prev, ld))
    g_a, g_M = DB.zeros(ld, np.float32), DB.zeros((ld, ld), np.float32)
    capi.channel_attention_bwd(DB.from_numpy(pad_cols(dOut, ld)), d_e, d_sc, d_v, d_a, d_M, nu, ld, d_de, False, d_dh, True, d_dv, g_a, g_M)
    for k in range(3):
        check("rel_err(d_de[k].numpy()[:, :dim], des[k])", rel_err(d_de[k].numpy()[:, :dim], des[k]), 1e-5)
    check("rel_err(d_dh.numpy()[:, :dim], prev + dOut / 2)", rel_err(d_dh.numpy()[:, :dim], prev + dOut / 2), 1e-6)
    check("rel_err(g_a.numpy()[:dim], da[0])", rel_err(g_a.numpy()[:dim], da[0]), 1e-5)
    check("rel_err(g_M.numpy()[:dim, :dim], dM)", rel_err(g_M.numpy()[:dim, :dim], dM), 1e-5)
    # --- hierarchical mutual information, channel 0 and the dense purchase channel
    for ch in (0, 2):
        em = (rng.standard_normal((nu, dim)) * 0.5).astype(np.float32)
        perm = _perms(rng, nu, dim)[0]
        want_loss, want_dem = m.hss(em, m.H[ch], perm)
        from qrec_amd.graph import SpmmPlan, _csr_triple
        plan, planT = SpmmPlan(*_csr_triple(H[ch]), ld), SpmmPlan(*_csr_triple(H[ch].T), ld)
        d_em, d_edge, d_dem, d_dedge, d_tot = (DB.zeros((nu, ld), np.float32) for _ in range(5))
        d_em.upload(pad_cols(em, ld))
        capi.spmm_csr(plan, d_em, d_edge, ld)
        p1, k2, p2, k3, p3 = (np.asarray(x, np.int32) for x in perm)
        inv = lambda p: np.argsort(p).astype(np.int32)
        bufs = [DB.from_numpy(x) for x in (p1, inv(p1), p2, inv(p2), k2, inv(k2), p3, inv(p3), k3, inv(k3))]
        loss = DB.zeros(1, np.float64)
        capi.hss_loss_grad(d_em, d_edge, nu, dim, ld, bufs, 1.0, DB(capi.hss_scratch_bytes(nu), np.uint8), d_dem, d_dedge, loss)
        capi.spmm_csr(planT, d_dedge, d_tot, ld, d_addend=d_dem, addend_scale=1.0)
        check_rel("MIM loss", float(loss.numpy()[0]), want_loss, 1e-5)
        check("rel_err(d_tot.numpy()[:, :dim], want_dem)", rel_err(d_tot.numpy()[:, :dim], want_dem), 1e-5)
        assert not d_tot.numpy()[:, dim:].any()


def test_device_permutations_are_permutations_and_look_uniform():
    """qrec_random_permutation (Philox keys + rocPRIM radix sort) and qrec_small_permutations (Fisher-Yates): valid
    permutations with correct inverses, different per stream id, reproducible, positions uniformly spread."""
    n = 31668
    ws = DB(capi.random_permutations_scratch_bytes(n, 6), np.uint8)
    p, q = DB((6, n), np.int32), DB((6, n), np.int32)
    capi.random_permutations(n, 6, 7, 3, ws, p, q)
    seen = [r.copy() for r in p.numpy()]
    for a, b in zip(seen, q.numpy()):
        assert np.array_equal(np.sort(a), np.arange(n)) and np.array_equal(a[b], np.arange(n))
    capi.random_permutations(n, 6, 7, 3, ws, p, None)
    assert np.array_equal(p.numpy()[5], seen[5]) and not np.array_equal(seen[0], seen[1])
    capi.random_permutations(n, 6, 7, 4, ws, p, None)
    assert not np.array_equal(p.numpy()[0], seen[0])
    first = np.array([s[0] for s in seen]); assert len(set(first.tolist())) == 6
    # mean displacement of a uniform permutation is n/3
    disp = np.mean([np.abs(s - np.arange(n)).mean() for s in seen])
    assert abs(disp / (n / 3) - 1) < 0.02
    cp, ci = DB((64, 50), np.int32), DB((64, 50), np.int32)
    capi.small_permutations(50, 64, 3, 9, cp, ci)
    P_, I_ = cp.numpy(), ci.numpy()
    assert all(np.array_equal(np.sort(r), np.arange(50)) for r in P_) and all(np.array_equal(r[i], np.arange(50)) for r, i in zip(P_, I_))
    counts = np.bincount(P_[:, 0], minlength=50); assert counts.max() <= 8            # 64 draws over 50 values


@pytest.mark.parametrize("L", [1, 2])
def test_mhcn_training_steps_match_restatement(L):
    """MHCNTrainer vs the restated model over several steps with the same injected shuffles: rec loss, self-supervised
    loss, and after Adam all 20 parameter tensors."""
    rng = np.random.default_rng(60 + L)
    nu, ni, d, H, Rm, w, U0, V0 = _mhcn_problem(rng)
    ref = T.MHCN(U0, V0, w, H, Rm, L, lr=0.002, reg=0.01, ss_rate=0.05)
    tr = MHCNTrainer(U0, V0, w, H, Rm, L, 0.002, 0.01, 0.05)
    B = 256
    for step in range(4):
        u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, ni, B).astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
        perms = _perms(rng, nu, d)
        want_rec, want_ss, _, _ = ref.loss_and_grads(u, i, j, perms)
        ref.train_step(u, i, j, perms)
        tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, perms=perms)
        rec, ss = tr.losses()
        check_rel("MHCN rec loss", rec, want_rec, 1e-5, ctx=step); check_rel("MHCN ss loss", ss, want_ss, 1e-5, ctx=step)
        got = tr.parameters()
        for k in ref.w:
            check("rel_err(got[k], ref.w[k])", rel_err(got[k], ref.w[k]), 1e-5, ctx=(step, k))
        check("rel_err(got['U'], ref.U)", rel_err(got["U"], ref.U), 1e-5, ctx=step)
        check("rel_err(got['V'], ref.V)", rel_err(got["V"], ref.V), 1e-5, ctx=step)
    fu, fi, _ = ref.forward()
    Ud, Vd = tr.final_embeddings()
    check("rel_err(Ud, fu)", rel_err(Ud, fu), 1e-5)
    check("rel_err(Vd, fi)", rel_err(Vd, fi), 1e-5)
    # without injected shuffles the device draws its own, new ones every step
    tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B)
    a = tr.rowp.numpy().copy()
    tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B)
    b = tr.rowp.numpy()
    assert all(np.array_equal(np.sort(r), np.arange(nu)) for r in a) and not np.array_equal(a, b) and np.isfinite(tr.losses()).all()
    assert len({tuple(r[:8]) for r in a}) == 9


def test_mhcn_class_runs_stock_conf_shape_with_social_data(tmp_path):
    """Drop-in MHCN with config/MHCN.conf's keys on FilmTrust + its trust file: relation loader -> pruning -> motif
    graphs -> training with device-drawn shuffles, evaluated every epoch, best epoch kept; the CPython generator ends
    where the batch stream alone leaves it (the shuffles of the mutual-information loss are TF-side randomness)."""
    from qrec_amd.model.ranking.MHCN import MHCN
    from qrec_amd.util.io import FileIO
    meta, z = load_golden("mhcn_graphs_filmtrust")
    sz = load_golden("sept_graphs_filmtrust")[1]
    name = lambda c: f"u{c}" if c >= 0 else f"x{-1 - c}"
    path = tmp_path / "trust.txt"
    path.write_text("".join(f"{name(a)} {name(b)} {w:g}\n" for a, b, w in zip(sz["raw_follower"].tolist(), sz["raw_followee"].tolist(), sz["raw_weight"].tolist())))
    conf = conf_from_text(meta["conf"])
    conf["num.factors"] = "16"; conf["num.max.epoch"] = "3"; conf["learnRate"] = "-init 0.002 -max 1"
    uid, iid = z["train_uid"].tolist(), z["train_iid"].tolist()
    train = [[f"u{u}", f"i{i}", 1.0] for u, i in zip(uid, iid)]
    test = [[f"u{u}", f"i{(i * 7 + 3) % meta['n_items']}", 1.0] for u, i in zip(uid[::19], iid[::19])]
    random.seed(23); np.random.seed(23)
    buf = io.StringIO()
    with redirect_stdout(buf):
        m = MHCN(conf, train, test, FileIO.loadRelationship(conf, str(path)))
        measure = m.execute()
    out = buf.getvalue()
    assert len(m.social.relation) == meta["relations_kept"]
    rec = [float(l.split("rec loss:")[1]) for l in out.splitlines() if "rec loss:" in l]
    n_batches = -(-len(train) // 2000)
    assert len(rec) == 3 * n_batches and np.isfinite(rec).all() and np.mean(rec[-n_batches:]) < np.mean(rec[:n_batches])
    assert out.count("Quick Ranking Performance") == 3 and any(x.startswith("Recall") for x in measure)
    assert m.U is m.bestU and m.U.shape == (meta["n_users"], 16) and m.V.shape == (meta["n_items"], 16)
    # generator: shuffle + negatives only
    E, I = len(train), meta["n_items"]
    random.seed(23)
    rows = list(range(E)); rated = {}
    for uu, ii in zip(uid, iid):
        rated.setdefault(uu, set()).add(ii)
    for ep in range(3):
        random.shuffle(rows)
        for r in rows:
            neg = random.choice(range(I))
            while neg in rated[uid[r]]:
                neg = random.choice(range(I))
    want = capi.state_from_python(random.getstate())
    random.seed(23); np.random.seed(23)
    with redirect_stdout(io.StringIO()):
        MHCN(conf, train, test, FileIO.loadRelationship(conf, str(path))).execute()
    assert np.array_equal(capi.state_from_python(random.getstate()), want)


@pytest.mark.parametrize("model,extra", [("SEPT", "SEPT=-n_layer 2 -ss_rate 0.005 -drop_rate 0.3 -ins_cnt 5"), ("TBPR", "TBPR=-regT 0.01")])
def test_social_models_run_from_conf_files_with_cross_validation(tmp_path, model, extra):
    """``python -m qrec_amd.main <conf>`` with a ``social`` file and ``-cv 2`` (QRec.py:44-46, 62-101): the relation list is
    loaded once, every fold's model is built in the parent WITH it (and prunes it to its own training users), runs in its
    own process, and the averaged measures are written."""
    import os, subprocess, sys
    rng = np.random.default_rng(33)
    n = 6000
    rows = [f"user{u} item{i} {r}" for u, i, r in zip(rng.integers(0, 150, n), rng.integers(0, 220, n), rng.choice([1, 2, 3, 4, 5], n))]
    (tmp_path / "ratings.txt").write_text("\n".join(rows) + "\n")
    rel = {(int(a), int(b)) for a, b in zip(rng.integers(0, 170, 900), rng.integers(0, 170, 900)) if a != b}     # users 150..169 never rate
    (tmp_path / "trust.txt").write_text("".join(f"user{a}\tuser{b}\n" for a, b in sorted(rel)))
    conf = {"ratings": "./ratings.txt", "social": "./trust.txt", "ratings.setup": "-columns 0 1 2", "social.setup": "-columns 0 1",
            "model.name": model, "evaluation.setup": "-cv 2 -b 1", "item.ranking": "on -topN 10", "num.factors": "16",
            "num.max.epoch": "3", "batch_size": "512", "learnRate": "-init 0.01 -max 1", "reg.lambda": "-u 0.01 -i 0.01 -b 0.2 -s 0.2",
            "output.setup": "off -dir ./results/"}
    (tmp_path / "m.conf").write_text("".join(f"{k}={v}\n" for k, v in conf.items()) + extra + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""), QREC_QUIET="1")
    run = subprocess.run([sys.executable, "-m", "qrec_amd.main", "m.conf"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert "loading social data..." in run.stdout and "The result of 2-fold cross validation:" in run.stdout
    out = list((tmp_path / "results").glob(f"{model}@*-2-fold-cv.txt"))
    assert len(out) == 1
    res = out[0].read_text().splitlines()
    assert [r.split(":")[0] for r in res] == ["Top 10", "Precision", "Recall", "F1", "NDCG"]
    assert all(0.0 <= float(r.split(":")[1]) <= 1.0 for r in res[1:])
