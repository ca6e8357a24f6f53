"""The workspaces of the entry points that are NOT told their buffer's size (csrc/common.h, Carver: each layout is stated once and
the size entry point walks it on a null base).  Per entry point, at the smallest shape its own tests use: a buffer of exactly
the stated bytes followed by a 4096-byte tail of 0xA5 keeps its tail, and every output has the bits of a run in a buffer twice
the size.

Bit-identity includes the loss sums that end in fp64 atomics (SEPT, MHCN's MIM; InfoNCE issues one atomic at this size): the
inputs are built so that every term is a float32 value in [2^-5, 2^3] (bounds at the cases), a few hundred of them, so every fp64
addition is exact -- at most 3 + 23 + 10 bits wide -- and the order the atomics land in cannot show."""
import numpy as np
import pytest

import cdae_cases
import irgan_cases
from helpers import pad_cols, same_bits

pytestmark = pytest.mark.gpu
TAIL = 4096


@pytest.fixture(scope="module", autouse=True)
def _device():
    from qrec_amd import capi
    capi.init(0)
    yield


def _guarded(need, factor=1):
    from qrec_amd.capi import DeviceBuffer
    ws = DeviceBuffer(factor * need + TAIL, np.uint8)
    ws.fill_bytes(0xA5)
    return ws


def _twice(what, need, run):
    """run(ws) -> dict of outputs, in the stated bytes + tail and in twice the bytes: the tail intact, the outputs the same bits"""
    assert need > 0
    ws = _guarded(need)
    a = run(ws)
    tail = ws.numpy()[need:]
    assert tail.size == TAIL and (tail == 0xA5).all(), (what, int(np.flatnonzero(tail != 0xA5)[0]))
    same_bits(what + ", stated workspace against twice the size", a, run(_guarded(need, 2)))
    assert any(np.asarray(v).any() for v in a.values()), what


# ---- the contrastive pair: n = 65 rows of stride 32, padded to 128 inside the workspace ------------------------------------------------
N, LD, DIM = 65, 32, 16


def _tables(rng, count, rows=200):
    """rows b + e of one unit vector b, |e| <= 0.1: every cosine between two rows is >= (1 - 0.2 - 0.01) / 1.21 = 0.65, so at
    tau = 0.1 an exponential lies in [e^6.5, e^10], the share of 3 positives among 65 in [1.4e-3, 0.62] and -log of it in [0.48, 6.6]"""
    b = rng.standard_normal(DIM); b /= np.linalg.norm(b)
    return [(b + rng.uniform(-0.1, 0.1, (rows, DIM)) / np.sqrt(DIM)).astype(np.float32) for _ in range(count)]


def test_info_nce_stays_inside_its_stated_workspace():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer as DB
    rng = np.random.default_rng(65)
    S1, S2 = (DB.from_numpy(pad_cols(t, LD)) for t in _tables(rng, 2))
    rows = DB.from_numpy(rng.permutation(200)[:N].astype(np.int32))

    def run(ws):
        out, out2, loss = DB.zeros((200, LD), np.float32), DB.zeros((200, LD), np.float32), DB.zeros(1, np.float64)
        capi.info_nce_loss_grad(S1, S2, 2.0, rows, N, LD, 0.2, 0.5, ws, out, loss, d_out2=out2)
        return dict(out=out.numpy(), out2=out2.numpy(), loss=loss.numpy())
    _twice("InfoNCE n=65 ld=32", capi.info_nce_workspace_bytes(N, LD), run)


def test_sept_ssl_stays_inside_its_stated_workspace():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer as DB
    rng = np.random.default_rng(66)
    k = 3
    S = [DB.from_numpy(pad_cols(t, LD)) for t in _tables(rng, 4)]
    rows = DB.from_numpy(rng.permutation(200)[:N].astype(np.int32))
    ordered = capi.OrderedScatter()          # the positives' scatter in a fixed order: no float atomic in the run

    def run(ws):
        dS = [DB.zeros((200, LD), np.float32) for _ in range(4)]
        loss, labels = DB.zeros(1, np.float64), DB.zeros((3, N, k), np.int32)
        capi.sept_ssl_loss_grad(*S, rows, N, LD, k, 0.25, ws, *dS, loss, labels, ordered=ordered)
        out = {f"dS{v}": d.numpy() for v, d in enumerate(dS)}
        out.update(loss=loss.numpy(), labels=labels.numpy())
        return out
    _twice("SEPT n=65 ld=32 k=3", capi.sept_ssl_workspace_bytes(N, LD, k), run)


# ---- CDAE -------------------------------------------------------------------------------------------------------------------------------
def test_cdae_step_calls_stay_inside_their_stated_workspace():
    """qrec_cdae_decode, _hidden_bwd and _loss share one workspace; nh = 20, B = 1 is tests/cdae_cases.py's smallest case"""
    from qrec_amd import capi
    from qrec_amd.autoencoder import CdaeTrainer
    nh, B = 20, 1
    p, L, reg = cdae_cases.kernel_case(nh, B)

    def run(ws):
        tr = CdaeTrainer(p["W_enc"], p["W_dec"], p["b_enc"], p["b_dec"], p["V"], 0.01, reg)
        tr._reserve(B, L.n_live)
        tr.ws = ws
        tr.forward_backward(L)
        assert tr.ws is ws
        out = dict(h=tr.h.numpy(), dz=tr.dz.numpy(), g=tr.g.numpy()[:L.n_live], loss=np.array([tr.loss()]))
        out.update({f"grad_{k}": v for k, v in tr.raw_gradients().items()})
        return out
    _twice("CDAE step nh=20 B=1", capi.cdae_workspace_bytes(B, 32), run)


def test_cdae_draw_stays_inside_its_stated_workspace():
    """B = 3 rows over 33 items: two bitmap words per row"""
    from qrec_amd import capi
    from qrec_amd.autoencoder import DeviceBatchStream
    B, ni = 3, 33
    rng = np.random.default_rng(33)
    rows = [np.sort(rng.permutation(ni)[:k]).astype(np.int32) for k in (1, 4, 0, 6, 2, 5, 3)]
    rows[1][-1] = ni - 1                       # a bit in the second word
    indptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
    items = np.concatenate(rows)
    vals = rng.integers(1, 9, items.size).astype(np.float32) / 2

    def run(ws):
        ds = DeviceBatchStream(indptr, items, vals, ni, B, 0.9, seed=5)
        ds.ws = ws
        lists = ds.draw(0)
        out = {k: getattr(lists, k).numpy() for k in lists.NAMES}
        out["cand"] = ds.cand_count.numpy()
        return out
    _twice("CDAE draw B=3 n_items=33", capi.cdae_draw_workspace_bytes(B, ni), run)


# ---- IRGAN ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["negatives", "mixture"])
def test_irgan_row_weights_stay_inside_their_stated_workspace(mode):
    """B = 2 rows over 257 items: two logits tiles per row"""
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    from qrec_amd.gan import IrganTrainer
    B, ni, d = 2, 257, irgan_cases.WIDTHS[0]
    v, csr = irgan_cases.kernel_case(ni, d)
    users = DeviceBuffer.from_numpy(np.arange(B, dtype=np.int32))
    m = capi.IRGAN_NEGATIVES if mode == "negatives" else capi.IRGAN_MIXTURE

    def run(ws):
        tr = IrganTrainer(v, csr[0], csr[1], 0.001, 0.001, seed=11)
        tr._reserve_rows(B)
        tr.row_ws = ws
        tr.row_weights(tr.gen, users, B, m)
        assert tr.row_ws is ws
        return dict(z=tr.z.numpy()[:B], w=tr.w.numpy()[:B], p=tr.p.numpy()[:B], csum=tr.csum.numpy()[:B])
    _twice(f"IRGAN {mode} rows B=2 n_items=257", capi.irgan_row_workspace_bytes(B, ni), run)


# ---- MHCN -------------------------------------------------------------------------------------------------------------------------------
NU, MD = 300, 24            # tests/test_gpu_graph.py::_mhcn_problem's rows, its smallest width (stride 32)


def test_hss_loss_grad_stays_inside_its_stated_scratch():
    """entries in [-1/4, 1/4]: every score difference stays in [-3, 3], every loss term -log sigmoid in [2^-5, 2^2]"""
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer as DB
    rng = np.random.default_rng(24)
    em, edge = (DB.from_numpy(pad_cols(rng.uniform(-0.25, 0.25, (NU, MD)).astype(np.float32), LD)) for _ in range(2))
    p1, k2, p2, k3, p3 = (rng.permutation(n).astype(np.int32) for n in (NU, MD, NU, MD, NU))
    inv = lambda p: np.argsort(p).astype(np.int32)
    perms = [DB.from_numpy(x) for x in (p1, inv(p1), p2, inv(p2), k2, inv(k2), p3, inv(p3), k3, inv(k3))]

    def run(ws):
        dem, dedge, loss = DB.zeros((NU, LD), np.float32), DB.zeros((NU, LD), np.float32), DB.zeros(1, np.float64)
        capi.hss_loss_grad(em, edge, NU, MD, LD, perms, 1.0, ws, dem, dedge, loss)
        return dict(dem=dem.numpy(), dedge=dedge.numpy(), loss=loss.numpy())
    _twice("MHCN MIM rows=300 ld=32", capi.hss_scratch_bytes(NU), run)


def test_channel_attention_bwd_stays_inside_its_stated_scratch():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer as DB
    rng = np.random.default_rng(25)
    tab = lambda r=NU: DB.from_numpy(pad_cols(rng.standard_normal((r, MD)).astype(np.float32), LD))
    es, half, dOut = [tab() for _ in range(3)], tab(), tab()
    att = DB.from_numpy(pad_cols(rng.uniform(-0.5, 0.5, (1, MD)).astype(np.float32), LD)[0])
    mat = DB.from_numpy(pad_cols(np.pad(rng.uniform(-0.3, 0.3, (MD, MD)).astype(np.float32), ((0, LD - MD), (0, 0))), LD))
    v, score, out = DB.zeros(256, np.float32), DB.zeros((NU, 4), np.float32), DB.zeros((NU, LD), np.float32)
    capi.channel_attention_fwd(es, att, mat, half, NU, LD, v, score, out)

    def run(ws):
        de = [DB.zeros((NU, LD), np.float32) for _ in range(3)]
        dh, g_a, g_M = DB.zeros((NU, LD), np.float32), DB.zeros(LD, np.float32), DB.zeros((LD, LD), np.float32)
        capi.channel_attention_bwd(dOut, es, score, v, att, mat, NU, LD, de, False, dh, False, ws, g_a, g_M)
        res = {f"de{k}": d.numpy() for k, d in enumerate(de)}
        res.update(dh=dh.numpy(), g_att=g_a.numpy(), g_att_mat=g_M.numpy())
        return res
    _twice("MHCN channel attention backward rows=300 ld=32", 4 * capi.channel_attention_scratch_floats(), run)


# ---- evaluation (csrc/eval_block.hip, csrc/eval_fused.hip): the block layout and the fused layout ------------------------------------------------------------
def _ranked_inside(what, rk, users, N):
    """the ranker's one call for `users` in a scratch of exactly the bytes the library states for it"""
    from qrec_amd.capi import DeviceBuffer as DB
    n = users.size

    def run(ws):
        rk._scratch, rk._d_ids, rk._d_sc, rk._cap = ws, DB.zeros((n, N), np.int32), DB.zeros((n, N), rk.dtype), (n, N)
        ids, sc = rk.topk(users, N)
        assert rk._scratch is ws
        return dict(ids=ids, scores=sc)
    _twice(what, rk._scratch_bytes(n, N), run)


def test_heap_only_evaluation_stays_inside_its_stated_scratch():
    """fp64, 129 users x 257 items: below 8,192 items only the score block of the block layout is touched"""
    from qrec_amd.interactions import user_item_csr
    from qrec_amd.ranking import DeviceRanker
    rng = np.random.default_rng(129)
    nu, ni, d, N = 129, 257, 50, 20
    U, V = rng.standard_normal((nu, d)), rng.standard_normal((ni, d))
    rated = user_item_csr(rng.integers(0, nu, 4 * nu), rng.integers(0, ni, 4 * nu), np.ones(4 * nu), nu, ni)
    _ranked_inside("evaluation fp64 129x257", DeviceRanker(U, V, rated), rng.permutation(nu).astype(np.int32), N)


def test_sliced_evaluation_stays_inside_its_stated_scratch():
    """fp32, 96 users x 8,200 items, tables as tests/test_gpu_eval.py::test_sliced_topk_and_its_exact_fallbacks builds them (user k
    is the k-th unit vector): 7 users tie inside their N + 1 best, are flagged by the merge and redone by the exact wavefront
    kernel -- flags, the flagged list and its counter, the last arrays of the block layout, are written and read"""
    from qrec_amd.interactions import user_item_csr
    from qrec_amd.ranking import DeviceRanker
    rng = np.random.default_rng(8200)
    nu, ni, N = 96, 8200, 20
    V = np.empty((ni, nu), np.float32)
    for k in range(nu):
        V[:, k] = rng.permutation(ni) - ni // 3
    for k in rng.permutation(nu)[:7]:
        V[:, k] = rng.integers(-5, 40, ni)
    rated = user_item_csr(rng.integers(0, nu, 500), rng.integers(0, ni, 500), np.ones(500), nu, ni)
    _ranked_inside("evaluation fp32 96x8200, sliced", DeviceRanker(np.eye(nu, dtype=np.float32), V, rated), rng.permutation(nu).astype(np.int32), N)


@pytest.mark.parametrize("route", ["bf16", "f32-filter", "bf16-two-tiles"])
def test_fused_evaluation_stays_inside_its_stated_scratch(route, monkeypatch):
    """fp32, d = 64, 65 users (one past user padding) x 16,417 items (past the fused boundary, ragged last tile), tables as
    tests/test_gpu_eval.py::test_fused_route_equals_the_block_route builds them: users whose scores are all negative or all 0
    and duplicated popular items flag users, so stage (D) writes the fallback region at the layout's end"""
    from qrec_amd.interactions import user_item_csr
    from qrec_amd.ranking import DeviceRanker
    for k, v in {"bf16": {}, "f32-filter": {"QREC_EVAL_F32_FILTER": "1"}, "bf16-two-tiles": {"QREC_EVAL_NU": "2"}}[route].items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(16417)
    nu, ni, d, N = 80, 16384 + 33, 64, 20
    pop = (np.arange(ni, dtype=np.float64) + 1) ** -0.5
    V = (rng.standard_normal((ni, d)) * 0.3 + pop[:, None] * 2.0).astype(np.float32)
    U = (rng.standard_normal((nu, d)) * 0.3 + 0.5).astype(np.float32)
    U[::7] = -np.abs(U[::7])
    U[3::50] = 0.0
    V[5000:5040] = V[100:140]
    uu = rng.integers(0, nu, 30 * nu); ii = (rng.integers(0, ni, 30 * nu) ** 2 // ni).astype(np.int64)
    rated = user_item_csr(uu, ii, np.ones(uu.size), nu, ni)
    _ranked_inside(f"evaluation fp32 65x16417, fused {route}", DeviceRanker(U, V, rated), rng.permutation(nu)[:65].astype(np.int32), N)


def _rated_with_values(rng, nu, ni, per_user):
    from qrec_amd.interactions import CSR
    iid = np.concatenate([np.sort(rng.permutation(ni)[:per_user]) for _ in range(nu)]).astype(np.int32)
    return CSR(np.arange(nu + 1, dtype=np.int64) * per_user, iid, rng.integers(1, 9, iid.size) / 2)


def test_sigmoid_bias_evaluation_stays_inside_its_stated_scratch():
    """40 users x 1,003 items, 24 hidden units at stride 32: the shape of tests/test_gpu_cdae.py's ranker"""
    from qrec_amd.capi import DeviceBuffer as DB
    from qrec_amd.ranking import SigmoidBiasRanker
    rng = np.random.default_rng(1003)
    nu, ni, nh = 40, 1003, 24
    H, W = (pad_cols(rng.uniform(-0.5, 0.5, (r, nh)).astype(np.float32), LD) for r in (nu, ni))
    b = rng.uniform(-1.0, 1.0, ni).astype(np.float32)
    rk = SigmoidBiasRanker(DB.from_numpy(H), DB.from_numpy(W), DB.from_numpy(b), nu, ni, nh, LD, _rated_with_values(rng, nu, ni, 30))
    _ranked_inside("sigmoid-bias evaluation 40x1003", rk, rng.permutation(nu).astype(np.int32), 10)


def test_sparse_row_sigmoid_bias_evaluation_stays_inside_its_stated_scratch():
    """73 users x 477 items at stride 480: the shape of tests/test_gpu_cfgan.py's ranker"""
    from qrec_amd.capi import DeviceBuffer as DB
    from qrec_amd.ranking import SparseRowSigmoidRanker
    rng = np.random.default_rng(477)
    nu, ni = 73, 477
    ld = -(-ni // 32) * 32
    W = pad_cols(rng.uniform(-0.2, 0.2, (ni, ni)).astype(np.float32), ld)
    b = pad_cols(rng.uniform(-1.0, 1.0, (1, ni)).astype(np.float32), ld)[0]
    rk = SparseRowSigmoidRanker(DB.from_numpy(W), DB.from_numpy(b), nu, ni, ld, _rated_with_values(rng, nu, ni, 20))
    _ranked_inside("sparse-row sigmoid-bias evaluation 73x477", rk, rng.permutation(nu).astype(np.int32), 12)
