"""Shapes, inputs and float64 references of the direct tests of MHCN's row kernels (csrc/mhcn.hip, qrec_buir_wgrad for the gates'
dW / db, qrec_l2norm_rows_accum / _bwd), shared by tests/test_gpu_mhcn_shapes.py (the kernels against these references) and
tests/test_mhcn_cases_cpu.py (these references against the pinned restatement oracle/tfmodels.py, against central differences, and the
restatement's own float32 distance to them at every case).  numpy only (motif_problem alone builds its graphs with the oracle); every
reference is float64 throughout.

Row counts.  One trip of a 256-thread block covers 4 * 64 / LPR rows, LPR = ld / 4: 32 / 16 / 8 / 4 rows at stride 32 / 64 / 128 / 256.
  small    n below one wavefront's rows (8 / 4 / 2): the gates keep the whole wavefront alive, its tail lanes clamped to row n - 1
  d == ld  no pad column at all; n no multiple of the rows per wavefront (4 and 2)
  512 cap  the gates and everything that feeds a column sum stop at 512 blocks = 16,384 / 8,192 / 4,096 / 2,048 rows per trip: a
           few rows more and the first threads of the first blocks take a second row, so that the loop increment, the per-thread
           accumulation before the block's column sum and the sum over all 512 partial rows run
  2,048    att_fwd_kernel and hss_grad_kernel stop at 2,048 blocks = 16,384 / 8,192 rows at stride 128 / 256
  4,096    the l2norm pair stops at 4,096 blocks = 16,384 rows at stride 256
The gates (and qrec_buir_wgrad behind them) serve strides up to 128 only; attention, the MIM loss and the l2norm pair up to 256."""
import numpy as np

SMALL = [(1, 24, 32), (3, 50, 64), (1, 100, 128)]
FULL_WIDTH = [(301, 64, 64), (303, 128, 128)]
CAP_512 = [(16421, 24, 32), (8197, 50, 64), (4099, 100, 128), (4099, 128, 128)]
CAP_512_WIDE = [(2051, 200, 256)]
CAP_2048 = [(16387, 100, 128), (8195, 200, 256)]

GATE_CASES = SMALL + FULL_WIDTH + CAP_512                       # (n, d, ld)
ROW_CASES = GATE_CASES + CAP_512_WIDE + CAP_2048                # attention and the MIM loss
L2NORM_CASES = SMALL + FULL_WIDTH + [(16389, 200, 256), (1000, 100, 128), (1000, 200, 256)]
SAME_BITS_CASES = CAP_512

# Arguments, spread so that every value occurs at a small (first five) and at a wrapped (the rest) case.
GATE_ARGS = {   # case -> (accumulate into dX, dy_scale)
    (1, 24, 32): (True, 1.0), (3, 50, 64): (False, 0.25), (1, 100, 128): (True, 0.25), (301, 64, 64): (False, 1.0), (303, 128, 128): (True, 1.0),
    (16421, 24, 32): (False, 0.25), (8197, 50, 64): (True, 1.0), (4099, 100, 128): (False, 1.0), (4099, 128, 128): (True, 0.25)}
ATT_ARGS = {    # case -> (half given to the forward pass, accumulate into de, dhalf: None / "overwrite" / "accumulate")
    (1, 24, 32): (True, False, "accumulate"), (3, 50, 64): (False, True, None), (1, 100, 128): (True, True, "overwrite"),
    (301, 64, 64): (False, False, "accumulate"), (303, 128, 128): (True, False, None),
    (16421, 24, 32): (False, True, "overwrite"), (8197, 50, 64): (True, False, "accumulate"), (4099, 100, 128): (False, False, None),
    (4099, 128, 128): (True, True, "overwrite"), (2051, 200, 256): (False, True, "accumulate"), (16387, 100, 128): (True, False, None),
    (8195, 200, 256): (False, True, "overwrite")}
HSS_SCALE = {   # case -> scale (the trainer passes ss_rate)
    (1, 24, 32): 1.0, (3, 50, 64): 0.05, (1, 100, 128): 0.05, (301, 64, 64): 1.0, (303, 128, 128): 0.05,
    (16421, 24, 32): 0.05, (8197, 50, 64): 1.0, (4099, 100, 128): 0.05, (4099, 128, 128): 1.0, (2051, 200, 256): 0.05,
    (16387, 100, 128): 1.0, (8195, 200, 256): 0.05}

GUARD_ROWS = 8                       # rows past n in every output table, pre-filled with SENTINEL: must come back untouched
SENTINEL = np.float32(-12345.0)


def case_id(case):
    """16421x24x32: no blank, so that the parity ledger's test name (cut at the first blank) keeps the whole case"""
    return "x".join(str(c) for c in case)


def _rng(kind, n, d, ld):
    return np.random.default_rng([kind, n, d, ld])


def _table(rng, n, d):
    """N(0, s), s drawn from 0.3 ... 1"""
    return (rng.standard_normal((n, d)) * rng.uniform(0.3, 1.0)).astype(np.float32)


def gate_inputs(n, d, ld):
    rng = _rng(1, n, d, ld)
    lim = np.sqrt(6.0 / (2 * d))                        # the Glorot limit of the reference's d x d weights
    return dict(X=_table(rng, n, d), W=rng.uniform(-lim, lim, (d, d)).astype(np.float32), b=rng.uniform(-0.5, 0.5, (1, d)).astype(np.float32),
                dY=_table(rng, n, d), prev=_table(rng, n, d))


def attention_inputs(n, d, ld):
    rng = _rng(2, n, d, ld)
    lim = np.sqrt(6.0 / (2 * d))
    return dict(es=[_table(rng, n, d) for _ in range(3)], a=rng.uniform(-0.5, 0.5, (1, d)).astype(np.float32),
                M=rng.uniform(-lim, lim, (d, d)).astype(np.float32), half=_table(rng, n, d), dOut=_table(rng, n, d),
                de_prev=[_table(rng, n, d) for _ in range(3)], dhalf_prev=_table(rng, n, d))


def hss_inputs(n, d, ld):
    """em and an INDEPENDENT edge table (not H em), the call's five shuffles (p1, k2, p2, k3, p3).  edge is scaled by 2 / sqrt(d), as a
    row-normalised average of em rows is shorter than they are: the scores em . edge then have a spread of at most 2 whatever d is.
    Unscaled, d = 100 puts single scores at +-10, where 1 - sigmoid() keeps three digits in float32 and the n = 1 case measures
    that cancellation (fp32 restatement 3e-6 from the reference) rather than the kernel."""
    rng = _rng(3, n, d, ld)
    return dict(em=_table(rng, n, d), edge=(_table(rng, n, d) * np.float32(2.0 / np.sqrt(d))).astype(np.float32),
                perm=(rng.permutation(n), rng.permutation(d), rng.permutation(n), rng.permutation(d), rng.permutation(n)))


def l2norm_inputs(n, d, ld):
    """one all-zero row (the 1e-12 clamp) and one row scaled by 1e-4 where there are rows to spare"""
    rng = _rng(4, n, d, ld)
    X = _table(rng, n, d)
    if n > 77:
        X[5] = 0; X[77] *= np.float32(1e-4)
    return dict(X=X, S0=_table(rng, n, d), dS=_table(rng, n, d))


def motif_problem(rng, nu=300, ni=260, d=24, E=5000, Rn=1800):
    """tests/test_gpu_graph.py::_mhcn_problem: the motif graphs and the joint adjacency of a random purchase / follow graph, the 18 weight
    tensors at their Glorot limits, N(0, 0.3) embeddings -> H, R, weights, U0, V0"""
    from oracle import tfmodels as T
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
    return H, Rm, w, U0, V0


# ---- float64 references ----------------------------------------------------------------------------------------------------
def _f64(*xs):
    return [None if x is None else np.asarray(x, np.float64) for x in xs]


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def gate_ref(X, W, b, dY, dy_scale, dX_prev=None):
    """self_gating (MHCN.py:109-112) and its gradient for the incoming dy_scale * dY -> Y, S, Q, dX, dW, db.
    Y = X * S, S = sigmoid(X W + b);  Q = d pre-activation;  dX (+ dX_prev) = dy * S + Q W^T;  dW = X^T Q;  db = column sums of Q"""
    X, W, b, dY, dX_prev = _f64(X, W, b, dY, dX_prev)
    S = _sigmoid(X @ W + b.reshape(1, -1))
    g = float(dy_scale) * dY
    Q = g * X * S * (1.0 - S)
    dX = g * S + Q @ W.T
    if dX_prev is not None:
        dX = dX + dX_prev
    return X * S, S, Q, dX, X.T @ Q, Q.sum(0)


def attention_ref(es, a, M, half, dOut, de_prev=None, dhalf_prev=None):
    """channel_attention (MHCN.py:113-121) -> v, score, out, de[3], dhalf, g_a, g_M.
    v = M a^T;  score = softmax_k(e_k . v);  out = sum_k score_k e_k (+ half / 2);  with dw = d loss / d (e_k . v):
    de_k (+ de_prev[k]) = score_k dOut + dw_k v;  dhalf (+ dhalf_prev) = dOut / 2;  dv = sum_rows sum_k dw_k e_k;  g_a = M^T dv;  g_M = dv (x) a"""
    es = _f64(*es)
    a, M, half, dOut, dhalf_prev = _f64(a, M, half, dOut, dhalf_prev)
    a = a.reshape(-1)
    v = M @ a
    w = np.stack([e @ v for e in es], 1)
    ex = np.exp(w - w.max(1, keepdims=True))
    sc = ex / ex.sum(1, keepdims=True)
    out = sum(sc[:, k:k + 1] * es[k] for k in range(3))
    if half is not None:
        out = out + half / 2.0
    dsc = np.stack([(dOut * e).sum(1) for e in es], 1)
    dw = sc * (dsc - (sc * dsc).sum(1, keepdims=True))
    de = [sc[:, k:k + 1] * dOut + dw[:, k:k + 1] * v[None, :] for k in range(3)]
    if de_prev is not None:
        de = [g + p for g, p in zip(de, _f64(*de_prev))]
    dhalf = dOut / 2.0 + (0.0 if dhalf_prev is None else dhalf_prev)
    dv = sum(dw[:, k] @ es[k] for k in range(3))
    return v, sc, out, de, dhalf, M.T @ dv, np.outer(dv, a)


def _nls(x):
    """-log(sigmoid(x))"""
    return np.logaddexp(0.0, -x)


def hss_ref(em, edge, perm, scale):
    """hierarchical_self_supervision (MHCN.py:184-206) with edge as an input -> loss (unscaled), scale * d loss / d em, scale * d loss / d edge
    (the partial derivatives: edge = H em and its H^T product stay outside).  perm = (p1, k2, p2, k3, p3): row_shuffle for neg1, column
    then row shuffle for neg2, column then row shuffle for the global term.  The d graph / n term of graph = mean(edge) is included."""
    em, edge = _f64(em, edge)
    p1, k2, p2, k3, p3 = (np.asarray(p, np.int64) for p in perm)
    n = em.shape[0]
    e2, e3 = edge[:, k2][p2], edge[:, k3][p3]
    pos, neg1, neg2 = (em * edge).sum(1), (em[p1] * edge).sum(1), (e2 * em).sum(1)
    graph = edge.mean(0)
    pg, ng = edge @ graph, e3 @ graph
    loss = float(_nls(pos - neg1).sum() + _nls(neg1 - neg2).sum() + _nls(pg - ng).sum())
    c1, c2, c3 = -(1.0 - _sigmoid(pos - neg1)), -(1.0 - _sigmoid(neg1 - neg2)), -(1.0 - _sigmoid(pg - ng))
    d_pos, d_neg1, d_neg2 = c1, c2 - c1, -c2
    q1, q2, q3 = np.argsort(p1), np.argsort(p2), np.argsort(p3)            # x[p] = y  <=>  the gradient of x is dy[q], q = p^-1
    k2inv, k3inv = np.argsort(k2), np.argsort(k3)
    dem = d_pos[:, None] * edge + d_neg2[:, None] * e2 + (d_neg1[:, None] * edge)[q1]
    dgraph = (c3[:, None] * (edge - e3)).sum(0)
    dedge = (d_pos[:, None] * em + d_neg1[:, None] * em[p1] + c3[:, None] * graph[None, :] + (d_neg2[:, None] * em)[q2][:, k2inv]
             - (c3[:, None] * graph[None, :])[q3][:, k3inv] + dgraph[None, :] / n)
    return loss, float(scale) * dem, float(scale) * dedge


def l2norm_ref(X, S0, dS):
    """tf.nn.l2_normalize(x, 1) = x * rsqrt(max(sum x^2, 1e-12)) added into S0, and the gradient of that term -> inv, S, dX"""
    X, S0, dS = _f64(X, S0, dS)
    inv = 1.0 / np.sqrt(np.maximum((X * X).sum(1), 1e-12))
    z = X * inv[:, None]
    return inv, S0 + z, (dS - z * (z * dS).sum(1, keepdims=True)) * inv[:, None]
