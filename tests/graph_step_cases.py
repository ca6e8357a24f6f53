"""Shapes, inputs and float64 references of the direct tests of the kernels every graph model's training step shares: the batch BPR
loss (csrc/graph.hip bpr_batch_kernel), BUIR's batch kernel (csrc/buir.hip), the noise perturbation (csrc/contrastive.hip
perturb_kernel) and the three element-wise sweeps (Adam, scale_copy, the EMA).  Shared by tests/test_gpu_graph_steps.py (the kernels
against these references) and tests/test_graph_step_cases_cpu.py (the fp32 numpy restatement's own distance to them, and the
properties the cases promise).  numpy only; every reference is float64 throughout, evaluated on the float32 inputs and the float32
values of the scalar arguments the kernels receive.

Where the loops wrap.  One 256-thread block holds 4 * 64 / LPR groups of LPR lanes, one group per batch element or row.
  batch BPR    LPR 16 / 16 / 32 / 64 at stride 32 / 64 / 128 / 256 (stride 32 is the one layout with two columns per lane), at most
               256 blocks = 4,096 / 4,096 / 2,048 / 1,024 groups: a few elements more and the first groups take a second one
  BUIR batch   LPR 8 / 16 / 32 at stride 32 / 64 / 128, at most 256 blocks = 8,192 / 4,096 / 2,048 groups
  perturbation LPR = stride / 4, at most 2,048 blocks = 65,536 / 32,768 / 16,384 / 8,192 rows
  element-wise float4 per thread, at most 2,048 blocks = 2,097,152 elements per trip

The measure.  One norm over a table hides a single wrong row among thousands of right ones, so every table is judged row by row:
the 2-norm distance of an output row to the reference row over the row's SCALE, and the maximum over the rows is what is held.
  scattered sum   scale = the sum of the 2-norms of the fp64 addends of that row (the row's prior content is one of them): what a
                  sum's rounding error is proportional to, also where the addends cancel
  plain function  scale = the reference row's norm, floored at the table's median row norm"""
import numpy as np

from mhcn_cases import GUARD_ROWS, SENTINEL, case_id  # noqa: F401  (re-exported to the two test files)

TOL = 1e-5                           # the project's parity contract

# ---- cases: (B or n, d, ld) -------------------------------------------------------------------------------------------------
BPR_SMALL = [(1, 24, 32), (3, 50, 64), (5, 100, 128), (2, 200, 256)]           # groups idle in the last wavefront
BPR_WRAPPED = [(4101, 24, 32), (4101, 50, 64), (2051, 100, 128), (2051, 128, 128), (1029, 200, 256)]
BPR_THREE_TRIPS = [(8197, 64, 64)]
BPR_CASES = BPR_SMALL + BPR_WRAPPED + BPR_THREE_TRIPS
BPR_ARGS = {    # case -> (div, reg, dE starts from a non-zero table)
    (1, 24, 32): (1.0, 0.01, False), (3, 50, 64): (3.0, 0.01, True), (5, 100, 128): (1.0, 0.01, True), (2, 200, 256): (3.0, 0.01, False),
    (4101, 24, 32): (3.0, 0.01, True), (4101, 50, 64): (1.0, 0.01, False), (2051, 100, 128): (3.0, 0.0, False),
    (2051, 128, 128): (1.0, 0.01, True), (1029, 200, 256): (3.0, 0.01, True), (8197, 64, 64): (1.0, 0.01, False)}
BPR_EPS = np.float32(1e-7)           # util/loss.py:3-6 (10e-8)
SATURATED = 12.0                     # |score| of the triplets placed on purpose
# No other score may reach this.  g carries the rounding of s in 1 - s, half an ulp of s = 3e-8 over 1 - s, and where reg = 0 a row with
# one lookup measures just that: 1 - sigmoid(4) = 0.018 keeps it below 1.7e-6.
SCORE_CEILING = 4.0

BUIR_SMALL = [(1, 24, 32), (3, 50, 64), (2, 100, 128)]
BUIR_WRAPPED = [(8195, 24, 32), (4099, 50, 64), (2051, 100, 128), (2051, 128, 128)]
BUIR_CASES = BUIR_SMALL + BUIR_WRAPPED
BUIR_ARGS = {   # case -> (L: div = L + 1, bias all zero, dS starts from a non-zero table)
    (1, 24, 32): (1, False, False), (3, 50, 64): (2, True, True), (2, 100, 128): (1, False, True),
    (8195, 24, 32): (2, False, True), (4099, 50, 64): (1, True, False), (2051, 100, 128): (2, False, False), (2051, 128, 128): (1, False, True)}
BUIR_USERS, BUIR_ITEMS = 300, 260
BUIR_ZERO_USER, BUIR_ZERO_ITEM = 7, 11        # the all-zero ONLINE row (user) and the all-zero TARGET row (item)

PERTURB_SMALL = [(1, 24, 32), (3, 50, 64), (301, 64, 64), (5, 200, 256)]
PERTURB_WRAPPED = [(65541, 24, 32), (32773, 50, 64), (16389, 100, 128), (8197, 200, 256)]
PERTURB_CASES = PERTURB_SMALL + PERTURB_WRAPPED
PERTURB_ARGS = {  # case -> (perturb_rows: out of place with d_src, with d_accum)
    (1, 24, 32): (False, True), (3, 50, 64): (True, False), (301, 64, 64): (True, True), (5, 200, 256): (False, False),
    (65541, 24, 32): (True, False), (32773, 50, 64): (False, True), (16389, 100, 128): (False, False), (8197, 200, 256): (True, True)}
PERTURB_SUBSET_CASES = [(301, 64, 64), (16389, 100, 128)]
PERTURB_EPS = np.float32(0.1)
PERTURB_SEED, PERTURB_STREAMS = 0x1234567ABCDEF, ((7 << 32) | 3, 11)    # both halves of the seed and of one stream id in use
PERTURB_ROWS_PER_TRIP = {32: 65536, 64: 32768, 128: 16384, 256: 8192}
REPLAY_ROWS = 64                     # rows replayed on the host at the table's start, its end and either side of the first wrap

ELEMENTWISE_N = [4, 2_097_152, 4_194_564]     # one float4; the cap exactly; two full trips and a ragged third
ELEMENTWISE_GUARD = 64               # sentinel words past n_elems
EMA_TAU = np.float32(0.995)
SCALE_ALPHA = np.float32(0.37)
ADAM_STEPS, ADAM_LR, ADAM_GRAD_SCALE = 3, 0.01, np.float32(1 / 3)
ADAM_L2 = {4: 0.01, 2_097_152: 0.0, 4_194_564: 0.01}
# check_rel's abs_tol: three times the largest absolute distance of the fp32 numpy restatement from the fp64 reference over the three
# sizes (tests/test_graph_step_cases_cpu.py measures it on these inputs and holds each constant to its measurement)
ABS_TOL_SCALE_COPY = 2.6e-7          # measured 8.61e-8
ABS_TOL_EMA = 1.4e-6                 # measured 4.55e-7
ABS_TOL_ADAM_THETA = 3.4e-5          # measured 1.11e-5: where g = grad / 3 + l2 theta nearly cancels, Adam still moves theta by ~lr
ABS_TOL_ADAM_M = 9.5e-8              # measured 3.14e-8
ABS_TOL_ADAM_V = 3.4e-9              # measured 1.12e-9


def _rng(kind, n, d, ld):
    return np.random.default_rng([kind, n, d, ld])


def _f64(*xs):
    return [None if x is None else np.asarray(x, np.float64) for x in xs]


def _row_norms(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).sum(1))


# ---- the measure ----------------------------------------------------------------------------------------------------------------
def row_error(got, want, scale):
    """max over the rows of |got[r] - want[r]| / scale[r]; a row of scale 0 has to be met exactly (it counts as infinitely wrong if not)"""
    err = _row_norms(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    scale = np.asarray(scale, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def plain_scale(want):
    """the scale of a row that is a plain function of its inputs: its norm, floored at the table's median row norm"""
    norms = _row_norms(want)
    return np.maximum(norms, np.median(norms))


def plain_row_error(got, want):
    return row_error(got, want, plain_scale(want))


# ---- batch BPR ----------------------------------------------------------------------------------------------------------------------
def bpr_inputs(B, d, ld):
    """S (float32 [nu + ni, d]), the triplets, the table dE starts from, and what was placed on purpose.  The rows are div * N(0, sigma),
    sigma^2 = 0.8 / sqrt(2 d): the scores u . (i - j) of the mean rows have a spread of 0.8 at every d.  Placed: element 1 repeats
    element 0; every fifth element up to five has i == j; from B = 1000 on, four elements score +12 and four -12 on rows of their own
    (user 2 with items 3 and 4 in both orders, so that each of the three rows also collects addends of ordinary size: alone, the
    float32 1 - sigmoid(12) = 6e-6 keeps two digits and would be what the row measures); user 0 / item 0 of the large tables and the
    last user / item of both are named by no triplet."""
    rng = _rng(10, B, d, ld)
    div = BPR_ARGS[(B, d, ld)][0]
    nu, ni = (37, 29) if B < 1000 else (1500, 1100)
    sigma = np.sqrt(0.8 / np.sqrt(2.0 * d))
    S = (rng.standard_normal((nu + ni, d)) * (div * sigma)).astype(np.float32)
    u = rng.integers(1, nu - 1, B).astype(np.int32); i = rng.integers(1, ni - 1, B).astype(np.int32); j = rng.integers(1, ni - 1, B).astype(np.int32)
    placed = np.zeros(B, bool)
    if B >= 2:
        u[1], i[1], j[1] = u[0], i[0], j[0]
    same = np.arange(2, B, max(B // 5, 1))[:5]
    j[same] = i[same]
    if B >= 1000:
        w = rng.standard_normal(d)
        a = np.sqrt(SATURATED / 2.0 / (w * w).sum())                   # ub = a w, ib = a w, jb = -a w: score = 2 a^2 |w|^2
        S[2] = (div * a * w).astype(np.float32); S[nu + 3] = S[2]; S[nu + 4] = -S[2]
        keep = (u == 2) | (i == 3) | (i == 4) | (j == 3) | (j == 4)    # no ordinary triplet on the placed rows: their scores would be large too
        u[keep & (u == 2)] = 5; i[keep & ((i == 3) | (i == 4))] = 6; j[keep & ((j == 3) | (j == 4))] = 6
        at = np.arange(7, B, B // 8)[:8]
        u[at] = 2; i[at[:4]], j[at[:4]] = 3, 4; i[at[4:]], j[at[4:]] = 4, 3
        placed[at] = True
    prev = (rng.standard_normal((nu + ni, d)) * 0.1).astype(np.float32)
    return dict(S=S, u=u, i=i, j=j, nu=nu, ni=ni, prev=prev, placed=placed)


def bpr_scores(t, div):
    S = np.asarray(t["S"], np.float64) / float(div)
    return (S[t["u"]] * (S[t["nu"] + t["i"]] - S[t["nu"] + t["j"]])).sum(1)


def bpr_ref(S, u, i, j, nu, div, reg, eps=BPR_EPS, prev=None):
    """embedding_lookup x3, util/loss.py:3-6 bpr_loss and the batch l2 term of LightGCN.py:22-30 with their gradients
    -> loss, dE, the scale of every row of dE, the row bitmap.
    ub = S[u] / div, ib = S[nu + i] / div, jb = S[nu + j] / div;  s = sigmoid(ub . ib - ub . jb);
    loss = sum -log(s + eps) + reg / 2 (|ub|^2 + |ib|^2 + |jb|^2);  g = -s (1 - s) / (s + eps);
    dE[u] += g (ib - jb) + reg ub;  dE[nu + i] += g ub + reg ib;  dE[nu + j] += -g ub + reg jb     (on top of prev)"""
    S = np.asarray(S, np.float64) / float(np.float32(div))
    reg, eps = float(np.float32(reg)), float(np.float32(eps))
    ru, ri, rj = np.asarray(u, np.int64), nu + np.asarray(i, np.int64), nu + np.asarray(j, np.int64)
    ub, ib, jb = S[ru], S[ri], S[rj]
    s = 1.0 / (1.0 + np.exp(-((ub * ib).sum(1) - (ub * jb).sum(1))))
    loss = float((-np.log(s + eps)).sum() + 0.5 * reg * ((ub * ub).sum() + (ib * ib).sum() + (jb * jb).sum()))
    g = (-(s * (1.0 - s)) / (s + eps))[:, None]
    rows = np.concatenate([ru, ri, rj])
    adds = np.concatenate([g * (ib - jb) + reg * ub, g * ub + reg * ib, -g * ub + reg * jb])
    dE = np.zeros(S.shape) if prev is None else np.asarray(prev, np.float64).copy()
    scale = _row_norms(dE)
    np.add.at(dE, rows, adds); np.add.at(scale, rows, _row_norms(adds))
    return loss, dE, scale, row_bitmap(rows, S.shape[0]), (rows, adds)


def row_bitmap(rows, n_rows, guard_words=2):
    """bit r of word r >> 5 for every listed row, (n_rows + 31) / 32 words and ``guard_words`` more that stay zero"""
    words = np.zeros((n_rows + 31) // 32 + guard_words, np.uint32)
    rows = np.unique(rows)
    np.bitwise_or.at(words, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    return words


# ---- BUIR batch -----------------------------------------------------------------------------------------------------------------------
def buir_inputs(B, d, ld):
    """online and target tables div * N(0, s) over 300 users and 260 items, W within the Glorot limit, a bias in +-0.5 (all zero where
    BUIR_ARGS says so: only then does the all-zero online row give q = 0 and reach the 1e-12 clamp of |q|).  Element 0 pairs the
    all-zero online row (user 7) with the all-zero target row (item 11); elements 1 and 2, where there are any, pair each of the two
    with an ordinary row."""
    rng = _rng(11, B, d, ld)
    L, zero_bias, _ = BUIR_ARGS[(B, d, ld)]
    nu, ni, div = BUIR_USERS, BUIR_ITEMS, float(L + 1)
    S_on = (rng.standard_normal((nu + ni, d)) * (div * rng.uniform(0.3, 1.0))).astype(np.float32)
    S_tar = (rng.standard_normal((nu + ni, d)) * (div * rng.uniform(0.3, 1.0))).astype(np.float32)
    S_on[BUIR_ZERO_USER] = 0; S_tar[nu + BUIR_ZERO_ITEM] = 0
    lim = np.sqrt(6.0 / (2 * d))
    W = rng.uniform(-lim, lim, (d, d)).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, (1, d)).astype(np.float32) * np.float32(0.0 if zero_bias else 1.0)
    u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, ni, B).astype(np.int32)
    u[0], i[0] = BUIR_ZERO_USER, BUIR_ZERO_ITEM
    if B >= 3:
        u[1], i[1] = BUIR_ZERO_USER, 12
        u[2], i[2] = 8, BUIR_ZERO_ITEM
    prev = (rng.standard_normal((nu + ni, d)) * 0.1).astype(np.float32)
    return dict(S_on=S_on, S_tar=S_tar, W=W, b=b, u=u, i=i, nu=nu, ni=ni, div=div, prev=prev)


def buir_ref(S_on, S_tar, W, b, u, i, nu, div, prev=None):
    """BUIR.py:105-129 for one batch -> loss, Xb, Gb (2B rows each: the users' pairs first, the items' from row B), dS, the scale of
    every row of dS.  Side 0 takes x = online[u], t = target[nu + i], side 1 x = online[nu + i], t = target[u], all over div:
    q = tanh(x W + b);  c = cos(q, t) with tf.math.l2_normalize's 1e-12 clamp under both roots;  loss = sum (1 - c) / 2;
    dq = -(that - c qhat) / |q| / 2;  dPre = dq (1 - q^2);  dS[row of x] += dPre W^T  (un-divided, on top of prev)"""
    S_on, S_tar, W, b = _f64(S_on, S_tar, W, b)
    div = float(np.float32(div))
    ru, ri = np.asarray(u, np.int64), nu + np.asarray(i, np.int64)
    rx, rt = np.concatenate([ru, ri]), np.concatenate([ri, ru])
    x, t = S_on[rx] / div, S_tar[rt] / div
    q = np.tanh(x @ W + b.reshape(1, -1))
    iq = 1.0 / np.sqrt(np.maximum((q * q).sum(1), 1e-12))[:, None]
    it = 1.0 / np.sqrt(np.maximum((t * t).sum(1), 1e-12))[:, None]
    qh, th = q * iq, t * it
    c = (qh * th).sum(1)[:, None]
    loss = float(((1.0 - c) * 0.5).sum())
    dpre = (th - qh * c) * (-0.5 * iq) * (1.0 - q * q)
    dx = dpre @ W.T
    dS = np.zeros(S_on.shape) if prev is None else np.asarray(prev, np.float64).copy()
    scale = _row_norms(dS)
    np.add.at(dS, rx, dx); np.add.at(scale, rx, _row_norms(dx))
    return loss, x, dpre, dS, scale


# ---- perturbation --------------------------------------------------------------------------------------------------------------------
def perturb_inputs(n, d, ld):
    """x = N(0, 0.1) -- the error is measured on e - x against eps = 0.1, and the float32 sum x + delta carries half an ulp of x per
    entry: at N(0, 1) and d = 200 that alone is 4e-6 of eps -- with exact zeros in row 0 (and in row n / 2), two noise tables U[0, 1)
    with one all-zero row each (from three rows on), some entries carrying a forced sign (helpers.encode_forced_signs: +1, -1 or 0 against sign(x)), and
    the table the accumulators start from"""
    from helpers import encode_forced_signs
    rng = _rng(12, n, d, ld)
    x = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    x[0, :3] = 0; x[n // 2, d - 1] = 0
    noises = []
    for v in range(2):
        nz = rng.random((n, d)).astype(np.float32)
        forced = rng.random((n, d)) < 0.02
        forced[0, 1] = forced[0, 4] = True                              # a sign forced onto an exact zero, and onto an ordinary entry
        sign = rng.integers(-1, 2, (n, d))
        nz = np.where(forced, encode_forced_signs(nz, sign), nz).astype(np.float32)
        if n >= 3:
            nz[(n - 1) // 2 if v == 0 else n - 1] = 0                   # l2_normalize's clamp
        noises.append(nz)
    acc0 = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    marked = rng.random(n) < 0.1
    marked[[0, n - 1]] = True
    return dict(x=x, noise=noises, acc0=acc0, marked=marked)


def decode_noise(noise):
    """include/qrec_hip.h, qrec_perturb_rows -> the magnitude u and the forced sign (2 = not forced)"""
    noise = np.asarray(noise, np.float64)
    a = np.abs(noise)
    return np.where(a >= 4, a - 4, np.where(a >= 2, a - 2, noise)), np.where(a >= 4, 0.0, np.where(a >= 2, np.sign(noise), 2.0))


def perturb_delta_ref(x, noise, eps=PERTURB_EPS):
    """SimGCL.py:33-35: e - x = sign(x) * noise / max(|noise|, 1e-6) * eps, the sign taken from the noise where it carries one"""
    x = np.asarray(x, np.float64)
    mag, forced = decode_noise(noise)
    inv = 1.0 / np.sqrt(np.maximum((mag * mag).sum(1), 1e-12))[:, None]
    return np.where(forced != 2.0, forced, np.sign(x)) * (mag * inv) * float(np.float32(eps))


def delta_error(got, x, delta, eps=PERTURB_EPS):
    """max over the rows of |(got - x) - delta| / eps"""
    moved = np.asarray(got, np.float64) - np.asarray(x, np.float64)
    return row_error(moved, delta, np.full(moved.shape[0], float(np.float32(eps))))


def replay_rows(n, ld):
    """the rows whose device-drawn noise the host replays: 64 at the table's start, 64 at its end, 64 either side of the first wrap"""
    wrap = PERTURB_ROWS_PER_TRIP[ld]
    rows = set(range(min(REPLAY_ROWS, n))) | set(range(max(n - REPLAY_ROWS, 0), n))
    if n > wrap:
        rows |= set(range(wrap - REPLAY_ROWS, min(wrap + REPLAY_ROWS, n)))
    return np.array(sorted(rows), np.int64)


def philox_noise(rows, d, ld, seed, stream_id, row0=0):
    """the uniforms perturb_kernel draws for the listed rows (float64 [len(rows), d]; exact: 24-bit numbers).  Lane r of the row's
    ld / 4 lanes owns columns [4 r, 4 r + 4): counter {row + row0, ((row + row0) >> 32) ^ (r << 8), stream_lo, stream_hi}, key = seed,
    uniform = (word >> 8) * 2^-24"""
    from oracle import c as O
    out = np.zeros((len(rows), ld))
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for k, row in enumerate(rows):
        g = int(row) + row0
        for r in range(ld // 4):
            w = O.philox4x32_10((g & 0xFFFFFFFF, ((g >> 32) & 0xFFFFFFFF) ^ (r << 8), stream_id & 0xFFFFFFFF, (stream_id >> 32) & 0xFFFFFFFF), key)
            out[k, 4 * r:4 * r + 4] = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return out[:, :d]


# ---- element-wise ---------------------------------------------------------------------------------------------------------------------
def elementwise_inputs(n):
    rng = np.random.default_rng([13, n])
    return dict(src=rng.standard_normal(n).astype(np.float32), target=rng.standard_normal(n).astype(np.float32),
                theta=rng.standard_normal(n).astype(np.float32), grads=[rng.standard_normal(n).astype(np.float32) for _ in range(ADAM_STEPS)])


def scale_copy_ref(src, alpha=SCALE_ALPHA):
    return float(np.float32(alpha)) * np.asarray(src, np.float64)


def ema_ref(target, online, tau=EMA_TAU):
    """BUIR.py:120-123: target * tau + online * (1 - tau)"""
    tau = float(np.float32(tau))
    return np.asarray(target, np.float64) * tau + np.asarray(online, np.float64) * (1.0 - tau)


def adam_alphas(steps=ADAM_STEPS, lr=ADAM_LR):
    """the float32 alpha of every step, as the host hands it over (oracle/tfmodels.py::AdamTF114.alpha)"""
    from oracle import tfmodels as T
    opt, out = T.AdamTF114((1,), lr), []
    for _ in range(steps):
        out.append(float(opt.alpha()))
        opt.b1p = np.float32(opt.b1p * opt.b1); opt.b2p = np.float32(opt.b2p * opt.b2)
    return out


def adam_ref(theta, grads, l2, grad_scale=ADAM_GRAD_SCALE, beta1=0.9, beta2=0.999, eps=1e-8):
    """TF 1.14's ApplyAdam with g = grad_scale * G + l2 * theta, float64 on the float32 values of every scalar -> theta, m, v"""
    f = lambda s: float(np.float32(s))
    theta = np.asarray(theta, np.float64).copy()
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    for alpha, G in zip(adam_alphas(len(grads)), grads):
        g = f(grad_scale) * np.asarray(G, np.float64) + f(l2) * theta
        m += (g - m) * (1.0 - f(beta1))
        v += (g * g - v) * (1.0 - f(beta2))
        theta -= (m * alpha) / (np.sqrt(v) + f(eps))
    return theta, m, v
