"""MHCN's row kernels (csrc/mhcn.hip; qrec_buir_wgrad behind the gates; qrec_l2norm_rows_accum / _bwd) against the float64 references
of tests/mhcn_cases.py at the row counts where their grid-stride loops wrap and at every row stride they serve -- the existing MHCN
tests run 300 rows at strides 32 / 64, which is 10 to 19 blocks of one trip each.  Every comparison is norm-wise to 1e-5
(tests/test_mhcn_cases_cpu.py holds the fp32 restatement to 3e-6 of the same references on the same inputs); pad columns must be
exactly zero and the guard rows past n must come back byte for byte."""
import numpy as np
import pytest

import mhcn_cases as MC
from helpers import check, check_rel, pad_cols, rel_err
from oracle import tfmodels as T
from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.graph import MHCNTrainer, ordered_reductions

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    yield


@pytest.fixture(autouse=True)
def _parity_mode():
    with ordered_reductions():
        yield


def _bits_differ(a, b):
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)))


def _guarded(n, ld, rows=None, width=None):
    """an output table of n + GUARD_ROWS rows, sentinel everywhere (a row the kernel skips shows up as the sentinel), or ``rows`` (n x d)
    padded to the stride in its first n rows where the kernel accumulates"""
    host = np.full((n + MC.GUARD_ROWS, ld if width is None else width), MC.SENTINEL, np.float32)
    if rows is not None:
        host[:n] = pad_cols(rows, host.shape[1])
    return DB.from_numpy(host)


def _rows(what, buf, n, d, pad_value=0.0):
    """the n x d block of a guarded output table, after checking its pad columns and its guard rows"""
    host = buf.numpy()
    guard = np.full((MC.GUARD_ROWS, host.shape[1]), MC.SENTINEL, np.float32)
    assert host[n:].tobytes() == guard.tobytes(), f"{what}: rows past n were written"
    assert (host[:n, d:] == np.float32(pad_value)).all(), f"{what}: pad columns are not {pad_value}"
    return host[:n, :d]


def _pad2(w, ld):
    return pad_cols(np.pad(w, ((0, ld - w.shape[0]), (0, 0))), ld)


def _hold(what, got, want, case):
    check(f"{what}: rel_err to the fp64 reference", rel_err(got, want), TOL, ctx=case)


@pytest.mark.parametrize("case", MC.GATE_CASES, ids=MC.case_id)
def test_gate_kernels_and_their_weight_gradient_match_fp64(case):
    """qrec_gate_fwd, qrec_gate_bwd and qrec_buir_wgrad straight after it.  S's pad columns are sigmoid(0) = 0.5 by construction (the
    backward kernel masks them out of Q); every other table's are zero."""
    n, d, ld = case
    accumulate, dy_scale = MC.GATE_ARGS[case]
    t = MC.gate_inputs(n, d, ld)
    Y, S, Q, dX, dW, db = MC.gate_ref(t["X"], t["W"], t["b"], t["dY"], dy_scale, t["prev"] if accumulate else None)
    d_X, d_W, d_b = DB.from_numpy(pad_cols(t["X"], ld)), DB.from_numpy(_pad2(t["W"], ld)), DB.from_numpy(pad_cols(t["b"], ld)[0])
    d_Y, d_S, d_Q = _guarded(n, ld), _guarded(n, ld), _guarded(n, ld)
    d_dX = _guarded(n, ld, t["prev"] if accumulate else None)
    capi.gate_fwd(d_X, d_W, d_b, n, ld, d_Y, d_S)
    _hold("gate Y", _rows("Y", d_Y, n, d), Y, case); _hold("gate S", _rows("S", d_S, n, d, 0.5), S, case)
    capi.gate_bwd(d_X, d_S, DB.from_numpy(pad_cols(t["dY"], ld)), d_W, n, d, ld, d_Q, d_dX, accumulate, dy_scale=dy_scale)
    _hold("gate Q", _rows("Q", d_Q, n, d), Q, case); _hold("gate dX", _rows("dX", d_dX, n, d), dX, case)
    gW, gb = DB.from_numpy(np.full((ld, ld), MC.SENTINEL, np.float32)), DB.from_numpy(np.full(ld, MC.SENTINEL, np.float32))
    capi.buir_wgrad(d_X, d_Q, n, ld, DB(capi.buir_wgrad_scratch_bytes(ld), np.uint8), gW, gb)
    gW, gb = gW.numpy(), gb.numpy()
    _hold("gate dW", gW[:d, :d], dW, case); _hold("gate db", gb[:d], db, case)
    assert not gW[d:].any() and not gW[:, d:].any() and not gb[d:].any()


def _attention_on_device(case, t):
    """one forward and one backward call with the case's arguments -> the device buffers"""
    n, d, ld = case
    with_half, accumulate, dh = MC.ATT_ARGS[case]
    d_e = [DB.from_numpy(pad_cols(e, ld)) for e in t["es"]]
    d_a, d_M = DB.from_numpy(pad_cols(t["a"], ld)[0]), DB.from_numpy(_pad2(t["M"], ld))
    d_v, d_ws = DB.from_numpy(np.full(256, MC.SENTINEL, np.float32)), DB(capi.channel_attention_scratch_floats(), np.float32)
    d_sc, d_out = _guarded(n, ld, width=4), _guarded(n, ld)
    capi.channel_attention_fwd(d_e, d_a, d_M, DB.from_numpy(pad_cols(t["half"], ld)) if with_half else None, n, ld, d_v, d_sc, d_out)
    d_de = [_guarded(n, ld, p if accumulate else None) for p in t["de_prev"]]
    d_dh = None if dh is None else _guarded(n, ld, t["dhalf_prev"] if dh == "accumulate" else None)
    g_a, g_M = DB.zeros(ld, np.float32), DB.zeros((ld, ld), np.float32)
    capi.channel_attention_bwd(DB.from_numpy(pad_cols(t["dOut"], ld)), d_e, d_sc, d_v, d_a, d_M, n, ld, d_de, accumulate, d_dh, dh == "accumulate",
                               d_ws, g_a, g_M)
    return d_v, d_sc, d_out, d_de, d_dh, g_a, g_M


@pytest.mark.parametrize("case", MC.ROW_CASES, ids=MC.case_id)
def test_channel_attention_matches_fp64(case):
    n, d, ld = case
    with_half, accumulate, dh = MC.ATT_ARGS[case]
    t = MC.attention_inputs(n, d, ld)
    v, sc, out, de, dhalf, ga, gM = MC.attention_ref(t["es"], t["a"], t["M"], t["half"] if with_half else None, t["dOut"],
                                                     t["de_prev"] if accumulate else None, t["dhalf_prev"] if dh == "accumulate" else None)
    d_v, d_sc, d_out, d_de, d_dh, g_a, g_M = _attention_on_device(case, t)
    got_v = d_v.numpy()
    _hold("attention v", got_v[:d], v, case)
    assert not got_v[d:ld].any() and (got_v[ld:] == MC.SENTINEL).all()
    _hold("attention score", _rows("score", d_sc, n, 3), sc, case)
    _hold("attention out", _rows("out", d_out, n, d), out, case)
    for k in range(3):
        _hold(f"attention de{k}", _rows(f"de{k}", d_de[k], n, d), de[k], case)
    if dh is not None:
        _hold("attention dhalf", _rows("dhalf", d_dh, n, d), dhalf, case)
    g_a, g_M = g_a.numpy(), g_M.numpy()
    _hold("attention g_a", g_a[:d], ga, case); _hold("attention g_M", g_M[:d, :d], gM, case)
    assert not g_a[d:].any() and not g_M[d:].any() and not g_M[:, d:].any()


def _hss_on_device(case, t):
    n, d, ld = case
    p1, k2, p2, k3, p3 = (np.asarray(x, np.int32) for x in t["perm"])
    inv = lambda p: np.argsort(p).astype(np.int32)
    perms = [DB.from_numpy(x) for x in (p1, inv(p1), p2, inv(p2), k2, inv(k2), p3, inv(p3), k3, inv(k3))]
    d_dem, d_dedge, loss = _guarded(n, ld), _guarded(n, ld), DB.zeros(1, np.float64)
    capi.hss_loss_grad(DB.from_numpy(pad_cols(t["em"], ld)), DB.from_numpy(pad_cols(t["edge"], ld)), n, d, ld, perms, MC.HSS_SCALE[case],
                       DB(capi.hss_scratch_bytes(n), np.uint8), d_dem, d_dedge, loss)
    return float(loss.numpy()[0]), d_dem, d_dedge


@pytest.mark.parametrize("case", MC.ROW_CASES, ids=MC.case_id)
def test_hierarchical_mutual_information_matches_fp64(case):
    n, d, ld = case
    t = MC.hss_inputs(n, d, ld)
    want_loss, dem, dedge = MC.hss_ref(t["em"], t["edge"], t["perm"], MC.HSS_SCALE[case])
    loss, d_dem, d_dedge = _hss_on_device(case, t)
    check_rel("MIM loss vs the fp64 reference", loss, want_loss, TOL, ctx=case)
    _hold("hss dem", _rows("dem", d_dem, n, d), dem, case); _hold("hss dedge", _rows("dedge", d_dedge, n, d), dedge, case)


@pytest.mark.parametrize("case", MC.SAME_BITS_CASES, ids=MC.case_id)
def test_column_sums_have_the_same_bits_on_every_launch_when_threads_own_several_rows(case):
    """past the 512-block cap a thread adds several rows before its block's column sum: g_a, g_M (through dv), de, dem and dedge (through
    graph and d graph) of two launches on the same inputs are the same words.  The fp64 loss ends in atomics: equal to 1e-12."""
    t = MC.attention_inputs(*case)
    runs = [_attention_on_device(case, t) for _ in range(2)]
    (_, _, _, de_a, _, ga_a, gM_a), (_, _, _, de_b, _, ga_b, gM_b) = runs
    for name, a, b in [("g_a", ga_a, ga_b), ("g_M", gM_a, gM_b)] + [(f"de{k}", de_a[k], de_b[k]) for k in range(3)]:
        check(f"attention {name}, two launches: 32-bit words that differ", _bits_differ(a.numpy(), b.numpy()), 0, inclusive=True, ctx=case)
    t = MC.hss_inputs(*case)
    (loss_a, dem_a, dedge_a), (loss_b, dem_b, dedge_b) = (_hss_on_device(case, t) for _ in range(2))
    check("hss dem, two launches: 32-bit words that differ", _bits_differ(dem_a.numpy(), dem_b.numpy()), 0, inclusive=True, ctx=case)
    check("hss dedge, two launches: 32-bit words that differ", _bits_differ(dedge_a.numpy(), dedge_b.numpy()), 0, inclusive=True, ctx=case)
    check_rel("MIM loss, second launch vs first", loss_b, loss_a, 1e-12, ctx=case)


@pytest.mark.parametrize("case", MC.L2NORM_CASES, ids=MC.case_id)
def test_l2norm_pair_matches_fp64(case):
    n, d, ld = case
    t = MC.l2norm_inputs(n, d, ld)
    inv, S, dX = MC.l2norm_ref(t["X"], t["S0"], t["dS"])
    d_X, d_S, d_inv = DB.from_numpy(pad_cols(t["X"], ld)), _guarded(n, ld, t["S0"]), _guarded(n, 1, width=1)
    capi.l2norm_rows_accum(d_X, n, ld, d_S, d_inv)
    got_inv = _rows("1/|row|", d_inv, n, 1)[:, 0]
    _hold("l2norm 1/|row|", got_inv, inv, case); _hold("l2norm S", _rows("S", d_S, n, d), S, case)
    d_out = _guarded(n, ld)
    capi.l2norm_rows_bwd(d_X, d_inv, DB.from_numpy(pad_cols(t["dS"], ld)), n, ld, d_out)
    got = _rows("dX", d_out, n, d)
    _hold("l2norm dX", got, dX, case)
    if n > 77:                                                   # at the clamp: 1e6 and d * 1e6, like tf
        assert got_inv[5] == np.float32(1e6)
        np.testing.assert_array_equal(got[5], t["dS"][5] * np.float32(1e6))


def test_mhcn_training_steps_match_restatement_past_the_block_cap():
    """MHCNTrainer vs the restated model with 8,197 users at d = 50 (stride 64: 512 blocks hold 8,192 rows): two steps with injected
    shuffles, both losses and all 20 parameter tensors.  The one check that the trainer's per-channel offsets into its shuffle tables
    (4 nu bytes apart) and its scratch carve hold at a wrapped grid."""
    rng = np.random.default_rng(8197)
    nu, ni, d, B = 8197, 300, 50, 256
    H, Rm, w, U0, V0 = MC.motif_problem(rng, nu, ni, d, E=30000, Rn=12000)
    ref = T.MHCN(U0, V0, w, H, Rm, 1, lr=0.002, reg=0.01, ss_rate=0.05)
    tr = MHCNTrainer(U0, V0, w, H, Rm, 1, 0.002, 0.01, 0.05)
    for step in range(2):
        u = rng.integers(0, nu, B).astype(np.int32); i = rng.integers(0, ni, B).astype(np.int32); j = rng.integers(0, ni, B).astype(np.int32)
        perms = [(rng.permutation(nu), rng.permutation(d), rng.permutation(nu), rng.permutation(d), rng.permutation(nu)) for _ in range(3)]
        want_rec, want_ss, _, _ = ref.loss_and_grads(u, i, j, perms)
        ref.train_step(u, i, j, perms)
        tr.train_step_async(DB.from_numpy(u), DB.from_numpy(i), DB.from_numpy(j), B, perms=perms)
        rec, ss = tr.losses()
        check_rel("MHCN rec loss, 8,197 users", rec, want_rec, TOL, ctx=step); check_rel("MHCN ss loss, 8,197 users", ss, want_ss, TOL, ctx=step)
        got = tr.parameters()
        assert len(ref.w) == 18
        for k in ref.w:
            check(f"MHCN {k}, 8,197 users: rel_err to the restatement", rel_err(got[k], ref.w[k]), TOL, ctx=step)
        check("MHCN U, 8,197 users: rel_err to the restatement", rel_err(got["U"], ref.U), TOL, ctx=step)
        check("MHCN V, 8,197 users: rel_err to the restatement", rel_err(got["V"], ref.V), TOL, ctx=step)
