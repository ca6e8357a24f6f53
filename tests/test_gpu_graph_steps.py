"""The kernels every graph model's training step shares -- qrec_bpr_batch_loss_grad (csrc/graph.hip), qrec_buir_batch_loss_grad
(csrc/buir.hip), qrec_perturb_rows / qrec_perturb_two_views (csrc/contrastive.hip), qrec_adam_step, qrec_scale_copy, qrec_ema_update --
against the float64 references of tests/graph_step_cases.py, at every row stride they serve and at the sizes where their grid-stride
loops take a second and a third trip.  Every table is held ROW BY ROW (graph_step_cases: the worst row's distance over that row's
scale) to 1e-5; tests/test_graph_step_cases_cpu.py holds the fp32 numpy restatement to a third of that on the same inputs.  Pad
columns must be exactly zero, the guard rows past every output table must come back byte for byte, and so must every row a call has
no business with."""
import numpy as np
import pytest

import graph_step_cases as GC
from helpers import check, check_rel, pad_cols
from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB

pytestmark = pytest.mark.gpu
TOL = GC.TOL


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    yield


def _bits_differ(a, b):
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)))


def _guarded_host(n, ld, rows=None):
    """n + GUARD_ROWS rows of the sentinel (a row the kernel skips shows up as the sentinel), or ``rows`` (n x d) padded to the stride
    in the first n"""
    host = np.full((n + GC.GUARD_ROWS, ld), GC.SENTINEL, np.float32)
    if rows is not None:
        host[:n] = pad_cols(rows, ld)
    return host


def _guarded(n, ld, rows=None):
    return DB.from_numpy(_guarded_host(n, ld, rows))


def _rows(what, buf, n, d):
    """the n x d block of a guarded output table, after checking its pad columns and its guard rows"""
    host = buf.numpy()
    guard = np.full((GC.GUARD_ROWS, host.shape[1]), GC.SENTINEL, np.float32)
    assert host[n:].tobytes() == guard.tobytes(), f"{what}: rows past n were written"
    assert (host[:n, d:] == 0).all(), f"{what}: pad columns are not zero"
    return host[:n, :d]


def _pad2(w, ld):
    return pad_cols(np.pad(w, ((0, ld - w.shape[0]), (0, 0))), ld)


def _same_words(what, a, b, case):
    check(f"{what}: 32-bit words that differ", _bits_differ(a, b), 0, inclusive=True, ctx=case)


# ---- batch BPR ----------------------------------------------------------------------------------------------------------------------
def _bpr_on_device(case, t, ordered):
    B, d, ld = case
    div, reg, nonzero = GC.BPR_ARGS[case]
    nu, n_rows = t["nu"], t["nu"] + t["ni"]
    start = t["prev"] if nonzero else np.zeros_like(t["prev"])
    d_dE, d_loss = _guarded(n_rows, ld, start), DB.zeros(1, np.float64)
    d_mask = DB.zeros((n_rows + 31) // 32 + 2, np.uint32)
    capi.bpr_batch_loss_grad(DB.from_numpy(pad_cols(t["S"], ld)), div, nu, n_rows, ld, DB.from_numpy(t["u"]), DB.from_numpy(t["i"]),
                             DB.from_numpy(t["j"]), B, float(GC.BPR_EPS), reg, d_dE, d_loss, d_row_mask=d_mask, ordered=ordered)
    return _rows("dE", d_dE, n_rows, d), float(d_loss.numpy()[0]), d_mask.numpy(), start


@pytest.mark.parametrize("case", GC.BPR_CASES, ids=GC.case_id)
def test_bpr_batch_loss_grad_matches_fp64_row_by_row(case):
    """float atomics and the ordered workspace: all eight instantiations of bpr_batch_kernel over the case table"""
    t = GC.bpr_inputs(*case)
    div, reg, nonzero = GC.BPR_ARGS[case]
    want_loss, dE, scale, words, (rows, _) = GC.bpr_ref(t["S"], t["u"], t["i"], t["j"], t["nu"], div, reg, prev=t["prev"] if nonzero else None)
    untouched = np.setdiff1d(np.arange(dE.shape[0]), rows)
    assert untouched.size >= 2
    runs = [("atomics", None), ("ordered", capi.OrderedScatter()), ("ordered again", capi.OrderedScatter())]
    got = {}
    for mode, ordered in runs:
        got[mode] = g, loss, mask, start = _bpr_on_device(case, t, ordered)
        check(f"bpr dE, {mode}: worst row error over the sum of its addends' norms", GC.row_error(g, dE, scale), TOL, ctx=case)
        check_rel(f"bpr loss, {mode}, vs the fp64 reference", loss, want_loss, TOL, ctx=case)
        assert g[untouched].tobytes() == start[untouched].tobytes(), f"{mode}: a row no triplet names was written"
        assert np.array_equal(mask, words), f"{mode}: the row bitmap is not that of unique(u, nu + i, nu + j)"
    _same_words("bpr dE, two ordered launches", got["ordered"][0], got["ordered again"][0], case)
    check_rel("bpr loss, second ordered launch vs first", got["ordered again"][1], got["ordered"][1], 1e-12, ctx=case)


# ---- BUIR batch -----------------------------------------------------------------------------------------------------------------------
def _buir_on_device(case, t, ordered):
    B, d, ld = case
    nu, n_rows = t["nu"], t["nu"] + t["ni"]
    start = t["prev"] if GC.BUIR_ARGS[case][2] else np.zeros_like(t["prev"])
    d_dS, d_X, d_G, d_loss = _guarded(n_rows, ld, start), _guarded(2 * B, ld), _guarded(2 * B, ld), DB.zeros(1, np.float64)
    capi.buir_batch_loss_grad(DB.from_numpy(pad_cols(t["S_on"], ld)), DB.from_numpy(pad_cols(t["S_tar"], ld)), t["div"], nu, ld,
                              DB.from_numpy(_pad2(t["W"], ld)), DB.from_numpy(pad_cols(t["b"], ld)[0]), DB.from_numpy(t["u"]), DB.from_numpy(t["i"]),
                              B, d_dS, d_X, d_G, d_loss, ordered=ordered)
    return _rows("dS", d_dS, n_rows, d), _rows("Xb", d_X, 2 * B, d), _rows("Gb", d_G, 2 * B, d), float(d_loss.numpy()[0]), start


@pytest.mark.parametrize("case", GC.BUIR_CASES, ids=GC.case_id)
def test_buir_batch_loss_grad_matches_fp64_row_by_row(case):
    """all three strides in both modes; stride 128 is the launch that asks for more than 64 KiB of dynamic LDS"""
    t = GC.buir_inputs(*case)
    prev = t["prev"] if GC.BUIR_ARGS[case][2] else None
    want_loss, Xb, Gb, dS, scale = GC.buir_ref(t["S_on"], t["S_tar"], t["W"], t["b"], t["u"], t["i"], t["nu"], t["div"], prev)
    untouched = np.setdiff1d(np.arange(dS.shape[0]), np.concatenate([t["u"], t["nu"] + t["i"]]))
    got = {}
    for mode, ordered in [("atomics", None), ("ordered", capi.OrderedScatter()), ("ordered again", capi.OrderedScatter())]:
        got[mode] = g_dS, g_X, g_G, loss, start = _buir_on_device(case, t, ordered)
        check(f"buir Xb, {mode}: worst row error over the row's norm", GC.plain_row_error(g_X, Xb), TOL, ctx=case)
        check(f"buir Gb, {mode}: worst row error over the row's norm", GC.plain_row_error(g_G, Gb), TOL, ctx=case)
        check(f"buir dS, {mode}: worst row error over the sum of its addends' norms", GC.row_error(g_dS, dS, scale), TOL, ctx=case)
        check_rel(f"buir loss, {mode}, vs the fp64 reference", loss, want_loss, TOL, ctx=case)
        assert g_dS[untouched].tobytes() == start[untouched].tobytes(), f"{mode}: a row no batch element names was written"
    _same_words("buir dS, two ordered launches", got["ordered"][0], got["ordered again"][0], case)
    check_rel("buir loss, second ordered launch vs first", got["ordered again"][3], got["ordered"][3], 1e-12, ctx=case)


# ---- perturbation --------------------------------------------------------------------------------------------------------------------
def _noise(nz, ld):
    """the noise table at the stride, its pad columns holding numbers too (the kernel takes the first d)"""
    out = np.full((nz.shape[0], ld), 0.5, np.float32)
    out[:, :nz.shape[1]] = nz
    return DB.from_numpy(out)


def _hold_delta(what, got, x, delta, case):
    check(f"{what}: worst row error of e - x over eps", GC.delta_error(got, x, delta), TOL, ctx=case)


@pytest.mark.parametrize("case", GC.PERTURB_CASES, ids=GC.case_id)
def test_perturb_rows_with_injected_noise_matches_fp64(case):
    n, d, ld = case
    out_of_place, with_accum = GC.PERTURB_ARGS[case]
    t = GC.perturb_inputs(*case)
    x, nz = t["x"], t["noise"][0]
    delta = GC.perturb_delta_ref(x, nz)
    d_emb = _guarded(n, ld, None if out_of_place else x)
    d_acc = _guarded(n, ld, t["acc0"]) if with_accum else None
    capi.perturb_rows(d_emb, n, d, ld, float(GC.PERTURB_EPS), _noise(nz, ld), d_accum=d_acc, d_src=DB.from_numpy(pad_cols(x, ld)) if out_of_place else None)
    got = _rows("emb", d_emb, n, d)
    _hold_delta("perturb_rows", got, x, delta, case)
    still = (x == 0) & (GC.decode_noise(nz)[1] == 2)
    assert still.any() and not got[still].any(), "sign(0) moved an entry"
    if with_accum:
        want = t["acc0"].astype(np.float64) + x.astype(np.float64) + delta
        check("perturb_rows accum: worst row error over the row's norm", GC.plain_row_error(_rows("accum", d_acc, n, d), want), TOL, ctx=case)


def _two_views(case, t, noises=None, streams=(0, 0), rows=None, prior=None):
    """qrec_perturb_two_views into five tables that start from the sentinel (or from ``prior``) -> emb1, emb2, sum1, sum2, src_sum"""
    n, d, ld = case
    outs = [_guarded(n, ld) if prior is None else DB.from_numpy(prior) for _ in range(5)]
    d_n = [None, None] if noises is None else [_noise(nz, ld) for nz in noises]
    capi.perturb_two_views(DB.from_numpy(pad_cols(t["x"], ld)), outs[0], outs[1], n, d, ld, float(GC.PERTURB_EPS), d_n[0], d_n[1], GC.PERTURB_SEED,
                           streams[0], streams[1], outs[2], outs[3], outs[4], rows=rows)
    return outs


_VIEW_TABLES = ("emb1", "emb2", "sum1", "sum2", "src_sum")


@pytest.mark.parametrize("case", GC.PERTURB_CASES, ids=GC.case_id)
def test_perturb_two_views_with_injected_noise_matches_fp64_and_assigns_the_sums(case):
    n, d, ld = case
    t = GC.perturb_inputs(*case)
    e1, e2, s1, s2, ss = (_rows(name, buf, n, d) for name, buf in zip(_VIEW_TABLES, _two_views(case, t, t["noise"])))
    for v, e in enumerate((e1, e2)):
        _hold_delta(f"perturb_two_views view {v + 1}", e, t["x"], GC.perturb_delta_ref(t["x"], t["noise"][v]), case)
    # the sums started from the sentinel: assigned, not added to
    _same_words("two views: sum1 vs emb1", s1, e1, case); _same_words("two views: sum2 vs emb2", s2, e2, case)
    _same_words("two views: src_sum vs the source", ss, t["x"], case)


@pytest.mark.parametrize("case", GC.PERTURB_SUBSET_CASES, ids=GC.case_id)
def test_perturb_row_subset_writes_the_listed_rows_only(case):
    """about a tenth of the rows through capi.RowSubset (capacity above the count): both entry points"""
    n, d, ld = case
    t = GC.perturb_inputs(*case)
    x, marked = t["x"], t["marked"]
    idx = np.nonzero(marked)[0]
    words = np.zeros((n + 31) // 32, np.uint32)
    np.bitwise_or.at(words, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    sub = capi.RowSubset(idx.size + 37).from_mask(DB.from_numpy(words), n, idx.size + 37)
    assert int(sub.count.numpy()[0]) == idx.size
    eps, d_x = float(GC.PERTURB_EPS), DB.from_numpy(pad_cols(x, ld))
    prior = _guarded_host(n, ld, np.random.default_rng(n).standard_normal((n, d)).astype(np.float32))
    # one view
    full, full_acc = _guarded(n, ld), _guarded(n, ld, t["acc0"])
    capi.perturb_rows(full, n, d, ld, eps, _noise(t["noise"][0], ld), d_accum=full_acc, d_src=d_x)
    part, part_acc = DB.from_numpy(prior), _guarded(n, ld, t["acc0"])
    capi.perturb_rows(part, n, d, ld, eps, _noise(t["noise"][0], ld), d_accum=part_acc, d_src=d_x, rows=sub)
    full, part, full_acc, part_acc = full.numpy(), part.numpy(), full_acc.numpy(), part_acc.numpy()
    _same_words("perturb_rows, listed rows vs the full call", part[idx], full[idx], case)
    _same_words("perturb_rows accum, listed rows vs the full call", part_acc[idx], full_acc[idx], case)
    _hold_delta("perturb_rows, listed rows", part[idx, :d], x[idx], GC.perturb_delta_ref(x, t["noise"][0])[idx], case)
    keep = np.setdiff1d(np.arange(n + GC.GUARD_ROWS), idx)
    assert part[keep].tobytes() == prior[keep].tobytes() and part_acc[keep].tobytes() == _guarded_host(n, ld, t["acc0"])[keep].tobytes()
    # two views
    full = [b.numpy() for b in _two_views(case, t, t["noise"])]
    part = [b.numpy() for b in _two_views(case, t, t["noise"], rows=sub, prior=prior)]
    for name, f, p in zip(_VIEW_TABLES, full, part):
        _same_words(f"perturb_two_views {name}, listed rows vs the full call", p[idx], f[idx], case)
        assert p[keep].tobytes() == prior[keep].tobytes(), f"{name}: a row outside the subset was written"
    _hold_delta("perturb_two_views view 2, listed rows", part[1][idx, :d], x[idx], GC.perturb_delta_ref(x, t["noise"][1])[idx], case)


def _drawn(case, x, stream_id, row0=0):
    """qrec_perturb_rows with device-drawn noise, out of place"""
    n, d, ld = x.shape[0], case[1], case[2]
    d_emb = _guarded(n, ld)
    capi.perturb_rows(d_emb, n, d, ld, float(GC.PERTURB_EPS), None, seed=GC.PERTURB_SEED, stream_id=stream_id, d_src=DB.from_numpy(pad_cols(x, ld)),
                      philox_row0=row0)
    return _rows("emb", d_emb, n, d)


@pytest.mark.parametrize("case", GC.PERTURB_CASES, ids=GC.case_id)
def test_perturb_device_noise_is_the_hosts_philox_replay(case):
    """the draws replayed with oracle.c.philox4x32_10 for 64 rows at the table's start, its end and either side of the first wrap; the
    two views against two single calls; a block of rows as a table of its own with philox_row0"""
    n, d, ld = case
    t = GC.perturb_inputs(*case)
    x, (sa, sb) = t["x"], GC.PERTURB_STREAMS
    rows = GC.replay_rows(n, ld)
    one = [_drawn(case, x, s) for s in (sa, sb)]
    for s, e in zip((sa, sb), one):
        delta = GC.perturb_delta_ref(x[rows], GC.philox_noise(rows, d, ld, GC.PERTURB_SEED, s))
        _hold_delta(f"perturb_rows, drawn noise, stream {s:#x}", e[rows], x[rows], delta, case)
    e1, e2, s1, s2, _ = (_rows(name, buf, n, d) for name, buf in zip(_VIEW_TABLES, _two_views(case, t, None, (sa, sb))))
    _same_words("drawn noise: view 1 vs perturb_rows with its stream", e1, one[0], case)
    _same_words("drawn noise: view 2 vs perturb_rows with its stream", e2, one[1], case)
    _same_words("drawn noise: sum1 vs emb1", s1, e1, case); _same_words("drawn noise: sum2 vs emb2", s2, e2, case)
    lo = n // 3
    hi = min(n, lo + 300)
    _same_words("a block of rows as a table of its own with philox_row0", _drawn(case, x[lo:hi], sa, row0=lo), one[0][lo:hi], case)
    far = (1 << 32) + 5                                   # the counter's second word
    k = min(n, 8)
    delta = GC.perturb_delta_ref(x[:k], GC.philox_noise(np.arange(k), d, ld, GC.PERTURB_SEED, sa, row0=far))
    _hold_delta("perturb_rows, drawn noise, philox_row0 past 2^32", _drawn(case, x[:k], sa, row0=far), x[:k], delta, case)


# ---- element-wise ---------------------------------------------------------------------------------------------------------------------
def _flat(values, n):
    """n elements and ELEMENTWISE_GUARD sentinel words past them"""
    host = np.full(n + GC.ELEMENTWISE_GUARD, GC.SENTINEL, np.float32)
    if values is not None:
        host[:n] = values
    return DB.from_numpy(host)


def _head(what, buf, n):
    host = buf.numpy()
    assert (host[n:] == GC.SENTINEL).all(), f"{what}: words past n_elems were written"
    return host[:n]


@pytest.mark.parametrize("n", GC.ELEMENTWISE_N)
def test_scale_copy_and_ema_update_match_fp64_on_every_grid_trip(n):
    t = GC.elementwise_inputs(n)
    d_dst = _flat(None, n)
    capi.scale_copy(d_dst, _flat(t["src"], n), n, float(GC.SCALE_ALPHA))
    check_rel("scale_copy vs the fp64 reference", _head("scale_copy", d_dst, n), GC.scale_copy_ref(t["src"]), TOL, ctx=n, abs_tol=GC.ABS_TOL_SCALE_COPY)
    d_tar = _flat(t["target"], n)
    capi.ema_update(d_tar, _flat(t["src"], n), float(GC.EMA_TAU), n)
    check_rel("ema_update vs the fp64 reference", _head("ema_update", d_tar, n), GC.ema_ref(t["target"], t["src"]), TOL, ctx=n, abs_tol=GC.ABS_TOL_EMA)


@pytest.mark.parametrize("n", GC.ELEMENTWISE_N)
def test_adam_step_matches_fp64_on_every_grid_trip(n):
    """three steps with grad_scale = 1 / 3, with and without grad_l2"""
    t = GC.elementwise_inputs(n)
    l2 = GC.ADAM_L2[n]
    d_th, d_m, d_v = _flat(t["theta"], n), _flat(np.zeros(n, np.float32), n), _flat(np.zeros(n, np.float32), n)
    for alpha, G in zip(GC.adam_alphas(), t["grads"]):
        capi.adam_step(d_th, d_m, d_v, _flat(G, n), n, float(GC.ADAM_GRAD_SCALE), alpha, grad_l2=l2)
    theta, m, v = GC.adam_ref(t["theta"], t["grads"], l2)
    check_rel("adam theta vs the fp64 reference", _head("theta", d_th, n), theta, TOL, ctx=(n, l2), abs_tol=GC.ABS_TOL_ADAM_THETA)
    check_rel("adam m vs the fp64 reference", _head("m", d_m, n), m, TOL, ctx=(n, l2), abs_tol=GC.ABS_TOL_ADAM_M)
    check_rel("adam v vs the fp64 reference", _head("v", d_v, n), v, TOL, ctx=(n, l2), abs_tol=GC.ABS_TOL_ADAM_V)
