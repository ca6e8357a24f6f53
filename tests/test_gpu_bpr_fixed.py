"""The fixed-point flavour of the item-major BPR epoch (QREC_HW_FIXED: csrc/bpr_sgd.hip bpr_hogwild_item_kernel<..., FIX>, csrc/reduce.hip
fixed_convert_in_kernel and epoch_close_kernel<..., FIX>): tables are int32 = rint(x * 2^26) between convert-in and the epoch close,
every delta is an integer atomic add.

On conflict-free lists (tests/conflict_free.py) the epoch has one right answer, the sequential recurrence: compared with ``O.bpr_sgd`` in
fp64 at the 1e-5 of the float kernels' tests, on one group, the default grid and an odd grid, both addressing flavours, every template
instantiation; full grid and one group bit for bit.  The codec against its numpy restatement (tests/fixed_codec.py); the range guard; and
a device-driven run on colliding triplets against the same run with float deltas."""
import numpy as np
import pytest

from oracle import c as O
from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.engine import BprSgd, DeviceTables, padded_ld

import fixed_codec as FX
from conflict_free import chunks_are_row_disjoint, conflict_free_triplets
from helpers import check, rel_err

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5     # the float kernels' bound (tests/test_gpu_bpr_grid.py)
LR, REG_U, REG_I = 0.05, 0.01, 0.02
UNUSED = 3         # rows at the end of both tables that no triplet names


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    info = capi.device_info()
    assert info["arch"].startswith("gfx950"), info
    yield


def _driver(lr=LR):
    st = np.zeros(capi.DRV_WORDS, np.float64); st[capi.DRV_LR] = lr
    return DB.from_numpy(st)


def _fixed_epoch(t, sgd, dim, chunk, groups, flush, n=None):
    """convert-in, the SGD launch, the close: what ``BprSgd.epoch_device_async`` enqueues.  Returns (driver state, log row of the epoch)"""
    drv, log = _driver(), DB.zeros((1, capi.DRV_LOG_WORDS), np.float64)
    sgd.d_stats.fill_bytes(0)
    capi.bpr_fixed_convert_in(t.P, t.n_users, t.Q, t.n_items, t.ld, drv)
    capi.bpr_sgd_hogwild_item_major(t.P, t.Q, dim, t.ld, sgd.d_u, sgd.d_i, sgd.d_j, sgd.n if n is None else n, chunk, groups, flush, 0.0,
                                    REG_U, REG_I, sgd.d_stats, d_driver_state=drv, variant=capi.HW_FIXED)
    capi.epoch_close_fixed(t.P, t.n_users, t.Q, t.n_items, t.ld, sgd.d_stats, drv, REG_U, REG_I, 1.0, 0.0, log, 1)
    return drv.numpy(), log.numpy()[0]


def _rows_per_block(block):
    return (5, 12) if block >= 16 else (3, 6) if block >= 7 else (1, 2)


def _problem(seed, dim, n_blocks, block, tail):
    rng = np.random.default_rng(seed)
    nu, ni = _rows_per_block(block)
    u, i, j = conflict_free_triplets(rng, n_blocks, block, nu, ni, tail)
    P0 = rng.random((n_blocks * nu + UNUSED, dim), dtype=np.float32) / 3
    Q0 = rng.random((n_blocks * ni + UNUSED, dim), dtype=np.float32) / 3
    return u, i, j, P0, Q0


def _oracle(P0, Q0, us, is_, js):
    Pr, Qr = P0.astype(np.float64), Q0.astype(np.float64)
    lref = O.bpr_sgd(Pr, Qr, np.ascontiguousarray(us), np.ascontiguousarray(is_), np.ascontiguousarray(js), LR, REG_U, REG_I) if len(us) else 0.0
    return Pr, Qr, lref


def _hold_to_oracle(what, t, dim, P0, Q0, Pr, Qr, lref, state, log):
    """tables, loss and the close's sums after a fixed-point epoch against the fp64 recurrence; pad columns exactly zero; rows that no
    triplet names changed by the codec's round trip and nothing else"""
    assert state[capi.DRV_FAILED] == 0.0 and state[capi.DRV_EPOCHS] == 1.0
    Pf, Qf = t.P.numpy(), t.Q.numpy()
    check(f"{what}: P vs the sequential recurrence", rel_err(Pf[:, :dim], Pr), F32_TOL)
    check(f"{what}: Q vs the sequential recurrence", rel_err(Qf[:, :dim], Qr), F32_TOL)
    if lref:
        check(f"{what}: loss", abs(log[2] - lref) / lref, F32_TOL)
    assert (Pf[:, dim:] == 0).all() and (Qf[:, dim:] == 0).all()
    assert np.array_equal(Pf[-UNUSED:, :dim], FX.round_trip(P0[-UNUSED:])) and np.array_equal(Qf[-UNUSED:, :dim], FX.round_trip(Q0[-UNUSED:]))
    # the close's sums are those of the fp32 tables it wrote
    check(f"{what}: sum P*P of the close", abs(log[4] - (Pf.astype(np.float64) ** 2).sum()) / max(log[4], 1e-300), 1e-12)
    check(f"{what}: sum Q*Q of the close", abs(log[5] - (Qf.astype(np.float64) ** 2).sum()) / max(log[5], 1e-300), 1e-12)
    return Pf, Qf


# (chunk, flush_every, item_run): the shipped default; whole item runs; odd sizes with flushes inside the runs; short runs; a flush per triplet
DEFAULT_CFG, WHOLE, ODD, SHORT, EVERY = (32, 16, 16), (64, 64, 0), (7, 3, 7), (32, 8, 8), (8, 1, 8)


def _default_groups(dim):
    return 256 * 4 * {32: 4, 64: 4, 128: 2, 256: 1}[padded_ld(dim, np.float32)]


def _case(dim, ptr64, cfg, groups, tail):
    g = "default_grid" if groups == 0 else f"{groups}_groups"
    return pytest.param(dim, ptr64, cfg, groups, tail, id=f"d{dim}-{'ptr64' if ptr64 else 'desc'}-chunk{cfg[0]}_flush{cfg[1]}_run{cfg[2]}-{g}-tail{tail}")


CASES = [
    _case(64, False, DEFAULT_CFG, 0, 5), _case(64, True, ODD, 37, 2), _case(64, True, EVERY, 0, 3),
    _case(50, False, WHOLE, 37, 7), _case(50, True, DEFAULT_CFG, 0, 9),
    _case(8, False, EVERY, 0, 3), _case(8, True, ODD, 37, 2),
    _case(128, False, DEFAULT_CFG, 0, 5), _case(128, True, SHORT, 37, 3),
    _case(200, False, DEFAULT_CFG, 0, 5), _case(200, True, ODD, 37, 3),
]


@pytest.mark.parametrize("dim,ptr64,cfg,groups,tail", CASES)
def test_fixed_point_epoch_on_conflict_free_input_is_the_sequential_recurrence(dim, ptr64, cfg, groups, tail, monkeypatch):
    """Default grid: more chunks than groups, so groups run one and two rounds; odd grid: 37 groups (ends inside a wavefront), 6 and 7
    rounds; every list ends in a short tail chunk.  Then the same order on ONE group: the oracle again, and the same bits -- every row
    receives its integer deltas from one group in program order, and the copy a group forwards is what memory holds."""
    chunk, flush, item_run = cfg
    block = item_run if item_run > 0 else chunk
    n_chunks = _default_groups(dim) + 1001 if groups == 0 else groups * 6 + 5
    u, i, j, P0, Q0 = _problem(dim * 1000 + chunk + tail, dim, n_chunks * (chunk // block), block, tail)
    assert -(-u.size // chunk) == n_chunks and 0 < u.size % chunk < chunk          # a short tail chunk
    if ptr64:
        monkeypatch.setenv("QREC_FORCE_64BIT_ADDRESSING", "1")
    t = DeviceTables(P0, Q0, np.float32)
    sgd = BprSgd(t, u, i, schedule="item", item_run=item_run); sgd.set_negatives(j)
    us, is_, js = sgd.d_u.numpy()[:sgd.n], sgd.d_i.numpy()[:sgd.n], sgd.d_j.numpy()[:sgd.n]
    assert chunks_are_row_disjoint(us, is_, js, chunk)
    Pr, Qr, lref = _oracle(P0, Q0, us, is_, js)
    Pf, Qf = _hold_to_oracle("fixed point, full grid", t, dim, P0, Q0, Pr, Qr, lref, *_fixed_epoch(t, sgd, dim, chunk, groups, flush))
    t.upload(P0, Q0)
    P1, Q1 = _hold_to_oracle("fixed point, one group", t, dim, P0, Q0, Pr, Qr, lref, *_fixed_epoch(t, sgd, dim, chunk, 1, flush))
    assert np.array_equal(Pf.view(np.uint32), P1.view(np.uint32)), "P: full grid and one group differ in some bit"
    assert np.array_equal(Qf.view(np.uint32), Q1.view(np.uint32)), "Q: full grid and one group differ in some bit"


@pytest.mark.parametrize("ptr64", [False, True])
@pytest.mark.parametrize("dim", [64, 128, 200, 8])
@pytest.mark.parametrize("n", [0, 1, 33])
def test_fixed_point_epoch_degenerate_lengths(dim, n, ptr64, monkeypatch):
    """no triplet (the tables make the codec's round trip and nothing else), one triplet, and chunk + 1 triplets (a second chunk of one),
    on the default grid, which the launcher clamps to the number of chunks"""
    chunk, flush, item_run = DEFAULT_CFG
    u, i, j, P0, Q0 = _problem(dim + 7 * n, dim, 3, item_run, 1)
    assert u.size == chunk + 1
    if ptr64:
        monkeypatch.setenv("QREC_FORCE_64BIT_ADDRESSING", "1")
    t = DeviceTables(P0, Q0, np.float32)
    if n < 2:
        u, i, j = u[:1], i[:1], j[:1]
    sgd = BprSgd(t, u, i, schedule="item", item_run=item_run); sgd.set_negatives(j)
    us, is_, js = sgd.d_u.numpy()[:n], sgd.d_i.numpy()[:n], sgd.d_j.numpy()[:n]
    assert chunks_are_row_disjoint(us, is_, js, chunk)
    Pr, Qr, lref = _oracle(P0, Q0, us, is_, js)
    Pf, Qf = _hold_to_oracle(f"fixed point, {n} triplet(s)", t, dim, P0, Q0, Pr, Qr, lref, *_fixed_epoch(t, sgd, dim, chunk, 0, flush, n=n))
    if n == 0:
        assert np.array_equal(Pf[:, :dim], FX.round_trip(P0)) and np.array_equal(Qf[:, :dim], FX.round_trip(Q0))


def test_codec_on_the_device_is_the_numpy_restatement():
    """convert-in leaves rint(x * 2^26) (ties to even), the close writes float(q) * 2^-26 back: 0, +-one quantum, half-way cases, the
    largest value in range, and a table of ordinary values; |x - back| <= 2^-27"""
    rng = np.random.default_rng(5)
    edge = FX.edge_values()
    dim = 64
    P0 = np.concatenate([edge, (rng.random(3 * dim - edge.size, dtype=np.float32) - 0.5) * 31]).astype(np.float32).reshape(3, dim)
    Q0 = (rng.random((1037, dim), dtype=np.float32) / 3).astype(np.float32)
    t = DeviceTables(P0, Q0, np.float32)
    drv, stats = _driver(), DB.zeros(capi.STATS_WORDS, np.float64)
    capi.bpr_fixed_convert_in(t.P, t.n_users, t.Q, t.n_items, t.ld, drv)
    assert np.array_equal(t.P.numpy().view(np.int32), FX.encode(P0)) and np.array_equal(t.Q.numpy().view(np.int32), FX.encode(Q0))
    assert drv.numpy()[capi.DRV_FAILED] == 0.0
    capi.epoch_close_fixed(t.P, t.n_users, t.Q, t.n_items, t.ld, stats, drv, REG_U, REG_I, 1.0, 0.0)
    Pb, Qb = t.P.numpy(), t.Q.numpy()
    assert np.array_equal(Pb, FX.round_trip(P0)) and np.array_equal(Qb, FX.round_trip(Q0))
    assert np.abs(Pb.astype(np.float64) - P0).max() <= 2.0 ** -27 and np.abs(Qb.astype(np.float64) - Q0).max() <= 2.0 ** -27
    st = drv.numpy()
    assert st[capi.DRV_EPOCHS] == 1.0 and st[capi.DRV_FAILED] == 0.0
    assert st[capi.DRV_LAST_LOSS] == pytest.approx(REG_U * (Pb.astype(np.float64) ** 2).sum() + REG_I * (Qb.astype(np.float64) ** 2).sum(), rel=1e-12)


def _colliding(seed=9, U=300, I=200, n=5000, dim=64):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, U, n).astype(np.int32); i = rng.integers(0, I, n).astype(np.int32)
    js = [np.where((jj := rng.integers(0, I, n).astype(np.int32)) == i, (jj + 1) % I, jj).astype(np.int32) for _ in range(3)]
    P0 = rng.random((U, dim), dtype=np.float32) / 3; Q0 = rng.random((I, dim), dtype=np.float32) / 3
    return u, i, js, P0, Q0


def _driven(u, i, js, P0, Q0, accum, epochs=3, groups=0):
    t = DeviceTables(P0, Q0, np.float32)
    sgd = BprSgd(t, u, i, schedule="item"); sgd.accum = accum
    sgd.start_device_driver(LR, log_capacity=8)
    assert sgd.fixed_accum(groups) == (accum == "i32")
    for k in range(epochs):
        sgd.set_negatives(js[k % len(js)])
        sgd.epoch_device_async(REG_U, REG_I, 1.0, tol=0.0, groups=groups)
    return t, sgd


@pytest.mark.parametrize("bad", [16.0, -16.0, np.inf, -np.inf, np.nan])
def test_a_table_out_of_range_fails_the_run_and_nothing_wraps(bad):
    """convert-in meets 16.0, an infinity or a NaN: FAILED, no epoch is counted, this epoch's SGD launch and the epochs enqueued behind
    it are no-ops, and the close still hands fp32 tables back -- every other element its round trip, the bad one saturated on its own side"""
    u, i, js, P0, Q0 = _colliding()
    Q0 = Q0.copy(); Q0[17, 5] = bad
    t, sgd = _driven(u, i, js, P0, Q0, "i32", epochs=3)
    st = sgd.driver_state()
    assert st["failed"] and not st["converged"] and st["epochs"] == 0
    assert sgd.d_drv.numpy()[capi.DRV_FAILED] == 1.0                 # the tables are fp32 again
    Pb, Qb = t.P.numpy(), t.Q.numpy()
    assert np.array_equal(Pb, FX.round_trip(P0)) and np.array_equal(Qb, FX.round_trip(Q0))
    assert np.isfinite(Qb).all() and np.abs(Qb).max() <= 32.0
    if not np.isnan(bad):
        assert np.sign(Qb[17, 5]) == np.sign(bad) and abs(Qb[17, 5]) >= 16.0


@pytest.mark.parametrize("side", [1.0, -1.0])
def test_a_step_that_leaves_the_range_fails_the_run_and_nothing_wraps(side):
    """every value is inside the range at convert-in; one triplet's step takes P[u][0] from +-15.99 to +-16.012 (the other columns pull
    the score to -32, so the step is lr * (Q[i] - Q[j]) = 0.03 in full, less lr * regU * 16): the SGD launch raises FAILED, the close writes the tables
    back and counts no epoch, the next epochs are no-ops, and no element has changed its sign"""
    dim = 8
    u, i, js, P0, Q0 = _colliding(dim=dim)
    uu, ii, jj = P0.shape[0], Q0.shape[0], Q0.shape[0] + 1           # a user and two items of its own: nobody else moves these rows
    u, i, js = np.append(u, uu).astype(np.int32), np.append(i, ii).astype(np.int32), [np.append(j, jj).astype(np.int32) for j in js]
    P0 = np.concatenate([P0, np.full((1, dim), -10.0 * side, np.float32)]); P0[uu, 0] = 15.99 * side
    Q0 = np.concatenate([Q0, np.full((1, dim), 0.3 * side, np.float32), np.full((1, dim), -0.3 * side, np.float32)])
    assert np.abs(P0).max() < 16 and np.abs(Q0).max() < 16
    t, sgd = _driven(u, i, js, P0, Q0, "i32", epochs=1)
    st = sgd.driver_state()
    assert st["failed"] and st["epochs"] == 0 and sgd.d_drv.numpy()[capi.DRV_FAILED] == 1.0
    P1, Q1 = t.P.numpy(), t.Q.numpy()
    assert np.isfinite(P1).all() and np.isfinite(Q1).all() and max(np.abs(P1).max(), np.abs(Q1).max()) < 32.0
    assert abs(P1[uu, 0]) >= 16.0 and np.sign(P1[uu, 0]) == side
    big = np.abs(P0) > 1.0                                            # an element that wrapped would have jumped to the other side
    assert np.array_equal(np.sign(P1[:, :dim][big]), np.sign(P0[big]))
    for k in range(2):
        sgd.set_negatives(js[1]); sgd.epoch_device_async(REG_U, REG_I, 1.0, tol=0.0)
    assert sgd.driver_state()["epochs"] == 0
    assert np.array_equal(t.P.numpy(), P1) and np.array_equal(t.Q.numpy(), Q1)


def _driven_losses(data, accum, groups, runs):
    out = []
    for _ in range(runs):
        _, sgd = _driven(*data, accum, groups=groups)
        assert not sgd.driver_state()["failed"]
        out.append(sgd.driver_log()[:, :2].copy())          # per epoch: loss, learning rate used
    return np.array(out)


def test_driven_run_on_one_group_integer_against_float_deltas():
    """three device-driven epochs on 5,000 colliding triplets (300 users, 200 items) on ONE group, where a run is a function of its
    inputs and the same rows still repeat inside every chunk: the same bold-driver decisions, and the loss within the 2e-4 that
    bench.py's docstring records between two float runs of one build (measured: 3461.332750 / 3461.332729, 3394.649424 / 3394.649438,
    3353.171178 / 3353.171195 = 6e-9)"""
    data = _colliding()
    f, i = _driven_losses(data, "f32", 1, 1)[0], _driven_losses(data, "i32", 1, 1)[0]
    assert f.shape == i.shape == (3, 2) and np.array_equal(f[:, 1], i[:, 1])
    for k in range(3):
        check(f"driven run on one group, epoch {k + 1}: loss, integer against float deltas", abs(f[k, 0] - i[k, 0]) / f[k, 0], 2e-4)


def test_driven_run_on_eight_groups_integer_deltas_inside_the_float_runs_spread():
    """the same three epochs with eight groups in flight on the 200 items -- real collisions, and a Hogwild run is no longer a function
    of its inputs.  bench.py's 2e-4 is a figure of the Yelp2018 shape; two FLOAT runs of this set differ by up to 2e-3 (measured, eight
    runs each: float 3429.7 .. 3435.6, 3359.1 .. 3364.8, 3321.5 .. 3328.1; integer 3429.8 .. 3434.6, 3357.7 .. 3364.0, 3320.6 .. 3328.2).
    So the tolerance is the float kernel's own, taken here and now: six float runs span [lo, hi] per epoch, and every one of three
    integer runs must lie in [lo - (hi - lo), hi + (hi - lo)] -- a seventh float run leaves that interval about once in a thousand
    times, a one-sided shift of two spreads always does.  Same bold-driver decisions in every run.

    The default grid of this set (157 groups, the whole epoch in flight at once) is not asserted on: there the loss follows what sits
    in front of the SGD grid more than the number format.  Measured, eight runs each, epoch means: float 2885.9 / 2791.3 / 2704.6; float
    with one streaming pass over the tables in front of its grid, as convert-in is in front of the integer one, 2853.4 / 2771.2 / 2665.8;
    integer 2839.3 / 2763.6 / 2657.4 (each within +-10 of its mean): 1.6 % between float and integer, 1.1 % of it from the pass alone.
    At the Yelp2018 shape, 25 epochs: integer against float -1.8e-4 .. -3.5e-4 at the last epoch, float against float 7e-5
    (profiles/bpr_fixed_accum.json)."""
    data = _colliding()
    f, i = _driven_losses(data, "f32", 8, 6), _driven_losses(data, "i32", 8, 3)
    assert (f[:, :, 1] == f[0, :, 1]).all() and (i[:, :, 1] == f[0, :, 1]).all()
    for k in range(3):
        lo, hi = f[:, k, 0].min(), f[:, k, 0].max()
        print(f"8 groups, epoch {k + 1}: float {lo:.3f} .. {hi:.3f}, integer {i[:, k, 0].min():.3f} .. {i[:, k, 0].max():.3f}")
        outside = max(lo - i[:, k, 0].min(), i[:, k, 0].max() - hi, 0.0)
        check(f"driven run on eight groups, epoch {k + 1}: integer runs' distance from the float runs' span, in spans", outside / (hi - lo), 1.0,
              inclusive=True, kind="statistical")


def test_driven_run_on_the_default_grid_takes_the_same_decisions():
    """the default grid of the same set (see above for its losses): three epochs, the same learning rate epoch by epoch, finite tables"""
    data = _colliding()
    tf, sf = _driven(*data, "f32")
    ti, si = _driven(*data, "i32")
    lf, li = sf.driver_log(), si.driver_log()
    assert lf.shape[0] == li.shape[0] == 3 and not si.driver_state()["failed"]
    assert np.array_equal(lf[:, 1], li[:, 1]) and sf.driver_state()["lr"] == si.driver_state()["lr"]
    assert np.isfinite(ti.P.numpy()).all() and np.isfinite(ti.Q.numpy()).all()


def test_auto_takes_integer_deltas_only_where_they_pay(monkeypatch):
    """``BprSgd.fixed_accum``: a device-driven, single-GPU, item-major, atomic-delta, fp32 epoch; under ``auto`` at least 8 triplets per
    table row and more than one group (asked for, or left by the launcher's clamp to the number of chunks); QREC_BPR_ACCUM and the
    object's own ``accum`` override ``auto`` but never the first list"""
    monkeypatch.delenv("QREC_BPR_ACCUM", raising=False)
    rng = np.random.default_rng(2)

    def make(n, U=20, I=20, dtype=np.float32, schedule="item", p_update="atomic", driver=True):
        t = DeviceTables(rng.random((U, 8)) / 3, rng.random((I, 8)) / 3, dtype)
        s = BprSgd(t, rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32), schedule=schedule, p_update=p_update)
        if driver:
            s.start_device_driver(LR, 4)
        return s

    assert make(320).fixed_accum() and not make(319).fixed_accum()                       # 8 x (20 + 20) rows
    assert not make(320).fixed_accum(groups=1) and make(320).fixed_accum(groups=2)
    assert not make(32, U=2, I=2).fixed_accum(chunk=32) and make(33, U=2, I=2).fixed_accum(chunk=32)      # one chunk = one group
    for kw in (dict(driver=False), dict(schedule="user"), dict(p_update="rmw"), dict(dtype=np.float64)):
        s = make(320, **kw)
        assert not s.fixed_accum(), kw
        s.accum = "i32"
        assert not s.fixed_accum(), kw
    monkeypatch.setenv("QREC_BPR_ACCUM", "f32")
    assert not make(320).fixed_accum()
    monkeypatch.setenv("QREC_BPR_ACCUM", "i32")
    s = make(10)
    assert s.fixed_accum(groups=1)
    s.accum = "f32"
    assert not s.fixed_accum()
    s.accum = "auto"
    assert not s.fixed_accum() and make(320).fixed_accum()
