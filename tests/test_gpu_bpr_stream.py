"""The per-triplet instruction stream of the BPR throughput kernels (qrec_amd/csrc/bpr_sgd.hip): the loss in its one-evaluation form
where one wavefront holds scores of both signs, and the integer flavour's range flag, kept as a running maximum of magnitude bits, at
the edge of the range -- in register 0 and register 3 of a lane, in group 0 and in a later group of a wavefront."""
from math import gcd

import numpy as np
import pytest

from oracle import c as O
from qrec_amd import capi
from qrec_amd.engine import BprSgd, DeviceTables

import fixed_codec as FX
from helpers import check

pytestmark = pytest.mark.gpu

DIM = 64
GPW = 4                      # groups of 16 lanes per wavefront at d = 64


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    info = capi.device_info()
    assert info["arch"].startswith("gfx950"), info
    yield


def _item_major_chunk_of_slot(n_chunks):
    """launch_hogwild_item: time slot s (= the group's id in the first round) runs chunk (s * stride) mod n_chunks"""
    stride = max(1, int(n_chunks * 0.6180339887498949))
    while gcd(stride, n_chunks) != 1:
        stride += 1
    return [(s * stride) % n_chunks for s in range(n_chunks)]


# ---------------------------------------------------------------------------------------------------------------------------------
# loss at both signs inside one wavefront
# ---------------------------------------------------------------------------------------------------------------------------------
MIXED = [-120.0, 20.0, -1e-3, 0.0, 1e-3, -20.0, 120.0]      # consecutive slots alternate in sign
POSITIVE_TAIL = [20.0, 120.0]                                 # the expected sum is 8e-9: held at absolute 1e-6


def _scores_problem(seq, copies, chunk_of_slot):
    """one-triplet chunks, every triplet on rows of its own: slot s holds x = P[u].(Q[i] - Q[j]) = seq[s mod len], spread evenly over the
    64 columns (P = 0.5 everywhere, Q[i] - Q[j] = x / 32 everywhere).  Every table value is put on the integer flavour's 2^-26 grid first,
    so that the float kernels, the integer kernel and the fp64 oracle read the same numbers (the scores are then the nominal ones to
    within 1e-3 relative; `x` returns what they are).  Positive items ascend with the position, so that the item-major stored order is
    the given order."""
    n = len(seq) * copies
    x_of_chunk = np.zeros(n)
    for s in range(n):
        x_of_chunk[chunk_of_slot[s]] = seq[s % len(seq)]
    P0 = np.full((n, DIM), 0.5, np.float32)
    Q0 = np.zeros((2 * n, DIM), np.float32)
    Q0[0::2] = (x_of_chunk / 64)[:, None]
    Q0[1::2] = -(x_of_chunk / 64)[:, None]
    P0, Q0 = FX.round_trip(P0), FX.round_trip(Q0)
    u = np.arange(n, dtype=np.int32); i = (2 * u).astype(np.int32); j = (2 * u + 1).astype(np.int32)
    x = (P0.astype(np.float64) * (Q0[i].astype(np.float64) - Q0[j].astype(np.float64))).sum(1)
    return u, i, j, P0, Q0, x


def _hold_loss(what, got, want):
    if want < 1.0:
        check(f"{what}: |loss - oracle| (expected sum below 1)", abs(got - want), 1e-6)
    else:
        check(f"{what}: loss vs the fp64 oracle, relative", abs(got - want) / want, 1e-6)


@pytest.mark.parametrize("groups", [1, 0], ids=["one_group", "default_grid"])
@pytest.mark.parametrize("seq", [MIXED, POSITIVE_TAIL], ids=["mixed_signs", "positive_tail"])
@pytest.mark.parametrize("kernel", ["item_f32", "item_i32", "user_f32"])
def test_loss_with_both_signs_inside_one_wavefront(kernel, seq, groups):
    """lr = 0, chunk = 1: the launch is a sum of -log sigmoid(x) over scores of which the four groups of a wavefront hold different
    signs -- the case in which a two-armed softplus runs both arms.  Sums against O.bpr_sgd in fp64."""
    n = len(seq) * 4
    item = kernel.startswith("item")
    chunk_of_slot = _item_major_chunk_of_slot(n) if item else list(range(n))
    u, i, j, P0, Q0, x = _scores_problem(seq, 4, chunk_of_slot)
    if seq is MIXED:
        assert np.allclose(x[chunk_of_slot[:7]], MIXED, rtol=1e-3, atol=0)
        for w in range(n // GPW):           # every wavefront of the default grid holds both signs
            xs = x[chunk_of_slot[GPW * w:GPW * w + GPW]]
            assert (xs > 0).any() and (xs < 0).any(), (w, xs)
    Pr, Qr = P0.astype(np.float64), Q0.astype(np.float64)
    want = O.bpr_sgd(Pr, Qr, u, i, j, 0.0, 0.0, 0.0)
    t = DeviceTables(P0, Q0, np.float32)
    sgd = BprSgd(t, u, i, schedule="item" if item else "user"); sgd.set_negatives(j)
    assert np.array_equal(sgd.d_u.numpy()[:n], u) and np.array_equal(sgd.d_i.numpy()[:n], i)         # the stored order is the given one
    if kernel == "item_i32":
        sgd.accum = "i32"
        sgd.start_device_driver(0.0, log_capacity=2)
        assert sgd.fixed_accum(groups, 1)
        sgd.epoch_device_async(0.0, 0.0, 1.0, tol=0.0, chunk=1, groups=groups)
        st = sgd.driver_state()
        assert not st["failed"] and st["epochs"] == 1
        got = float(sgd.driver_log()[0, 2])
    else:
        sgd.d_stats.fill_bytes(0)
        if item:
            capi.bpr_sgd_hogwild_item_major(t.P, t.Q, DIM, t.ld, sgd.d_u, sgd.d_i, sgd.d_j, n, 1, groups, 16, 0.0, 0.0, 0.0, sgd.d_stats)
        else:
            capi.bpr_sgd_hogwild(t.P, t.Q, DIM, t.ld, sgd.d_u, sgd.d_i, sgd.d_j, n, 1, groups, 0.0, 0.0, 0.0, sgd.d_stats)
        got = float(sgd.loss())
    print(f"{kernel} {'mixed' if seq is MIXED else 'positive'} groups={groups}: loss {got!r} oracle {want!r}")
    _hold_loss(f"{kernel}, {groups} groups", got, want)
    P1, Q1 = t.P.numpy(), t.Q.numpy()
    assert np.array_equal(P1, P0) and np.array_equal(Q1, Q0)          # lr = 0 on grid values: nothing moves


# ---------------------------------------------------------------------------------------------------------------------------------
# the range flag at its edge
# ---------------------------------------------------------------------------------------------------------------------------------
BELOW = float(np.nextafter(np.float32(16), np.float32(0)))          # 16 - 2^-20
N_TRIPLETS = 7


def _edge_problem(target, col, last, side):
    """3 users x 4 items.  One triplet (u0, a, b) on rows of its own, every value of those rows zero except columns `col` and `col2` (the same
    lane's next register), chosen so that both dot products cancel exactly: x = 0, sigmoid = 1/2, the step gsc = lr / 2 without
    rounding, and with the step below ONE element of the new P[u] (`target` "P"), of the new Q[j] ("Qj") or of the running Q[i] ("Qi")
    goes from 15 to exactly 16 while every other element stays below 10.  The six other triplets use the other two users and items.
    `last`: the triplet's positive item is the largest, so it is stored last and runs in a later group of its wavefront."""
    rng = np.random.default_rng(11)
    P0 = (rng.random((3, DIM), dtype=np.float32) / 3).astype(np.float32)
    Q0 = (rng.random((4, DIM), dtype=np.float32) / 3).astype(np.float32)
    col2 = (col + 16) % DIM
    a, b, others = (3, 2, (0, 1)) if last else (0, 1, (2, 3))
    pu, qi, qj = (np.zeros(DIM, np.float32) for _ in range(3))
    if target == "P":        # p1 = 15 + (lr/2) * 16, lr = 1/8; Q[i], Q[j] move by gsc * p1 = 1
        pu[col], qi[col], qj[col] = 15.0, 8.0, -8.0
        pu[col2], qi[col2], qj[col2] = 15.0, -8.0, 8.0
        lr = 1.0 / 8
    elif target == "Qj":     # p1 = -6 + (1/8)(-16) = -8, b = 15 - (1/8)(-8) = 16, lr = 1/4
        pu[col], qi[col], qj[col] = -6.0, -1.0, 15.0
        pu[col2], qi[col2], qj[col2] = 6.0, -8.0, 8.0
        lr = 1.0 / 4
    else:                    # p1 = 6 + (1/8)(16) = 8, a = 15 + (1/8)(8) = 16, lr = 1/4
        pu[col], qi[col], qj[col] = 6.0, 15.0, -1.0
        pu[col2], qi[col2], qj[col2] = 6.0, -8.0, 8.0
        lr = 1.0 / 4
    P0[0], Q0[a], Q0[b] = side * pu, side * qi, side * qj
    u = np.array([0] + [1, 2] * 3, np.int32)
    i = np.array([a] + [others[0]] * 3 + [others[1]] * 3, np.int32)
    j = np.array([b] + [others[1]] * 3 + [others[0]] * 3, np.int32)
    where = {"P": ("P", 0), "Qj": ("Q", b), "Qi": ("Q", a)}[target]
    return u, i, j, P0, Q0, lr, where


@pytest.mark.parametrize("last", [False, True], ids=["group0", "later_group"])
@pytest.mark.parametrize("col", [0, 53], ids=["col0", "lane5_reg3"])
@pytest.mark.parametrize("edge", ["below", "plus16", "minus16", "overflow"])
@pytest.mark.parametrize("target", ["P", "Qj", "Qi"])
def test_range_flag_at_the_edge(target, edge, col, last):
    """A driven integer epoch in one-triplet chunks.  "below": the step is scaled by 1 - 2^-20, which lands the element on
    nextafter(16, 0) exactly (P: 15 + (1 - 2^-20); Q: 15 + (1 - 2^-20)(1 - 2^-22), which rounds there) -- no flag, one epoch counted, and
    the table holds that very value.  "plus16" / "minus16": the element is exactly +-16.0 -- FAILED, no epoch, nothing wrapped.
    "overflow": lr = 3e38.  +inf and NaN cannot be hit one at a time: every new value has the form v - c v, which is NaN for v = +-inf,
    so the nearest reachable case is the one where the step overflows, the intermediate is +-inf and the tested value NaN."""
    side = -1.0 if edge == "minus16" else 1.0
    u, i, j, P0, Q0, lr, (tab, row) = _edge_problem(target, col, last, side)
    assert max(np.abs(P0).max(), np.abs(Q0).max()) < 16
    if edge == "below":
        lr *= 1.0 - 2.0 ** -20
    elif edge == "overflow":
        lr = 3e38
    t = DeviceTables(P0, Q0, np.float32)
    sgd = BprSgd(t, u, i, schedule="item"); sgd.accum = "i32"
    # where the triplet runs: stored position -> time slot -> group of its wavefront
    pos = int(np.flatnonzero(sgd.d_u.numpy()[:N_TRIPLETS] == 0)[0])
    slot = _item_major_chunk_of_slot(N_TRIPLETS).index(pos)
    assert (slot % GPW > 0) == last and col % 16 == (0 if col == 0 else 5) and col // 16 == (0 if col == 0 else 3)
    sgd.set_negatives(j)
    sgd.start_device_driver(lr, log_capacity=4)
    assert sgd.fixed_accum(0, 1)
    sgd.epoch_device_async(0.0, 0.0, 1.0, tol=0.0, chunk=1)
    st = sgd.driver_state()
    P1, Q1 = t.P.numpy(), t.Q.numpy()
    got = float((P1 if tab == "P" else Q1)[row, col])
    print(f"{target} {edge} col {col} slot {slot}: element {got!r} failed {st['failed']} epochs {st['epochs']}")
    assert np.isfinite(P1).all() and np.isfinite(Q1).all() and max(np.abs(P1).max(), np.abs(Q1).max()) <= 32.0
    if edge == "below":
        assert not st["failed"] and st["epochs"] == 1
        assert got == BELOW
        return
    assert st["failed"] and st["epochs"] == 0 and sgd.d_drv.numpy()[capi.DRV_FAILED] == 1.0
    if edge != "overflow":
        assert abs(got) >= 16.0 and np.sign(got) == side and max(np.abs(P1).max(), np.abs(Q1).max()) < 32.0
        for X0, X1 in ((P0, P1), (Q0, Q1)):                               # an element that wrapped would have changed sides
            big = np.abs(X0) > 1.0
            assert np.array_equal(np.sign(X1[:, :DIM][big]), np.sign(X0[big]))
    sgd.set_negatives(j); sgd.epoch_device_async(0.0, 0.0, 1.0, tol=0.0, chunk=1)      # the epochs behind it are no-ops
    assert sgd.driver_state()["epochs"] == 0
    assert np.array_equal(t.P.numpy(), P1) and np.array_equal(t.Q.numpy(), Q1)
