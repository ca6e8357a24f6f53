"""The throughput BPR kernels (csrc/bpr_sgd.hip: bpr_hogwild_item_kernel, bpr_hogwild_kernel) on MANY groups, held to the oracle at 1e-5.

A Hogwild epoch on real data has no single right answer, so the full-grid tests of test_gpu_bpr.py can only bound it to a few percent.
On a conflict-free input (tests/conflict_free.py: no two chunks of the launched order share a row of P or Q) it has one: the sequential
recurrence over the stored order, on any grid, under any update policy.  Everything that exists only because there are many groups -- the
slot -> chunk map, the persistent loop and its clamps, the per-group LDS index tiles and row reductions of groups that share a wavefront,
every template instantiation, the load + store policies and the 64-bit addressing flavour -- is compared here with ``O.bpr_sgd`` in fp64 at
the north-star tolerance, and with the same kernel run by ONE group bit for bit."""
import numpy as np
import pytest

from oracle import c as O
from qrec_amd import capi
from qrec_amd.capi import DeviceBuffer as DB
from qrec_amd.engine import BprSgd, DeviceTables, padded_ld

from conflict_free import chunks_are_row_disjoint, conflict_free_triplets
from helpers import check, rel_err

pytestmark = pytest.mark.gpu

F32_TOL = 1e-5     # north_star: "within 1e-5 relative on fp32 embeddings/loss"
LR, REG_U, REG_I = 0.05, 0.01, 0.02
UNUSED = 3         # rows at the end of both tables that no triplet names
BIG = 10 ** 9      # more groups than the launchers allow: clamped to max_groups

ITEM_POLICY = {capi.HW_DEFAULT: "atomic", capi.HW_P_RMW: "p_rmw", capi.HW_PQ_RMW: "pq_rmw"}
USER_POLICY = {capi.HW_DEFAULT: "atomic", capi.HW_SC1_ATOMIC: "sc1_atomic", capi.HW_PLAIN_RMW: "plain_rmw", capi.HW_SC1_RMW: "sc1_rmw"}


@pytest.fixture(scope="module", autouse=True)
def _device():
    capi.init(0)
    info = capi.device_info()
    assert info["arch"].startswith("gfx950"), info
    yield


def _grid_limits(dim):
    """(default_groups, max_groups) of the launchers for this row width (launch_hogwild / launch_hogwild_item: 256 blocks of 4 wavefronts
    of GPW groups, at most 8 times that)"""
    gpw = {32: 4, 64: 4, 128: 2, 256: 1}[padded_ld(dim, np.float32)]
    return 256 * 4 * gpw, 256 * 8 * 4 * gpw


def _n_chunks_for(groups, dim):
    default, most = _grid_limits(dim)
    if groups == 0:
        return 3 * default + 1001          # default grid: groups of ONE wavefront run 3 and 4 rounds
    if groups == BIG:
        return most + most // 2 + 3        # the clamp to max_groups, then a second round for half of the groups
    return groups * 6 + 5                  # a grid that ends inside a wavefront, 6 and 7 rounds


def _rows_per_block(block):
    """(users, items) a block owns: few enough that rows repeat all the time inside a block"""
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
    lref = O.bpr_sgd(Pr, Qr, np.ascontiguousarray(us), np.ascontiguousarray(is_), np.ascontiguousarray(js), LR, REG_U, REG_I)
    return Pr, Qr, lref


def _hold_to_oracle(what, t, sgd, dim, P0, Q0, Pr, Qr, lref):
    """the tables and the loss after a launch against the fp64 recurrence; pad columns zero; rows of no block untouched"""
    Pg, Qg = t.download()
    check(f"{what}: P vs the sequential recurrence", rel_err(Pg, Pr), F32_TOL)
    check(f"{what}: Q vs the sequential recurrence", rel_err(Qg, Qr), F32_TOL)
    check(f"{what}: loss", abs(sgd.loss() - lref) / lref, F32_TOL)
    Pf, Qf = t.P.numpy(), t.Q.numpy()
    assert (Pf[:, dim:] == 0).all() and (Qf[:, dim:] == 0).all()
    assert np.array_equal(Pf[-UNUSED:, :dim], P0[-UNUSED:]) and np.array_equal(Qf[-UNUSED:, :dim], Q0[-UNUSED:])
    return Pf, Qf


def _stored(sgd):
    return sgd.d_u.numpy()[:sgd.n], sgd.d_i.numpy()[:sgd.n], sgd.d_j.numpy()[:sgd.n]


# ---------------------------------------------------------------------------------------------
# item-major kernel
# ---------------------------------------------------------------------------------------------
def _launch_item(t, sgd, dim, chunk, groups, flush, variant):
    sgd.d_stats.fill_bytes(0)
    capi.bpr_sgd_hogwild_item_major(t.P, t.Q, dim, t.ld, sgd.d_u, sgd.d_i, sgd.d_j, sgd.n, chunk, groups, flush, LR, REG_U, REG_I, sgd.d_stats,
                                    variant=variant)


def _item_case(dim, variant, ptr64, cfg, groups, tail, companion):
    g = {0: "default_grid", BIG: "max_groups"}.get(groups, f"{groups}_groups")
    name = f"d{dim}-{ITEM_POLICY[variant]}-{'ptr64' if ptr64 else 'desc'}-chunk{cfg[0]}_flush{cfg[1]}_run{cfg[2]}-{g}-tail{tail}"
    return pytest.param(dim, variant, ptr64, cfg, groups, tail, companion, id=name)


# (chunk, flush_every, item_run): the shipped default; whole item runs; odd sizes with flushes inside the runs; short runs; a flush per triplet
DEFAULT_CFG, WHOLE, ODD, SHORT, EVERY = (32, 16, 16), (64, 64, 0), (7, 3, 7), (32, 8, 8), (8, 1, 8)

ITEM_CASES = [
    # d = 64 and 50: <16, 4>, four groups per wavefront
    _item_case(64, capi.HW_DEFAULT, False, DEFAULT_CFG, 0, 5, True),
    _item_case(64, capi.HW_P_RMW, False, EVERY, BIG, 3, False),
    _item_case(64, capi.HW_PQ_RMW, True, WHOLE, 37, 0, False),
    _item_case(64, capi.HW_DEFAULT, True, ODD, BIG, 2, True),
    _item_case(64, capi.HW_DEFAULT, False, SHORT, 37, 0, True),
    _item_case(50, capi.HW_P_RMW, True, DEFAULT_CFG, 0, 9, False),
    _item_case(50, capi.HW_DEFAULT, False, WHOLE, 37, 7, True),
    # d = 8: <16, 2>
    _item_case(8, capi.HW_DEFAULT, False, EVERY, BIG, 3, True),
    _item_case(8, capi.HW_PQ_RMW, False, DEFAULT_CFG, 0, 0, False),
    _item_case(8, capi.HW_P_RMW, True, ODD, 37, 2, False),
    _item_case(8, capi.HW_DEFAULT, True, WHOLE, 37, 11, False),
    # d = 128: <32, 4>, two groups per wavefront
    _item_case(128, capi.HW_DEFAULT, False, DEFAULT_CFG, 0, 5, True),
    _item_case(128, capi.HW_PQ_RMW, False, ODD, BIG, 3, False),
    _item_case(128, capi.HW_P_RMW, True, SHORT, 37, 0, False),
    _item_case(128, capi.HW_DEFAULT, True, WHOLE, 0, 11, True),      # whole item runs: the short tail chunk is visited mid-epoch
    # d = 200: <64, 4>, one group per wavefront
    _item_case(200, capi.HW_DEFAULT, False, DEFAULT_CFG, 0, 5, True),
    _item_case(200, capi.HW_P_RMW, False, EVERY, BIG, 3, False),
    _item_case(200, capi.HW_PQ_RMW, True, WHOLE, 0, 7, False),
    _item_case(200, capi.HW_DEFAULT, True, ODD, 37, 3, True),
]


@pytest.mark.parametrize("dim,variant,ptr64,cfg,groups,tail,companion", ITEM_CASES)
def test_item_major_full_grid_on_conflict_free_input_is_the_sequential_recurrence(dim, variant, ptr64, cfg, groups, tail, companion, monkeypatch):
    """No two chunks of the stored order share a row (asserted on the order read back from the device), so the launch must give the
    oracle's recurrence over that order to fp32 rounding -- with atomic deltas and with the lossy load + store policies alike, since
    nothing collides.

    Bit-level companion (atomic policy): every row receives its deltas from one wavefront, in program order, and a chunk is walked front
    to back on any grid, so the tables after the full-grid launch equal the tables after a ONE-group launch of the same order bit for bit
    (the loss does not: its fp64 atomic adds arrive in another order)."""
    chunk, flush, item_run = cfg
    block = item_run if item_run > 0 else chunk
    n_chunks = _n_chunks_for(groups, dim)
    u, i, j, P0, Q0 = _problem(dim * 1000 + chunk + tail, dim, n_chunks * (chunk // block), block, tail)
    assert -(-u.size // chunk) == n_chunks
    if ptr64:
        monkeypatch.setenv("QREC_FORCE_64BIT_ADDRESSING", "1")
    t = DeviceTables(P0, Q0, np.float32)
    sgd = BprSgd(t, u, i, schedule="item", item_run=item_run); sgd.set_negatives(j)
    us, is_, js = _stored(sgd)
    assert np.array_equal(us, u[sgd.perm]) and np.array_equal(is_, i[sgd.perm]) and np.array_equal(js, j[sgd.perm])
    assert chunks_are_row_disjoint(us, is_, js, chunk)
    Pr, Qr, lref = _oracle(P0, Q0, us, is_, js)
    _launch_item(t, sgd, dim, chunk, groups, flush, variant)
    Pf, Qf = _hold_to_oracle("item-major, full grid, conflict-free", t, sgd, dim, P0, Q0, Pr, Qr, lref)
    if companion:
        assert variant == capi.HW_DEFAULT
        t.upload(P0, Q0)
        _launch_item(t, sgd, dim, chunk, 1, flush, variant)
        _hold_to_oracle("item-major, one group, conflict-free", t, sgd, dim, P0, Q0, Pr, Qr, lref)
        assert np.array_equal(Pf.view(np.uint32), t.P.numpy().view(np.uint32)), "P: full grid and one group differ in some bit"
        assert np.array_equal(Qf.view(np.uint32), t.Q.numpy().view(np.uint32)), "Q: full grid and one group differ in some bit"


@pytest.mark.parametrize("p_update,n_blocks,tail", [("atomic", 41_000, 3), ("rmw", 41_000, 0), ("atomic", 12_001, 5)])
def test_item_major_epoch_as_the_benchmark_launches_it_is_the_sequential_recurrence(p_update, n_blocks, tail):
    """through the object, with ``launch_grid()``'s (chunk, groups) as bench.py passes them: ``grid_for_epoch`` may halve the chunk down to
    8 (and cap the groups on a short epoch), so the blocks are 8 triplets -- a halved chunk is still a union of whole blocks"""
    dim = 64
    u, i, j, P0, Q0 = _problem(n_blocks + tail, dim, n_blocks, 8, tail)
    t = DeviceTables(P0, Q0, np.float32)
    sgd = BprSgd(t, u, i, schedule="item", item_run=8, p_update=p_update); sgd.set_negatives(j)
    assert sgd.p_update == p_update and sgd.item_variant == (capi.HW_P_RMW if p_update == "rmw" else capi.HW_DEFAULT)
    chunk, groups = sgd.launch_grid()
    assert chunk % 8 == 0 and (groups == 0) == (n_blocks > 40_000)       # the long epoch takes the default grid, the short one a capped grid
    us, is_, js = _stored(sgd)
    assert chunks_are_row_disjoint(us, is_, js, chunk)
    Pr, Qr, lref = _oracle(P0, Q0, us, is_, js)
    sgd.epoch_throughput_async(LR, REG_U, REG_I, chunk=chunk, groups=groups)
    _hold_to_oracle(f"item-major, launch_grid() = ({chunk}, {groups}), P[u] by {p_update}", t, sgd, dim, P0, Q0, Pr, Qr, lref)


@pytest.mark.parametrize("dim", [64, 128, 200, 8])
@pytest.mark.parametrize("n_chunks,n", [(1, None), (3, None), (1, 1), (0, 0)])
def test_item_major_degenerate_launches(dim, n_chunks, n):
    """fewer groups than one wavefront holds (one chunk, three chunks), a single triplet, and no triplet at all (the call returns without
    touching the tables or the statistics) -- on the default grid, which the launcher clamps to the number of chunks"""
    chunk, flush, item_run = DEFAULT_CFG
    u, i, j, P0, Q0 = _problem(dim + 7 * n_chunks, dim, max(1, n_chunks) * 2, item_run, 5 if n_chunks == 3 else 1 if n == 1 else 0)
    if n is not None:
        u, i, j = u[:n], i[:n], j[:n]
    t = DeviceTables(P0, Q0, np.float32)
    if u.size == 0:
        stats = DB.from_numpy(np.full(capi.STATS_WORDS, 7.5)); idx = DB.zeros(1, np.int32)
        capi.bpr_sgd_hogwild_item_major(t.P, t.Q, dim, t.ld, idx, idx, idx, 0, chunk, 0, flush, LR, REG_U, REG_I, stats)
        assert np.array_equal(t.P.numpy()[:, :dim], P0) and np.array_equal(t.Q.numpy()[:, :dim], Q0) and (stats.numpy() == 7.5).all()
        return
    sgd = BprSgd(t, u, i, schedule="item", item_run=item_run); sgd.set_negatives(j)
    us, is_, js = _stored(sgd)
    assert -(-us.size // chunk) == n_chunks and chunks_are_row_disjoint(us, is_, js, chunk)
    Pr, Qr, lref = _oracle(P0, Q0, us, is_, js)
    for variant in ITEM_POLICY:
        t.upload(P0, Q0)
        _launch_item(t, sgd, dim, chunk, 0, flush, variant)
        _hold_to_oracle(f"item-major, {n_chunks} chunk(s), {us.size} triplets, {ITEM_POLICY[variant]}", t, sgd, dim, P0, Q0, Pr, Qr, lref)


# ---------------------------------------------------------------------------------------------
# user-major kernel
# ---------------------------------------------------------------------------------------------
def _launch_user(t, sgd, dim, chunk, groups, variant):
    sgd.d_stats.fill_bytes(0)
    capi.bpr_sgd_hogwild(t.P, t.Q, dim, t.ld, sgd.d_u, sgd.d_i, sgd.d_j, sgd.n, chunk, groups, LR, REG_U, REG_I, sgd.d_stats, variant)


def _user_case(dim, variant, ptr64, chunk, groups, tail, companion):
    g = {0: "default_grid", BIG: "max_groups"}.get(groups, f"{groups}_groups")
    return pytest.param(dim, variant, ptr64, chunk, groups, tail, companion,
                        id=f"d{dim}-{USER_POLICY[variant]}-{'ptr64' if ptr64 else 'desc'}-chunk{chunk}-{g}-tail{tail}")


USER_CASES = [
    _user_case(64, capi.HW_DEFAULT, False, 8, 0, 5, True),
    _user_case(64, capi.HW_SC1_ATOMIC, True, 7, BIG, 3, False),
    _user_case(64, capi.HW_PLAIN_RMW, False, 64, 37, 0, False),
    _user_case(64, capi.HW_SC1_RMW, False, 1, BIG, 0, False),
    _user_case(50, capi.HW_SC1_RMW, True, 64, 37, 9, False),
    _user_case(50, capi.HW_DEFAULT, True, 8, BIG, 0, True),
    _user_case(8, capi.HW_DEFAULT, False, 8, BIG, 3, True),
    _user_case(8, capi.HW_PLAIN_RMW, True, 64, 37, 0, False),
    _user_case(8, capi.HW_SC1_ATOMIC, False, 7, 0, 2, False),
    _user_case(8, capi.HW_DEFAULT, False, 1, 0, 0, False),
    _user_case(128, capi.HW_DEFAULT, False, 64, 0, 5, True),
    _user_case(128, capi.HW_SC1_RMW, False, 7, BIG, 3, False),
    _user_case(128, capi.HW_PLAIN_RMW, True, 8, 37, 0, False),
    _user_case(128, capi.HW_SC1_ATOMIC, True, 1, 0, 0, False),
    _user_case(200, capi.HW_DEFAULT, False, 64, 0, 5, True),
    _user_case(200, capi.HW_PLAIN_RMW, False, 8, BIG, 3, False),
    _user_case(200, capi.HW_SC1_RMW, True, 7, 37, 4, False),
    _user_case(200, capi.HW_DEFAULT, True, 1, BIG, 0, True),
    _user_case(200, capi.HW_SC1_ATOMIC, False, 64, 37, 0, False),
]


@pytest.mark.parametrize("dim,variant,ptr64,chunk,groups,tail,companion", USER_CASES)
def test_user_major_full_grid_on_conflict_free_input_is_the_sequential_recurrence(dim, variant, ptr64, chunk, groups, tail, companion, monkeypatch):
    """test_gpu_bpr.py's conflict-free test (d = 64, atomic deltas, chunk 8, private items used once) on every instantiation, policy,
    addressing flavour and grid, with rows that repeat inside a block: a block is a chunk of the user-major order, which is stored as
    given.  Same reference, same bound, same bit-level companion against ONE group as the item-major test above."""
    n_chunks = _n_chunks_for(groups, dim)
    u, i, j, P0, Q0 = _problem(dim * 1000 + chunk + tail + 1, dim, n_chunks, chunk, tail)
    assert -(-u.size // chunk) == n_chunks
    if ptr64:
        monkeypatch.setenv("QREC_FORCE_64BIT_ADDRESSING", "1")
    t = DeviceTables(P0, Q0, np.float32)
    sgd = BprSgd(t, u, i); sgd.set_negatives(j)
    us, is_, js = _stored(sgd)
    assert np.array_equal(us, u) and np.array_equal(is_, i) and np.array_equal(js, j)
    assert chunks_are_row_disjoint(us, is_, js, chunk)
    Pr, Qr, lref = _oracle(P0, Q0, us, is_, js)
    _launch_user(t, sgd, dim, chunk, groups, variant)
    Pf, Qf = _hold_to_oracle("user-major, full grid, conflict-free", t, sgd, dim, P0, Q0, Pr, Qr, lref)
    if companion:
        assert variant == capi.HW_DEFAULT
        t.upload(P0, Q0)
        _launch_user(t, sgd, dim, chunk, 1, variant)
        _hold_to_oracle("user-major, one group, conflict-free", t, sgd, dim, P0, Q0, Pr, Qr, lref)
        assert np.array_equal(Pf.view(np.uint32), t.P.numpy().view(np.uint32)), "P: full grid and one group differ in some bit"
        assert np.array_equal(Qf.view(np.uint32), t.Q.numpy().view(np.uint32)), "Q: full grid and one group differ in some bit"


@pytest.mark.parametrize("dim", [64, 128, 200, 8])
@pytest.mark.parametrize("n_chunks,n", [(1, None), (3, None), (1, 1), (0, 0)])
def test_user_major_degenerate_launches(dim, n_chunks, n):
    chunk = 32
    u, i, j, P0, Q0 = _problem(dim + 11 * n_chunks, dim, max(1, n_chunks), chunk, 5 if n_chunks == 3 else 1 if n == 1 else 0)
    if n is not None:
        u, i, j = u[:n], i[:n], j[:n]
    t = DeviceTables(P0, Q0, np.float32)
    if u.size == 0:
        stats = DB.from_numpy(np.full(capi.STATS_WORDS, 7.5)); idx = DB.zeros(1, np.int32)
        capi.bpr_sgd_hogwild(t.P, t.Q, dim, t.ld, idx, idx, idx, 0, chunk, 0, LR, REG_U, REG_I, stats)
        assert np.array_equal(t.P.numpy()[:, :dim], P0) and np.array_equal(t.Q.numpy()[:, :dim], Q0) and (stats.numpy() == 7.5).all()
        return
    sgd = BprSgd(t, u, i); sgd.set_negatives(j)
    us, is_, js = _stored(sgd)
    assert -(-us.size // chunk) == n_chunks and chunks_are_row_disjoint(us, is_, js, chunk)
    Pr, Qr, lref = _oracle(P0, Q0, us, is_, js)
    for variant in USER_POLICY:
        t.upload(P0, Q0)
        _launch_user(t, sgd, dim, chunk, 0, variant)
        _hold_to_oracle(f"user-major, {n_chunks} chunk(s), {us.size} triplets, {USER_POLICY[variant]}", t, sgd, dim, P0, Q0, Pr, Qr, lref)
