"""Device-side state and epoch drivers of the embedding-training hot path.

``DeviceTables`` keeps the user/item embedding tables resident in HBM for the whole
training run (row-major, row stride ``ld`` padded so one row is a whole number of 64-byte
segments); ``BprSgd`` / ``MfSgd`` run one epoch per call through the C ABI
(include/qrec_hip.h).  Nothing here computes on the host: a missing or failing
libqrec_hip.so raises.
"""
from __future__ import annotations

import os

import numpy as np

from . import capi
from .capi import DeviceBuffer
from .interactions import CSR


def padded_ld(d: int, dtype) -> int:
    """Row stride in elements.  fp32 tables use 32/64/128/256 so that the throughput kernel
    can map a row onto 16/32/64 lanes; fp64 tables (order-exact kernels only) 16/32/64/128 so that the scheduled kernel
    can put a row on the 16 lanes of one DPP row with 16-byte accesses (four triplets per wavefront, bpr_exact.hip);
    wider fp64 rows stay unpadded (one triplet per wavefront).  Pad columns are zero and stay zero under every update."""
    if np.dtype(dtype) == np.float64:
        for ld in (16, 32, 64, 128):
            if d <= ld:
                return ld
        return d
    for ld in (32, 64, 128, 256):
        if d <= ld:
            return ld
    raise ValueError(f"embedding size {d} > 256 is not supported by the fp32 kernels")


class DeviceTables:
    def __init__(self, P: np.ndarray, Q: np.ndarray, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self.code = capi.F64 if self.dtype == np.float64 else capi.F32
        self.n_users, self.d = P.shape
        self.n_items = Q.shape[0]
        assert Q.shape[1] == self.d
        self.ld = padded_ld(self.d, self.dtype)
        self.P = DeviceBuffer.from_numpy(self._pad(P))
        self.Q = DeviceBuffer.from_numpy(self._pad(Q))

    def _pad(self, a: np.ndarray) -> np.ndarray:
        out = np.zeros((a.shape[0], self.ld), dtype=self.dtype)
        out[:, :self.d] = a
        return out

    def upload(self, P: np.ndarray, Q: np.ndarray):
        self.P.upload(self._pad(P)); self.Q.upload(self._pad(Q))

    def download(self, dtype=np.float64):
        """(P, Q) as host arrays [rows, d] (pad columns dropped)."""
        return (np.ascontiguousarray(self.P.numpy()[:, :self.d], dtype=dtype),
                np.ascontiguousarray(self.Q.numpy()[:, :self.d], dtype=dtype))

    def sumsq(self, scratch: DeviceBuffer, stream=None):
        """(sum P*P, sum Q*Q) -- model/ranking/BPR.py:40."""
        capi.sumsq(self.P, self.code, self.n_users, self.d, self.ld, scratch, stream)
        p = float(scratch.numpy(stream)[0])
        capi.sumsq(self.Q, self.code, self.n_items, self.d, self.ld, scratch, stream)
        return p, float(scratch.numpy(stream)[0])


def balanced_chunk(n: int, groups: int = 4096, lo: int = 26, hi: int = 40, prefer: int = 32) -> int:
    """Chunk length for the throughput kernels.  Their ``groups`` persistent groups each take ceil(n_chunks/groups)
    or one fewer chunks, and the epoch ends when the busiest group does: with 9.56 chunks per group (Yelp2018 shape at
    chunk 32) 44% of the groups idle through the last chunk.  Pick the length in [lo, hi] whose chunk count divides most
    evenly over the groups (measured: 0.607 ms at chunk 30, 0.583 at 32, 0.577 at 31 and 34)."""
    if n <= 0:
        return prefer
    best, best_cost = prefer, None
    for c in range(lo, hi + 1):
        per = -(-n // c) / groups
        if per <= 1:                       # fewer chunks than groups: nothing to balance
            cost = 0.0
        else:
            cost = -(-per // 1) / per - 1.0      # ceil(per)/per - 1 = idle share of the last round
        key = (round(cost, 4), abs(c - prefer))
        if best_cost is None or key < best_cost:
            best, best_cost = c, key
    return best


# `auto` (QREC_SCHEDULE unset): which throughput schedule an epoch runs under -- ONE-PASS always: "item" when a few items collect most
# interactions (their rows would take the per-triplet atomics of the user-major kernel), else "user" (measured 2.1 vs 1.6 G/s at the
# Zipf-0.6 Yelp2018 shape).
# (The two-pass "deferred negatives" schedule of rounds 3-5 -- one atomic row update per triplet, 0.62 of the roofline on tables that
# live in HBM -- is gone: outside the +-0.002 Recall bar at the last epoch in every setting measured at the size that figure was quoted on,
# profiles/r05_auto_regime_25m.json, r05_fresh_coefficient_25m.json.  Round 6 reaches the same 0.63 with ONE pass: resolve_p_update below.)


def resolve_schedule(n_triplets: int, item_degrees=None, requested: str = "auto"):
    """(schedule, None) for ``BprSgd`` (the second entry was the deferred schedule's sub-epoch count, rounds 3-5); ``item_degrees``: positives per item (None = unknown: treated as skewed)"""
    if requested != "auto":
        return requested, None
    if item_degrees is None:
        return "item", None
    deg = np.asarray(item_degrees)
    return ("item" if deg.size and deg.max() > 20 * max(deg.mean(), 1e-9) else "user"), None


# How P[u] is written by the item-major kernel (round 6).  "atomic": the exact per-sample delta through the L2 atomic units (two atomic
# row updates per triplet: the kernel's bound, 0.43-0.46 of the HBM roofline).  "rmw": sc1 load + sc1 write-through store (QREC_HW_P_RMW,
# include/qrec_hip.h) -- ONE atomic row update per triplet, 0.63-0.64 of the roofline; an update of the same user's row that lands between
# another group's load and store is lost.  How many are: the collision density
#     c = (groups in flight) x sum_u (n_u / n)^2         (expected number of other groups holding the same user while one does)
# Measured, paired Recall@20 against order-exact training (profiles/r06_item_rmw.json; |gap| at the reference's peak / at the last epoch):
#     c = 0.003 .. 0.008  (650 k users, 25 M triplets, d = 128)   rmw 0.0010 / 0.0002, 0.0011 / 0.0002   atomic 0.0008 / 0.0002, 0.0010 / 0.0003
#     c = 0.033           (160 k users, 6 M triplets)              rmw 0.0010 / 0.0010, 0.0018 / 0.0003   atomic 0.0001 / 0.0001, 0.0015 / 0.0005
#     c = 0.17            (Yelp2018 shape, 31.7 k users)           rmw 0.0005 / 0.0009 with a 10 % loss gap   atomic 0.0004 / 0.0000, loss gap 0.2 %
#     c ~ 0.2 .. 2        (lastfm under BPR.conf, 1.9 k users)     rmw mean gap over 16 seeds -0.019 +- 0.001   atomic +0.0000 +- 0.0008
# `auto` therefore takes "rmw" only where c <= P_RMW_MAX_COLLISION = 0.01 -- config #4's shape (10 M users: c = 0.0005), its single-GPU
# slice (0.003), never the Yelp2018 shape, never the reference's own small datasets.
P_RMW_MAX_COLLISION = 0.01
DEFAULT_GROUPS = 4096


def collision_density(user_counts, groups: int = DEFAULT_GROUPS) -> float:
    """groups x sum_u (n_u / n)^2 for the triplets-per-user counts of an epoch"""
    c = np.asarray(user_counts, dtype=np.float64)
    n = float(c.sum())
    return float(groups * np.square(c / n).sum()) if n > 0 else 0.0


def resolve_p_update(user_counts, groups: int = DEFAULT_GROUPS, requested: str = "auto") -> str:
    """"atomic" or "rmw" for the item-major kernel's P[u] updates; ``requested``: "auto" (by collision density), or one of the two"""
    if requested in ("atomic", "rmw"):
        return requested
    if requested != "auto":
        raise ValueError("p_update must be 'auto', 'atomic' or 'rmw'")
    return "rmw" if collision_density(user_counts, groups) <= P_RMW_MAX_COLLISION else "atomic"


# How the item-major kernel's atomic deltas are accumulated in a device-driven run (QREC_BPR_ACCUM).  "i32": fixed point -- the tables
# are int32 = rint(x * 2^26) between the epoch's convert-in pass and its close (QREC_HW_FIXED, include/qrec_hip.h), because the L2
# atomic units retire integer adds faster than float adds.  "f32": the float deltas.  Only where the whole epoch is the library's own
# three launches on one GPU: a device-driven run (``start_device_driver``), no ``dist``, item-major, P[u] by atomic deltas, fp32 tables;
# everything else stays float whatever is asked.  "auto" takes "i32" where it pays, by the figures of the gate measurement
# (tools/ubench/atomics4_u32.hip, profiles/bpr_fixed_accum.json): the integer adds save ~0.087 ns per triplet, the two conversion passes
# cost ~0.18 ns per table row, and the gain has to be twice the cost -- n >= FIXED_MIN_TRIPLETS_PER_ROW x (users + items) -- and never on
# ONE group (asked for, or all that is left once the launcher has clamped the groups to the number of chunks), which is the deterministic
# sequential recurrence, bit for bit the host-driven loop's, and nowhere near the atomic units' rate.
FIXED_MIN_TRIPLETS_PER_ROW = 8


def resolve_accum(requested: str | None = None) -> str:
    """"auto", "f32" or "i32" from ``requested`` or QREC_BPR_ACCUM"""
    r = requested if requested is not None else os.environ.get("QREC_BPR_ACCUM", "auto")
    if r not in ("auto", "f32", "i32"):
        raise ValueError("QREC_BPR_ACCUM must be auto, f32 or i32")
    return r


MIN_ROUNDS = 8
ITEM_RUN = 16           # item-major stored order: the item-sorted list in runs of this many triplets (BprSgd.__init__)


def grid_for_epoch(n: int, chunk: int, min_rounds: int = MIN_ROUNDS, groups: int = 4096, min_chunk: int = 8):
    """(chunk, groups) of ONE launch over a whole epoch of n triplets such that every persistent group walks at least ``min_rounds``
    chunks one after the other, whatever the epoch's size (round 5).  The kernels' launchers clamp the groups to the number of chunks:
    an epoch with fewer chunks than groups (the reference's lastfm split: 74 k triplets = 2.3 k chunks of 32) is in flight ALL AT ONCE --
    one round of the grid, where the Yelp2018 shape's 1.25 M triplets make ~9.5.  Shorter chunks first (down to ``min_chunk``), then
    fewer groups.  ``groups`` 0 in the result = the launcher's default (nothing to cap).  ``min_rounds`` <= 1: unchanged."""
    if min_rounds <= 1 or n <= 0:
        return chunk, 0
    c = chunk
    while c > min_chunk and -(-n // c) < min_rounds * groups:
        c = max(min_chunk, c // 2)
    n_chunks = -(-n // c)
    if n_chunks >= min_rounds * groups:
        return c, 0
    return c, int(max(1, n_chunks // min_rounds))


def launch_chunk(n: int, chunk: int, groups: int = 4096, lo: int = 4) -> int:
    """Chunk length for ONE launch over n triplets of an epoch that is cut into batches (several ranks: reconciliation / exchange batches).
    A batch of a few ten thousand triplets in chunks of 32 occupies a fraction of the 4,096 persistent groups for one chunk's latency
    (measured, tools/probe_strong_scaling_bound.py: 19.5 k-triplet batches at 8 ranks, 38 us each however small); shorter chunks spread
    the same triplets over the idle groups.  Never longer than the epoch's chunk; at least `lo`."""
    if n >= 2 * groups * chunk:
        return chunk
    return int(max(lo, min(chunk, -(-n // groups))))


def stride_runs(n: int, run: int) -> np.ndarray:
    """positions 0..n-1 cut into runs of ``run`` consecutive ones, the runs in golden-ratio stride order (run r of the result is
    run (r * stride) mod n_runs of the input, stride ~ 0.618 n_runs made coprime): consecutive runs of the result are far apart in
    the input.  A short tail (n mod run positions) goes last, so every run of the result starts at a multiple of ``run``."""
    import math
    n_runs = n // run
    if n_runs == 0:
        return np.arange(n, dtype=np.int64)
    stride = max(int(n_runs * 0.6180339887498949), 1)
    while math.gcd(stride, n_runs) != 1:
        stride += 1
    slots = (np.arange(n_runs, dtype=np.int64) * stride) % n_runs
    at = (slots[:, None] * run + np.arange(run, dtype=np.int64)[None, :]).ravel()
    return np.concatenate([at, np.arange(n_runs * run, n, dtype=np.int64)])


class BprSgd:
    """One BPR epoch per call over a fixed (u, i) triplet list (user-major PositiveSet
    order, model/ranking/BPR.py:31-34); negatives ``j`` come per epoch either from the
    host (exact CPython stream) or from the device Philox sampler.

    Device-side epoch statistics live in one small buffer (sum -log sigma, sum P*P, sum Q*Q, ticket) so
    that an epoch costs a single 24-byte read-back -- or none at all: with ``start_device_driver`` the
    epoch's loss, the convergence test and the bold-driver learning-rate update (BPR.py:40,
    base/iterativeRecommender.py:56-63,88-104) run on the device and epochs are enqueued back to back.  The Philox sampler for
    epoch k+1 runs on a side stream underneath the SGD kernel of epoch k (double-buffered
    negatives); the SGD kernel is bound by the L2 atomic units, the sampler by integer ALU,
    so they overlap almost perfectly."""

    def __init__(self, tables: DeviceTables, u: np.ndarray, i: np.ndarray, pos: CSR | None = None,
                 schedule: str = "user", n_items: int | None = None, batches: int = 1, chunk: int = 32,
                 item_run: int | None = None, p_update: str = "atomic"):
        """``schedule``: "user" keeps the reference's user-major order (required by the order-exact
        kernel); "item" stores the same triplets sorted by positive item for the item-major
        throughput kernel (``self.perm`` maps scheduled position -> reference position).
        ``batches`` > 1 (row-sharded item table, qrec_amd/dist.py): the epoch is trained in that many launches, over
        the triplet ranges ``self.batch_bounds``.  User-major: consecutive ranges.  Item-major: the sorted list is dealt
        to the batches ``chunk`` triplets at a time, round-robin, so that the chunks of one hot item are spread over
        all batches exactly as the kernel's strided visiting order spreads them over a single launch (a batch of
        CONSECUTIVE item-sorted triplets would put all work on a hot row into one launch: measured, 16 % higher loss
        after 14 epochs on the ML-1M shape); batch starts stay multiples of ``chunk``, item runs stay intact."""
        if schedule not in ("user", "item"):
            raise ValueError("schedule must be 'user' or 'item'")
        self.t = tables
        # size of the item catalogue the triplets' ids refer to: the table's rows, except when this process holds only a
        # row shard of the item table (qrec_amd/dist.py) and the ids are global
        self.n_items = int(n_items) if n_items is not None else tables.n_items
        self.n = int(u.size)
        self.schedule = schedule
        self.chunk = int(chunk)             # the chunk the stored order is dealt to the batches in = the chunk to launch epochs with
        # groups a reconciliation batch (replicated layout, K > 1) spreads over: a batch of a few ten thousand triplets is bound by the
        # per-group chain of dependent row reads (~1.9 us per triplet), not by the atomic units -- more groups, shorter chains
        self.batch_groups = 4096
        # ONE launch per epoch: at least MIN_ROUNDS rounds of the grid whatever the epoch's size (grid_for_epoch); `launch_grid()` is what
        # the epoch drivers pass to the kernels
        self._epoch_grid = grid_for_epoch(self.n, self.chunk) if max(1, int(batches)) == 1 else (self.chunk, 0)
        # item-major only: how P[u] is written (resolve_p_update above; "auto" decides by the collision density of THESE triplets under the
        # launcher's default grid).  Explicit "atomic" is the constructor's default: callers opt in to "auto" (the drop-in BPR class and
        # bench.py do), so that a test or a measurement never changes kernels behind the caller's back.
        self.collision = collision_density(np.bincount(np.asarray(u), minlength=1)) if self.n else 0.0
        self.p_update = resolve_p_update(np.bincount(np.asarray(u), minlength=1) if self.n else [], requested=p_update) if schedule == "item" else "atomic"
        self.item_variant = capi.HW_P_RMW if self.p_update == "rmw" else capi.HW_DEFAULT
        self.perm = None
        u = np.ascontiguousarray(u, dtype=np.int32); i = np.ascontiguousarray(i, dtype=np.int32)
        batches = max(1, int(batches))
        per = -(-self.n // batches) if self.n else 0
        self.batch_bounds = [min(b * per, self.n) for b in range(batches + 1)]
        # Item-major stored order (round 4): the item-sorted list is cut into RUNS of `item_run` triplets and the runs are laid out
        # in golden-ratio stride order, so that consecutive runs belong to different items -- a chunk of 32 is two runs of 16.  A
        # positive item's row still rides in registers along its run (one atomic flush per run), but it takes 16 steps in a row
        # instead of 32: measured with NO GPU involved (tools/order_sensitivity.py, profiles/r04_order_sensitivity.json), sequential
        # fp64 training in the 32-run order ends 0.003-0.004 of Recall@20 away from the reference's user-major order on data with
        # structure -- above the +-0.002 bar before any parallel execution -- while the 8-run order stays as close as a random
        # order does; runs of 16 cost nothing measurable either way and are the default (profiles/r04_item_run_timing.txt).  item_run = 0
        # keeps whole item runs (rounds 1-3).  A constructor parameter only: the sampler's negatives depend on the stored order, so an
        # environment variable here would change results behind the caller's back.
        self.item_run = int(item_run if item_run is not None else ITEM_RUN)
        if schedule == "item":
            self.perm = np.argsort(i, kind="stable")
            if self.item_run > 0 and self.n > self.item_run:
                self.perm = self.perm[stride_runs(self.n, self.item_run)]
            if batches > 1 and self.n:
                n_chunks, tail = -(-self.n // chunk), self.n % chunk
                whole = np.arange(n_chunks - 1 if tail else n_chunks)
                dealt = [whole[b::batches] for b in range(batches)]
                order = np.concatenate(dealt + ([np.array([n_chunks - 1])] if tail else []))
                at = (order[:, None] * chunk + np.arange(chunk)[None, :]).ravel()
                self.perm = self.perm[at[at < self.n]]
                sizes = [len(x) * chunk for x in dealt]
                sizes[-1] += tail
                self.batch_bounds = [0] + np.cumsum(sizes).tolist()
            u, i = np.ascontiguousarray(u[self.perm]), np.ascontiguousarray(i[self.perm])
        self.h_u, self.h_i, self.h_j = u, i, None          # host copies: the order-exact mode schedules the epoch on the host
        self._exact = {}
        self.d_u = DeviceBuffer.from_numpy(u)
        self.d_i = DeviceBuffer.from_numpy(i)
        self.d_j = DeviceBuffer(max(self.n, 1), np.int32)
        self.d_j_next = None
        self.d_stats = DeviceBuffer.zeros(capi.STATS_WORDS, np.float64)
        self.d_loss = self.d_stats          # element 0
        self._pos_dev = None
        self._side = None
        self._sampled = None
        self._prefetched_epoch = None
        self._sgd_start = None
        self._own_events = None
        self._consumed = [None, None]        # events: "the SGD kernel that read [d_j, d_j_next] has finished"
        self.d_drv = self.d_log = None
        self._log_capacity = 0
        self.accum = None                    # None: QREC_BPR_ACCUM decides at each epoch (resolve_accum); "auto" / "f32" / "i32": this object's choice
        if pos is not None:
            srt = pos.sorted_rows()
            self._pos_dev = (DeviceBuffer.from_numpy(srt.indptr), DeviceBuffer.from_numpy(srt.indices))

    def launch_grid(self, min_rounds: int | None = None):
        """(chunk, groups) for the whole-epoch launch of the one-pass schedules (groups 0 = the launcher's default grid)"""
        if min_rounds is None:
            return self._epoch_grid
        return grid_for_epoch(self.n, self.chunk, min_rounds) if len(self.batch_bounds) == 2 else (self.chunk, 0)

    # -- negatives ---------------------------------------------------------------------------
    def set_negatives(self, j: np.ndarray, stream=None):
        """``j`` in the reference's (user-major) triplet order; re-ordered to the schedule's."""
        j = np.ascontiguousarray(j, dtype=np.int32)
        if self.perm is not None:
            j = np.ascontiguousarray(j[self.perm])
        self.h_j = j
        self.d_j.upload(j, stream)

    def negatives_reference_order(self) -> np.ndarray:
        """current negatives as a host array in the reference's triplet order"""
        j = self.d_j.numpy()
        if self.perm is None:
            return j
        out = np.empty_like(j); out[self.perm] = j
        return out

    def sample_negatives_device(self, seed: int, epoch: int, stream=None):
        if self._pos_dev is None:
            raise RuntimeError("BprSgd was built without the positives CSR")
        capi.philox_bpr_sample(self._pos_dev[0], self._pos_dev[1], self.d_u, self.n, self.n_items,
                               seed, epoch, self.d_j, stream)

    def prefetch_negatives_device(self, seed: int, epoch: int):
        """Enqueue the sampler for `epoch` on the side stream into the spare buffer."""
        if self._pos_dev is None:
            raise RuntimeError("BprSgd was built without the positives CSR")
        if self._side is None:
            self._side = capi.Stream(); self._sampled = capi.Event()
            self.d_j_next = DeviceBuffer(max(self.n, 1), np.int32)
        if self._consumed[1] is not None:      # the spare buffer may still be read by an enqueued SGD kernel
            capi.stream_wait_event(self._side, self._consumed[1])
        if self._sgd_start is not None:
            capi.stream_wait_event(self._side, self._sgd_start)
        capi.philox_bpr_sample(self._pos_dev[0], self._pos_dev[1], self.d_u, self.n, self.n_items,
                               seed, epoch, self.d_j_next, self._side)
        self._sampled.record(self._side)
        self._prefetched_epoch = epoch

    def take_prefetched_negatives(self, epoch: int, stream=None):
        """Make `stream` wait for the prefetched negatives of `epoch` and switch to them."""
        if self._prefetched_epoch != epoch:
            raise RuntimeError(f"negatives of epoch {epoch} were not prefetched")
        capi.stream_wait_event(stream, self._sampled)
        self.d_j, self.d_j_next = self.d_j_next, self.d_j
        self._consumed.reverse()
        self._prefetched_epoch = None

    def mark_negatives_consumed(self, stream=None):
        """Record, after enqueueing the SGD kernel that reads the current negatives, that their buffer is
        free again once the stream gets here (only needed when epochs are enqueued without host syncs)."""
        if self._consumed[0] is None:
            self._consumed[0] = capi.Event()
        self._consumed[0].record(stream)

    # -- epochs ------------------------------------------------------------------------------------
    def epoch_ordered(self, lr: float, regU: float, regI: float, stream=None, width: int | None = None) -> float:
        """Strictly order-respecting pass (reference semantics).  Returns sum(-log sigmoid).
        The epoch's dependence DAG is list-scheduled on the host (``qrec_bpr_exact_schedule``, ~30 ms per 1.25 M
        triplets) into steps of at most ``width`` independent triplets, executed by one workgroup of ``width`` wavefronts
        (``qrec_bpr_sgd_scheduled``): same values as the one-wavefront walker bit for bit, ~n/6 steps instead of n.
        ``width`` 1 (or env QREC_EXACT_WIDTH=1) selects the walker."""
        import os
        if self.schedule != "user":
            raise RuntimeError("the order-exact kernel needs the reference's user-major order")
        t = self.t
        if width is None:
            width = int(os.environ.get("QREC_EXACT_WIDTH", "0")) or 8     # measured: 8 wavefronts cover the DAG's width (214 k steps vs 209 k at 16) at 2/3 of the step time
        width = min(width, capi.bpr_exact_width(t.code, t.d))
        if width <= 1 or self.n == 0 or self.h_j is None:
            capi.bpr_sgd_ordered(t.P, t.Q, t.code, t.d, t.ld, self.d_u, self.d_i, self.d_j, self.n, lr, regU, regI,
                                 self.d_stats, stream)
            return float(self.d_stats.head(1, stream)[0])
        prep = self.prepare_ordered(self.h_j, width=width, slot=0, stream=stream, reorder=False)
        self.run_prepared(prep, lr, regU, regI, stream)
        return float(self.d_stats.head(1, stream)[0])

    # -- order-exact epochs, pipelined: the host side of epoch k + 1 under the kernel of epoch k ---------------------
    def exact_width(self, width: int | None = None) -> int:
        import os
        if width is None:
            width = int(os.environ.get("QREC_EXACT_WIDTH", "0")) or 8
        return min(width, capi.bpr_exact_width(self.t.code, self.t.d))

    def prepare_ordered(self, j: np.ndarray, width: int | None = None, slot: int = 0, stream=None, reorder: bool = True):
        """Host side of one order-exact epoch: the dependence DAG of (u, i, j) list-scheduled (``qrec_bpr_exact_schedule``)
        and uploaded into schedule buffer ``slot`` (0 / 1) on ``stream``.  Sampling does not look at the embeddings, so
        this can run while the PREVIOUS epoch's kernel is still executing (pass a side stream: a copy on the kernel's
        stream would queue behind it).  ``j``: negatives in the reference's triplet order.  Returns the handle for
        ``run_prepared``; None when the one-wavefront walker has to be used (width <= 1)."""
        if self.schedule != "user":
            raise RuntimeError("the order-exact kernel needs the reference's user-major order")
        t = self.t
        width = self.exact_width(width)
        j = np.ascontiguousarray(j, dtype=np.int32)
        if reorder and self.perm is not None:
            j = np.ascontiguousarray(j[self.perm])
        if width <= 1 or self.n == 0:
            return None
        kind, slots = capi.bpr_exact_kind(t.code, t.ld, width)
        if kind and max(max(t.n_users, t.n_items) * t.ld, self.n) * t.dtype.itemsize >= 0xFFFFFF00:
            kind, slots = 0, 0            # the four-per-wavefront kernel addresses the tables AND its per-triplet log with 32-bit offsets
        entries, off = capi.bpr_exact_schedule(self.h_u, self.h_i, j, t.n_users, self.n_items, width, registers=bool(kind))
        x = self._exact
        if "xlog" not in x:
            x["xlog"] = DeviceBuffer(self.n + capi.EXACT_XLOG_PAD, t.dtype)
            x["scratch"] = DeviceBuffer.zeros(capi.EXACT_SCRATCH_WORDS, np.float64)
        key = f"slot{slot}"
        if key not in x:
            x[key] = (DeviceBuffer((self.n, 8), np.int32), DeviceBuffer(3 * self.n + 2, np.int32))     # step offsets: the register schedule may leave steps empty (<= 3 n steps)
        d_entries, d_off = x[key]
        d_entries.upload(entries, stream)
        d_off.upload_head(off, stream)
        steps = int(off.size - 1)
        # four triplets per wavefront (rows of 16 .. 128 elements): the schedule goes on in the fixed-width layout, expanded on the
        # device behind the upload (same stream)
        d_wide = None
        if kind:
            need = (steps + capi.EXACT_WIDE_PAD) * slots * 8
            wkey = f"wide{slot}"
            if wkey not in x or x[wkey].shape[0] < need:
                x[wkey] = DeviceBuffer(int(need * 1.1) + 64, np.int32)
            d_wide = x[wkey]
            capi.bpr_exact_expand(d_entries, d_off, steps, slots, d_wide, stream)
        # the host arrays stay referenced by the handle: an asynchronous copy may still be reading them when this returns
        return {"entries": d_entries, "off": d_off, "steps": steps, "width": width, "j": j, "host": (entries, off), "slots": slots, "wide": d_wide,
                "kind": kind}

    def run_prepared(self, prep, lr: float, regU: float, regI: float, stream=None):
        """enqueue the scheduled kernel of a prepared epoch (no host synchronisation; the loss lands in the stats buffer)"""
        t, x = self.t, self._exact
        self.h_j = prep["j"]
        self.exact_steps = prep["steps"]
        if prep.get("kind"):
            capi.bpr_sgd_scheduled_wide(t.P, t.Q, t.n_users, t.n_items, t.code, t.d, t.ld, prep["wide"], prep["steps"],
                                        prep["slots"], self.n, lr, regU, regI, x["xlog"], x["scratch"], self.d_stats, stream)
        else:
            capi.bpr_sgd_scheduled(t.P, t.Q, t.code, t.d, t.ld, prep["entries"], prep["off"], prep["steps"], prep["width"], self.n, lr, regU, regI,
                                   x["xlog"], x["scratch"], self.d_stats, stream)

    def epoch_throughput_async(self, lr: float, regU: float, regI: float, chunk: int = 32,
                               variant: int = capi.HW_DEFAULT, stream=None, groups: int = 0, flush_every: int = 16):
        """Hogwild pass (fp32 tables); enqueue only -- read the loss with ``loss()``/``epoch_stats()``.
        User-major schedule: P[u] register-resident, atomics on Q[i], Q[j].  Item-major schedule:
        Q[i] register-resident (flushed + re-read every ``flush_every`` triplets), atomics on P[u],
        Q[j] -- ~20% faster because the atomic units see flatter target rows."""
        if self.t.dtype != np.float32:
            raise TypeError("throughput mode needs fp32 tables")
        capi.memset(self.d_stats.ptr, 0, 8, stream)
        if self.schedule == "item":
            capi.bpr_sgd_hogwild_item_major(self.t.P, self.t.Q, self.t.d, self.t.ld, self.d_u, self.d_i, self.d_j,
                                            self.n, chunk, groups, flush_every, lr, regU, regI, self.d_stats, stream, variant=self.item_variant)
        else:
            capi.bpr_sgd_hogwild(self.t.P, self.t.Q, self.t.d, self.t.ld, self.d_u, self.d_i, self.d_j,
                                 self.n, chunk, groups, lr, regU, regI, self.d_stats, variant, stream)

    # -- device-resident loss / convergence / learning-rate schedule ------------------------------------
    def start_device_driver(self, lr0: float, log_capacity: int = 1024):
        """Put the bold-driver state (include/qrec_hip.h QREC_DRV_*) on the device: lRate = lr0, lastLoss = 0."""
        st = np.zeros(capi.DRV_WORDS, np.float64); st[capi.DRV_LR] = lr0
        self.d_drv = DeviceBuffer.from_numpy(st)
        self.d_log = DeviceBuffer.zeros((max(log_capacity, 1), capi.DRV_LOG_WORDS), np.float64)
        self._log_capacity = log_capacity
        self._own_events = [capi.Event() for _ in range(4)]
        self._grid_events = [capi.Event(), capi.Event()]
        self.d_stats.fill_bytes(0)

    def epoch_device_async(self, regU: float, regI: float, max_lr: float, tol: float = 1e-3, chunk: int = 32,
                           variant: int = capi.HW_DEFAULT, stream=None, groups: int = 0, flush_every: int = 16,
                           events=None, dist=None, after_start=None):
        """One throughput epoch with everything after it (BPR.py:40 loss terms, isConverged,
        updateLearningRate) enqueued on the device: no host synchronisation.  ``events`` = (before, after)
        capi.Event pair recorded around the SGD kernel.  ``dist`` (one process per GPU, qrec_amd/dist.py): a
        ``ReplicatedStep`` or ``ShardedStep`` -- the collectives are enqueued on the same stream, between the kernels.
        ``after_start``: called once the event that releases the next epoch's sampler is recorded (in front of the epoch's first
        SGD grid) -- the place to enqueue that sampler (``prefetch_negatives_device``) when something inside this epoch is to
        wait for it: the sharded layout plans the next epoch in front of this epoch's last batch."""
        if self.d_drv is None:
            raise RuntimeError("call start_device_driver() first")
        t = self.t
        # Two event records per epoch.  `start` (before the SGD grid) releases the next epoch's sampler: it is
        # dispatched just after this epoch's SGD grid -- measured, a sampler that already sits on the CUs when
        # the (one block per CU, persistent) SGD grid arrives skews its placement and costs 30% (0.78 vs 0.59 ms).
        # `end` (after it) frees the negatives buffer for the sampler after next.
        start, end = events if events else (self._own_events[0], self._own_events[1])
        fixed = dist is None and self.fixed_accum(groups, chunk)
        if fixed:       # in front of the start event: the event still sits right in front of the SGD grid
            capi.bpr_fixed_convert_in(t.P, t.n_users, t.Q, t.n_items, t.ld, self.d_drv, stream)
        start.record(stream)
        self._sgd_start = start
        if dist is not None and dist.mode == "sharded":
            # the first batch's SGD grid comes behind its fetch (gather, exchange): the sampler must not be released by the epoch's
            # start event -- it would sit on the CUs when the grid arrives (the 30% case above; measured again in round 3, 0.83 vs
            # 0.79 ms/epoch) -- but by one recorded right in front of that grid
            def first_grid(st):
                if after_start is not None:
                    grid = self._grid_events[0]; self._grid_events.reverse()
                    grid.record(st); self._sgd_start = grid
                    after_start()

            dist.exchange.run_epoch(lambda t0, nb, cache, rows, ci, cj, st: self._launch_sgd(
                t.P, cache, self.d_u.ptr + 4 * t0, ci, cj, nb, launch_chunk(nb, chunk), groups, flush_every, regU, regI, variant, st, q_rows=rows), stream,
                next_epoch=(lambda: dist.next_epoch(self)), before_first_sgd=first_grid)
        else:
            if after_start is not None:
                after_start()
            K = len(self.batch_bounds) - 1
            if dist is not None and dist.mode == "replicated" and K > 1:
                # replicated item table reconciled K times per epoch (round 4): between two syncs a rank does not see the other
                # ranks' updates of the rows they share, and with ONE sync per epoch that window is the whole epoch -- measured on
                # data with structure (tools/paired_recall.py, profiles/r04_paired_recall.json) the summed stale deltas overshoot
                # and training diverges at five times BPR.conf's rate.  Batch b = the b-th range of the stored order (item-major:
                # chunks dealt round-robin, so every batch sees every hot item); the last batch's sync is the fused epoch close.
                for b in range(K):
                    t0, nb = self.batch_bounds[b], self.batch_bounds[b + 1] - self.batch_bounds[b]
                    if nb:
                        bg = self.batch_groups
                        self._launch_sgd(t.P, t.Q, self.d_u.ptr + 4 * t0, self.d_i.ptr + 4 * t0, self.d_j.ptr + 4 * t0, nb, launch_chunk(nb, chunk, groups=bg),
                                         groups if groups else (bg if bg != 4096 else 0), flush_every, regU, regI, variant, stream)
                    if b + 1 < K:
                        dist.sync_tables(stream)
            else:
                self._launch_sgd(t.P, t.Q, self.d_u, self.d_i, self.d_j, self.n, chunk, groups, flush_every, regU, regI, variant, stream,
                                 fixed=fixed)
        end.record(stream)
        self._consumed[0] = end
        self._own_events.reverse()
        if dist is None:
            if fixed:
                capi.epoch_close_fixed(t.P, t.n_users, t.Q, t.n_items, t.ld, self.d_stats, self.d_drv, regU, regI, max_lr,
                                       tol, self.d_log, self._log_capacity, stream)
            else:
                capi.epoch_close(t.P, t.n_users, t.Q, t.n_items, t.code, t.ld, self.d_stats, self.d_drv, regU, regI, max_lr,
                                 tol, self.d_log, self._log_capacity, stream)
            return
        if dist.mode == "sharded":      # sum P*P and sum Q*Q are over disjoint row shards: all three terms add over ranks
            capi.epoch_sums(t.P, t.n_users, t.Q, t.n_items, t.code, t.ld, self.d_stats, self.d_drv, stream)
            dist.comm.allreduce(self.d_stats, 3, capi.F64, stream)
        elif dist.sync_p is None:       # users sharded, items replicated: ONE collective carries the deltas and {sum -log sigma, sum P*P}
            sq = dist.sync_q
            capi.dist_epoch_pre(t.P, t.n_users, t.ld, t.Q, sq.start, sq.delta, t.n_items, self.d_stats, self.d_drv, stream)
            dist.comm.allreduce_pair(sq.delta, sq.n, capi.F32, self.d_stats, 2, capi.F64, stream)
            capi.dist_epoch_post(t.Q, sq.start, sq.delta, t.n_items, t.ld, self.d_stats, self.d_drv, regU, regI, max_lr, tol,
                                 self.d_log, self._log_capacity, stream)
            return
        else:                           # both tables replicated (drop-in classes: every rank evaluates from whole tables)
            dist.sync_p.sync(stream)
            dist.sync_q.sync(stream, extra=(self.d_stats, 1, capi.F64))
            capi.epoch_sums(t.P, t.n_users, t.Q, t.n_items, t.code, t.ld, self.d_stats, self.d_drv, stream)
        capi.epoch_decide(self.d_stats, self.d_drv, regU, regI, max_lr, tol, self.d_log, self._log_capacity, stream)

    def fixed_accum(self, groups: int = 0, chunk: int = 32) -> bool:
        """whether a single-GPU device-driven epoch of this object, launched on ``groups`` groups (0 = the launcher's default) in chunks of
        ``chunk``, accumulates its deltas as integers (resolve_accum above)"""
        if not (self.d_drv is not None and self.schedule == "item" and self.p_update == "atomic" and self.t.dtype == np.float32
                and len(self.batch_bounds) == 2 and self.n > 0):
            return False
        accum = resolve_accum(self.accum)
        if accum != "auto":
            return accum == "i32"
        one_group = groups == 1 or self.n <= chunk          # the launcher clamps the groups to the number of chunks
        return not one_group and self.n >= FIXED_MIN_TRIPLETS_PER_ROW * (self.t.n_users + self.t.n_items)

    def _launch_sgd(self, P, Q, d_u, d_i, d_j, n, chunk, groups, flush_every, regU, regI, variant, stream, q_rows=None, fixed=False):
        """the throughput kernel of the schedule on (P, Q) -- Q is the item table, or a shard's row cache with the
        triplets' item ids rewritten to its rows; learning rate and stop flags come from the device-side driver.  ``fixed``: the
        tables are in fixed point (``epoch_device_async`` put them there and closes the epoch with ``epoch_close_fixed``)"""
        t = self.t
        if self.schedule == "item":
            capi.bpr_sgd_hogwild_item_major(P, Q, t.d, t.ld, d_u, d_i, d_j, n, chunk, groups, flush_every, 0.0, regU, regI,
                                            self.d_stats, stream, self.d_drv, p_rows=t.n_users, q_rows=q_rows,
                                            variant=capi.HW_FIXED if fixed else self.item_variant)
        else:
            capi.bpr_sgd_hogwild(P, Q, t.d, t.ld, d_u, d_i, d_j, n, chunk, groups, 0.0, regU, regI, self.d_stats, variant,
                                 stream, self.d_drv, p_rows=t.n_users, q_rows=q_rows)

    def driver_state(self, stream=None) -> dict:
        s = self.d_drv.numpy(stream)
        return {"lr": float(s[capi.DRV_LR]), "last_loss": float(s[capi.DRV_LAST_LOSS]), "epochs": int(s[capi.DRV_EPOCHS]),
                "converged": bool(s[capi.DRV_CONVERGED]), "failed": bool(s[capi.DRV_FAILED])}

    def driver_log(self, stream=None) -> np.ndarray:
        """rows {loss, lr used, sum(-log sigma), lastLoss - loss, sum P*P, sum Q*Q, -, -} of the epochs closed so far"""
        n = min(self.driver_state(stream)["epochs"], self._log_capacity)
        return self.d_log.numpy(stream)[:n].copy()

    def enqueue_epoch_stats(self, stream=None):
        """sum P*P and sum Q*Q into the stats buffer, next to the epoch's sum(-log sigma) -- BPR.py:40,53"""
        t = self.t
        capi.sumsq(t.P, t.code, t.n_users, t.d, t.ld, self.d_stats.ptr + 8, stream)
        capi.sumsq(t.Q, t.code, t.n_items, t.d, t.ld, self.d_stats.ptr + 16, stream)

    def read_epoch_stats(self, stream=None):
        s = self.d_stats.head(3, stream)
        return float(s[0]), float(s[1]), float(s[2])

    def epoch_stats(self, stream=None):
        """(sum -log sigma, sum P*P, sum Q*Q) after the enqueued epoch.  One read-back; this is the epoch's
        only host synchronisation."""
        self.enqueue_epoch_stats(stream)
        return self.read_epoch_stats(stream)

    def loss(self, stream=None) -> float:
        return float(self.d_stats.head(1, stream)[0])


class MfSgd:
    """Rating-prediction MF family on the device, order-exact: BasicMF (model/rating/BasicMF.py:9-26),
    PMF (model/rating/PMF.py:9-28), SVD (model/rating/SVD.py:13-35), EE (model/rating/EE.py:15-34)."""

    def __init__(self, tables: DeviceTables, n: int, variant: int = capi.MF_BASIC, Bu=None, Bi=None):
        self.t = tables
        self.n = n
        self.variant = variant
        self.d_u = DeviceBuffer(max(n, 1), np.int32)
        self.d_i = DeviceBuffer(max(n, 1), np.int32)
        self.d_r = DeviceBuffer(max(n, 1), np.float64)
        self.d_stats = DeviceBuffer.zeros(5, np.float64)      # err^2, sum P^2, sum Q^2, sum Bu^2, sum Bi^2
        self.d_Bu = self.d_Bi = None
        if variant in (capi.MF_SVD, capi.MF_EE):
            self.d_Bu = DeviceBuffer.from_numpy(np.ascontiguousarray(Bu, dtype=tables.dtype))
            self.d_Bi = DeviceBuffer.from_numpy(np.ascontiguousarray(Bi, dtype=tables.dtype))

    def epoch(self, u, i, r, lr: float, regU: float = 0.0, regI: float = 0.0, regB: float = 0.0,
              global_mean: float = 0.0, stream=None) -> float:
        """one pass over the rows in the given order; returns sum(error^2)"""
        self.d_u.upload(np.ascontiguousarray(u, dtype=np.int32), stream)
        self.d_i.upload(np.ascontiguousarray(i, dtype=np.int32), stream)
        self.d_r.upload(np.ascontiguousarray(r, dtype=np.float64), stream)
        capi.mf_sgd_ordered(self.t.P, self.t.Q, self.t.code, self.t.d, self.t.ld, self.d_u, self.d_i,
                            self.d_r, self.n, lr, self.d_stats, stream, self.variant, regU, regI, self.d_Bu,
                            self.d_Bi, regB, global_mean)
        return float(self.d_stats.head(1, stream)[0])

    def sumsq_terms(self, stream=None):
        """(sum P^2, sum Q^2, sum Bu^2, sum Bi^2) for the epoch-end regularisers (PMF.py:25, SVD.py:32-33)"""
        t = self.t
        capi.sumsq(t.P, t.code, t.n_users, t.d, t.ld, self.d_stats.ptr + 8, stream)
        capi.sumsq(t.Q, t.code, t.n_items, t.d, t.ld, self.d_stats.ptr + 16, stream)
        if self.d_Bu is not None:
            capi.sumsq(self.d_Bu, t.code, t.n_users, 1, 1, self.d_stats.ptr + 24, stream)
            capi.sumsq(self.d_Bi, t.code, t.n_items, 1, 1, self.d_stats.ptr + 32, stream)
        s = self.d_stats.numpy(stream)
        return float(s[1]), float(s[2]), float(s[3]), float(s[4])

    def biases(self):
        return self.d_Bu.numpy().astype(np.float64), self.d_Bi.numpy().astype(np.float64)



class SocialSgd:
    """The social-trust rating models on the device, order-exact, fp64 (model/rating/{SoRec,SoReg,SocialMF,RSTE,SREE}.py).
    Holds P, Q (``tables``), Z (SoRec) or Bu/Bi (SREE), the walk of the social pass (``steps``: a social.UserSteps for
    SocialMF / SoReg / SREE, a social.Relations for SoRec; RSTE: social.followee_csr_by_user) and its level schedule, built
    here once.  One call per pass: ``rating_pass`` (mf_ordered_kernel -- PMF for SoRec and SoReg, SocialMF's copies,
    EE for SREE -- or RSTE's own kernel), then ``social_pass``, which adds the pass' loss terms onto the rating loss
    in the reference's order and returns the sum; ``sumsq_terms`` for the epoch-end regularisers."""
    KINDS = ("SoRec", "SoReg", "SocialMF", "RSTE", "SREE")
    _VARIANT = {"SoRec": capi.MF_PMF, "SoReg": capi.MF_PMF, "SocialMF": capi.MF_SOCIALMF, "SREE": capi.MF_EE}
    _MODE = {"SocialMF": capi.SOCIAL_SOCIALMF, "SoReg": capi.SOCIAL_SOREG, "SREE": capi.SOCIAL_SREE}

    def __init__(self, tables: DeviceTables, n: int, kind: str, steps, Z=None, Bu=None, Bi=None, schedule=None):
        if kind not in self.KINDS:
            raise ValueError(f"unknown social model {kind!r}")
        if tables.dtype != np.float64:
            raise ValueError("the social models run on fp64 tables")
        self.t, self.n, self.kind, self.steps = tables, n, kind, steps
        up = lambda a, dt: DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=dt) if np.size(a) else np.zeros(1, dt))
        if kind == "RSTE":
            ptr, ids, w, den = steps
            self.d_fe_ptr, self.d_fe_ids, self.d_fe_w, self.d_den = up(ptr, np.int64), up(ids, np.int32), up(w, np.float64), up(den, np.float64)
            self.d_u = DeviceBuffer(max(n, 1), np.int32); self.d_i = DeviceBuffer(max(n, 1), np.int32)
            self.d_r = DeviceBuffer(max(n, 1), np.float64)
            self.d_stats = DeviceBuffer.zeros(3, np.float64)         # err^2, sum P^2, sum Q^2
            return
        self.mf = MfSgd(tables, n, self._VARIANT[kind], Bu, Bi)
        self.d_stats = self.mf.d_stats
        if kind == "SoRec":
            self.d_Z = DeviceBuffer.from_numpy(tables._pad(np.asarray(Z, dtype=np.float64)))
            self.d_su, self.d_sv, self.d_st, self.d_sw = up(steps.u, np.int32), up(steps.v, np.int32), up(steps.t, np.float64), up(steps.w, np.float64)
            self.n_steps = self.n_slots = steps.n
            self.d_zsum = DeviceBuffer.zeros(1, np.float64)
        else:
            self.d_user = up(steps.user, np.int32)
            self.d_fe_ptr, self.d_fe_ids, self.d_fe_w = up(steps.fe_ptr, np.int64), up(steps.fe_ids, np.int32), up(steps.fe_w, np.float64)
            self.d_fr_ptr = self.d_fr_ids = self.d_fr_w = None
            if kind == "SoReg":
                self.d_fr_ptr, self.d_fr_ids, self.d_fr_w = up(steps.fr_ptr, np.int64), up(steps.fr_ids, np.int32), up(steps.fr_w, np.float64)
            self.n_steps = steps.n_steps
            self.n_slots = self.n_steps if kind == "SocialMF" else int(steps.fe_ptr[-1])
        self.d_slots = DeviceBuffer(max(self.n_slots, 1), np.float64)
        self.set_schedule(schedule if schedule is not None else steps.schedule(tables.n_users))

    def set_schedule(self, sched):
        """run the social pass by ``sched`` (social.Schedule); social.sequential_schedule(n_steps) is the plain walk"""
        assert sched.order.size == self.n_steps
        self.schedule = sched
        self.d_order = DeviceBuffer.from_numpy(np.ascontiguousarray(sched.order, dtype=np.int32) if sched.order.size else np.zeros(1, np.int32))
        self.d_level_ptr = DeviceBuffer.from_numpy(np.ascontiguousarray(sched.level_ptr, dtype=np.int32))
        self.n_waves = max(1, min(capi.SOCIAL_MAX_WAVES, sched.max_width))

    def rating_pass(self, u, i, r, lr: float, regU: float, regI: float, regB: float = 0.0, global_mean: float = 0.0,
                    alpha: float = 0.0, stream=None) -> float:
        """one pass over the ratings in the given (current trainingData) order; returns its loss"""
        if self.kind != "RSTE":
            return self.mf.epoch(u, i, r, lr, regU, regI, regB, global_mean, stream)
        self.d_u.upload(np.ascontiguousarray(u, dtype=np.int32), stream)
        self.d_i.upload(np.ascontiguousarray(i, dtype=np.int32), stream)
        self.d_r.upload(np.ascontiguousarray(r, dtype=np.float64), stream)
        t = self.t
        capi.rste_sgd_ordered(t.P, t.Q, t.d, t.ld, self.d_fe_ptr, self.d_fe_ids, self.d_fe_w, self.d_den, self.d_u, self.d_i, self.d_r,
                              self.n, lr, alpha, regU, regI, self.d_stats, stream)
        return float(self.d_stats.head(1, stream)[0])

    def social_pass(self, lr: float, coef: float, regZ: float = 0.0, start: float | None = None, stream=None) -> float:
        """the social half of the epoch (coef: regS for SoRec and SocialMF, alpha for SoReg and SREE); its loss terms are
        added one by one in walk order onto the running loss -- the rating pass' loss, or ``start`` when given (SREE adds
        its bias term first) -- and that sum is returned"""
        t, s = self.t, self.schedule
        if start is not None:
            self.d_stats.upload_head(np.array([start], dtype=np.float64), stream)
        if self.kind == "SoRec":
            capi.sorec_relation_pass(t.P, self.d_Z, t.d, t.ld, self.d_su, self.d_sv, self.d_st, self.d_sw, self.n_steps, self.d_order,
                                     self.d_level_ptr, s.n_levels, self.n_waves, lr, coef, regZ, self.d_slots, stream)
        else:
            capi.social_user_pass(self._MODE[self.kind], t.P, t.d, t.ld, self.d_user, self.n_steps, self.d_fe_ptr, self.d_fe_ids,
                                  self.d_fe_w, self.d_fr_ptr, self.d_fr_ids, self.d_fr_w, self.d_order, self.d_level_ptr, s.n_levels,
                                  self.n_waves, lr, coef, self.d_slots, stream)
        capi.loss_fold(self.d_stats, self.d_slots, self.n_slots, stream)
        return float(self.d_stats.head(1, stream)[0])

    def sumsq_terms(self, stream=None):
        """(sum P^2, sum Q^2, sum Z^2 or 0, sum Bu^2 or 0, sum Bi^2 or 0)"""
        t = self.t
        if self.kind == "RSTE":
            capi.sumsq(t.P, t.code, t.n_users, t.d, t.ld, self.d_stats.ptr + 8, stream)
            capi.sumsq(t.Q, t.code, t.n_items, t.d, t.ld, self.d_stats.ptr + 16, stream)
            st = self.d_stats.numpy(stream)
            return float(st[1]), float(st[2]), 0.0, 0.0, 0.0
        sp, sq, sbu, sbi = self.mf.sumsq_terms(stream)
        sz = 0.0
        if self.kind == "SoRec":
            capi.sumsq(self.d_Z, t.code, t.n_users, t.d, t.ld, self.d_zsum, stream)
            sz = float(self.d_zsum.numpy(stream)[0])
        return sp, sq, sz, sbu, sbi

    def Z(self):
        return np.ascontiguousarray(self.d_Z.numpy()[:, :self.t.d], dtype=np.float64)

    def biases(self):
        return self.mf.biases()


class SocialHSgd:
    """LOCABAL and SocialFD on the device, order-exact, fp64 (model/rating/{LOCABAL,SocialFD}.py): the two social models
    whose passes carry a dense d x d matrix H.  Holds P, Q (``tables``), H, LOCABAL's per-user weight array (``W``: 0 for a
    user in no relation) or SocialFD's biases, and the walk of the social pass (``steps``: a social.Edges for LOCABAL, a
    social.UserSteps in data.user order for SocialFD).  Every step rewrites H, so there is no schedule: one workgroup
    walks a pass step by step (social.hip).  ``rating_pass`` then ``social_pass`` as in :class:`SocialSgd`: the social
    pass' loss terms are added onto the running loss one by one in walk order; ``sumsq_terms`` includes sum H^2.
    ``n_waves``: wavefronts of the workgroup, 0 = chosen from d; the results do not depend on it."""
    KINDS = ("LOCABAL", "SocialFD")

    def __init__(self, tables: DeviceTables, n: int, kind: str, steps, H, W=None, Bu=None, Bi=None, n_waves: int = 0):
        if kind not in self.KINDS:
            raise ValueError(f"unknown model {kind!r}")
        if tables.dtype != np.float64:
            raise ValueError("the social models run on fp64 tables")
        if tables.d > capi.SOCIAL_H_MAX_D:
            raise ValueError(f"{kind} supports num.factors <= {capi.SOCIAL_H_MAX_D} (the d x d matrix H stays in LDS), got {tables.d}")
        self.t, self.n, self.kind, self.steps, self.n_waves = tables, n, kind, steps, n_waves
        up = lambda a, dt: DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=dt) if np.size(a) else np.zeros(1, dt))
        H = np.ascontiguousarray(H, dtype=np.float64)
        assert H.shape == (tables.d, tables.d)
        self.d_H = DeviceBuffer.from_numpy(H)
        self.d_u = DeviceBuffer(max(n, 1), np.int32); self.d_i = DeviceBuffer(max(n, 1), np.int32)
        self.d_r = DeviceBuffer(max(n, 1), np.float64)
        self.d_stats = DeviceBuffer.zeros(6, np.float64)             # loss, sum P^2, Q^2, H^2, Bu^2, Bi^2
        self.d_Bu = self.d_Bi = self.d_W = None
        if kind == "LOCABAL":
            assert np.size(W) == tables.n_users
            self.d_W = up(W, np.float64)
            self.d_eu, self.d_ek, self.d_es = up(steps.u, np.int32), up(steps.k, np.int32), up(steps.sim, np.float64)
            self.n_steps = self.n_slots = steps.n
        else:
            self.d_Bu, self.d_Bi = up(Bu, np.float64), up(Bi, np.float64)
            self.d_user, self.d_fe_ptr, self.d_fe_ids = up(steps.user, np.int32), up(steps.fe_ptr, np.int64), up(steps.fe_ids, np.int32)
            self.n_steps = steps.n_steps
            self.n_slots = int(steps.fe_ptr[-1]) if self.n_steps else 0
        self.d_slots = DeviceBuffer(max(self.n_slots, 1), np.float64)

    def rating_pass(self, u, i, r, lr: float, regU: float, regI: float, eta: float = 0.0, alpha: float = 0.0,
                    global_mean: float = 0.0, stream=None) -> float:
        """one pass over the ratings in the given (current trainingData) order; returns its loss (SocialFD: err^2 and the
        band term per rating, in that order)"""
        if self.n:                                       # no rows: nothing to upload, the pass is a no-op with loss 0
            self.d_u.upload(np.ascontiguousarray(u, dtype=np.int32), stream)
            self.d_i.upload(np.ascontiguousarray(i, dtype=np.int32), stream)
            self.d_r.upload(np.ascontiguousarray(r, dtype=np.float64), stream)
        t = self.t
        if self.kind == "LOCABAL":
            capi.locabal_sgd_ordered(t.P, t.Q, t.d, t.ld, self.d_W, self.d_u, self.d_i, self.d_r, self.n, lr, regU, regI, self.d_stats,
                                     stream)
        else:
            capi.socialfd_sgd_ordered(t.P, t.Q, self.d_Bu, self.d_Bi, self.d_H, t.d, t.ld, self.d_u, self.d_i, self.d_r, self.n, lr, regU,
                                      regI, eta, alpha, global_mean, self.d_stats, self.n_waves, stream)
        return float(self.d_stats.head(1, stream)[0])

    def social_pass(self, lr: float, alpha: float = 0.0, regS: float = 0.0, eta: float = 0.0, beta: float = 0.0,
                    start: float | None = None, stream=None) -> float:
        """the social half of the epoch (LOCABAL: alpha, regS; SocialFD: eta, beta); its loss terms are added one by one
        in walk order onto the running loss -- the rating pass' loss, or ``start`` when given -- and that sum is returned"""
        t = self.t
        if start is not None:
            self.d_stats.upload_head(np.array([start], dtype=np.float64), stream)
        if self.kind == "LOCABAL":
            capi.locabal_social_pass(t.P, self.d_H, t.d, t.ld, self.d_eu, self.d_ek, self.d_es, self.n_steps, lr, alpha, regS,
                                     self.d_slots, self.n_waves, stream)
        else:
            capi.socialfd_social_pass(t.P, self.d_H, t.d, t.ld, self.d_user, self.n_steps, self.d_fe_ptr, self.d_fe_ids, lr, eta, beta,
                                      self.d_slots, self.n_waves, stream)
        capi.loss_fold(self.d_stats, self.d_slots, self.n_slots, stream)
        return float(self.d_stats.head(1, stream)[0])

    def sumsq_terms(self, stream=None):
        """(sum P^2, sum Q^2, sum H^2, sum Bu^2 or 0, sum Bi^2 or 0)"""
        t = self.t
        capi.sumsq(t.P, t.code, t.n_users, t.d, t.ld, self.d_stats.ptr + 8, stream)
        capi.sumsq(t.Q, t.code, t.n_items, t.d, t.ld, self.d_stats.ptr + 16, stream)
        capi.sumsq(self.d_H, t.code, t.d, t.d, t.d, self.d_stats.ptr + 24, stream)
        if self.d_Bu is not None:
            capi.sumsq(self.d_Bu, t.code, t.n_users, 1, 1, self.d_stats.ptr + 32, stream)
            capi.sumsq(self.d_Bi, t.code, t.n_items, 1, 1, self.d_stats.ptr + 40, stream)
        s = self.d_stats.numpy(stream)
        return tuple(float(x) for x in s[1:6])

    def H(self):
        return self.d_H.numpy().astype(np.float64)

    def biases(self):
        return self.d_Bu.numpy().astype(np.float64), self.d_Bi.numpy().astype(np.float64)


class SvdppSgd:
    """SVD++ on the device, order-exact (model/rating/SVDPlusPlus.py:25-62): P, Q, the implicit-feedback table Y and
    the biases stay resident; ``rated`` = every user's train items in ``data.userRated`` order."""

    def __init__(self, tables: DeviceTables, Y, Bu, Bi, rated: CSR, n: int):
        self.t, self.n = tables, n
        dt = tables.dtype
        Yp = np.zeros((Y.shape[0], tables.ld), dtype=dt); Yp[:, :tables.d] = Y
        self.d_Y = DeviceBuffer.from_numpy(Yp)
        self.d_Bu = DeviceBuffer.from_numpy(np.ascontiguousarray(Bu, dtype=dt))
        self.d_Bi = DeviceBuffer.from_numpy(np.ascontiguousarray(Bi, dtype=dt))
        self.d_indptr = DeviceBuffer.from_numpy(rated.indptr.astype(np.int64))
        self.d_items = DeviceBuffer.from_numpy(rated.indices.astype(np.int32) if rated.indices.size else np.zeros(1, np.int32))
        self.d_u = DeviceBuffer(max(n, 1), np.int32); self.d_i = DeviceBuffer(max(n, 1), np.int32)
        self.d_r = DeviceBuffer(max(n, 1), np.float64)
        self.d_stats = DeviceBuffer.zeros(6, np.float64)     # err^2, sum P^2, Q^2, Y^2, Bu^2, Bi^2

    def epoch(self, u, i, r, lr, regU, regI, regB, regY, global_mean, stream=None) -> float:
        self.d_u.upload(np.ascontiguousarray(u, dtype=np.int32), stream)
        self.d_i.upload(np.ascontiguousarray(i, dtype=np.int32), stream)
        self.d_r.upload(np.ascontiguousarray(r, dtype=np.float64), stream)
        t = self.t
        capi.svdpp_sgd_ordered(t.P, t.Q, self.d_Y, self.d_Bu, self.d_Bi, t.code, t.d, t.ld, self.d_indptr, self.d_items,
                               self.d_u, self.d_i, self.d_r, self.n, lr, regU, regI, regB, regY, global_mean, self.d_stats, stream)
        return float(self.d_stats.head(1, stream)[0])

    def sumsq_terms(self, stream=None):
        """(sum P^2, sum Q^2, sum Y^2, sum Bu^2, sum Bi^2) -- SVDPlusPlus.py:64-65"""
        t = self.t
        for k, (buf, rows, d, ld) in enumerate(((t.P, t.n_users, t.d, t.ld), (t.Q, t.n_items, t.d, t.ld), (self.d_Y, t.n_items, t.d, t.ld),
                                                (self.d_Bu, t.n_users, 1, 1), (self.d_Bi, t.n_items, 1, 1))):
            capi.sumsq(buf, t.code, rows, d, ld, self.d_stats.ptr + 8 * (k + 1), stream)
        s = self.d_stats.numpy(stream)
        return tuple(float(x) for x in s[1:6])

    def download(self):
        return (self.d_Y.numpy()[:, :self.t.d].astype(np.float64), self.d_Bu.numpy().astype(np.float64),
                self.d_Bi.numpy().astype(np.float64))


class RatingEvaluator:
    """evalRatings / rating_performance of the rating models on the device (base/recommender.py:88-110,
    base/iterativeRecommender.py:103-113): every test pair's ``checkRatingBoundary(predictForRating(u, i))`` and the
    MAE / RMSE strings of ``Measure.ratingMeasure``, from the tables where the SGD objects keep them.

    ``form`` names the class's predictForRating (capi.RATING_*).  The evaluator BINDS device buffers and copies none:
    ``tables`` (a DeviceTables), and by keyword ``Bu`` / ``Bi`` (MfSgd.d_Bu / d_Bi), ``Y`` with ``rated`` = (d_indptr,
    d_items, host indptr) (SvdppSgd), ``H`` (SocialHSgd.d_H), ``followees`` = (d_ptr, d_ids, d_w, d_den) (SocialSgd, RSTE)
    and ``alpha``.  Its own buffers -- the test pairs, the two mean arrays, predictions, error slots, SVD++'s imp rows --
    are allocated once.  ``uid`` / ``iid``: the pairs' ids, -1 = a name the training set does not know.  Ids outside
    [-1, table size), METRIC at d > capi.SOCIAL_H_MAX_D and non-fp64 tables raise ValueError before anything is launched."""
    FORMS = {"DOT": capi.RATING_DOT, "BIASED": capi.RATING_BIASED, "SVDPP": capi.RATING_SVDPP, "EUCLID": capi.RATING_EUCLID,
             "METRIC": capi.RATING_METRIC, "RSTE": capi.RATING_RSTE}

    def __init__(self, form, tables: DeviceTables, uid, iid, rating, scale, user_means, item_means, global_mean: float, *,
                 Bu=None, Bi=None, Y=None, rated=None, H=None, followees=None, alpha: float = 0.0):
        self.form = self.FORMS[form] if isinstance(form, str) else int(form)
        if self.form not in self.FORMS.values():
            raise ValueError(f"unknown rating form {form!r}")
        if tables.dtype != np.float64:
            raise ValueError("the rating evaluator runs on fp64 tables")
        if self.form == capi.RATING_METRIC and tables.d > capi.SOCIAL_H_MAX_D:
            raise ValueError(f"the METRIC form supports num.factors <= {capi.SOCIAL_H_MAX_D} (the d x d matrix H stays in LDS), got {tables.d}")
        needs = {capi.RATING_BIASED: (Bu, Bi), capi.RATING_SVDPP: (Bu, Bi, Y, rated), capi.RATING_EUCLID: (Bu, Bi),
                 capi.RATING_METRIC: (Bu, Bi, H), capi.RATING_RSTE: (followees,)}.get(self.form, ())
        if any(x is None for x in needs):
            raise ValueError("the form's device buffers are missing (Bu/Bi, Y and rated, H or followees)")
        self.t = tables
        self.lo, self.hi = float(scale[0]), float(scale[-1])
        self.global_mean, self.alpha = float(global_mean), float(alpha)
        self.d_Bu, self.d_Bi, self.d_Y, self.d_H = Bu, Bi, Y, H
        self.d_fe = followees if followees is not None else (None, None, None, None)
        um = np.ascontiguousarray(user_means, dtype=np.float64); im = np.ascontiguousarray(item_means, dtype=np.float64)
        if um.shape != (tables.n_users,) or im.shape != (tables.n_items,):
            raise ValueError("user_means / item_means must have one entry per table row")
        uid, iid, rating = self._checked_pairs(uid, iid, rating)
        self.n = n = uid.size
        up = lambda a: DeviceBuffer.from_numpy(a if a.size else np.zeros(1, a.dtype))
        self.d_umean, self.d_imean = up(um), up(im)
        self.d_uid, self.d_iid, self.d_rating = up(uid), up(iid), up(rating)
        self.d_pred = DeviceBuffer.zeros(max(n, 1), np.float64)
        self.d_abs = DeviceBuffer(max(n, 1), np.float64); self.d_sq = DeviceBuffer(max(n, 1), np.float64)
        self.d_sums = DeviceBuffer.zeros(2, np.float64)
        self.d_imp = self.d_users = None
        if self.form == capi.RATING_SVDPP:
            self.d_rated_ptr, self.d_rated_items, host_ptr = rated
            if np.asarray(host_ptr).size != tables.n_users + 1:
                raise ValueError("rated: one CSR row per user")
            self.d_imp = DeviceBuffer.zeros((tables.n_users, tables.ld), np.float64)
            self._set_users(uid, iid)

    def _checked_pairs(self, uid, iid, rating):
        uid = np.ascontiguousarray(uid, dtype=np.int32); iid = np.ascontiguousarray(iid, dtype=np.int32)
        rating = np.ascontiguousarray(rating, dtype=np.float64)
        if not (uid.ndim == 1 and uid.shape == iid.shape == rating.shape):
            raise ValueError("uid, iid and rating must be one-dimensional and of one length")
        if uid.size and (uid.min() < -1 or uid.max() >= self.t.n_users or iid.min() < -1 or iid.max() >= self.t.n_items):
            raise ValueError(f"test pair ids must lie in [-1, {self.t.n_users}) for users and [-1, {self.t.n_items}) for items")
        return uid, iid, rating

    def _set_users(self, uid, iid):
        """SVD++: the distinct users whose imp row a pair reads"""
        users = np.unique(uid[(uid >= 0) & (iid >= 0)]).astype(np.int32)
        self.n_test_users = users.size
        self.d_users = DeviceBuffer.from_numpy(users if users.size else np.zeros(1, np.int32))

    def set_pairs(self, uid, iid, rating):
        """other test pairs of the SAME count (the buffers are allocated once); bad ids raise and change nothing"""
        uid, iid, rating = self._checked_pairs(uid, iid, rating)
        if uid.size != self.n:
            raise ValueError(f"set_pairs: this evaluator holds {self.n} pairs, got {uid.size}")
        if self.n:
            self.d_uid.upload(uid); self.d_iid.upload(iid); self.d_rating.upload(rating)
            if self.form == capi.RATING_SVDPP:
                self._set_users(uid, iid)

    @classmethod
    def from_host(cls, form, P, Q, uid, iid, rating, scale, user_means, item_means, global_mean, *, Bu=None, Bi=None, Y=None,
                  rated: CSR | None = None, H=None, followees=None, alpha: float = 0.0):
        """the same evaluator over host arrays, uploaded here (tests and tools); ``rated``: a CSR of every user's train items
        in userRated order, ``followees``: (ptr, ids, w, den) as social.followee_csr_by_user returns them"""
        P = np.asarray(P); Q = np.asarray(Q)
        if P.dtype != np.float64 or Q.dtype != np.float64:
            raise ValueError("the rating evaluator runs on fp64 tables")
        form_id = cls.FORMS[form] if isinstance(form, str) else int(form)
        if form_id == capi.RATING_METRIC and P.shape[1] > capi.SOCIAL_H_MAX_D:
            raise ValueError(f"the METRIC form supports num.factors <= {capi.SOCIAL_H_MAX_D} (the d x d matrix H stays in LDS), got {P.shape[1]}")
        t = DeviceTables(P, Q, np.float64)
        up = lambda a, dt: None if a is None else DeviceBuffer.from_numpy(np.ascontiguousarray(a, dtype=dt) if np.size(a) else np.zeros(1, dt))
        kw = dict(Bu=up(Bu, np.float64), Bi=up(Bi, np.float64), H=up(H, np.float64), alpha=alpha)
        if Y is not None:
            kw["Y"] = DeviceBuffer.from_numpy(t._pad(np.asarray(Y, dtype=np.float64)))
            kw["rated"] = (up(rated.indptr, np.int64), up(rated.indices, np.int32), rated.indptr)
        if followees is not None:
            ptr, ids, w, den = followees
            kw["followees"] = (up(ptr, np.int64), up(ids, np.int32), up(w, np.float64), up(den, np.float64))
        return cls(form, t, uid, iid, rating, scale, user_means, item_means, global_mean, **kw)

    def _predict(self, stream=None):
        """the unrounded predictions into d_pred"""
        t, aux = self.t, None
        if self.form == capi.RATING_SVDPP:
            capi.rating_implicit(self.d_Y, t.code, t.n_items, t.d, t.ld, self.d_rated_ptr, self.d_rated_items, self.d_users,
                                 self.n_test_users, t.n_users, self.d_imp, stream)
            aux = self.d_imp
        elif self.form == capi.RATING_METRIC:
            aux = self.d_H
        ptr, ids, w, den = self.d_fe
        capi.rating_predict(self.form, t.code, t.P, t.Q, t.n_users, t.n_items, t.d, t.ld, self.d_uid, self.d_iid, self.n, self.d_pred,
                            self.global_mean, self.d_Bu, self.d_Bi, aux, ptr, ids, w, den, self.d_umean, self.d_imean, self.alpha, stream)

    def _run(self, stream=None):
        self._predict(stream)
        capi.rating_boundary(self.d_pred, self.n, self.lo, self.hi, stream)

    def raw_predictions(self, stream=None) -> np.ndarray:
        """float64[n]: predictForRating of every pair, before the clamp and the rounding"""
        self._predict(stream)
        return self.d_pred.numpy(stream)[:self.n]

    def predictions(self, stream=None) -> np.ndarray:
        """float64[n]: checkRatingBoundary(predictForRating(u, i)) of every pair"""
        self._run(stream)
        return self.d_pred.numpy(stream)[:self.n]

    def error_sums(self, stream=None):
        """(sum |r - p|, sum (r - p)^2) over the pairs, each added in pair order like Python's sum()"""
        self._run(stream)
        capi.rating_errors(self.d_rating, self.d_pred, self.n, self.d_abs, self.d_sq, stream)
        self.d_sums.fill_bytes(0, stream)
        capi.loss_fold(self.d_sums.ptr, self.d_abs, self.n, stream)
        capi.loss_fold(self.d_sums.ptr + 8, self.d_sq, self.n, stream)
        s = self.d_sums.numpy(stream)
        return float(s[0]), float(s[1])

    def measure(self, stream=None):
        """["MAE:...\\n", "RMSE:...\\n"] as Measure.ratingMeasure forms them (util/measure.py:59-71)"""
        import math
        if self.n == 0:
            return ["MAE:0\n", "RMSE:0\n"]
        s_abs, s_sq = self.error_sums(stream)
        return ["MAE:" + str(s_abs / self.n) + "\n", "RMSE:" + str(math.sqrt(s_sq / self.n)) + "\n"]


class AlsSolver:
    """Implicit-feedback ALS (model/ranking/WRMF.py:17-67) with both fp64 tables resident: ``X`` (users) and ``Y`` (items) in
    one ``DeviceTables`` (P = X, Q = Y), the rating CSR by user and by item with confidences ``c = alpha * r``, G and the
    workspaces.  ``epoch()`` = G = Y^T Y, every user's solve (the loss taken from the rows of X before it), G = X^T X, every
    item's solve; it returns the loss.  Every sum has a fixed order: two runs from the same tables are bit-identical."""

    def __init__(self, X: np.ndarray, Y: np.ndarray, uid: np.ndarray, iid: np.ndarray, rating: np.ndarray, lam: float,
                 alpha: float = 10.0):
        n_users, n_items = X.shape[0], Y.shape[0]
        self.t = DeviceTables(X, Y, np.float64)
        self.d, self.ld, self.lam = self.t.d, self.t.ld, float(lam)
        u = np.asarray(uid, dtype=np.int32); i = np.asarray(iid, dtype=np.int32)
        c = alpha * np.asarray(rating, dtype=np.float64)
        self.halves = []
        for rows, cols, n_rows in ((u, i, n_users), (i, u, n_items)):
            order = np.argsort(rows, kind="stable")
            indptr = np.zeros(n_rows + 1, dtype=np.int64)
            np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
            ws = capi.als_solve_workspace_bytes(indptr, self.ld)
            self.halves.append(dict(n=n_rows, indptr=indptr, d_indptr=DeviceBuffer.from_numpy(indptr),
                                    d_indices=DeviceBuffer.from_numpy(np.ascontiguousarray(cols[order], dtype=np.int32)),
                                    d_c=DeviceBuffer.from_numpy(np.ascontiguousarray(c[order])), ws_bytes=ws))
        self.ws_bytes = max(h["ws_bytes"] for h in self.halves)
        self.d_ws = DeviceBuffer((max(self.ws_bytes, 256),), np.uint8)
        self.gram_ws_bytes = capi.als_gram_workspace_bytes(max(n_users, n_items), self.ld)
        self.d_gram_ws = DeviceBuffer((self.gram_ws_bytes,), np.uint8)
        self.d_G = DeviceBuffer((self.ld, self.ld), np.float64)
        self.d_loss = DeviceBuffer.zeros((1,), np.float64)

    def half(self, side: int, with_loss: bool, stream=None):
        """side 0: solve the users' rows of X against Y; 1: the items' rows of Y against X"""
        h = self.halves[side]
        F, X = (self.t.Q, self.t.P) if side == 0 else (self.t.P, self.t.Q)
        f_rows = self.halves[1 - side]["n"]
        capi.als_gram(F, f_rows, self.d, self.ld, self.d_G, self.d_gram_ws, self.gram_ws_bytes, stream)
        capi.als_solve_rows(F, f_rows, self.d_G, X, h["n"], self.d, self.ld, h["d_indptr"], h["d_indices"], h["d_c"], self.lam,
                            self.d_loss if with_loss else None, self.d_ws, self.ws_bytes, stream)

    def epoch(self, stream=None) -> float:
        self.half(0, True, stream)
        self.half(1, False, stream)
        return float(self.d_loss.numpy(stream)[0])

    def download(self):
        """(X, Y) as fp64 host arrays [rows, d]"""
        return self.t.download(np.float64)



def _csr_by(rows: np.ndarray, cols: np.ndarray, n_rows: int):
    """(indptr int64, indices int32) of the pairs grouped by row, columns ascending within a row"""
    order = np.lexsort((cols, rows))
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=indptr[1:])
    return indptr, np.ascontiguousarray(cols[order], dtype=np.int32)


class ExposureSolver:
    """Exposure-weighted ALS (model/ranking/ExpoMF.py, model/ranking/SERec.py) with everything resident on the device: theta
    (users) and beta (items) in one fp64 ``DeviceTables`` (P = theta, Q = beta), the observed pairs by user and by item, the
    prior state and the workspaces.  ``epoch()`` solves every user's row, then every item's row against the new theta, then
    updates the prior with the new tables (the old prior enters that pass's posterior).

    The prior: ExpoMF keeps one mu per item.  SERec (``t`` given: followee counts per user) starts from the constant
    ``mu0`` and afterwards keeps ``A_sum`` per item; mu[u, i] = m(t[u], A_sum[i]) is formed inside the kernels, so no
    users x items array exists.  The reference picks the item half's prior branch by comparing sizes (ExpoMF.py:104,
    SERec.py:141); with as many users as items it takes the user branch for the items too, and so does this class.
    Every sum has a fixed order: two runs from the same state are bit-identical."""

    def __init__(self, theta: np.ndarray, beta: np.ndarray, uid: np.ndarray, iid: np.ndarray, lam: float, lam_y: float,
                 mu0: float = float(np.float32(0.01)), a: float = 1.0, b: float = 99.0, s: float = 2.2, t: np.ndarray | None = None):
        self.n_users, self.n_items = theta.shape[0], beta.shape[0]
        self.t = DeviceTables(theta, beta, np.float64)
        self.d, self.ld, self.lam, self.lam_y = self.t.d, self.t.ld, float(lam), float(lam_y)
        self.a, self.b, self.s = float(a), float(b), float(s)
        u = np.asarray(uid, dtype=np.int64); i = np.asarray(iid, dtype=np.int64)
        self.by_user = [DeviceBuffer.from_numpy(x) for x in _csr_by(u, i, self.n_users)]
        self.by_item = [DeviceBuffer.from_numpy(x) for x in _csr_by(i, u, self.n_items)]
        self.social = t is not None
        self.d_mu = DeviceBuffer.from_numpy(np.full(self.n_items, mu0, dtype=np.float64))
        self.d_t = DeviceBuffer.from_numpy(np.ascontiguousarray(t, dtype=np.float64)) if self.social else None
        self.d_asum = DeviceBuffer.zeros((max(self.n_items, 1),), np.float64)
        self.has_asum = False           # SERec: mu is the constant mu0 until the first prior update
        self.ws_bytes = max(capi.expo_solve_workspace_bytes(self.n_users, self.ld), capi.expo_solve_workspace_bytes(self.n_items, self.ld))
        self.d_ws = DeviceBuffer((self.ws_bytes,), np.uint8)
        self.prior_ws_bytes = capi.expo_prior_workspace_bytes(self.n_users, self.n_items)
        self.d_prior_ws = DeviceBuffer((self.prior_ws_bytes,), np.uint8)

    def _prior(self, half: str):
        """the prior descriptor of a pass: half in ("user", "item", "expo")"""
        same = self.n_users == self.n_items              # the reference's size test picks the user branch (see the class doc)
        if self.social and self.has_asum:
            mode = capi.EXPO_PRIOR_SOCIAL_T_COL if half == "item" and not same else capi.EXPO_PRIOR_SOCIAL_T_ROW
        else:
            mode = capi.EXPO_PRIOR_ROW if half == "item" and not same else capi.EXPO_PRIOR_COL
        return capi.expo_prior_desc(mode, self.lam_y, v=self.d_mu, t=self.d_t, a_sum=self.d_asum, a=self.a, b=self.b, s=self.s,
                                    n_users=self.n_users)

    def half(self, side: int, stream=None):
        """side 0: every user's row of theta against beta; 1: every item's row of beta against theta"""
        F, X, n_cols, n_rows, csr = ((self.t.Q, self.t.P, self.n_items, self.n_users, self.by_user) if side == 0 else
                                     (self.t.P, self.t.Q, self.n_users, self.n_items, self.by_item))
        capi.expo_solve_rows(F, n_cols, X, n_rows, self.d, self.ld, csr[0], csr[1], self._prior("user" if side == 0 else "item"),
                             self.lam, self.d_ws, self.ws_bytes, stream)

    def update_prior(self, stream=None):
        """A_sum[i] = sum_u A_ui with the new tables and the old prior; ExpoMF's mu, or SERec's A_sum, from it"""
        capi.expo_prior(self.t.P, self.n_users, self.t.Q, self.n_items, self.d, self.ld, self.by_item[0], self.by_item[1],
                        self._prior("expo"), self.d_asum, None if self.social else self.d_mu, self.d_prior_ws, self.prior_ws_bytes,
                        stream)
        self.has_asum = True

    def epoch(self, stream=None):
        self.half(0, stream)
        self.half(1, stream)
        self.update_prior(stream)

    def prior_state(self):
        """ExpoMF: mu per item.  SERec: (t per user, A_sum per item), or (t, None) while mu is still the constant mu0."""
        if not self.social:
            return self.d_mu.numpy()[:self.n_items].copy()
        return self.d_t.numpy().copy(), (self.d_asum.numpy()[:self.n_items].copy() if self.has_asum else None)

    def download(self):
        """(theta, beta, prior) as fp64 host arrays; prior as in ``prior_state``"""
        theta, beta = self.t.download(np.float64)
        return theta, beta, self.prior_state()


def serec_mu(t: np.ndarray, a_sum: np.ndarray, n_users: int, a: float = 1.0, b: float = 99.0, s: float = 2.2) -> np.ndarray:
    """SERec's prior mu[u, i] for the users t covers (SERec.py:92-95, T.dot(tile(A_sum)) = t_u A_i): [len(t), len(a_sum)]"""
    S = np.asarray(t, dtype=np.float64)[:, None] * np.asarray(a_sum, dtype=np.float64)[None, :]
    return (a + a_sum[None, :] + (s - 1) * S - 1) / (a + b + (s - 1) * S + n_users - 2)

def _take_rows(csr: CSR, rows: np.ndarray):
    """(indptr, indices, values) of the CSR's rows ``rows`` (-1: an empty row), in that order"""
    rows = np.asarray(rows, dtype=np.int64)
    lens = np.where(rows >= 0, np.diff(csr.indptr)[np.maximum(rows, 0)] if csr.n_rows else 0, 0).astype(np.int64)
    indptr = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    starts = np.where(rows >= 0, csr.indptr[np.maximum(rows, 0)] if csr.n_rows else 0, 0)
    src = np.repeat(starts - indptr[:-1], lens) + np.arange(indptr[-1], dtype=np.int64)
    return indptr, np.ascontiguousarray(csr.indices[src], dtype=np.int32), np.ascontiguousarray(csr.values[src], dtype=np.float64)


def _inverted(csr: CSR, n_keys: int, label_of: np.ndarray):
    """key -> (label of the row, value), labels ascending within a key: the sweep's candidate side"""
    lab = label_of[csr.row_ids()].astype(np.int32)
    order = np.lexsort((lab, csr.indices))
    indptr = np.zeros(n_keys + 1, dtype=np.int64)
    np.cumsum(np.bincount(csr.indices, minlength=n_keys), out=indptr[1:])
    return indptr, np.ascontiguousarray(lab[order]), np.ascontiguousarray(csr.values[order], dtype=np.float64)


def libm_squares(x: np.ndarray) -> np.ndarray:
    """``v ** 2`` of every element as Python computes it: the C library's pow(v, 2.0), which is not always the correctly
    rounded v * v that the device (or numpy's square) would give -- the reference's similarities square this way
    (util/qmath.py:25-27,57-60), so the kernels take these squares as inputs"""
    return np.fromiter((v ** 2 for v in np.asarray(x, dtype=np.float64).tolist()), dtype=np.float64, count=np.size(x))


def _dev(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return DeviceBuffer.from_numpy(a) if a.size else DeviceBuffer((1,), dtype)


class CoRatingKnn:
    """Neighbourhood of UserKNN / ItemKNN (model/rating/{UserKNN,ItemKNN}.py, util/qmath.py:19-115) on the device.

    ``rows`` is the candidates' CSR in the reference's dict order (users -> items for UserKNN, items -> users for ItemKNN),
    ``means`` their means, ``query_ids`` the candidate id of every query (test user / test item, in testSet order) or -1.
    The queries that are candidates get the labels 0 .. m - 1 in query order, the other candidates m .. in id order, so that
    the query x query block of the similarity rows is contiguous.  ``run()`` sweeps every query row (``S[t][label]``, all rows
    resident) and takes each query's first ``k`` neighbours by the reference's candidate sequence;
    ``predict()`` walks them for a batch of test rows."""

    def __init__(self, measure: int, rows: CSR, n_keys: int, means: np.ndarray, query_ids: np.ndarray, k: int):
        if k > capi.KNN_MAX_K:
            raise ValueError(f"num.neighbors = {k} is above the supported maximum of {capi.KNN_MAX_K}")
        if k < 1:
            raise ValueError(f"num.neighbors = {k} must be at least 1")
        self.measure, self.k = int(measure), int(k)
        self.n_cands, self.n_keys = rows.n_rows, int(n_keys)
        q = np.asarray(query_ids, dtype=np.int64)
        self.n_queries = int(q.size)
        in_q = q[q >= 0]
        self.m = int(in_q.size)
        rest = np.setdiff1d(np.arange(self.n_cands, dtype=np.int64), in_q, assume_unique=True)
        self.lab2id = np.concatenate([in_q, rest]).astype(np.int32)
        self.id2lab = np.empty(self.n_cands, dtype=np.int32)
        self.id2lab[self.lab2id] = np.arange(self.n_cands, dtype=np.int32)
        self.q_label = np.where(q >= 0, self.id2lab[np.maximum(q, 0)] if self.n_cands else -1, -1).astype(np.int32)
        self.test_code = np.where(q >= 0, q, -1 - np.arange(q.size)).astype(np.int32)
        means = np.asarray(means, dtype=np.float64)
        q_indptr, q_keys, q_vals = _take_rows(rows, q)
        c_indptr, c_labels, c_vals = _inverted(rows, self.n_keys, self.id2lab)
        s_bytes = self.n_queries * self.n_cands * 8
        self.ws_bytes = capi.knn_topk_workspace_bytes(self.n_queries, self.m)
        hbm = capi.device_info()["hbm_bytes"]
        need = s_bytes + self.ws_bytes + 3 * (rows.nnz * 12 + self.n_cands * 16)
        if need > 0.9 * hbm:
            raise MemoryError(f"the similarity rows of {self.n_queries} queries x {self.n_cands} candidates and the transposed query "
                              f"block need {need / 2**30:.1f} GiB; the device has {hbm / 2**30:.1f} GiB")
        q_means = np.where(q >= 0, means[np.maximum(q, 0)] if means.size else 0.0, 0.0)
        c_means = means[self.lab2id]
        if self.measure == capi.KNN_PCC:
            q_sq = libm_squares(q_vals - np.repeat(q_means, np.diff(q_indptr)))
            c_sq = libm_squares(c_vals - c_means[c_labels])
        else:
            q_sq, c_sq = libm_squares(q_vals), libm_squares(c_vals)
        self.d_q = [_dev(q_indptr, np.int64), _dev(q_keys, np.int32), _dev(q_vals, np.float64), _dev(q_means, np.float64),
                    _dev(q_sq, np.float64)]
        self.d_c = [_dev(c_indptr, np.int64), _dev(c_labels, np.int32), _dev(c_vals, np.float64), _dev(c_sq, np.float64),
                    _dev(c_means, np.float64)]
        self.d_S = DeviceBuffer((max(self.n_queries, 1), max(self.n_cands, 1)), np.float64)
        self.d_ws = DeviceBuffer((self.ws_bytes,), np.uint8)
        self.d_q_label, self.d_test_code, self.d_lab2id = _dev(self.q_label, np.int32), _dev(self.test_code, np.int32), _dev(self.lab2id, np.int32)
        self.d_ids = DeviceBuffer((max(self.n_queries, 1), self.k), np.int32)
        self.d_vals = DeviceBuffer((max(self.n_queries, 1), self.k), np.float64)
        self.d_counts = DeviceBuffer.zeros((max(self.n_queries, 1),), np.int32)

    def sweep(self, stream=None):
        capi.knn_sweep(self.measure, self.n_queries, *self.d_q, self.n_keys, *self.d_c[:4], self.n_cands, self.d_c[4], self.d_S,
                       max(self.n_cands, 1), None, 0, stream)

    def topk(self, stream=None):
        if self.n_cands:
            capi.knn_topk(self.n_queries, self.d_S, self.n_cands, self.m, self.d_q_label, self.d_test_code, self.d_lab2id, self.n_cands,
                          self.k, self.d_ids, self.d_vals, self.d_counts, self.d_ws, self.ws_bytes, stream)

    def run(self, stream=None):
        self.sweep(stream)
        self.topk(stream)

    def similarities(self, queries=None) -> np.ndarray:
        """S[t][candidate id] = similarity(row of query t, row of the candidate), query t's row being x1 -- for the given query
        indices (default: all), as fp64 [len, n_cands]"""
        queries = np.arange(self.n_queries) if queries is None else np.asarray(queries, dtype=np.int64)
        out = np.empty((queries.size, self.n_cands), dtype=np.float64)
        for a, t in enumerate(queries.tolist()):
            out[a] = self.d_S.read_rows(int(t), 1)[0][self.id2lab]
        return out

    def neighbours(self):
        """(ids [n_queries, k] -- candidate id, or -1 - s for the query s that is no candidate --, similarities, counts)"""
        n = self.n_queries
        counts = self.d_counts.numpy()[:n]
        return self.d_ids.numpy()[:n], self.d_vals.numpy()[:n], counts

    def predict(self, mode: int, row_query, row_other, row_base, members: CSR, nb_means, stream=None):
        """(pred, status) of test rows: mode 0 (UserKNN) looks up item row_other in each neighbour's row of ``members`` (users'
        ratings, items ascending), mode 1 (ItemKNN) each neighbour item in user row_other's row"""
        n = int(np.asarray(row_query).size)
        if n == 0:
            return np.zeros(0), np.zeros(0, np.int32)
        d_pred, d_status = DeviceBuffer((n,), np.float64), DeviceBuffer((n,), np.int32)
        nb_means = np.asarray(nb_means, dtype=np.float64)
        capi.knn_predict(mode, n, _dev(row_query, np.int32), _dev(row_other, np.int32), _dev(row_base, np.float64), self.d_ids,
                         self.d_vals, self.d_counts, self.n_queries, self.k, members.n_rows, _dev(members.indptr, np.int64),
                         _dev(members.indices, np.int32), _dev(members.values, np.float64), nb_means.size, _dev(nb_means, np.float64),
                         d_pred, d_status, stream)
        return d_pred.numpy(stream), d_status.numpy(stream)


class SlopeOneSolver:
    """SlopeOne (model/rating/SlopeOne.py) on the device: test items in batches; per batch the deviation rows
    ``diffAverage[i][j]`` / ``freq[i][j]`` of every training item j are swept into a scratch buffer and the test rows of the
    batch's items predicted from it.  The full table is never kept."""

    def __init__(self, item_rows: CSR, user_rows: CSR, query_items: np.ndarray, batch: int | None = None):
        self.n_items, self.n_users = item_rows.n_rows, user_rows.n_rows
        q = np.asarray(query_items, dtype=np.int64)
        self.n_queries = int(q.size)
        if batch is None:           # about 1 GiB of scratch
            batch = max(1, min(self.n_queries, (1 << 30) // max(12 * self.n_items, 1)))
        self.batch = int(batch)
        self.d_q = [_dev(a, t) for a, t in zip(_take_rows(item_rows, q), (np.int64, np.int32, np.float64))]
        srt = user_rows.sorted_rows()
        self.d_us = [_dev(srt.indptr, np.int64), _dev(srt.indices, np.int32), _dev(srt.values, np.float64)]
        self.d_u = [_dev(user_rows.indptr, np.int64), _dev(user_rows.indices, np.int32), _dev(user_rows.values, np.float64)]
        self.ws_bytes = capi.slopeone_workspace_bytes(self.batch, self.n_items)
        self.d_ws = DeviceBuffer((self.ws_bytes,), np.uint8)

    def predict(self, row_query, row_user, row_base, stream=None):
        n = int(np.asarray(row_query).size)
        d_pred, d_status = DeviceBuffer((max(n, 1),), np.float64), DeviceBuffer((max(n, 1),), np.int32)
        d_rq, d_ru, d_rb = _dev(row_query, np.int32), _dev(row_user, np.int32), _dev(row_base, np.float64)
        for q0 in range(0, self.n_queries, self.batch):
            nq = min(self.batch, self.n_queries - q0)
            capi.slopeone_batch(q0, nq, *self.d_q, self.n_users, *self.d_us, self.n_items, n, d_rq, d_ru, d_rb, *self.d_u, d_pred,
                                d_status, self.d_ws, self.ws_bytes, stream)
        return d_pred.numpy(stream)[:n], d_status.numpy(stream)[:n]

    def deviations(self, q0: int, nq: int, stream=None):
        """(diffAverage [nq, n_items], freq [nq, n_items]) of queries [q0, q0 + nq): one batch swept, nothing predicted"""
        ws = capi.slopeone_workspace_bytes(nq, self.n_items)
        d_ws = DeviceBuffer((ws,), np.uint8)
        capi.slopeone_batch(q0, nq, *self.d_q, self.n_users, *self.d_us, self.n_items, 0, None, None, None, *self.d_u, None, None,
                            d_ws, ws, stream)
        raw = d_ws.numpy(stream)
        dev = raw[:nq * self.n_items * 8].view(np.float64).reshape(nq, self.n_items)
        freq = raw[nq * self.n_items * 8: nq * self.n_items * 12].view(np.int32).reshape(nq, self.n_items)
        return dev.copy(), freq.copy()


# ---- CoFactor (cofactor.hip) ------------------------------------------------------------------------------------------------
def sppmi_from_counts(indptr: np.ndarray, cols: np.ndarray, counts: np.ndarray, neg: int):
    """The SPPMI matrix of model/ranking/CoFactor.py:58-81 from the kept co-occurrence counts (CSR by item id, columns
    ascending): ``(ptr, idx, val)``, row i = the dict ``SPPMI[i]`` in its insertion order -- the order in which the item step
    adds its context terms.  Host code, O(nnz log nnz).

    The reference walks ``occurrence`` in the order its keys were first touched: item x at its own turn of the pair loop,
    or earlier, as the partner of its smallest kept neighbour a < x (during a's turn, after a itself and in ascending x).
    Walking item a in that order it visits a's partners b in ascending id and inserts b into SPPMI[a] and a into SPPMI[b]
    when the value is positive; the second visit of a pair finds both present.  So row x holds first the partners walked
    before x (in walk order), then the others in ascending id.  Values: ``max(log(count * D / (f_a * f_b)) - log(neg), 0)``
    with the C library's log (math.log, as the reference calls it), divided once by the largest."""
    import math
    n = indptr.size - 1
    deg = np.diff(indptr)
    rows = np.repeat(np.arange(n, dtype=np.int64), deg)
    cols = np.asarray(cols, dtype=np.int64)
    freq = np.bincount(rows, weights=np.asarray(counts, dtype=np.float64), minlength=n)      # integer-valued sums: exact
    D = float(freq.sum())
    empty = (np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64))
    if cols.size == 0:
        return empty
    upper = rows < cols
    arg = (np.asarray(counts, dtype=np.float64)[upper] * D) / (freq[rows[upper]] * freq[cols[upper]])
    log_neg = math.log(neg)
    pmi = np.fromiter((math.log(x) - log_neg for x in arg.tolist()), dtype=np.float64, count=arg.size)
    keep = pmi > 0
    if not keep.any():
        return empty
    a, b, v = rows[upper][keep], cols[upper][keep], pmi[keep] / pmi[keep].max()
    # the walk order of ``occurrence``'s keys, from the full counts
    has = np.flatnonzero(deg > 0)
    first = cols[indptr[has]]
    early = first < has
    walk = has[np.lexsort((np.where(early, has, -1), np.where(early, first, has)))]
    rank = np.full(n, n, dtype=np.int64)
    rank[walk] = np.arange(walk.size)
    x, y, val = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([v, v])
    before = rank[y] < rank[x]
    order = np.lexsort((np.where(before, rank[y], y), ~before, x))
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(x, minlength=n), out=ptr[1:])
    return ptr, np.ascontiguousarray(y[order], dtype=np.int32), np.ascontiguousarray(val[order])


class CoOccurrence:
    """Item-item co-occurrence of CoFactor (model/ranking/CoFactor.py:36-56) on the device and its SPPMI matrix.

    ``uid`` / ``iid``: the training pairs (duplicates count once).  ``counts()`` runs the two passes of cofactor.hip -- count
    the kept pairs (count > filt between items with >= filt raters), then fill a CSR allocated for exactly that many
    (``capacity``: refuse, with nothing written, when there are more) -- and ``sppmi(neg)`` finishes on the host
    (:func:`sppmi_from_counts`).  ``timings`` holds the milliseconds of the count / fill / host parts of the last run."""

    def __init__(self, uid: np.ndarray, iid: np.ndarray, n_users: int, n_items: int, filt: int, capacity: int | None = None):
        key = np.unique(np.asarray(uid, dtype=np.int64) * n_items + np.asarray(iid, dtype=np.int64))
        u, i = key // n_items, key % n_items
        self.n_users, self.n_items, self.filt, self.capacity, self.nnz = int(n_users), int(n_items), int(filt), capacity, int(key.size)
        u_indptr, u_items = _csr_by(u, i, n_users)
        i_indptr, i_users = _csr_by(i, u, n_items)
        self.d_u_indptr, self.d_u_items = _dev(u_indptr, np.int64), _dev(u_items, np.int32)
        self.d_i_indptr, self.d_i_users = _dev(i_indptr, np.int64), _dev(i_users, np.int32)
        self.ws_bytes = capi.cooc_workspace_bytes(n_items)
        self.d_ws = DeviceBuffer((self.ws_bytes,), np.uint8)
        self.timings = {}

    def counts(self, stream=None):
        """(indptr int64 [n_items + 1], cols int32, counts int32) of the kept pairs, columns ascending"""
        from time import perf_counter
        views = (self.d_i_indptr, self.d_i_users, self.n_items, self.nnz, self.d_u_indptr, self.d_u_items, self.n_users, self.nnz, self.filt)
        t0 = perf_counter()
        kept = capi.cooc_count(*views, self.d_ws, self.ws_bytes, stream)
        t1 = perf_counter()
        cap = kept if self.capacity is None else int(self.capacity)
        d_indptr = DeviceBuffer((self.n_items + 1,), np.int64)
        d_cols, d_counts = DeviceBuffer((max(cap, 1),), np.int32), DeviceBuffer((max(cap, 1),), np.int32)
        t2 = perf_counter()
        capi.cooc_fill(*views, d_indptr, d_cols, d_counts, cap, self.d_ws, self.ws_bytes, stream)
        t3 = perf_counter()
        self.kept = kept
        self.timings.update(count_ms=(t1 - t0) * 1e3, fill_ms=(t3 - t2) * 1e3)
        return d_indptr.numpy(stream), d_cols.head(kept, stream), d_counts.head(kept, stream)

    def sppmi(self, neg: int, stream=None):
        from time import perf_counter
        indptr, cols, counts = self.counts(stream)
        t0 = perf_counter()
        out = sppmi_from_counts(indptr, cols, counts, neg)
        self.timings["host_ms"] = (perf_counter() - t0) * 1e3
        return out


def cofactor_schedule(ptr: np.ndarray, idx: np.ndarray):
    """The level schedule of CoFactor's item sweep: step k is the k-th item with contexts (ascending id = ``data.item``
    order); it reads the rows of its contexts and writes its own, so level(i) = 1 + max level(earlier context).
    Returns (order: item ids level by level, level_ptr)."""
    from .social import level_schedule
    n = ptr.size - 1
    ctx = np.flatnonzero(np.diff(ptr) > 0)
    read_ptr = np.zeros(ctx.size + 1, dtype=np.int64)
    np.cumsum(np.diff(ptr)[ctx], out=read_ptr[1:])
    sched = level_schedule(n, read_ptr, idx, np.arange(ctx.size + 1, dtype=np.int64), ctx)
    return np.ascontiguousarray(ctx[sched.order], dtype=np.int32), np.ascontiguousarray(sched.level_ptr, dtype=np.int32)


class CoFactorSolver:
    """CoFactor's training (model/ranking/CoFactor.py:84-162) with every table resident in fp64: X, Y (an ``AlsSolver``:
    the user half is WRMF's), the context embeddings G and the biases w, c, the SPPMI CSR in the reference's neighbour
    order and the level schedule of the item sweep.  ``epoch()`` = Y^T Y, the user half with the loss, X^T X, the item
    half (cofactor.hip); it returns the loss.  Every sum has a fixed order: two runs are bit-identical."""

    def __init__(self, X, Y, G, w, c, uid, iid, rating, sppmi, lam: float, gamma: float, alpha: float = 10.0):
        self.als = AlsSolver(X, Y, uid, iid, rating, lam, alpha)
        t = self.als.t
        self.d, self.ld, self.lam, self.gamma = t.d, t.ld, float(lam), float(gamma)
        self.n_users, self.n_items = t.n_users, t.n_items
        self.d_Gt = DeviceBuffer.from_numpy(t._pad(np.asarray(G, dtype=np.float64)))
        self.d_w, self.d_c = _dev(w, np.float64), _dev(c, np.float64)
        ptr, idx, val = sppmi
        assert ptr.size == self.n_items + 1
        self.s_nnz = int(idx.size)
        self.d_s_ptr, self.d_s_idx, self.d_s_val = _dev(ptr, np.int64), _dev(idx, np.int32), _dev(val, np.float64)
        order, self.level_ptr = cofactor_schedule(ptr, idx)
        solo = np.flatnonzero(np.diff(ptr) == 0)
        self.n_ctx, self.n_solo = int(order.size), int(solo.size)
        self.d_order, self.d_solo = _dev(order, np.int32), _dev(solo, np.int32)
        widths = np.diff(self.level_ptr)
        self.schedule = dict(depth=int(widths.size), max_width=int(widths.max()) if widths.size else 0, items=self.n_ctx,
                             entries=self.s_nnz, longest_row=int(np.diff(ptr).max()) if self.n_items else 0)
        self.item_ws_bytes = capi.cofactor_item_workspace_bytes(self.n_items, self.n_ctx, self.ld)
        self.d_item_ws = DeviceBuffer((self.item_ws_bytes,), np.uint8)
        self.timings = {}

    def item_half(self, stream=None):
        a, h = self.als, self.als.halves[1]
        capi.als_gram(a.t.P, self.n_users, self.d, self.ld, a.d_G, a.d_gram_ws, a.gram_ws_bytes, stream)
        capi.cofactor_item_rows(a.t.P, self.n_users, a.d_G, a.t.Q, self.d_Gt, self.d_w, self.d_c, self.n_items, self.d, self.ld,
                                h["d_indptr"], h["d_indices"], h["d_c"], int(h["indptr"][-1]), self.d_s_ptr, self.d_s_idx, self.d_s_val,
                                self.s_nnz, self.d_order, self.level_ptr, self.d_solo, self.n_solo, self.lam, self.gamma,
                                self.d_item_ws, self.item_ws_bytes, stream)

    def epoch(self, stream=None) -> float:
        from time import perf_counter
        t0 = perf_counter()
        self.als.half(0, True, stream)
        loss = float(self.als.d_loss.numpy(stream)[0])
        t1 = perf_counter()
        self.item_half(stream)
        self.timings.update(user_half_ms=(t1 - t0) * 1e3, item_half_ms=(perf_counter() - t1) * 1e3)
        return loss

    def download(self):
        """(X, Y, G, w, c) as fp64 host arrays"""
        X, Y = self.als.download()
        return X, Y, np.ascontiguousarray(self.d_Gt.numpy()[:, :self.d]), self.d_w.head(self.n_items), self.d_c.head(self.n_items)
