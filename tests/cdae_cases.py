"""The recorded CDAE run (tests/golden/tf_cdae_filmtrust.npz) as inputs -- batches in dense and list form, start values, bounds --
and the synthetic kernel cases; shared by tests/test_cdae_cpu.py and tests/test_gpu_cdae.py."""
import functools
import json
import os

import numpy as np

import cdae_mirror as M
from helpers import GOLDEN, rel_err

GRAD_TOL = 1e-5         # the project's bar: 1e-5 relative Frobenius on fp32 quantities
FLOOR_FACTOR = 2.5      # as tests/diffusion_cases.py: two independent float32 roundings of one computation are sqrt(2) apart in expectation
NAME = "tf_cdae_filmtrust"
META = json.load(open(os.path.join(GOLDEN, "golden_tf_cdae.json")))[NAME]
YARD = np.load(os.path.join(GOLDEN, "tf_cdae_f64_yardstick.npz"))
VARS = M.VARS


@functools.lru_cache(None)
def load():
    return np.load(os.path.join(GOLDEN, NAME + ".npz"))


def floor_of(key, z):
    """distance of the reference's own float32 run from the same run in float64, computed from the two committed files"""
    return rel_err(z[key], YARD[f"{NAME}/{key}"].reshape(z[key].shape))


def trained_bound(key, z):
    return max(GRAD_TOL, FLOOR_FACTOR * floor_of(key, z))


def initial(z=None):
    z = load() if z is None else z
    return {v: z[f"init_{v}"] for v in VARS}


def ratings_matrix(z=None):
    z = load() if z is None else z
    R = np.zeros((META["n_users"], META["n_items"]), np.float32)
    R[z["train_uid"], z["train_iid"]] = z["train_r"]
    return R


@functools.lru_cache(None)
def dense_batches():
    """per recorded step (users, X, positive, negative, mask) as the reference fed them"""
    z = load()
    shape = (META["n_steps"], META["batch_size"], META["n_items"])
    bits = lambda k: np.unpackbits(z[k])[:int(np.prod(shape))].reshape(shape)
    pos, neg, mask = bits("positive_bits"), bits("negative_bits"), bits("mask_corruption_bits")
    R = ratings_matrix(z)
    return [(z["u_idx"][k], R[z["u_idx"][k]], pos[k], neg[k], mask[k]) for k in range(shape[0])]


@functools.lru_cache(None)
def list_batches():
    from qrec_amd.autoencoder import lists_from_dense
    return [lists_from_dense(*b) for b in dense_batches()]


@functools.lru_cache(None)
def mirror_run_f64():
    """the float64 sparse mirror over the recorded batches: (parameters, losses, first-step gradients) -- computed once"""
    return M.train(initial(), list_batches(), META["lr"], META["regU"], np.float64)


def train_test_lists(z=None):
    """the recorded split as the [user, item, rating] rows a drop-in class takes; names are u<id> / i<id>, test items the training
    set does not know are named x<k>"""
    z = load() if z is None else z
    train = [[f"u{u}", f"i{i}", float(r)] for u, i, r in zip(z["train_uid"].tolist(), z["train_iid"].tolist(), z["train_r"].tolist())]
    test = [[f"u{u}" if u >= 0 else f"w{k}", f"i{i}" if i >= 0 else f"x{k}", 1.0]
            for k, (u, i) in enumerate(zip(z["test_uid"].tolist(), z["test_iid"].tolist()))]
    return train, test


# ---- synthetic kernel cases -------------------------------------------------------------------------------------------------------
N_ITEMS = 1003
N_USERS = 300
EVERY_ROW_ITEM = 7            # live in every row that has a live slot (a positive in rows 1 and 2, a negative elsewhere)
DEAD_ITEMS = (0, 500, 1002)   # live in no row, kept as input in none: their gradient rows must be exactly zero
SATURATED_ITEM = 11           # its decoder row and bias put every logit at -15: the 1e-6 clamp and its zero gradient
# row kinds: (kept inputs, live slots).  A kept rated item IS a live positive (CDAE.py:76), so live >= kept.
ROW_KINDS = ((0, 0), (1, 1), (700, 760), (10, 63), (10, 64), (10, 65), (20, 569), (0, 30))
ROWS_OF = {1: (6,), 5: (0, 1, 2, 3, 4)}        # B = 64: all eight kinds, then rows of 2..40 kept inputs and five times as many negatives


def kernel_case(nh, B, seed=0):
    """(parameters, BatchLists, reg) with the list shapes the kernels can go wrong on: an empty row, a row with one kept input and one
    live slot, 700 kept inputs, live counts 63 / 64 / 65 / 569, a row with live slots and no kept input, the same user in rows 1, 3
    and 4, one item live in every non-empty row and three in none, a saturated slot as a positive (row 2) and as a negative, and in
    every row some rated items and negatives the mask drops."""
    from qrec_amd.autoencoder import lists_from_entries
    rng = np.random.default_rng([nh, B, seed])
    lim = np.sqrt(6.0 / (N_ITEMS + nh))
    p = dict(W_enc=rng.uniform(-lim, lim, (N_ITEMS, nh)), W_dec=rng.uniform(-lim, lim, (nh, N_ITEMS)),
             b_enc=rng.uniform(-0.3, 0.3, nh), b_dec=rng.uniform(-0.05, 0.05, N_ITEMS), V=rng.uniform(-0.1, 0.1, (N_USERS, nh)))
    p["W_dec"][:, SATURATED_ITEM] = 0.0; p["b_dec"][SATURATED_ITEM] = -15.0
    p = {k: v.astype(np.float32) for k, v in p.items()}
    users = rng.integers(0, N_USERS, B).astype(np.int32)
    if B >= 5:
        users[3] = users[4] = users[1]
    usable = np.setdiff1d(np.arange(N_ITEMS), np.array(DEAD_ITEMS + (EVERY_ROW_ITEM, SATURATED_ITEM)))
    kinds = ROWS_OF.get(B, tuple(range(len(ROW_KINDS))) + (None,) * (B - len(ROW_KINDS)))
    pr, pi, nr, ni, dropped = [], [], [], [], set()
    for b, kind in enumerate(kinds):
        if kind is None:
            n_in = int(rng.integers(2, 41)); n_live = 6 * n_in
        else:
            n_in, n_live = ROW_KINDS[kind]
        items = rng.permutation(usable).tolist()
        pos, neg = [], []
        if n_in:                                   # the shared item (and in the long row the saturated one) among the positives
            pos = [EVERY_ROW_ITEM] + ([SATURATED_ITEM] if n_in >= 700 else [])
            pos += [items.pop() for _ in range(n_in - len(pos))]
        if n_live > n_in:
            neg = ([] if n_in else [EVERY_ROW_ITEM]) + ([SATURATED_ITEM] if n_in < 700 and n_live - n_in >= 2 else [])
            neg += [items.pop() for _ in range(n_live - n_in - len(neg))]
        gone_p, gone_n = [items.pop() for _ in range(3)], [items.pop() for _ in range(4)]       # rated / sampled, mask = 0
        dropped.update((b, i) for i in gone_p + gone_n)
        pr += [b] * (len(pos) + 3); pi += pos + gone_p; nr += [b] * (len(neg) + 4); ni += neg + gone_n
    pr, pi, nr, ni = (np.array(a, np.int64) for a in (pr, pi, nr, ni))
    vals = rng.integers(1, 9, pr.size).astype(np.float32) / 2
    keep = lambda r, i: np.array([(int(a), int(c)) not in dropped for a, c in zip(r, i)], bool)
    L = lists_from_entries(users, N_ITEMS, pr, pi, vals, nr, ni, keep)
    for b, kind in enumerate(kinds):
        if kind is not None:
            assert (L.in_ptr[b + 1] - L.in_ptr[b], L.lv_ptr[b + 1] - L.lv_ptr[b]) == ROW_KINDS[kind], (b, kind)
    return p, L, 0.01
