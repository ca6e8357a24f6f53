"""The recorded CFGAN run (tests/golden/tf_cfgan_filmtrust.npz) as inputs -- batches in dense and list form, start values, bounds --
and the synthetic kernel cases; shared by tests/test_cfgan_cpu.py and tests/test_gpu_cfgan.py."""
import functools
import json
import os

import numpy as np

import cfgan_mirror as M
from helpers import GOLDEN, rel_err

GRAD_TOL = 1e-5         # the project's bar: 1e-5 relative Frobenius on fp32 quantities
FLOOR_FACTOR = 2.5      # as tests/cdae_cases.py: two independent float32 roundings of one computation are sqrt(2) apart in expectation
NAME = "tf_cfgan_filmtrust"
META = json.load(open(os.path.join(GOLDEN, "golden_tf_cfgan.json")))[NAME]
VARS = M.VARS
SPARSE = ("final_G_W1", "grad0_G_W1")


def _dense(z, key, idx, val):
    """final_G_W1 / grad0_G_W1 from their sparse form: init_G_W1 (resp. zero) everywhere but at the stored indices"""
    out = z["init_G_W1"].copy() if key == "final_G_W1" else np.zeros_like(z["init_G_W1"])
    out.ravel()[idx] = val
    return out


@functools.lru_cache(None)
def load():
    """the fixture as a dict, the two sparsely stored arrays dense"""
    z = dict(np.load(os.path.join(GOLDEN, NAME + ".npz")))
    for k in SPARSE:
        z[k] = _dense(z, k, z[k + "_idx"], z[k + "_val"])
    return z


@functools.lru_cache(None)
def yard():
    """the float64 run's trained variables, first-step gradients and losses, under the fixture's keys"""
    z, y = load(), np.load(os.path.join(GOLDEN, "tf_cfgan_f64_yardstick.npz"))
    out = {k.split("/")[1]: y[k] for k in y.files}
    for k in SPARSE:
        out[k] = _dense(z, k, z[k + "_idx"], out.pop(k + "_val"))
    return out


def floor_of(key, z=None):
    """distance of the reference's own float32 run from the same run in float64, computed from the two committed files"""
    z = load() if z is None else z
    return rel_err(z[key], yard()[key].reshape(z[key].shape))


def trained_bound(key, z=None):
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
    """per recorded epoch (users, C, mask, N_zr) as the reference fed them"""
    z = load()
    shape = (META["n_epochs"], META["batch_size"], META["n_items"])
    bits = lambda k: np.unpackbits(z[k])[:int(np.prod(shape))].reshape(shape)
    mask, zr = bits("mask_bits"), bits("N_zr_bits")
    R = ratings_matrix(z)
    return [(z["batch_uid"][k], R[z["batch_uid"][k]], mask[k], zr[k]) for k in range(shape[0])]


@functools.lru_cache(None)
def list_batches():
    from qrec_amd.autoencoder import cfgan_lists_from_dense
    return [cfgan_lists_from_dense(*b) for b in dense_batches()]


@functools.lru_cache(None)
def mirror_run_f64():
    """the float64 sparse mirror over the recorded batches: (parameters, d_losses, g_losses, first D gradients, first G gradients)"""
    return M.train(initial(), list_batches(), META["lr"], META["alpha"], np.float64)


def train_test_lists(z=None):
    """the recorded split as the [user, item, rating] rows a drop-in class takes; names are u<id> / i<id>, test items the training
    set does not know are named x<k>"""
    z = load() if z is None else z
    train = [[f"u{u}", f"i{i}", float(r)] for u, i, r in zip(z["train_uid"].tolist(), z["train_iid"].tolist(), z["train_r"].tolist())]
    test = [[f"u{u}" if u >= 0 else f"w{k}", f"i{i}" if i >= 0 else f"x{k}", 1.0]
            for k, (u, i) in enumerate(zip(z["test_uid"].tolist(), z["test_iid"].tolist()))]
    return train, test


# ---- synthetic kernel cases -------------------------------------------------------------------------------------------------------
# n_items below, at and across the 4-float vector width, the 32-float row padding and the sweep's 1024-column chunk
ITEM_COUNTS = (5, 33, 257, 1030)
BATCHES = (1, 5, 64)
N_USERS = 40
EVERY_ROW_ITEM = 1      # rated by every user, so by every batch row: its row of G_W1 takes a term from each of them, in batch-row order
UNRATED_ITEM = 2        # rated by nobody: its row of G_W1 has an exactly zero gradient
SATURATED_ITEM = 3      # rated by nobody and in every row's mask; G_b1 = 40 there: r_hat rounds to 1 and r_hat (1 - r_hat) is an exact 0
ALPHA = 0.01


def kernel_case(ni, B, seed=0):
    """(parameters, BatchLists) with the shapes the kernels can go wrong on: the same user in rows 1, 3 and 4 (B >= 5), an item every
    row rated and one no row rated, the last item rated by row 0's user and the last but one among the mask positions (columns in the
    sweep's second chunk at n_items = 1030), a user with more rated items and a row with more mask positions than a workgroup has
    threads (n_items = 1030), a saturated mask position in every row, row 0 with N_zr and mask disjoint (B >= 5) and the last row with
    a common position.  B = 1 has one row, so only the second of the two."""
    from qrec_amd.autoencoder import cfgan_lists
    rng = np.random.default_rng([ni, B, seed])
    special = {EVERY_ROW_ITEM, UNRATED_ITEM, SATURATED_ITEM}
    free = np.array([i for i in range(ni) if i not in special])
    rated = []
    for u in range(N_USERS):
        want = 300 if u == 1 and ni > 600 else int(rng.integers(0, min(free.size, 40) + 1))
        row = set(rng.permutation(free)[:min(want, free.size - 1)].tolist()) | {EVERY_ROW_ITEM}
        rated.append(row)
    rated[0].add(ni - 1)
    users = rng.integers(0, N_USERS, B).astype(np.int32)
    users[0] = 0
    if B >= 5:
        users[3] = users[4] = users[1] = 1
    pr, pi, mr, mi, zr, zi = [], [], [], [], [], []
    for n, u in enumerate(users):
        mine = sorted(rated[u])
        pr += [n] * len(mine); pi += mine
        unrated = np.array([i for i in range(ni) if i not in rated[u] and i != SATURATED_ITEM])
        rng.shuffle(unrated)
        n_mask = min(unrated.size // 2, 300 if n == B - 1 and ni > 600 else int(rng.integers(1, 30)))
        mask_neg, rest = unrated[:n_mask].tolist(), unrated[n_mask:]
        mask_neg.append(SATURATED_ITEM)
        if ni - 2 not in rated[u] and ni - 2 not in mask_neg:
            mask_neg.append(ni - 2)
            rest = rest[rest != ni - 2]
        zr_neg = rest[:int(rng.integers(0, 20))].tolist()            # row 0 (and some others): disjoint from the mask
        if n == B - 1 or (n > 0 and rng.random() < 0.5):
            zr_neg += mask_neg[:1 + int(rng.integers(0, 3))] + [SATURATED_ITEM]
        mr += [n] * len(mask_neg); mi += mask_neg; zr += [n] * len(zr_neg); zi += zr_neg
    vals = (rng.integers(1, 9, len(pr)) / 2).astype(np.float32)
    L = cfgan_lists(users, ni, np.array(pr), np.array(pi), vals, np.array(mr), np.array(mi), np.array(zr, np.int64), np.array(zi, np.int64))
    lim = np.sqrt(6.0 / (2 * ni))
    p = dict(G_W1=rng.uniform(-lim, lim, (ni, ni)), G_b1=rng.uniform(-0.05, 0.05, ni), D_W1=rng.uniform(-lim, lim, 2 * ni),
             D_b1=np.array([0.1]))
    p["G_b1"][SATURATED_ITEM] = 40.0
    p = {k: v.astype(np.float32) for k, v in p.items()}
    flags = [L.lv_label[L.lv_ptr[n]:L.lv_ptr[n + 1]] for n in range(B)]
    assert flags[-1].any() and (B == 1 or not flags[0].any())
    assert (np.diff(L.in_cptr)[EVERY_ROW_ITEM], np.diff(L.in_cptr)[UNRATED_ITEM]) == (B, 0)
    assert np.diff(L.lv_cptr)[SATURATED_ITEM] == B
    return p, L
