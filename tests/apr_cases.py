"""The recorded APR runs (tests/golden/tf_apr_filmtrust.npz: the reference file's feed; tf_apr_paper_filmtrust.npz: the paper's) as
inputs -- batches, start values, bounds -- and the synthetic kernel cases; shared by tests/test_apr_cpu.py and tests/test_gpu_apr.py."""
import functools
import json
import os

import numpy as np

from helpers import GOLDEN

TOL = 1e-5              # the project's bar, here on max |got - want| / max |want|
FLOOR_FACTOR = 2.5      # as tests/test_gpu_tf_golden.py: two independent float32 roundings of one computation are sqrt(2) apart in expectation
NAMES = dict(reference="tf_apr_filmtrust", paper="tf_apr_paper_filmtrust")
META = json.load(open(os.path.join(GOLDEN, "golden_tf_apr.json")))


def err(got, want) -> float:
    """max |got - want| / max |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300)) if got.size else 0.0


def bits_zero(a) -> bool:
    """every element +0.0, bit for bit"""
    a = np.ascontiguousarray(a, np.float32)
    return not a.view(np.uint32).any()


@functools.lru_cache(None)
def load(mode):
    return dict(np.load(os.path.join(GOLDEN, NAMES[mode] + ".npz")))


@functools.lru_cache(None)
def yard(mode):
    """the float64 run's moving arrays under the fixture's keys"""
    y = np.load(os.path.join(GOLDEN, "tf_apr_f64_yardstick.npz"))
    pre = NAMES[mode] + "/"
    return {k[len(pre):]: y[k] for k in y.files if k.startswith(pre)}


def floor_of(mode, key) -> float:
    """distance of the reference's own float32 run from the same run in float64, from the two committed files"""
    return err(load(mode)[key], yard(mode)[key])


def trained_bound(mode, key) -> float:
    return max(TOL, FLOOR_FACTOR * floor_of(mode, key))


def batches(mode):
    z = load(mode)
    o = z["batch_offsets"]
    return [(z["batch_u"][o[k]:o[k + 1]], z["batch_i"][o[k]:o[k + 1]], z["batch_j"][o[k]:o[k + 1]]) for k in range(o.size - 1)]


def joint(z, prefix):
    return np.concatenate([z[prefix + "_U"], z[prefix + "_V"]])


def dense_delta(z, tag, n_rows):
    """the perturbation tables after the first / last update, joint, from their touched rows"""
    D = np.zeros((n_rows, z[f"delta_{tag}_val"].shape[1]), z[f"delta_{tag}_val"].dtype)
    D[z[f"delta_{tag}_rows"]] = z[f"delta_{tag}_val"]
    return D


def hyper(mode):
    m = META[NAMES[mode]]
    return dict(lr=m["lr"], reg=m["regU"], reg_adv=m["regA"], eps=m["eps"], n_pretrain=m["n_pretrain_steps"])


def train_test_lists(mode):
    """the recorded split as the [user, item, rating] rows a drop-in class takes; names are u<id> / i<id>, test entries the training set
    does not know are named w<k> / x<k>"""
    z = load(mode)
    train = [[f"u{u}", f"i{i}", float(r)] for u, i, r in zip(z["train_uid"].tolist(), z["train_iid"].tolist(), z["train_r"].tolist())]
    test = [[f"u{u}" if u >= 0 else f"w{k}", f"i{i}" if i >= 0 else f"x{k}", 1.0]
            for k, (u, i) in enumerate(zip(z["test_uid"].tolist(), z["test_iid"].tolist()))]
    return train, test


# ---- synthetic kernel cases ---------------------------------------------------------------------------------------------------------
DIMS = ((8, 32), (50, 64), (64, 64), (128, 128))        # d / ld: pad lanes at 8/32 and 50/64, none at 64/64 and 128/128
BATCHES = (1, 5, 64, 257)                               # one group; less than a wavefront's groups; a block; more than one block, odd
TABLES = ((3, 4), (300, 500))                           # every row collides; collisions are rare
REG, REG_ADV, EPS = 0.01, 2.0, 0.5


def draw_batch(rng, B, nu, ni):
    """(u, i, j), i != j.  On the small tables the first half of the items are mostly positives and the second half mostly negatives
    (one in ten the other way round): every item is a positive of some triplets and a negative of others, yet a row's sum is not the
    small difference of two large ones -- a case whose answer float32 cannot state to 1e-5 would test the generator, not the kernel.
    B >= 5: one user holds slots 1, 3, 4 and slot 2's positive is slot 0's negative."""
    u = rng.integers(0, nu, B)
    if ni <= 8:
        h = ni // 2
        cross = rng.random(B) < 0.1
        lo, hi = rng.integers(0, h, B), rng.integers(h, ni, B)
        i, j = np.where(cross, hi, lo), np.where(cross, lo, hi)
    else:
        i = rng.integers(0, ni, B)
        j = (i + 1 + rng.integers(0, ni - 1, B)) % ni
    if B >= 5:
        u[3] = u[4] = u[1]
        if j[0] != j[2]:
            i[2] = j[0]
    assert (i != j).all()
    return u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)


def kernel_case(d, B, nu, ni, seed=0):
    """(E float32 [nu + ni, d], first batch, second batch): the second overlaps the first (shared rows) on the small tables and
    partly on the large ones"""
    rng = np.random.default_rng([d, B, nu, ni, seed])
    E = (rng.uniform(-1, 1, (nu + ni, d)) * (1.5 / np.sqrt(d))).astype(np.float32)
    a, b = draw_batch(rng, B, nu, ni), draw_batch(rng, B, nu, ni)
    if B >= 2:
        b[0][0], b[1][0] = a[0][0], a[1][0]              # a row of the first call that the second call reads and rewrites
        if b[1][0] == b[2][0]:
            b[2][0] = (b[2][0] + 1) % ni
    return E, a, b


HAZARD = (64, 64, 64, 64, 2048)                         # d, ld, users, items, B


def hazard_case():
    """B = 2048 over 64 x 64 tables: every row is read by dozens of triplets of a call that also rewrites it"""
    d, _, nu, ni, B = HAZARD
    return kernel_case(d, B, nu, ni)


def long_run_case():
    """(d, ld, n_users, n_items, E, (u, v, n)): one user in all 257 slots, one long run of the walk.  Positives come from the first half
    of the items and negatives from the second, and the halves' embeddings are offset against each other, so the 257 terms of the user's
    row point one way instead of cancelling to a remainder float32 cannot state."""
    d, ld, nu, ni, B = 50, 64, 300, 500, 257
    rng = np.random.default_rng([d, B, 7])
    E = rng.uniform(-1, 1, (nu + ni, d)) * (1.5 / np.sqrt(d))
    E[nu:nu + ni // 2] += 0.5 / np.sqrt(d); E[nu + ni // 2:] -= 0.5 / np.sqrt(d)
    u = np.full(B, 7, np.int32)
    return d, ld, nu, ni, E.astype(np.float32), (u, rng.integers(0, ni // 2, B).astype(np.int32), rng.integers(ni // 2, ni, B).astype(np.int32))


def consecutive_case():
    """(d, ld, n_users, n_items, E, first, second): 64 triplets, then 5 on other users whose positive is one item throughout"""
    d, ld, nu, ni = 50, 64, 300, 500
    E = kernel_case(d, 64, nu, ni)[0]
    rng = np.random.default_rng(3)
    i32 = lambda a: a.astype(np.int32)
    first = (i32(rng.integers(0, 150, 64)), i32(rng.integers(0, 250, 64)), i32(rng.integers(250, 500, 64)))
    second = (i32(rng.integers(150, 300, 5)), np.full(5, 499, np.int32), i32(rng.integers(0, 100, 5)))
    return d, ld, nu, ni, E, first, second


def sweep():
    return [(d, ld, B, nu, ni) for d, ld in DIMS for B in BATCHES for nu, ni in TABLES]


def case_id(c):
    d, ld, B, nu, ni = c
    return f"d{d}-ld{ld}-B{B}-{nu}x{ni}"
