"""The recorded IRGAN run (tests/golden/tf_irgan_filmtrust.npz) as inputs -- draws, batches, start values, bounds -- and the built
kernel cases; shared by tests/test_irgan_cpu.py and tests/test_gpu_irgan.py."""
import functools
import json
import os

import numpy as np

import irgan_mirror as M
from helpers import GOLDEN, rel_err

GRAD_TOL = 1e-5         # the project's bar: 1e-5 relative Frobenius on fp32 quantities
MIRROR_TOL = 1e-9       # the float64 mirror against the reference's float64 run
FLOOR_FACTOR = 2.5      # as tests/cdae_cases.py: two independent float32 roundings of one computation are sqrt(2) apart in expectation
CDF_BAND = 1e-5         # a drawn index i must satisfy cdf[i - 1] - band <= x < cdf[i] + band against the mirror's float64 CDF
NAME = "tf_irgan_filmtrust"
META = json.load(open(os.path.join(GOLDEN, "golden_tf_irgan.json")))[NAME]
YARD = np.load(os.path.join(GOLDEN, "tf_irgan_f64_yardstick.npz"))
VARS = ("g_P", "g_Q", "g_b", "d_P", "d_Q", "d_b")
N_SNAPS = 6             # after the discriminator epoch, then after each generator pass


@functools.lru_cache(None)
def load():
    return np.load(os.path.join(GOLDEN, NAME + ".npz"))


def yard(key):
    return YARD[f"{NAME}/{key}"]


def floor_of(key, z):
    """distance of the reference's own float32 run from the same run in float64, computed from the two committed files"""
    return rel_err(z[key], yard(key).reshape(z[key].shape))


def trained_bound(key, z):
    return max(GRAD_TOL, FLOOR_FACTOR * floor_of(key, z))


def initial(z=None):
    z = load() if z is None else z
    return {v: z[f"init_{v}"] for v in VARS}


def positives(z=None):
    """user id -> rated item ids in the reference's order"""
    z = load() if z is None else z
    return {u: z["pos_items"][a:b].tolist() for u, (a, b) in enumerate(zip(z["pos_ptr"][:-1], z["pos_ptr"][1:])) if b > a}


def positives_csr(z=None):
    """the same as an ascending CSR over all users (what the trainer takes)"""
    z = load() if z is None else z
    ptr = z["pos_ptr"].astype(np.int64)
    items = np.concatenate([np.sort(z["pos_items"][a:b]) for a, b in zip(ptr[:-1], ptr[1:])]).astype(np.int32)
    return ptr, items


def draw_calls(z=None):
    """[(user, samples)] of every np.random.choice call: get_data's, then the generator's, pass by pass"""
    z = load() if z is None else z
    return [(int(u), z["draw_items"][a:b]) for u, a, b in zip(z["draw_user"], z["draw_ptr"][:-1], z["draw_ptr"][1:])]


def discriminator_batches(z=None):
    z = load() if z is None else z
    return [(z["dis_u"][a:b], z["dis_i"][a:b], z["dis_label"][a:b]) for a, b in zip(z["dis_ptr"][:-1], z["dis_ptr"][1:])]


def run_recorded(model, z=None):
    """the reference's epoch on ``model`` (a Mirror, or an adapter with discriminator_step(u, i, y) -> loss and gradients on request,
    generator_step(u, pos, samples), snapshot()) with the recorded draws injected: dict(losses_d, losses_g, grad0, grad1, snaps)"""
    z = load() if z is None else z
    order, pos, calls = z["user_order"].tolist(), positives(z), draw_calls(z)
    nu_t = len(order)
    rows = M.get_data_rows(order, pos, [c[1] for c in calls[:nu_t]])
    out = dict(losses_d=[], losses_g=[], snaps=[])
    for k, (u, i, y) in enumerate(M.discriminator_batches(rows, META["train_size"], META["batch_size"])):
        r = model.discriminator_step(u, i, y)
        out["losses_d"].append(r["loss"])
        if k == 0:
            out["grad0"] = {"d_P": r["gP"], "d_Q": r["gQ"], "d_b": r["gb"]}
    out["snaps"].append(model.snapshot())
    for k, (u, samples) in enumerate(calls[nu_t:]):
        r = model.generator_step(u, pos[u], samples)
        out["losses_g"].append(r["loss"])
        if k == 0:
            out["grad1"] = {"g_P": r["gP_full"], "g_Q": r["gQ"], "g_b": r["gb"]}
        if (k + 1) % nu_t == 0:
            out["snaps"].append(model.snapshot())
    out["losses_d"], out["losses_g"] = np.array(out["losses_d"]), np.array(out["losses_g"])
    return out


@functools.lru_cache(None)
def mirror_run(per_slot_regulariser=True):
    return run_recorded(M.Mirror(initial(), META["lr"], META["regU"], per_slot_regulariser))


def train_test_lists(z=None):
    """the recorded split as the [user, item, rating] rows a drop-in class takes; names are u<id> / i<id>, test items the training
    set does not know are named x<k>"""
    z = load() if z is None else z
    train = [[f"u{u}", f"i{i}", float(r)] for u, i, r in zip(z["train_uid"].tolist(), z["train_iid"].tolist(), z["train_r"].tolist())]
    test = [[f"u{u}" if u >= 0 else f"w{k}", f"i{i}" if i >= 0 else f"x{k}", 1.0]
            for k, (u, i) in enumerate(zip(z["test_uid"].tolist(), z["test_iid"].tolist()))]
    return train, test


def n_uniforms_of_an_epoch(z=None):
    """uniforms one epoch of the reference consumes: 2 |pos| per user in get_data, 3 |pos| per user in each of five generator passes"""
    z = load() if z is None else z
    n = int(sum(len(p) for p in positives(z).values()))
    return (M.NEG_PER_POS + M.GEN_PASSES * M.GEN_PER_POS) * n


# ---- built kernel cases ---------------------------------------------------------------------------------------------------------------
N_ITEMS = (1, 63, 64, 65, 257, 4097)         # one item, the wavefront / chunk boundary, more than one logits tile, more than one chunk row of the scan
WIDTHS = (8, 50, 64, 128)                    # 50: the stock conf's width (padding); 64 and 128: the bias column opens the next stride
N_USERS = 70
LOGIT_BAND = 10.0                            # |z| / T <= 10 in every case: exp stays far from float32's range at both temperatures
EDGE_UNIFORMS = (0.0, np.nextafter(1.0, 0.0), 0.5, 0.25, 1e-12)


def pos_sizes(n_items):
    """|pos| of the first rows: 1, n_items - 1 and 181 where the table allows; the other rows take small random sets"""
    return [k for k in (1, n_items - 1, 181) if 1 <= k < n_items]


def kernel_case(n_items, d, seed=0):
    """(variables, positives CSR over N_USERS users).  Tables are scaled so that |P[u] . Q[j] + b[j]| <= 2 = LOGIT_BAND * T at the
    tempered end; user 0 has |pos| = 1, user 1 all items but one, user 2 181 of them (where the table allows); a positive sits at item 0
    (users 0, 2, 3) and at the last item (users 1, 2, 4); users past 5 rated up to 12 random items."""
    rng = np.random.default_rng([n_items, d, seed])
    a = np.sqrt(1.5 / d)                       # |P . Q| <= d a^2 = 1.5, |b| <= 0.5
    v = {}
    for t in "gd":
        v[t + "_P"] = rng.uniform(-a, a, (N_USERS, d)); v[t + "_Q"] = rng.uniform(-a, a, (n_items, d)); v[t + "_b"] = rng.uniform(-0.5, 0.5, n_items)
    v = {k: x.astype(np.float32) for k, x in v.items()}
    rows = []
    for u in range(N_USERS):
        sizes = pos_sizes(n_items)
        if u < len(sizes):
            k = sizes[u]
            if k == 1:
                row = np.array([0])
            elif k == n_items - 1:
                row = np.arange(1, n_items)                  # all but item 0: the last item is a positive
            else:
                row = np.concatenate([[0, n_items - 1], rng.permutation(np.arange(1, n_items - 1))[:k - 2]])
        elif n_items > 2:
            k = int(rng.integers(1, min(12, n_items - 1) + 1))
            row = rng.permutation(n_items)[:k]
            if u == 3:
                row = np.union1d(row[:max(k - 1, 0)], [0])
            if u == 4:
                row = np.union1d(row[:max(k - 1, 0)], [n_items - 1])
        else:
            row = np.zeros(0, int)
        rows.append(np.unique(row).astype(np.int32))
    ptr = np.zeros(N_USERS + 1, np.int64); np.cumsum([r.size for r in rows], out=ptr[1:])
    items = np.concatenate(rows).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return v, (ptr, items)


def pos_of(csr, u):
    return csr[1][csr[0][u]:csr[0][u + 1]]


def in_band(cdf, x, idx, band=CDF_BAND):
    """every draw inside its CDF interval, widened by ``band`` on both sides: cdf[i - 1] - band <= x < cdf[i] + band"""
    idx = np.asarray(idx)
    lo = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
    return (lo - band <= x) & (x < cdf[idx] + band)


# ---- the throughput mode's distribution test ------------------------------------------------------------------------------------------
CHI2_LEVEL = 1e-6       # a user's draws are refused when a chi-square this unlikely or worse is observed
CHI2_REPEATS = 40       # get_data is drawn this many times (steps 0 .. 39) so that the pooled bins have counts to speak of


def chi_square_p(counts, prob, n):
    """p-value of Pearson's chi-square of ``counts`` (n draws) against ``prob``, items pooled in index order into bins of expected count
    >= 5 (the remainder joins the last bin); items of probability 0 must have count 0"""
    from scipy.stats import chi2
    assert not counts[prob == 0].any()
    expected = prob * n
    obs, exp, o, e = [], [], 0.0, 0.0
    for c, x in zip(counts, expected):
        o += c; e += x
        if e >= 5:
            obs.append(o); exp.append(e); o = e = 0.0
    if e > 0 and exp:
        obs[-1] += o; exp[-1] += e
    if len(exp) < 2:
        return 1.0
    obs, exp = np.array(obs), np.array(exp)
    return float(chi2.sf(((obs - exp) ** 2 / exp).sum(), len(exp) - 1))
