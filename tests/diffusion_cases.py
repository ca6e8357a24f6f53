"""The recorded DiffNet / DHCF runs (tests/golden/tf_diffnet_filmtrust.npz, tf_dhcf_filmtrust.npz) as inputs: batches, dropout
masks, start values -- shared by tests/test_diffusion_cpu.py and tests/test_gpu_diffusion.py."""
import json
import os

import numpy as np

from helpers import GOLDEN, rel_err

GRAD_TOL = 1e-5         # the project's bar: 1e-5 relative Frobenius on fp32 quantities
FLOOR_FACTOR = 2.5      # as tests/test_gpu_tf_golden.py: two independent float32 roundings of one computation are sqrt(2) apart in expectation
META = json.load(open(os.path.join(GOLDEN, "golden_tf_diffusion.json")))
YARD = np.load(os.path.join(GOLDEN, "tf_diffusion_f64_yardstick.npz"))
DIFFNET, DHCF = "tf_diffnet_filmtrust", "tf_dhcf_filmtrust"
VARS = {DIFFNET: ("U", "V", "weights0", "weights1"), DHCF: ("U", "V", "JU_1", "JU_2")}
DROP_RATE = 0.1         # DHCF.py:72


def load(name):
    return META[name], np.load(os.path.join(GOLDEN, name + ".npz"))


def batches(z):
    off = z["batch_offsets"]
    for k in range(off.size - 1):
        s = slice(off[k], off[k + 1])
        yield k, z["batch_u"][s], z["batch_i"][s], z["batch_j"][s]


def dhcf_masks(m, z, k):
    """0/1 keep decisions of step k per layer over the joint [users; items] rows: the stand-in's dropout draws are a function of
    (seed, run index, op index, shape); op order (meta random_ops): users L1 = 0, items L1 = 1, users L2 = 2, items L2 = 3"""
    from golden import tf1shim
    nu, ni, d = m["n_users"], m["n_items"], m["emb_size"]
    ops = sorted((r[0], tuple(r[2])) for r in m["random_ops"][0])
    assert [o for o, _ in ops] == [0, 1, 2, 3] and [s for _, s in ops] == [(nu, d), (ni, d), (nu, d), (ni, d)]
    draw = lambda op, n: (tf1shim.random_uniform(m["seed"], z["run_index"][k], op, (n, d)) >= DROP_RATE).astype(np.float32)
    return [np.concatenate([draw(2 * layer, nu), draw(2 * layer + 1, ni)]) for layer in range(2)]


def floor_of(name, key, z):
    """distance of the reference's own float32 run from the same run in float64, computed from the two committed files"""
    return rel_err(z[key], YARD[f"{name}/{key}"].reshape(z[key].shape))


def trained_bound(name, key, z):
    return max(GRAD_TOL, FLOOR_FACTOR * floor_of(name, key, z))
