"""The two synthetic SEPT graphs the sampler tests share (CPU structure checks, GPU value parity).

A: 37 users, 23 items, 300 training rows drawn with replacement (duplicates occur), 120 follow pairs with duplicated pairs, a self-follow,
   users who follow nobody and users who are only followed -- everything the union structure and count^2 can get wrong, in one block.
B: 700 users, 500 items, 5,000 rows, 3,000 pairs -- several blocks of every kernel, rows longer than the 16 lanes of the degree pass."""
import numpy as np

CASES = {"A": (37, 23, 300, 120), "B": (700, 500, 5000, 3000)}


def case(name: str):
    """(n_users, n_items, uid, iid, follower, followee), int32 ids"""
    nu, ni, E, R = CASES[name]
    rng = np.random.default_rng(1000 + nu)
    uid, iid = rng.integers(0, nu, E), rng.integers(0, ni, E)
    if name == "A":
        followers = np.arange(0, 20)                                         # users 20..36 follow nobody; 30..36 are only followed
        fo = rng.choice(followers, R - 12); fe = rng.integers(0, nu, R - 12)
        fe[:10] = np.arange(30, 37)[np.arange(10) % 7]
        dup = rng.integers(0, R - 12, 10)                                    # ten pairs twice, one of them three times
        fo = np.concatenate([fo, fo[dup], fo[dup[:1]], [5]]); fe = np.concatenate([fe, fe[dup], fe[dup[:1]], [5]])      # (5, 5): a self-follow
    else:
        fo, fe = rng.integers(0, nu, R), rng.integers(0, nu, R)
    assert fo.size == R
    return nu, ni, uid.astype(np.int32), iid.astype(np.int32), fo.astype(np.int32), fe.astype(np.int32)
