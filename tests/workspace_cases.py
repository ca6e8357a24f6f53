"""The shapes at which tests/golden/workspace_bytes.json pins the workspace sizes the library states: every branch of each layout
(row counts on both sides of a padding or segment boundary, every legal row stride, zero rows where the entry point allows it)."""
import itertools

import numpy as np

PAD_N = (0, 1, 63, 64, 65, 129)                  # the contrastive layouts pad n to a multiple of 64
ALS_DEGREES = ((), (0,), (3, 512, 7), (513,), (5, 2000, 512, 513, 0, 1024))     # QREC_ALS_SPLIT_DEGREE = 512, segments of 256

CPU_CASES = (
    [("info_nce", [n, ld]) for n, ld in itertools.product(PAD_N, (32, 64, 128, 256))]
    + [("sept_ssl", [n, ld, k]) for n, ld, k in itertools.product((0, 1, 64, 65), (32, 64, 128, 256), (1, 5))]
    + [("als_gram", [rows, ld]) for rows, ld in itertools.product((0, 1, 1000, 300000), (16, 32, 64, 128))]
    + [("als_solve", [list(deg), ld]) for deg, ld in itertools.product(ALS_DEGREES, (16, 32, 64, 128))]
    + [("cooc", [n]) for n in (1, 31, 32, 33, 8192, 8193, 20000)]                # QREC_COOC_TILE = 8192
    + [("cofactor_item", [n, c, ld]) for (n, c), ld in itertools.product(((0, 0), (1, 0), (1, 1), (33, 7), (1000, 1000)), (16, 32, 64, 128))]
    + [("expo_solve", [n, ld]) for n, ld in itertools.product((0, 1, 33, 1000), (16, 32, 64, 128))]
    + [("expo_prior", [r, c]) for r, c in itertools.product((0, 1, 2047, 2048, 2049, 5000), (0, 1, 33, 1000))]   # kPriorSegment = 2048
    + [("knn_topk", [q, m]) for q, m in ((0, 0), (1, 1), (3, 10), (4, 8), (5, 7), (100, 333))]
    + [("slopeone", [b, n]) for b, n in ((0, 0), (1, 1), (3, 7), (2, 11), (64, 1000))]
    + [("cdae", [B, ld]) for B, ld in itertools.product((0, 1, 3, 64), range(32, 257, 32))]
    + [("cdae_draw", [B, n]) for B, n in itertools.product((0, 1, 3), (1, 32, 33, 64, 65, 1000))]
    + [("irgan_row", [B, n]) for B, n in itertools.product((1, 2, 33, 65), (1, 255, 256, 257, 1000, 20000))]
    + [("irgan_gen", [n, ld, K]) for n, ld, K in itertools.product((1, 33, 63, 64, 65, 257, 1000), (32, 64, 128, 256), (0, 1, 5, 65, 1000))]
    + [("hss", [n]) for n in (0, 1, 1000)]
    + [("channel_attention", [])]
    + [("random_permutations", [n, c]) for n, c in ((0, 0), (1, 1), (37, 3))]       # small sorts: rocprim sizes them without a device
)


def stated_bytes(capi, fn, args):
    """what the library states for one case"""
    if fn == "als_solve":
        degrees, ld = args
        return capi.als_solve_workspace_bytes(np.concatenate([[0], np.cumsum(degrees, dtype=np.int64)]).astype(np.int64), ld)
    if fn == "hss":
        return capi.hss_scratch_bytes(*args)
    if fn == "random_permutations":
        return capi.random_permutations_scratch_bytes(*args)
    if fn == "channel_attention":
        return 4 * capi.channel_attention_scratch_floats()
    return getattr(capi, fn + "_workspace_bytes")(*args)
