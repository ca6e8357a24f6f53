"""The shapes at which tests/golden/workspace_bytes.json pins the workspace sizes the library states: every branch of each layout
(row counts on both sides of a padding or segment boundary, every legal row stride, zero rows where the entry point allows it)."""
import contextlib
import itertools
import os

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

# ---- the evaluation's scratch (csrc/eval_block.hip, csrc/eval_fused.hip): the one size that depends on switches read per call, so a case carries the
# environment it is recorded under.  Items: 32-item tile padding, the heap / sliced boundary 8192, the fused boundary 16384;
# users: 64-padding and the fallback's fb_users = max(n_b / 16, 256) switch at 4096; ld 96 is fused without bf16, 160 never
# fused; fused needs K + 1 <= 64.  The product is thinned, every value of every axis stays.
F32, F64 = 0, 1
EVAL_ITEMS = (1, 31, 32, 33, 8191, 8192, 16383, 16384, 16385, 40000)
EVAL_USERS = (0, 1, 63, 64, 65, 4095, 4096, 4112, 8192)
EVAL_LD, EVAL_K = (32, 64, 96, 128, 160), (1, 20, 63, 64, 100)
EVAL_SWITCHES = ("QREC_EVAL_BLOCK_PATH", "QREC_EVAL_F32_FILTER", "QREC_EVAL_NU")
EVAL_ENVS = ({}, {"QREC_EVAL_F32_FILTER": "1"}, {"QREC_EVAL_NU": "2"}, {"QREC_EVAL_BLOCK_PATH": "1"})
EVAL_GRID = list(itertools.product(EVAL_ITEMS, EVAL_USERS))

CPU_CASES += (
    [("score_topk", [F32, ni, nb, 64, 20, {}]) for ni, nb in EVAL_GRID]
    # every stride under every switch, on and past the fused boundary, on both sides of user padding and of the fb_users switch
    + [("score_topk", [F32, ni, nb, ld, 20, env])
       for ni, nb, ld, env in itertools.product((16384, 40000), (1, 65, 4112), EVAL_LD, EVAL_ENVS)]
    + [("score_topk", [F32, ni, 65, ld, K, env])
       for ni, ld, K, env in itertools.product((8192, 16385), (64, 96), EVAL_K, (EVAL_ENVS[0], EVAL_ENVS[3]))]
    + [("score_topk", [F64, ni, nb, ld, 20, {}]) for (ni, nb), ld in itertools.product(EVAL_GRID[::2], (16, 64))]
    + [("score_topk", [F64, 16385, 65, 16, K, env]) for K, env in itertools.product(EVAL_K, EVAL_ENVS)]
    + [(fn, [ni, nb]) for fn in ("score_topk_sigmoid_bias", "score_topk_sparse_row_sigmoid_bias") for ni, nb in EVAL_GRID]
)


@contextlib.contextmanager
def eval_switches(env):
    """exactly the given QREC_EVAL_* switches for the duration: the others unset, the caller's environment restored afterwards"""
    saved = {k: os.environ.pop(k, None) for k in EVAL_SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def stated_bytes(capi, fn, args):
    """what the library states for one case"""
    if fn == "score_topk":
        with eval_switches(args[-1]):
            return capi.score_topk_scratch_bytes(*args[:-1])
    if fn.startswith("score_topk_"):
        with eval_switches({}):
            return getattr(capi, fn + "_scratch_bytes")(*args)
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
