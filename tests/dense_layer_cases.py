"""Shapes and inputs of the direct dense-layer tests (csrc/dense_layer.hip, and NGCF's instantiations of the same kernels), shared by tests/test_gpu_dense_layer.py (the kernels
against the float64 mirror) and tests/test_diffusion_cpu.py (the headroom that makes the integer cases exact).  numpy only.

Row counts: each is the smallest at which a loop of the kernels (csrc/mfma_layer.h) behaves differently.  layer_grid caps the persistent kernels at
256 blocks x 4 wavefronts = 1,024 tiles of 32 rows = 32,768 rows:
  32,768  fills the capped grid exactly: every wavefront one tile, the prefetch condition false at the boundary
  32,801  two wavefronts take a second tile, the last tile holds one row
  69,669  two full rounds and a ragged third (last tile 5 rows); 545 slabs of 128 (ld <= 64) and 137 slabs of 512 (ld 128: 8-9 per
          slab class of wgrad_sum_kernel); 69,669 * ld / 4 float4 > 2,048 * 256 for every ld (dpre_relu's grid-stride loop);
          past dpre_norm's caps of 65,536 / 32,768 / 16,384 rows
  8,193   ld 128 only: 17 slabs, class 0 adds two slabs and every other class one"""
import numpy as np

MODES = ((True, False, True), (False, True, False), (True, True, False), (False, False, True))     # (X2, R, ReLU), as test_gpu_diffusion
SHAPES = ((32, 29), (32, 32), (64, 50), (64, 64), (128, 100), (128, 128))                             # (ld, d): d below ld (29, 50: d % 4 != 0), and d = ld
EXACT_ROWS = (32768, 32801, 69669)
EXACT_CASES = [(ld, d, n) for ld, d in SHAPES for n in EXACT_ROWS + ((8193,) if ld == 128 else ())]
REAL_CASES = [(ld, d, n) for ld, d in SHAPES for n in (32801, 69669)]
NORM_ROWS = (1, 77, 69669)
# dpre_norm: every d on every ld it fits, so that each instantiation sees partial float4 (d % 4 != 0) and unaligned column offsets
NORM_SHAPES = [(ld, d) for ld in (32, 64, 128) for d in (29, 32, 50, 64, 100, 128) if d <= ld]
NORM_CASES = [(ld, d, n) for ld, d in NORM_SHAPES for n in NORM_ROWS]
NORM_REAL_CASES = [(ld, d, n) for ld, d in ((32, 29), (64, 64), (128, 100)) for n in (77, 69669)]

# NGCF's instantiations (pre = (S + E) W1 + (E * S) W2, csrc/ngcf.hip): one forward and one backward per case
NGCF_EXACT_CASES = [(32, 29, 32801), (64, 64, 32801), (32, 29, 69669), (64, 64, 69669), (128, 100, 8193), (128, 100, 32801)]
NGCF_REAL_CASES = [(64, 50, 32801), (128, 128, 32801)]
# (ld, d, table rows, listed rows, the host's bound on the count): a row subset exists at ld <= 64 only.  77 of 1,000 under a bound
# of 128: the count comes from the device, the bound only sizes the launch.  32,801 of 40,000 under 33,000: the persistent loops
# wrap under a subset, and slab 257 of the 258 launched lies past the count and must add zeros
NGCF_SUBSET_CASES = [(ld, d, n, k, bound) for ld, d in ((32, 29), (64, 64)) for n, k, bound in ((1000, 77, 128), (40000, 32801, 33000))]

GUARD_ROWS = 40                      # rows past n in every output table, pre-filled with SENTINEL: must come back untouched
SENTINEL = np.float32(-12345.0)
EXACT_LIMIT = 2.0 ** 24              # integers below this are exact in fp32, and so is every partial sum of them in any order


def integer_inputs(ld, d, n):
    """X1, X2, R, dY, the prior contents of dX1 (n x d) and W (2d x d; one operand: its first d rows): integers in -2..2 as float32"""
    rng = np.random.default_rng(1000 * ld + d + n)
    f = lambda *s: rng.integers(-2, 3, s).astype(np.float32)
    return dict(X1=f(n, d), X2=f(n, d), R=f(n, d), dY=f(n, d), prior=f(n, d), W=f(2 * d, d))


def normal_inputs(ld, d, n):
    """the same tables as tests/test_gpu_diffusion.py::_layer_once draws them: standard normal, W * 0.3, empty operand rows"""
    rng = np.random.default_rng(2000 * ld + d + n)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    t = dict(X1=f(n, d), X2=f(n, d), R=f(n, d), dY=f(n, d), prior=f(n, d), W=f(2 * d, d) * np.float32(0.3))
    t["X1"][::3] = 0.0
    t["X2"][1::5] = 0.0
    return t


def operands(t, has2, has_r):
    """(X1, X2 or None, R or None, W) of one mode"""
    d = t["X1"].shape[1]
    return t["X1"], (t["X2"] if has2 else None), (t["R"] if has_r else None), (t["W"] if has2 else t["W"][:d])


def headroom(t):
    """{mode: max over the elements of every output of sum |a| |b| (+ |r|; + |prior dX1| for the accumulating backward)}, in
    float64: below EXACT_LIMIT every product and every partial sum of the integer cases is an integer fp32 holds exactly.
    |dpre| <= |dY| under the ReLU gate.  The one-operand weights are block 0 of the two-operand ones: six products serve all modes."""
    a = {k: np.abs(v.astype(np.float64)) for k, v in t.items()}
    d = a["X1"].shape[1]
    W0, W1 = a["W"][:d], a["W"][d:]
    f1, f2 = a["X1"] @ W0, a["X2"] @ W1
    dx1, dx2 = a["dY"] @ W0.T + a["prior"], a["dY"] @ W1.T
    g1, g2 = a["X1"].T @ a["dY"], a["X2"].T @ a["dY"]
    out = {}
    for has2, has_r, relu in MODES:
        fwd = f1 + (f2 if has2 else 0.0) + (a["R"] if has_r else 0.0)
        out[has2, has_r, relu] = float(max([fwd.max(), dx1.max(), g1.max()] + ([dx2.max(), g2.max()] if has2 else [])))
    return out


def ngcf_inputs(ld, d, n, integer):
    """E, S, the gradient block G (n x d) and W1, W2 (d x d): integers in -2..2, or standard normal with W * 0.3"""
    rng = np.random.default_rng(4000 * ld + d + n + (0 if integer else 1))
    f = (lambda *s: rng.integers(-2, 3, s).astype(np.float32)) if integer else (lambda *s: rng.standard_normal(s).astype(np.float32))
    t = dict(E=f(n, d), S=f(n, d), G=f(n, d), W1=f(d, d), W2=f(d, d))
    if not integer:
        t["W1"] *= np.float32(0.3); t["W2"] *= np.float32(0.3)
    return t


def ngcf_subset_ids(n, k):
    """k distinct rows of an n-row table in shuffled order, and one row that is NOT listed (it pads the id list up to the bound)"""
    perm = np.random.default_rng(n + k).permutation(n)
    return perm[:k].astype(np.int32), int(perm[k])


def ngcf_headroom(t):
    """(forward, backward, weight gradient): the largest sum of absolute products over the elements of pre, of dside and dE, and
    of gW1 and gW2, in float64.  With entries in -2..2: at most 16 d, 12 d and 8 n."""
    a = {k: np.abs(v.astype(np.float64)) for k, v in t.items()}
    add, mul = a["S"] + a["E"], a["E"] * a["S"]
    dA1, dA2 = a["G"] @ a["W1"].T, a["G"] @ a["W2"].T
    return (float((add @ a["W1"] + mul @ a["W2"]).max()), float(max((dA1 + dA2 * a["E"]).max(), (dA1 + dA2 * a["S"]).max())),
            float(max((add.T @ a["G"]).max(), (mul.T @ a["G"]).max())))


def norm_integer_inputs(ld, d, n):
    """dpre_norm: wide tables (wide_ld = 3 ld) non-zero EVERYWHERE ({-2, -1, 1, 2}: what lies beside the block shows up under a
    wrong offset or a missing column guard), dZ_next in -2..2, inv_norm from {0.5, 1, 2}, gate from {0, 0.5, 1, 2}; pad columns zero"""
    rng = np.random.default_rng(3000 * ld + d + n)
    nz = np.array([-2, -1, 1, 2], np.float32)
    wide = lambda: nz[rng.integers(0, 4, (n, 3 * ld))]
    padded = lambda a: np.concatenate([a, np.zeros((n, ld - d), np.float32)], 1)
    return dict(dAll=wide(), All=wide(), dZ=padded(rng.integers(-2, 3, (n, d)).astype(np.float32)),
                inv=np.array([0.5, 1, 2], np.float32)[rng.integers(0, 3, n)],
                gate=padded(np.array([0, 0.5, 1, 2], np.float32)[rng.integers(0, 4, (n, d))]))


def norm_headroom(t, d, col_off):
    """largest magnitude any intermediate of dpre = (dz - z (z.dz)) inv gate can take, from the absolute values"""
    dz = np.abs(t["dAll"][:, col_off:col_off + d].astype(np.float64)) + np.abs(t["dZ"][:, :d])
    z = np.abs(t["All"][:, col_off:col_off + d].astype(np.float64))
    return float(((dz + z * (z * dz).sum(1, keepdims=True)) * 2.0 * 2.0).max())


def dpre_norm_f64(dAll, All, col_off, dZ, inv, gate, d):
    """(dz - z (z.dz)) inv gate, dz = dAll block (+ dZ), z = All block"""
    dz = dAll[:, col_off:col_off + d].astype(np.float64)
    if dZ is not None:
        dz = dz + dZ[:, :d]
    z = All[:, col_off:col_off + d].astype(np.float64)
    return (dz - z * (z * dz).sum(1, keepdims=True)) * inv.astype(np.float64)[:, None] * gate[:, :d]


def activate_f64(pre, mask, keep):
    """l2_normalize(dropout(leaky_relu(pre, 0.2), keep)) with injected 0/1 keep decisions: (nxt, z, inv, gate)"""
    pre = pre.astype(np.float64)
    fac = mask.astype(np.float64) / keep
    nxt = np.where(pre > 0, pre, 0.2 * pre) * fac
    inv = 1.0 / np.sqrt(np.maximum((nxt ** 2).sum(1), 1e-12))
    return nxt, nxt * inv[:, None], inv, fac * np.where(pre > 0, 1.0, 0.2)


def worst_tile(got, want, rows=32):
    """the largest rel_err (Frobenius) over the tiles of `rows` consecutive rows: an error confined to one wavefront's tile is
    held to the bound on its own, not diluted in the table's norm.  A tile whose reference is all zero must be zero."""
    got = np.asarray(got, np.float64).reshape(len(got), -1); want = np.asarray(want, np.float64).reshape(len(want), -1)
    assert got.shape == want.shape
    at = np.arange(0, got.shape[0], rows)
    num = np.add.reduceat(((got - want) ** 2).sum(1), at); den = np.add.reduceat((want ** 2).sum(1), at)
    return float(np.sqrt(np.max(np.where(den > 0, num / np.maximum(den, 1e-300), np.where(num > 0, np.inf, 0.0)))))
