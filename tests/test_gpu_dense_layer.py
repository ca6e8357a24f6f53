"""csrc/dense_layer.hip where its persistent loops and wide paths run: every instantiation of the forward, backward, weight-gradient
and pointwise kernels against the float64 mirror (tests/diffusion_mirror.py) at the row counts of tests/dense_layer_cases.py.
Section 5 holds NGCF's instantiations of the same kernels (csrc/ngcf.hip) to the same harness, row subsets included.

Integer cases are bit for bit (np.array_equal, no tolerance): entries in -2..2, so every product and partial sum is an integer
below 2^24 (tests/test_diffusion_cpu.py checks that headroom) and fp32 is exact whatever the summation tree -- one stale 32-row
tile in 70,000 rows fails.  Real-valued cases hold C.GRAD_TOL per 32-row tile and per weight block, never over a whole table.
Every output table carries GUARD_ROWS extra rows of a sentinel that must come back untouched."""
import numpy as np
import pytest

import dense_layer_cases as D
import diffusion_cases as C
import diffusion_mirror as M
from helpers import check, pad_cols, rel_err, same_bits

pytestmark = pytest.mark.gpu

WS_TAIL = 4096                       # bytes of 0xA5 behind the workspace dense_layer_ws_bytes asks for: must stay 0xA5


def _db(a):
    from qrec_amd.capi import DeviceBuffer
    return DeviceBuffer.from_numpy(np.ascontiguousarray(a))


def _pad_w(W, d, ld):
    """(k*d x d) -> [k][ld][ld], zero-padded"""
    out = np.zeros((W.shape[0] // d, ld, ld), np.float32)
    for k in range(out.shape[0]):
        out[k, :d, :d] = W[k * d:(k + 1) * d]
    return out


def _guarded(n, ld, body=None):
    """an output table of n + GUARD_ROWS rows: SENTINEL everywhere, or `body` (n x d, zero-padded) over the first n rows"""
    h = np.full((n + D.GUARD_ROWS, ld), D.SENTINEL, np.float32)
    if body is not None:
        h[:n] = pad_cols(body, ld)
    return _db(h)


def _out(buf, n, d, what, ctx, ids=None):
    """read an output table back: guard rows untouched, pad columns zero; returns the n x d body.  ids: only these rows of the
    table were to be written -- every other row still holds the sentinel, and the body is the listed rows in list order"""
    h = buf.numpy()
    assert (h[n:] == D.SENTINEL).all(), f"{what}: rows at or past n_rows were written {ctx}"
    if ids is not None:
        unlisted = np.ones(n, bool); unlisted[ids] = False
        assert (h[:n][unlisted] == D.SENTINEL).all(), f"{what}: rows outside the listed subset were written {ctx}"
        h, n = h[ids], len(ids)
    assert not h[:n, d:].any(), f"{what}: pad columns are not zero {ctx}"
    return h[:n, :d]


def _workspace(n, ld, nw):
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    need = capi.dense_layer_ws_bytes(n, ld, nw)
    ws = DeviceBuffer(need + WS_TAIL, np.uint8)
    ws.fill_bytes(0xA5)
    return ws, need


class _Layer:
    """one (ld, d, n) with its tables on the device once, run in the four modes"""

    def __init__(self, t, ld, d, n):
        self.t, self.ld, self.d, self.n = t, ld, d, n
        dev = lambda a: _db(pad_cols(a, ld))
        self.X1, self.X2, self.R, self.dY = dev(t["X1"]), dev(t["X2"]), dev(t["R"]), dev(t["dY"])
        self.W = {1: _db(_pad_w(t["W"][:d], d, ld)), 2: _db(_pad_w(t["W"], d, ld))}
        self.f64 = {k: v.astype(np.float64) for k, v in t.items()}

    def run(self, has2, has_r, relu, repeat=False, device_gate=False, exact=False):
        """forward, dpre, backward, accumulating backward: the device's n x d bodies and the mirror's, by name.  device_gate: the
        ReLU gate of the mirror's backward is taken from the device's own Y (real values: float32 and float64 may disagree on the
        sign of a ~0 entry; the integer cases keep the mirror's, Y being exact).  repeat: the second launch must repeat the first's bits;
        exact: its dX2 and gW must equal the mirror bit for bit too."""
        from qrec_amd import capi
        ld, d, n, t, f = self.ld, self.d, self.n, self.t, self.f64
        ctx = dict(ld=ld, d=d, n=n, x2=has2, r=has_r, relu=relu)
        nw = 2 if has2 else 1
        X2d, Rd, Wd = (self.X2 if has2 else None), (self.R if has_r else None), self.W[nw]
        x1, x2, r, w = D.operands(f, has2, has_r)
        got, want = {}, {}
        Y = _guarded(n, ld)
        capi.dense_layer_fwd(self.X1, X2d, Wd, Rd, n, ld, relu, Y)
        got["Y"], want["Y"] = _out(Y, n, d, "Y", ctx), M.layer_fwd(x1, x2, w, r, relu)
        if relu:
            dpre = _guarded(n, ld)
            capi.dense_layer_dpre_relu(self.dY, Y, n, ld, dpre)
            got["dpre"], want["dpre"] = _out(dpre, n, d, "dpre", ctx), f["dY"] * ((got["Y"] if device_gate else want["Y"]) > 0)
        else:
            dpre = self.dY
        dpre_w = want["dpre"] if relu else f["dY"]
        want["dX1"], w2, wW = M.layer_bwd(dpre_w, x1, x2, w)
        want["gW"] = wW.reshape(nw, d, d)
        want["dX1_acc"] = f["prior"] + want["dX1"]
        if has2:
            want["dX2"] = w2
        def backward(acc):
            """one launch into fresh sentinel tables (accumulating: over the prior dX1): the n x d bodies, by name"""
            ws, need = _workspace(n, ld, nw)
            g1 = _guarded(n, ld, t["prior"] if acc else None)
            g2 = _guarded(n, ld) if has2 else None
            gW = _db(np.full((nw, ld, ld), D.SENTINEL, np.float32))
            capi.dense_layer_bwd(dpre, self.X1, X2d, Wd, n, ld, g1, g2, gW, ws, accumulate_dX1=acc)
            assert (ws.numpy()[need:] == 0xA5).all(), f"the weight gradient wrote past dense_layer_ws_bytes {ctx}"
            gWh = gW.numpy()
            assert not gWh[:, d:, :].any() and not gWh[:, :, d:].any(), f"gW: pad rows / columns are not zero {ctx}"
            out = dict(dX1=_out(g1, n, d, "dX1", ctx), gW=gWh[:, :d, :d])
            if has2:
                out["dX2"] = _out(g2, n, d, "dX2", ctx)
            return out

        got.update(backward(False))
        second = backward(True)                        # the accumulating launch; its dX2 and gW do not depend on the prior dX1
        got["dX1_acc"] = second.pop("dX1")
        for k in second:                               # ... and must equal the mirror like the first launch's
            assert exact is False or np.array_equal(second[k], want[k]), f"{k} of the accumulating launch {ctx}"
        if repeat:                                     # the fixed-order claim: a second launch, the same bits
            same_bits(f"dense layer ld={ld} d={d} n={n}", {k: got[k] for k in second}, second)
        assert got.keys() == want.keys()
        return got, want, ctx


# ---- 1. integers: bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld,d,n", D.EXACT_CASES)
def test_integer_layer_is_exact_in_every_instantiation_and_loop(ld, d, n):
    layer = _Layer(D.integer_inputs(ld, d, n), ld, d, n)
    for mode in D.MODES:
        got, want, ctx = layer.run(*mode, exact=True)
        for k in want:
            bad = np.argwhere(got[k] != want[k])             # array_equal, with the place of the first difference in the message
            assert np.array_equal(got[k], want[k]), f"{k}: {len(bad)} entries differ from the float64 mirror, the first at {bad[0].tolist()} {ctx}"


# ---- 2. real values: GRAD_TOL per tile and per weight block -------------------------------------------------------------------------
@pytest.mark.parametrize("ld,d,n", D.REAL_CASES)
def test_real_layer_holds_the_bar_in_every_tile_and_weight_block(ld, d, n):
    layer = _Layer(D.normal_inputs(ld, d, n), ld, d, n)
    for mode in D.MODES:
        got, want, ctx = layer.run(*mode, repeat=(n == 69669), device_gate=True)
        for k in ("Y", "dX1", "dX2", "dX1_acc"):
            if k in want:
                check(f"dense layer {k}: worst 32-row tile vs the mirror", D.worst_tile(got[k], want[k]), C.GRAD_TOL, ctx=ctx)
        if "dpre" in want:
            assert np.array_equal(got["dpre"], want["dpre"])
        for b in range(want["gW"].shape[0]):
            check("dense layer gW: worst weight block vs the mirror", rel_err(got["gW"][b], want["gW"][b]), C.GRAD_TOL, ctx=(ctx, b))


# ---- 3. dpre_norm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld,d,n", D.NORM_CASES)
def test_integer_dpre_norm_is_exact(ld, d, n):
    from qrec_amd import capi
    t = D.norm_integer_inputs(ld, d, n)
    dAll, All, dZ, inv, gate = (_db(t[k]) for k in ("dAll", "All", "dZ", "inv", "gate"))
    for col_off in (d, 2 * d):
        for with_next in (True, False):
            ctx = dict(ld=ld, d=d, n=n, col_off=col_off, dZ_next=with_next)
            dpre = _guarded(n, ld)
            capi.dense_layer_dpre_norm(dAll, All, 3 * ld, col_off, dZ if with_next else None, inv, gate, n, d, ld, dpre)
            got = _out(dpre, n, d, "dpre", ctx)
            want = D.dpre_norm_f64(t["dAll"], t["All"], col_off, t["dZ"] if with_next else None, t["inv"], t["gate"], d)
            bad = np.argwhere(got != want)
            assert np.array_equal(got, want), f"dpre: {len(bad)} entries differ from the float64 formula, the first at {bad[0].tolist()} {ctx}"


@pytest.mark.parametrize("ld,d,n", D.NORM_REAL_CASES)
def test_activate_then_dpre_norm_is_the_backward_of_the_activation(ld, d, n):
    """DHCF's step (DHCFTrainer.forward / train_step_async): qrec_ngcf_activate with injected masks at keep 0.9 leaves gate, 1/|nxt|
    and the normalised block; dpre_norm on those DEVICE outputs against the float64 backward of l2_normalize o dropout o leaky_relu
    taken from the pre-activations"""
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    rng = np.random.default_rng(ld + n)
    wide_ld, col_off, keep = 3 * ld, d, 0.9
    pre = rng.standard_normal((n, d)).astype(np.float32)
    mask = (rng.random((n, d)) >= 0.1).astype(np.float32)
    wide0 = rng.standard_normal((n, wide_ld)).astype(np.float32)           # what lies beside the block must survive
    dAll = rng.standard_normal((n, wide_ld)).astype(np.float32)
    dZ = pad_cols(rng.standard_normal((n, d)).astype(np.float32), ld)
    gate_d, wide_d = _db(pad_cols(pre, ld)), _db(wide0)
    nxt_d, inv_d = DeviceBuffer.zeros((n, ld), np.float32), DeviceBuffer.zeros(n, np.float32)
    capi.ngcf_activate(gate_d, n, d, ld, keep, _db(pad_cols(mask, ld)), 0, 0, nxt_d, wide_d, wide_ld, col_off, inv_d)
    nxt_w, z_w, inv_w, gate_w = D.activate_f64(pre, mask, keep)
    ctx = dict(ld=ld, d=d, n=n)
    nxt_h, wide_h, gate_h = nxt_d.numpy(), wide_d.numpy(), gate_d.numpy()
    assert not nxt_h[:, d:].any() and not gate_h[:, d:].any()
    keep_cols = np.r_[0:col_off, col_off + d:wide_ld]
    assert np.array_equal(wide_h[:, keep_cols], wide0[:, keep_cols])
    check("activate: un-normalised rows, worst tile", D.worst_tile(nxt_h[:, :d], nxt_w), C.GRAD_TOL, ctx=ctx)
    check("activate: normalised block, worst tile", D.worst_tile(wide_h[:, col_off:col_off + d], z_w), C.GRAD_TOL, ctx=ctx)
    check("activate: 1/|nxt|, worst tile", D.worst_tile(inv_d.numpy(), inv_w), C.GRAD_TOL, ctx=ctx)
    check("activate: backward gate, worst tile", D.worst_tile(gate_h[:, :d], gate_w), C.GRAD_TOL, ctx=ctx)
    dpre = _guarded(n, ld)
    capi.dense_layer_dpre_norm(_db(dAll), wide_d, wide_ld, col_off, _db(dZ), inv_d, gate_d, n, d, ld, dpre)
    want = D.dpre_norm_f64(dAll, np.concatenate([wide0[:, :col_off], z_w, wide0[:, col_off + d:]], 1), col_off, dZ, inv_w, gate_w, d)
    check("dpre_norm on the device's activation vs the float64 backward, worst tile", D.worst_tile(_out(dpre, n, d, "dpre", ctx), want),
          C.GRAD_TOL, ctx=ctx)


def test_dpre_norm_refuses_what_it_cannot_do():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    wide, x, v = DeviceBuffer.zeros((8, 96), np.float32), DeviceBuffer.zeros((8, 256), np.float32), DeviceBuffer.zeros(8, np.float32)
    with pytest.raises(capi.QRecError, match="outside the wide table"):
        capi.dense_layer_dpre_norm(wide, wide, 96, 68, None, v, x, 8, 29, 32, x)          # 68 + 29 > 96
    with pytest.raises(capi.QRecError, match="outside the wide table"):
        capi.dense_layer_dpre_norm(wide, wide, 96, -1, None, v, x, 8, 29, 32, x)
    for ld in (16, 48, 256):
        with pytest.raises(capi.QRecError, match="32, 64 or 128"):
            capi.dense_layer_dpre_norm(wide, wide, 96, 0, None, v, x, 8, 8, ld, x)
    assert not x.numpy().any()


# ---- 4. smaller items --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", [256, 1])
def test_fixed_order_batch_loss_assigns_every_slot(n_slots):
    """the slots hold garbage before the launch: a slot no triplet fell into must come back 0, the others their block's sum -- slot k
    gets triplets b with (b // 4) % n_slots == k -- and their sum is the float64 loss; two launches, the same bits"""
    from qrec_amd import capi
    rng = np.random.default_rng(4)
    nu, ni, ld, d, reg = 300, 500, 64, 50, 0.01
    S = np.zeros((nu + ni, ld), np.float32); S[:, :d] = rng.standard_normal((nu + ni, d)) * 0.3
    dS, S64 = _db(S), S.astype(np.float64)
    for B in (0, 1, 5, 2000):
        u, i, j = (rng.integers(0, m, max(B, 1)).astype(np.int32) for m in (nu, ni, ni))
        du, di, dj = _db(u), _db(i), _db(j)
        eu, ei, ej = S64[u[:B]], S64[nu + i[:B]], S64[nu + j[:B]]
        per = np.log1p(np.exp(-(eu * (ei - ej)).sum(1))) + 0.5 * reg * ((eu ** 2).sum(1) + (ei ** 2).sum(1) + (ej ** 2).sum(1))
        want = np.zeros(n_slots); np.add.at(want, (np.arange(B) // 4) % n_slots, per)
        runs = []
        for garbage in (-7.25e9, np.nan):
            slots = _db(np.full(n_slots, garbage, np.float64))
            capi.bpr_batch_loss_slots(dS, 1.0, nu, ld, du, di, dj, B, 0.0, reg, slots)
            runs.append(slots.numpy())
        ctx = dict(B=B, n_slots=n_slots)
        same_bits(f"fixed-order loss B={B}, {n_slots} slots", dict(slots=runs[0]), dict(slots=runs[1]))
        assert np.isfinite(runs[0]).all() and np.array_equal(runs[0] == 0, want == 0), f"slots without a triplet must be assigned 0 {ctx}"
        if B:
            check("fixed-order loss: sum of the slots vs float64", abs(runs[0].sum() - want.sum()) / want.sum(), C.GRAD_TOL, ctx=ctx)
            check("fixed-order loss: every slot vs float64", np.abs(runs[0] - want).max() / want.max(), C.GRAD_TOL, ctx=ctx)


@pytest.mark.parametrize("ld", [32, 64, 128])
def test_no_rows_zeroes_the_weight_gradient_and_writes_nothing_else(ld):
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    stale = np.full((8, ld), D.SENTINEL, np.float32)
    x, w = _db(np.ones((8, ld), np.float32)), _db(np.ones((2, ld, ld), np.float32))
    Y = _db(stale)
    for relu in (False, True):
        capi.dense_layer_fwd(x, x, w, x, 0, ld, relu, Y)
    capi.dense_layer_dpre_relu(x, x, 0, ld, Y)
    capi.dense_layer_dpre_norm(x, x, ld, 0, x, x, x, 0, ld, ld, Y)
    assert np.array_equal(Y.numpy(), stale)
    for nw in (1, 2):
        g1, g2, gW = _db(stale), (_db(stale) if nw == 2 else None), _db(np.full((2, ld, ld), D.SENTINEL, np.float32))
        ws = DeviceBuffer(capi.dense_layer_ws_bytes(0, ld, nw), np.uint8)
        capi.dense_layer_bwd(x, x, x if nw == 2 else None, w, 0, ld, g1, g2, gW, ws, accumulate_dX1=(nw == 2))
        h = gW.numpy()
        assert not h[:nw].any() and (h[nw:] == D.SENTINEL).all()
        assert np.array_equal(g1.numpy(), stale) and (g2 is None or np.array_equal(g2.numpy(), stale))


@pytest.mark.parametrize("ld", [32, 64, 128])
def test_workspace_size_steps_with_the_slab_count_and_four_bytes_less_is_refused(ld):
    """dense_layer_ws_bytes is one [n_w][ld][ld] fp32 partial per slab (128 rows, 512 at ld 128; one slab for no rows) -- exactly:
    the integer cases put a guard behind it, this one refuses anything smaller"""
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    slab = 512 if ld == 128 else 128
    w = DeviceBuffer.zeros((2, ld, ld), np.float32)
    for nw in (1, 2):
        assert capi.dense_layer_ws_bytes(0, ld, nw) == capi.dense_layer_ws_bytes(1, ld, nw) == nw * ld * ld * 4
        for k in (1, 2, 5):
            for n, slabs in ((slab * k, k), (slab * k + 1, k + 1)):
                need = capi.dense_layer_ws_bytes(n, ld, nw)
                assert need == slabs * nw * ld * ld * 4, (ld, nw, n)
                x = DeviceBuffer.zeros((n, ld), np.float32)
                g1, g2, gW = _guarded(n, ld), (_guarded(n, ld) if nw == 2 else None), _db(np.full((nw, ld, ld), D.SENTINEL, np.float32))
                short = DeviceBuffer(need - 4, np.uint8)
                with pytest.raises(capi.QRecError, match="workspace"):
                    capi.dense_layer_bwd(x, x, x if nw == 2 else None, w, n, ld, g1, g2, gW, short)
                for out in (g1, g2, gW):               # refused before any launch: nothing was written
                    assert out is None or (out.numpy() == D.SENTINEL).all()


# ---- 5. NGCF's instantiations: pre = (S + E) W1 + (E * S) W2 and its backward ---------------------------------------------------------
NGCF_OUT = ("pre", "dpre", "dside", "dE", "gW1", "gW2")


class _Ngcf:
    """one (ld, d, n) of qrec_ngcf_dense_fwd / qrec_ngcf_layer_bwd with its tables on the device once.  The backward is driven
    so that dpre IS the gradient block G: the wide table's block all zero, 1/|nxt| = 1, gate 1 on the d real columns and 0 on
    the pad, no dE_next -- (dz - z (z.dz)) * inv * gate = dz exactly.  What lies beside the block in the wide gradient is 3."""
    WIDE_PAD, COL_OFF = 8, 3

    def __init__(self, t, ld, d, n, ids=None, bound=0):
        from qrec_amd import capi
        self.ld, self.d, self.n, self.ids = ld, d, n, ids
        self.ctx = dict(ld=ld, d=d, n=n, listed=None if ids is None else len(ids), bound=bound)
        dev = lambda a: _db(pad_cols(a, ld))
        self.E, self.S, self.W1, self.W2 = dev(t["E"]), dev(t["S"]), _db(_pad_w(t["W1"], d, ld)[0]), _db(_pad_w(t["W2"], d, ld)[0])
        self.wide_ld = d + self.WIDE_PAD
        dAll = np.full((n, self.wide_ld), 3.0, np.float32); dAll[:, self.COL_OFF:self.COL_OFF + d] = t["G"]
        self.dAll, self.All = _db(dAll), _db(np.zeros((n, self.wide_ld), np.float32))
        self.inv, self.gate = _db(np.ones(n, np.float32)), dev(np.ones((n, d), np.float32))
        self.rows = None
        if ids is not None:                            # the id list is `bound` long: past the count it names a row that is NOT listed
            listed, spare = ids
            self.ids = listed
            self.rows = capi.RowSubset(bound)
            self.rows.rows.upload(np.concatenate([listed, np.full(bound - len(listed), spare, np.int32)]))
            self.rows.count.upload(np.array([len(listed)], np.int32))
            self.rows.bound = bound
        f = {k: v.astype(np.float64) for k, v in t.items()}
        if self.ids is not None:
            f.update({k: f[k][self.ids] for k in ("E", "S", "G")})
        dside, dE, gW1, gW2 = M.ngcf_bwd(f["G"], f["E"], f["S"], f["W1"], f["W2"])
        self.want = dict(pre=M.ngcf_fwd(f["E"], f["S"], f["W1"], f["W2"]), dpre=f["G"], dside=dside, dE=dE, gW1=gW1, gW2=gW2)

    def run(self):
        """one forward and one backward into fresh sentinel tables: the device's bodies by name (listed rows only, in list order)"""
        from qrec_amd import capi
        from qrec_amd.capi import DeviceBuffer
        ld, d, n, ctx = self.ld, self.d, self.n, self.ctx
        pre, dpre, dside, dE = (_guarded(n, ld) for _ in range(4))
        gW1, gW2 = (_db(np.full((ld, ld), D.SENTINEL, np.float32)) for _ in range(2))     # two allocations: not adjacent
        need = capi.ngcf_wgrad_partial_bytes(n, ld)
        partial = DeviceBuffer(need + WS_TAIL, np.uint8)
        partial.fill_bytes(0xA5)
        capi.ngcf_dense_fwd(self.E, self.S, self.W1, self.W2, n, ld, pre, rows=self.rows)
        capi.ngcf_layer_bwd(None, self.dAll, self.All, self.wide_ld, self.COL_OFF, self.inv, self.gate, self.E, self.S, self.W1, self.W2,
                            n, d, ld, dpre, dside, dE, partial, gW1, gW2, rows=self.rows)
        assert (partial.numpy()[need:] == 0xA5).all(), f"the weight gradient wrote past ngcf_wgrad_partial_bytes {ctx}"
        got = {k: _out(b, n, d, k, ctx, self.ids) for k, b in (("pre", pre), ("dpre", dpre), ("dside", dside), ("dE", dE))}
        for k, b in (("gW1", gW1), ("gW2", gW2)):
            h = b.numpy()
            assert not h[d:, :].any() and not h[:, d:].any(), f"{k}: pad rows / columns are not zero {ctx}"
            got[k] = h[:d, :d]
        assert got.keys() == self.want.keys() == set(NGCF_OUT)
        return got

    def assert_exact(self, got):
        for k in NGCF_OUT:
            bad = np.argwhere(got[k] != self.want[k])
            assert np.array_equal(got[k], self.want[k]), f"{k}: {len(bad)} entries differ from the float64 mirror, the first at {bad[0].tolist()} {self.ctx}"


@pytest.mark.parametrize("ld,d,n", D.NGCF_EXACT_CASES)
def test_integer_ngcf_layer_is_exact_in_every_instantiation_and_loop(ld, d, n):
    layer = _Ngcf(D.ngcf_inputs(ld, d, n, integer=True), ld, d, n)
    layer.assert_exact(layer.run())


@pytest.mark.parametrize("ld,d,n", D.NGCF_REAL_CASES)
def test_real_ngcf_layer_holds_the_bar_in_every_tile_and_weight_block(ld, d, n):
    layer = _Ngcf(D.ngcf_inputs(ld, d, n, integer=False), ld, d, n)
    got, want = layer.run(), layer.want
    assert np.array_equal(got["dpre"], want["dpre"]), "dpre is the gradient block itself"
    for k in ("pre", "dside", "dE"):
        check(f"NGCF layer {k}: worst 32-row tile vs the mirror", D.worst_tile(got[k], want[k]), C.GRAD_TOL, ctx=layer.ctx)
    for k in ("gW1", "gW2"):
        check(f"NGCF layer {k}: weight block vs the mirror", rel_err(got[k], want[k]), C.GRAD_TOL, ctx=layer.ctx)
    same_bits(f"NGCF layer ld={ld} d={d} n={n}", got, layer.run())          # the fixed-order claim: a second launch, the same bits


@pytest.mark.parametrize("ld,d,n,listed,bound", D.NGCF_SUBSET_CASES)
def test_integer_ngcf_layer_under_a_row_subset_touches_the_listed_rows_only(ld, d, n, listed, bound):
    """the count is read on the device (the bound only sizes the launch: the id list names an unlisted row from the count up to the
    bound), unlisted rows of pre, dside, dE and dpre keep their sentinel, listed rows and the weight gradients are exact"""
    layer = _Ngcf(D.ngcf_inputs(ld, d, n, integer=True), ld, d, n, ids=D.ngcf_subset_ids(n, listed), bound=bound)
    layer.assert_exact(layer.run())
