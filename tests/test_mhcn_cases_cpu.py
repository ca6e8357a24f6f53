"""The float64 references of tests/mhcn_cases.py, checked without a device: against the restatement that is pinned to the reference's
runs (oracle/tfmodels.py::MHCN.gate / attention / hss, l2_normalize_rows / _bwd), against central differences, and -- for every case of
the GPU table -- the float32 restatement's own distance to them, which has to stay well inside the 1e-5 the kernels are held to."""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import mhcn_cases as MC
from helpers import rel_err
from oracle import tfmodels as T


class _EdgeGiven:
    """stands where MHCN.hss expects the channel's H: ``dot`` hands back the edge table the case fixes, ``T.dot`` keeps the partial
    derivative w.r.t. edge and contributes nothing, so that hss returns the partial derivative w.r.t. em alone"""

    def __init__(self, edge):
        self.edge, self.dedge = edge, None
        self.T = SimpleNamespace(dot=self._keep)

    def dot(self, em):
        return self.edge

    def _keep(self, dedge):
        self.dedge = dedge
        return np.zeros_like(dedge)


def restated_gate(X, W, b, dY, dy_scale, prev):
    """the fp32 restatement's Y, S, Q, dX, dW, db for the same arguments as mhcn_cases.gate_ref"""
    f = np.float32
    Y, bwd = T.MHCN.gate(None, X, W, b)
    g = (f(dy_scale) * dY).astype(f)
    dX, dW, db = bwd(g)
    S = T._sigmoid((X @ W + b).astype(f))
    return Y, S, (g * X * S * (f(1) - S)).astype(f), dX if prev is None else (prev + dX).astype(f), dW, db[0]


def restated_attention(es, a, M, half, dOut, de_prev, dhalf_prev):
    f = np.float32
    out, sc, bwd = T.MHCN.attention(SimpleNamespace(w=dict(attention=a, attention_mat=M)), es)
    des, da, dM = bwd(dOut)
    if half is not None:
        out = (out + half / f(2)).astype(f)
    if de_prev is not None:
        des = [(p + g).astype(f) for p, g in zip(de_prev, des)]
    dhalf = (dOut / f(2)).astype(f) if dhalf_prev is None else (dhalf_prev + dOut / f(2)).astype(f)
    return (M @ a[0]).astype(f), sc, out, des, dhalf, da[0], dM


def restated_hss(em, edge, perm, scale):
    shim = _EdgeGiven(edge)
    loss, dem = T.MHCN.hss(None, em, shim, perm)
    return loss, np.float32(scale) * dem, np.float32(scale) * shim.dedge


def restated_l2norm(X, S0, dS):
    z, inv = T.l2_normalize_rows(X)
    return inv, (S0 + z).astype(np.float32), T.l2_normalize_bwd(X, inv, dS)


# ---- 1. the references against the pinned restatement, at the shape of the existing device test ------------------------------
@pytest.mark.parametrize("d", [24, 50])
def test_fp64_references_agree_with_the_pinned_restatement(d):
    rng = np.random.default_rng(d)
    n = 300
    H, _, w, _, _ = MC.motif_problem(rng, d=d)                  # test_gpu_graph.py::_mhcn_problem's shape
    W, b, a, M = w["gating2"], w["gating_bias2"], w["attention"], w["attention_mat"]
    tab = lambda s=1.0: (rng.standard_normal((n, d)) * s).astype(np.float32)
    worst = {}

    def hold(name, got, want):
        worst[name] = rel_err(got, want)
        assert worst[name] < 1e-5, (name, worst[name])
    X, dY, prev = tab(0.3), tab(), tab()
    for name, got, want in zip(("Y", "S", "Q", "dX", "dW", "db"), MC.gate_ref(X, W, b, dY, 0.25, prev), restated_gate(X, W, b, dY, 0.25, prev)):
        hold("gate " + name, got, want)
    es, half, dOut, de_prev, dh_prev = [tab() for _ in range(3)], tab(), tab(), [tab() for _ in range(3)], tab()
    got, want = MC.attention_ref(es, a, M, half, dOut, de_prev, dh_prev), restated_attention(es, a, M, half, dOut, de_prev, dh_prev)
    for name, g, w in zip(("v", "score", "out", "de", "dhalf", "g_a", "g_M"), got, want):
        for k, (gk, wk) in enumerate(zip(g, w) if name == "de" else [(g, w)]):
            hold(f"attention {name}{k if name == 'de' else ''}", gk, wk)
    # hss composed with H, as the device test composes the kernel with the SpMM: edge = H em, d em = partial + H^T partial
    for ch in (0, 2):
        em = tab(0.5)
        perm = (rng.permutation(n), rng.permutation(d), rng.permutation(n), rng.permutation(d), rng.permutation(n))
        Hc = H[ch].astype(np.float32).tocsr()
        want_loss, want_dem = T.MHCN.hss(None, em, Hc, perm)
        loss, dem, dedge = MC.hss_ref(em, Hc.dot(em).astype(np.float32), perm, 1.0)
        assert abs(loss - want_loss) <= 1e-5 * abs(want_loss)
        hold(f"hss d em, channel {ch}", dem + sp.csr_matrix(Hc, dtype=np.float64).T.dot(dedge), want_dem)
    X[5] = 0; X[77] *= np.float32(1e-4)
    for name, g, w in zip(("inv", "S", "dX"), MC.l2norm_ref(X, prev, dY), restated_l2norm(X, prev, dY)):
        hold("l2norm " + name, g, w)
    print({k: f"{v:.1e}" for k, v in worst.items()})


# ---- 2. the analytic gradients against central differences --------------------------------------------------------------------
def _central(f, x, h):
    g = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        keep = x[idx]
        x[idx] = keep + h; up = f()
        x[idx] = keep - h; down = f()
        x[idx] = keep
        g[idx] = (up - down) / (2 * h)
    return g


def test_fp64_gradients_agree_with_central_differences():
    """n = 12, d = 5, all in float64.  Step h = 1e-5: the truncation error of a central difference is h^2 f''' / 6 ~ 1e-10 relative and
    its rounding error eps |f| / h ~ 1e-16 * 10 / 1e-5 = 1e-10 absolute against gradients of order 0.1 ... 1, so the two meet near 1e-9;
    the bound is 1e-7 norm-wise.  Observed: 2e-11 ... 7e-10 over all eight gradients."""
    rng = np.random.default_rng(12)
    n, d, h, bound = 12, 5, 1e-5, 1e-7
    t = lambda *s: rng.standard_normal(s)
    worst = {}

    def hold(name, analytic, numeric):
        worst[name] = rel_err(analytic, numeric)
        assert worst[name] < bound, (name, worst[name])
    X, W, b, dY = t(n, d), t(d, d) * 0.5, t(1, d) * 0.3, t(n, d)
    _, _, _, dX, dW, db = MC.gate_ref(X, W, b, dY, 1.0)
    f = lambda: float((MC.gate_ref(X, W, b, dY, 1.0)[0] * dY).sum())
    hold("gate dX", dX, _central(f, X, h)); hold("gate dW", dW, _central(f, W, h)); hold("gate db", db, _central(f, b, h)[0])
    es, a, M, half, dOut = [t(n, d) for _ in range(3)], t(1, d) * 0.5, t(d, d) * 0.5, t(n, d), t(n, d)
    _, _, _, de, dhalf, g_a, g_M = MC.attention_ref(es, a, M, half, dOut)
    f = lambda: float((MC.attention_ref(es, a, M, half, dOut)[2] * dOut).sum())
    for k in range(3):
        hold(f"attention de{k}", de[k], _central(f, es[k], h))
    hold("attention dhalf", dhalf, _central(f, half, h))
    hold("attention g_a", g_a, _central(f, a, h)[0]); hold("attention g_M", g_M, _central(f, M, h))
    em, edge = t(n, d) * 0.5, t(n, d) * 0.5
    perm = (rng.permutation(n), rng.permutation(d), rng.permutation(n), rng.permutation(d), rng.permutation(n))
    _, dem, dedge = MC.hss_ref(em, edge, perm, 1.0)
    f = lambda: MC.hss_ref(em, edge, perm, 1.0)[0]
    hold("hss dem", dem, _central(f, em, h)); hold("hss dedge", dedge, _central(f, edge, h))
    print({k: f"{v:.1e}" for k, v in worst.items()})


# ---- 3. the fp32 restatement's own distance to the references, at every case of the device table --------------------------------
# Norm-wise; the kernels are held to 1e-5 against the same references.  Observed: the row-wise outputs stay below 5e-7 at every case;
# the sums over all rows are the worst -- gate db 1.8e-6 at 8197x50x64, attention g_a / g_M 2.5e-6 / 2.4e-6 at 16421x24x32 and
# 2.8e-6 / 2.9e-6 at 16387x100x128 (numpy adds the 16 k float32 rows of a mean-zero column one after the other).
HEADROOM = 3e-6


def _headroom(name, got, want, case):
    e = rel_err(got, want)
    assert e < HEADROOM, f"{name} at {case}: the fp32 restatement is {e:.2e} from the fp64 reference (change the input, not the bound)"
    return e


@pytest.mark.parametrize("case", MC.GATE_CASES, ids=MC.case_id)
def test_gate_restatement_is_within_headroom_of_the_fp64_reference(case):
    t = MC.gate_inputs(*case)
    acc, dy_scale = MC.GATE_ARGS[case]
    prev = t["prev"] if acc else None
    got = restated_gate(t["X"], t["W"], t["b"], t["dY"], dy_scale, prev)
    want = MC.gate_ref(t["X"], t["W"], t["b"], t["dY"], dy_scale, prev)
    print(case, {k: f"{_headroom('gate ' + k, g, w, case):.1e}" for k, g, w in zip(("Y", "S", "Q", "dX", "dW", "db"), got, want)})


@pytest.mark.parametrize("case", MC.ROW_CASES, ids=MC.case_id)
def test_attention_restatement_is_within_headroom_of_the_fp64_reference(case):
    t = MC.attention_inputs(*case)
    with_half, acc, dh = MC.ATT_ARGS[case]
    args = (t["es"], t["a"], t["M"], t["half"] if with_half else None, t["dOut"], t["de_prev"] if acc else None,
            t["dhalf_prev"] if dh == "accumulate" else None)
    got, want = restated_attention(*args), MC.attention_ref(*args)
    seen = {}
    for name, g, w in zip(("v", "score", "out", "de", "dhalf", "g_a", "g_M"), got, want):
        for k, (gk, wk) in enumerate(zip(g, w) if name == "de" else [(g, w)]):
            seen[f"{name}{k if name == 'de' else ''}"] = f"{_headroom('attention ' + name, gk, wk, case):.1e}"
    print(case, seen)


@pytest.mark.parametrize("case", MC.ROW_CASES, ids=MC.case_id)
def test_hss_restatement_is_within_headroom_of_the_fp64_reference(case):
    t = MC.hss_inputs(*case)
    got, want = restated_hss(t["em"], t["edge"], t["perm"], MC.HSS_SCALE[case]), MC.hss_ref(t["em"], t["edge"], t["perm"], MC.HSS_SCALE[case])
    assert abs(got[0] - want[0]) <= HEADROOM * abs(want[0])
    print(case, {k: f"{_headroom('hss ' + k, g, w, case):.1e}" for k, g, w in zip(("dem", "dedge"), got[1:], want[1:])})


@pytest.mark.parametrize("case", MC.L2NORM_CASES, ids=MC.case_id)
def test_l2norm_restatement_is_within_headroom_of_the_fp64_reference(case):
    t = MC.l2norm_inputs(*case)
    got, want = restated_l2norm(t["X"], t["S0"], t["dS"]), MC.l2norm_ref(t["X"], t["S0"], t["dS"])
    print(case, {k: f"{_headroom('l2norm ' + k, g, w, case):.1e}" for k, g, w in zip(("inv", "S", "dX"), got, want)})


def test_every_argument_value_occurs_at_a_small_and_at_a_wrapped_case():
    small = set(MC.SMALL + MC.FULL_WIDTH)
    for table, cases in ((MC.GATE_ARGS, MC.GATE_CASES), (MC.ATT_ARGS, MC.ROW_CASES), ({k: (v,) for k, v in MC.HSS_SCALE.items()}, MC.ROW_CASES)):
        assert set(table) == set(cases)
        for pos in range(len(next(iter(table.values())))):
            values = {v[pos] for v in table.values()}
            assert values == {table[c][pos] for c in cases if c in small} == {table[c][pos] for c in cases if c not in small}, (pos, values)


def test_trainer_refuses_more_than_128_factors_before_it_allocates():
    from qrec_amd.graph import MHCNTrainer
    with pytest.raises(ValueError, match="num.factors"):
        MHCNTrainer(np.zeros((4, 129), np.float32), np.zeros((3, 129), np.float32), {}, [], None, 1, 0.001, 0.01, 0.05)
