"""GPU side of IRGAN: the kernels of csrc/irgan.hip against the float64 mirror (tests/irgan_mirror.py) on built cases
(tests/irgan_cases.py::kernel_case), the trainer on the reference's recorded run (tests/golden/tf_irgan_filmtrust.npz) with its draws
injected, the drop-in class end to end in exact mode, and throughput mode.  Every numeric assertion goes through helpers.check."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import irgan_cases as C
import irgan_mirror as M
from helpers import check, conf_from_text, rel_err, same_bits

pytestmark = pytest.mark.gpu

K_DRAWS = 40            # draws per row in the kernel tests: the edge uniforms, then random ones (rows of one or two live items repeat heavily)


def _trainer(v, csr, lr=0.001, reg=0.001, **kw):
    from qrec_amd.gan import IrganTrainer
    return IrganTrainer(v, csr[0], csr[1], lr, reg, **kw)


def _uniforms(rng, B):
    x = rng.random((B, K_DRAWS))
    x[:, :len(C.EDGE_UNIFORMS)] = C.EDGE_UNIFORMS
    return x


def _rows_once(n_items, d, B, mode):
    """row weights and draws of the first B users: (trainer arrays, given uniforms, samples with given / device uniforms)"""
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    v, csr = C.kernel_case(n_items, d)
    tr = _trainer(v, csr, seed=11)
    users = np.arange(B, dtype=np.int32)
    tr.row_weights(tr.gen, DeviceBuffer.from_numpy(users), B, mode)
    x = _uniforms(np.random.default_rng([n_items, d, B, mode]), B)
    ptr = DeviceBuffer.from_numpy(np.arange(B + 1, dtype=np.int64) * K_DRAWS)
    n = B * K_DRAWS
    given, drawn, again = (DeviceBuffer.zeros(n, np.int32) for _ in range(3))
    capi.irgan_draw(tr.w, tr.csum, n_items, B, ptr, n, DeviceBuffer.from_numpy(x), 0, 0, given)
    capi.irgan_draw(tr.w, tr.csum, n_items, B, ptr, n, None, 11, 3, drawn)
    reported = DeviceBuffer.zeros(n, np.float64)
    capi.irgan_uniforms(B, ptr, n, 11, 3, reported)
    capi.irgan_draw(tr.w, tr.csum, n_items, B, ptr, n, reported, 0, 0, again)
    out = dict(w=tr.w.numpy()[:B], p=tr.p.numpy()[:B], csum=tr.csum.numpy()[:B], given=given.numpy().reshape(B, K_DRAWS),
               drawn=drawn.numpy().reshape(B, K_DRAWS), again=again.numpy().reshape(B, K_DRAWS), reported=reported.numpy().reshape(B, K_DRAWS))
    return v, csr, x, out


def _check_rows(n_items, d, B):
    from qrec_amd import capi
    for mode, name in ((capi.IRGAN_NEGATIVES, "negatives"), (capi.IRGAN_MIXTURE, "mixture")):
        v, csr, x, a = _rows_once(n_items, d, B, mode)
        what = f"IRGAN {name} n_items={n_items} d={d} B={B}"
        want_w, want_p, rows = [], [], []
        for u in range(B):
            pos = C.pos_of(csr, u)
            z = M.logits(v["g_P"], v["g_Q"], v["g_b"], u)
            if mode == capi.IRGAN_NEGATIVES:
                w = M.negative_weights(z, pos) if pos.size else np.exp(z / M.TEMPERATURE - (z / M.TEMPERATURE).max())
                p = None
            elif pos.size:
                p, w = M.mixture(z, pos)
            else:
                continue                                   # the mixture is not defined for a user without positives (lambda / 0)
            rows.append(u); want_w.append(w); want_p.append(p)
        if not rows:
            continue
        rows = np.array(rows); want_w = np.array(want_w)
        check(f"{what}: weights", rel_err(a["w"][rows], want_w), C.GRAD_TOL)
        if mode == capi.IRGAN_MIXTURE:
            check(f"{what}: p", rel_err(a["p"][rows], np.array(want_p)), C.GRAD_TOL)
        check(f"{what}: row totals", rel_err(a["csum"][rows, -1], want_w.sum(1)), C.GRAD_TOL)
        assert (np.diff(a["csum"], axis=1) >= 0).all()
        for k, u in enumerate(rows):
            cdf = M.cdf(want_w[k])
            for key, xs in (("given", x[u]), ("drawn", a["reported"][u])):
                idx = a[key][u]
                assert ((idx >= 0) & (idx < n_items)).all(), (what, key, u)
                assert C.in_band(cdf, xs, idx).all(), (what, key, u, idx[~C.in_band(cdf, xs, idx)], xs[~C.in_band(cdf, xs, idx)])
                assert (want_w[k][idx] > 0).all(), (what, key, u)                 # never an item of zero weight
                if mode == capi.IRGAN_NEGATIVES:
                    assert not np.isin(idx, C.pos_of(csr, u)).any(), (what, key, u)
        assert ((a["reported"] >= 0) & (a["reported"] < 1)).all()
        assert np.array_equal(a["drawn"], a["again"]), what       # device-drawn mode = given-uniform mode fed the reported uniforms
        if n_items > 64:
            assert (a["drawn"] != a["given"]).any()
        same_bits(what, a, _rows_once(n_items, d, B, mode)[3])


@pytest.mark.parametrize("d", C.WIDTHS)
@pytest.mark.parametrize("n_items", C.N_ITEMS)
def test_row_weights_and_draws_match_the_mirror_and_repeat_their_bits(n_items, d):
    _check_rows(n_items, d, 64)


@pytest.mark.parametrize("B", [1, 5])
def test_row_weights_and_draws_of_small_blocks(B):
    _check_rows(257, 50, B)
    _check_rows(65, 64, B)


def _steps_once(n_items, d, reg=0.01, lr=0.001):
    """per special user one generator step without update (raw gradients), then three generator and three discriminator steps with
    Adam; the mirror takes the samples the device drew"""
    v, csr = C.kernel_case(n_items, d)
    tr = _trainer(v, csr, lr=lr, reg=reg, seed=5, keep_raw_gradients=True)
    out, samples = {}, {}
    users = [u for u in (0, 1, 2, 9) if C.pos_of(csr, u).size]
    for u in users:
        tr.generator_step(u, apply=False)
        samples[u] = tr.last_samples().copy()
        out[f"reward_{u}"] = tr.last_rewards().copy(); out[f"loss_{u}"] = np.array([tr.loss()])
        out.update({f"{k}_{u}": x for k, x in tr.raw_gradients().items()})
    rng = np.random.default_rng([n_items, d])
    B = 37
    bu, bi = rng.integers(0, C.N_USERS, B).astype(np.int32), rng.integers(0, n_items, B).astype(np.int32)
    bu[:4] = bu[4]; bi[:3] = bi[5]                      # rows and items that occur several times in the batch
    by = (rng.random(B) < 0.4).astype(np.float32)
    tr.discriminator_step(bu, bi, by, apply=False)
    out["dis_loss"] = np.array([tr.loss()])
    out.update({f"dis_{k}": x for k, x in tr.raw_gradients().items()})
    trained = []
    for k in range(3):
        u = users[k % len(users)]
        tr.discriminator_step(bu, bi, by)
        tr.generator_step(u)
        trained.append((u, tr.last_samples().copy()))
    out.update({f"trained_{k}": x for k, x in tr.parameters().items()})
    return v, csr, tr, (bu, bi, by), samples, trained, out


@pytest.mark.parametrize("d", C.WIDTHS)
@pytest.mark.parametrize("n_items", C.N_ITEMS[1:])
def test_steps_match_the_mirror_and_repeat_their_bits(n_items, d):
    reg, lr = 0.01, 0.001
    v, csr, tr, (bu, bi, by), samples, trained, a = _steps_once(n_items, d, reg, lr)
    what = f"IRGAN n_items={n_items} d={d}"
    m = M.Mirror(v, lr, reg)
    for u, s in samples.items():
        pos = C.pos_of(csr, u)
        assert s.size == M.GEN_PER_POS * pos.size and ((s >= 0) & (s < n_items)).all()
        p, pn = M.mixture(M.logits(m.p["g_P"], m.p["g_Q"], m.p["g_b"], u), pos)
        rew = M.reward(m.p["d_P"], m.p["d_Q"], m.p["d_b"], u, s, p, pn)
        r = M.generator_gradients(m.p["g_P"], m.p["g_Q"], m.p["g_b"], u, s, rew, reg)
        check(f"{what} user {u}: rewards", rel_err(a[f"reward_{u}"], rew), C.GRAD_TOL)
        check(f"{what} user {u}: g", rel_err(a[f"g_{u}"], r["g"]), C.GRAD_TOL)
        check(f"{what} user {u}: loss", rel_err(a[f"loss_{u}"], r["loss"]), C.GRAD_TOL)
        gP = np.zeros_like(m.p["g_P"]); gP[u] = r["gP"]
        for k, want in (("g_P", gP), ("g_Q", r["gQ"]), ("g_b", r["gb"])):
            check(f"{what} user {u}: raw gradient of {k}", rel_err(a[f"{k}_{u}"], want), C.GRAD_TOL)
        absent = r["n"] == 0                              # rows of items no sample hit: exactly g_j P[u] (and g_j for the bias)
        assert np.array_equal(a[f"g_Q_{u}"][absent], a[f"g_{u}"][absent, None] * v["g_P"][u][None, :]), (what, u)
        assert np.array_equal(a[f"g_b_{u}"][absent], a[f"g_{u}"][absent]), (what, u)
        if u == 1:                                        # 3 (n_items - 1) samples over n_items items: heavy duplicates
            assert np.bincount(s).max() >= 3
    r = M.discriminator_gradients(m.p["d_P"], m.p["d_Q"], m.p["d_b"], bu, bi, by, reg)
    check(f"{what}: discriminator loss", rel_err(a["dis_loss"], r["loss"]), C.GRAD_TOL)
    check(f"{what}: dz", rel_err(a["dis_dz"], r["dz"]), C.GRAD_TOL)
    for k, want in (("d_P", r["gP"]), ("d_Q", r["gQ"]), ("d_b", r["gb"])):
        check(f"{what}: discriminator gradient of {k}", rel_err(a[f"dis_{k}"], want), C.GRAD_TOL)
    for u, s in trained:
        m.discriminator_step(bu, bi, by)
        m.generator_step(u, C.pos_of(csr, u), s)
    for k in C.VARS:
        check(f"{what}: {k} after three Adam steps", rel_err(a[f"trained_{k}"], m.p[k]), C.GRAD_TOL)
    assert tr.padding_is_zero()
    same_bits(what, a, _steps_once(n_items, d, reg, lr)[6])


def test_kernels_refuse_a_width_above_the_supported_one():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer
    buf = DeviceBuffer.zeros(4096, np.float32)
    for d, ld in ((300, 512), (64, 64), (256, 256)):
        with pytest.raises(capi.QRecError) as e:
            capi.irgan_row_weights(buf, buf, 1, 1, d, ld, buf, 1, buf, buf, capi.IRGAN_NEGATIVES, 0.2, 0.0, buf, buf, buf, buf, buf)
        assert e.value.code == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.QRecError) as e:
            capi.irgan_dis_slots(buf, buf, 1, 1, d, ld, buf, buf, buf, 1, 0.1, buf, buf, buf, buf, buf, buf, buf)
        assert e.value.code == capi.ERR_UNSUPPORTED
    v, csr = C.kernel_case(63, 8)
    wide = {k: np.zeros((x.shape[0], 256), np.float32) if x.ndim == 2 else x for k, x in v.items()}
    with pytest.raises(ValueError):
        _trainer(wide, csr)
    full = (np.array([0, 63] + [63] * (C.N_USERS - 1), np.int64), np.arange(63, dtype=np.int32))      # user 0 rated every item
    with pytest.raises(ValueError):
        _trainer(v, full)


# ---- the recorded run -------------------------------------------------------------------------------------------------------------------
class _Recorded:
    """the trainer behind the interface tests/irgan_cases.py::run_recorded drives"""

    def __init__(self):
        m = C.META
        self.tr = _trainer(C.initial(), C.positives_csr(), m["lr"], m["regU"], keep_raw_gradients=True)
        self.d_steps = self.g_steps = 0

    def discriminator_step(self, u, i, y):
        self.tr.discriminator_step(u, i, y)
        out = dict(loss=self.tr.loss())
        if self.d_steps == 0:
            g = self.tr.raw_gradients()
            out.update(gP=g["d_P"], gQ=g["d_Q"], gb=g["d_b"])
        self.d_steps += 1
        return out

    def generator_step(self, u, pos, samples):
        self.tr.generator_step(u, samples=samples)
        out = dict(loss=self.tr.loss())
        if self.g_steps == 0:
            g = self.tr.raw_gradients()
            out.update(gP_full=g["g_P"], gQ=g["g_Q"], gb=g["g_b"])
        self.g_steps += 1
        return out

    def snapshot(self):
        return self.tr.parameters()


def _run_fixture():
    rec = _Recorded()
    r = C.run_recorded(rec)
    out = dict(losses_d=r["losses_d"], losses_g=r["losses_g"])
    out.update({f"grad0_{k}": x for k, x in r["grad0"].items()})
    out.update({f"grad1_{k}": x for k, x in r["grad1"].items()})
    for k, snap in enumerate(r["snaps"]):
        out.update({f"snap{k}_{v}": x for v, x in snap.items()})
    assert rec.tr.padding_is_zero()
    return out


def test_trainer_reproduces_the_reference_run_twice_bit_identically():
    """first-step gradients of both train ops and all 610 losses at 1e-5 of the reference's run; every snapshot (after the
    discriminator epoch and after each generator pass; the last is the final state) at max(1e-5, 2.5 floors) of the reference's run
    and of its float64 re-run (floor = distance between the two committed files); a second run has the same bits"""
    z, a = C.load(), _run_fixture()
    check("IRGAN discriminator losses vs the reference run", rel_err(a["losses_d"], z["losses_d"]), C.GRAD_TOL)
    check("IRGAN generator losses vs the reference run", rel_err(a["losses_g"], z["losses_g"]), C.GRAD_TOL)
    for v in C.VARS:
        k = "grad0" if v.startswith("d_") else "grad1"
        check(f"IRGAN first-step gradient of {v}", rel_err(a[f"{k}_{v}"], z[f"{k}_{v}"]), C.GRAD_TOL)
    for s in range(C.N_SNAPS):
        for v in C.VARS:
            key = f"snap{s}_{v}"
            if not z[key].any():
                assert not a[key].any()                # the generator's bias before its first step
                continue
            bound = C.trained_bound(key, z)
            check(f"IRGAN floor of {key} (recorded)", C.floor_of(key, z), 1.0, kind="info")
            check(f"IRGAN {key} vs the reference run", rel_err(a[key], z[key]), bound, kind="floor")
            check(f"IRGAN {key} vs the float64 run", rel_err(a[key], C.yard(key)), bound, kind="floor")
    for v in C.VARS:
        assert np.array_equal(z[f"final_{v}"], z[f"snap5_{v}"])
    same_bits("IRGAN trainer", a, _run_fixture())


# ---- the drop-in class --------------------------------------------------------------------------------------------------------------------
def _measure_of(strings):
    out = {}
    for s in strings:
        if ":" in s:
            k, v = s.strip().split(":")
            out[k] = float(v)
    return out


def _model(monkeypatch, tmp_path, mode, seed=None):
    from qrec_amd.QRec import resolve_model
    monkeypatch.setenv("QREC_MODE", mode)
    if seed is not None:
        monkeypatch.setenv("QREC_SEED", str(seed))
    monkeypatch.chdir(tmp_path)
    train, test = C.train_test_lists()
    model = resolve_model("IRGAN")(conf_from_text(C.META["conf"]), train, test)
    with redirect_stdout(io.StringIO()):
        model.readConfiguration(); model.initializing_log()
        np.random.seed(41)                       # the initial variables come from numpy's global generator
        model.initModel()
    return model


def test_class_trains_in_exact_mode_on_the_reference_stream_and_evaluates_like_the_host(monkeypatch, tmp_path):
    """the class on the fixture's data: it consumes np.random.random_sample exactly as often as the reference's np.random.choice calls
    do (the generator-discriminator chain need not reproduce the reference's samples: a uniform within rounding of a CDF boundary may
    select the neighbouring item), its measure comes from the DeviceRanker, and the device lists are the numpy predictForRanking +
    heap lists on the trained tables -- scores at the same ids within 1e-5, and nothing left out that beats a list's last entry"""
    from qrec_amd.ranking import DeviceRanker
    from qrec_amd.util.measure import Measure
    from qrec_amd.util.qmath import find_k_largest
    z, m = C.load(), C.META
    model = _model(monkeypatch, tmp_path, "exact")
    assert model.user_order.tolist() == z["user_order"].tolist() and {u: p for u, p in model.pos.items()} == C.positives(z)
    buf = io.StringIO()
    with redirect_stdout(buf):
        np.random.seed(23)
        model.trainModel()
        after = np.random.get_state()
        model.evalRanking()
    want = np.random.RandomState(23)
    want.random_sample(m["n_uniforms"])
    assert np.array_equal(after[1], want.get_state()[1]) and after[2] == want.get_state()[2]
    assert len(model.draws) == 6 * len(model.user_order) and sum(s.size for _, s in model.draws) == m["n_uniforms"]
    for (u, s), (ru, rs) in zip(model.draws, C.draw_calls(z)):
        assert u == ru and s.size == rs.size
    for u, s in model.draws[:len(model.user_order)]:
        assert not set(s.tolist()) & set(model.pos[u])
    assert "g_epoch: 5" in buf.getvalue() and model.trainer.padding_is_zero()
    assert isinstance(model._ranker, DeviceRanker)
    got = _measure_of(model.measure)
    device = model.rank_all_test_users(10)
    rec_host, worst_score, worst_left = {}, 0.0, -np.inf
    for user in model.data.testSet_u:
        s = np.array(model.predictForRanking(user), dtype=np.float64)
        if model.data.containsUser(user):
            for item in model.data.trainSet_u[user]:
                s[model.data.item[item]] = 0
        ids, sc = find_k_largest(10, s)
        rec_host[user] = [(model.data.id2item[i], x) for i, x in zip(ids, sc)]
        dev_ids = [model.data.item[name] for name, _ in device[user]]
        dev_sc = np.array([x for _, x in device[user]])
        worst_score = max(worst_score, rel_err(dev_sc, s[dev_ids]))
        left = s.copy(); left[dev_ids] = -np.inf
        worst_left = max(worst_left, float(left.max() - dev_sc[-1]))
    check("IRGAN class: device list scores vs predictForRanking at the same ids", worst_score, C.GRAD_TOL)
    check("IRGAN class: best left-out host score above a device list's last score", worst_left, C.GRAD_TOL, inclusive=True)
    host = _measure_of(Measure.rankingMeasure(model.data.testSet_u, rec_host, [10]))
    for key in ("Recall", "NDCG"):
        check(f"IRGAN class: {key}@10, DeviceRanker vs the host procedure", abs(got[key] - host[key]), 0.002, inclusive=True, kind="statistical")


def test_class_trains_in_throughput_mode_bit_identically_without_the_host_generator(monkeypatch, tmp_path):
    runs = []
    for _ in range(2):
        model = _model(monkeypatch, tmp_path, "throughput", seed=7)
        np.random.seed(1)
        before = np.random.get_state()[1].copy()
        with redirect_stdout(io.StringIO()):
            model.trainModel()
            model.evalRanking()
        assert np.array_equal(np.random.get_state()[1], before) and not model.draws
        assert model.trainer.padding_is_zero()
        runs.append(model.trainer.parameters())
    same_bits("IRGAN throughput mode, QREC_SEED=7", runs[0], runs[1])
    other = _model(monkeypatch, tmp_path, "throughput", seed=8)
    with redirect_stdout(io.StringIO()):
        other.trainModel()
    assert not np.array_equal(other.trainer.parameters()["g_Q"], runs[0]["g_Q"])
    assert _measure_of(model.measure)["Recall"] > 0


def test_device_drawn_negatives_follow_the_mirrors_distribution_and_assemble_get_datas_rows():
    """throughput mode's get_data over the fixture's users: per user the frequencies of CHI2_REPEATS draws of 2 |pos| negatives against
    the mirror's prob (chi-square on pooled bins of expected count >= 5, refused at the 1e-6 level; numpy's own sampler is shown to
    pass at the same count in tests/test_irgan_cpu.py), and the rows assembled on the device"""
    z, m = C.load(), C.META
    order, pos = z["user_order"], C.positives(z)
    tr = _trainer(C.initial(), C.positives_csr(), m["lr"], m["regU"], seed=3)
    mir = M.Mirror(C.initial(), m["lr"], m["regU"])
    counts = np.zeros((order.size, m["n_items"]), np.int64)
    for step in range(C.CHI2_REPEATS):
        ptr, d_s, (d_u, d_i, d_y, n_rows) = tr.draw_negatives(order, None, step=step, assemble=True)
        s = d_s.numpy()
        for k in range(order.size):
            counts[k] += np.bincount(s[ptr[k]:ptr[k + 1]], minlength=m["n_items"])
    worst = 1.0
    for k, u in enumerate(order.tolist()):
        w = mir.negatives_weights(u, pos[u])
        assert not counts[k][w == 0].any()                                        # never a positive
        worst = min(worst, C.chi_square_p(counts[k], w / w.sum(), int(counts[k].sum())))
    check("IRGAN throughput draws: CHI2_LEVEL over the smallest chi-square p-value of a user", C.CHI2_LEVEL / max(worst, 1e-300), 1.0, kind="statistical")
    # the last call's rows: per user the positives ascending with label 1, then that call's draws with label 0
    ru, ri, ry = d_u.numpy()[:n_rows], d_i.numpy()[:n_rows], d_y.numpy()[:n_rows]
    want = M.get_data_rows(order.tolist(), {u: sorted(p) for u, p in pos.items()}, [s[ptr[k]:ptr[k + 1]] for k in range(order.size)])
    assert n_rows == 3 * m["n_train"] and all(np.array_equal(a, b) for a, b in zip((ru, ri, ry), want))
