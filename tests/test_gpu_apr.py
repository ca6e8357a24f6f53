"""GPU side of APR: the two kernels of csrc/apr.hip against the float64 mirror (tests/apr_mirror.py) on the cases of
tests/apr_cases.py, the trainer on both recorded runs of the reference's class (tests/golden/tf_apr_filmtrust.npz: the file's feed,
tf_apr_paper_filmtrust.npz: the paper's), and the drop-in class end to end in both modes.  Every numeric assertion goes through
helpers.check."""
import contextlib
import ctypes as CT
import io
import random
from contextlib import redirect_stdout

import numpy as np
import pytest

import apr_cases as C
import apr_mirror as M
from helpers import check, conf_from_text, pad_cols, same_bits

pytestmark = pytest.mark.gpu

MODES = ("reference", "paper")


@pytest.fixture(scope="module", autouse=True)
def _device():
    from qrec_amd import capi
    capi.init(0)
    yield


def _idx(a):
    from qrec_amd.capi import DeviceBuffer as DB
    return DB.from_numpy(np.ascontiguousarray(a, np.int32) if len(a) else np.zeros(1, np.int32))


class Tables:
    """the joint table and the perturbations of one case on the device, with what qrec_apr_perturb keeps between calls"""

    def __init__(self, E, nu, ld):
        from qrec_amd import capi
        from qrec_amd.capi import DeviceBuffer as DB
        self.capi, self.nu, self.n, self.d, self.ld = capi, nu, E.shape[0], E.shape[1], ld
        self.E = DB.from_numpy(pad_cols(np.asarray(E, np.float32), ld))
        self.D = DB.zeros((self.n, ld), np.float32)
        self.touched = capi.AprTouchedRows()
        self.ws = capi.AprWorkspace(capi.apr_perturb_workspace_bytes)
        self.step_ws = capi.AprWorkspace(capi.apr_step_workspace_bytes)
        self.dE = DB.zeros((self.n, ld), np.float32)
        self.loss = DB.zeros(3, np.float64)

    def set_delta(self, D):
        self.D.upload(pad_cols(np.asarray(D, np.float32), self.ld))

    def perturb(self, u, v, n):
        """one update; returns the whole padded perturbation buffer"""
        self.capi.apr_perturb(self.E, self.D, self.nu, self.n, self.d, self.ld, _idx(u), _idx(v), _idx(n), len(u), C.REG_ADV, C.EPS,
                              self.touched, self.ws)
        return self.D.numpy()

    def step(self, u, i, j, with_delta, ordered, reg=C.REG):
        """(losses [3], padded dE) of one qrec_apr_batch_loss_grad call"""
        self.dE.fill_bytes(0); self.loss.fill_bytes(0)
        self.capi.apr_batch_loss_grad(self.E, self.D if with_delta else None, self.nu, self.n, self.d, self.ld, _idx(u), _idx(i), _idx(j),
                                      len(u), reg, C.REG_ADV, self.dE, self.loss, ordered=self.step_ws if ordered else None)
        return self.loss.numpy(), self.dE.numpy()


def _check_delta(what, got, want, d, batch_rows, ctx):
    """a padded perturbation buffer against the mirror's table: live columns to 1e-5 of max |x|, pad lanes and the rows outside the
    batch +0 bit for bit"""
    check(f"{what}: perturbations vs the float64 mirror", C.err(got[:, :d], want), C.TOL, ctx=ctx)
    assert C.bits_zero(got[:, d:]), (what, "pad lanes", ctx)
    rest = np.ones(got.shape[0], bool); rest[batch_rows] = False
    assert C.bits_zero(got[rest]), (what, "rows outside the batch", ctx)
    assert np.isfinite(got).all()


def _rows(nu, u, v, n):
    return np.unique(np.concatenate([u, nu + np.asarray(v), nu + np.asarray(n)]))


# ---- the perturbation pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.sweep(), ids=C.case_id)
def test_perturbation_pass_matches_the_float64_mirror_over_two_calls(case):
    d, ld, B, nu, ni = case
    E, a, b = C.kernel_case(d, B, nu, ni)
    t, t2 = Tables(E, nu, ld), Tables(E, nu, ld)
    want = np.zeros(E.shape)
    for k, (u, v, n) in enumerate((a, b)):               # the second call reads the first call's rows and clears those it does not rewrite
        got, again = t.perturb(u, v, n), t2.perturb(u, v, n)
        want = M.perturb(E, want, nu, u, v, n, C.REG_ADV, C.EPS)
        _check_delta(f"APR perturb call {k}", got, want, d, _rows(nu, u, v, n), case)
        norms = np.linalg.norm(got[_rows(nu, u, v, n)].astype(np.float64), axis=1)
        check(f"APR perturb call {k}: |row| vs eps", np.abs(norms - C.EPS).max() / C.EPS, C.TOL, ctx=case)
        same_bits(f"APR perturb call {k}", dict(D=got), dict(D=again))


def test_one_user_repeated_through_the_batch_is_one_long_run():
    d, ld, nu, ni, E, (u, v, n) = C.long_run_case()
    got = Tables(E, nu, ld).perturb(u, v, n)
    _check_delta("APR perturb, one user in 257 slots", got, M.perturb(E, np.zeros(E.shape), nu, u, v, n, C.REG_ADV, C.EPS), d, _rows(nu, u, v, n), u.size)


@pytest.mark.parametrize("d,ld", C.DIMS)
def test_equal_positive_and_negative_feeds_leave_bit_zero_perturbations(d, ld):
    B, nu, ni = 257, 3, 4
    E, a, b = C.kernel_case(d, B, nu, ni)
    t = Tables(E, nu, ld)
    assert t.perturb(*a).any()                            # non-zero on entry: every row of the second call is read and rewritten
    got = t.perturb(b[0], b[2], b[2])
    assert C.bits_zero(got) and np.isfinite(got).all()
    L, _ = t.step(b[0], b[2], b[2], True, True)
    check("APR: adversarial loss term with every x' an exact 0 vs regAdv B ln 2", abs(L[2] - C.REG_ADV * B * M.LN2) / (C.REG_ADV * B * M.LN2), 1e-6)


def test_a_row_whose_gradient_is_exactly_zero_stays_zero():
    d, ld, nu, ni = 8, 32, 2, 3
    E = C.kernel_case(d, 1, nu, ni)[0]
    E[nu + 1] = E[nu + 0]                                 # two items with one embedding: the user's gradient is c' * 0
    u, v, n = np.array([1], np.int32), np.array([0], np.int32), np.array([1], np.int32)
    got = Tables(E, nu, ld).perturb(u, v, n)
    assert C.bits_zero(got[1]) and np.isfinite(got).all()
    _check_delta("APR perturb, a zero gradient row", got, M.perturb(E, np.zeros(E.shape), nu, u, v, n, C.REG_ADV, C.EPS), d, _rows(nu, u, v, n), None)
    assert got[nu + 0].any() and got[nu + 1].any()


def test_consecutive_calls_clear_the_previous_rows_and_an_empty_batch_clears_all():
    d, ld, nu, ni, E, first, second = C.consecutive_case()
    t = Tables(E, nu, ld)
    r1 = _rows(nu, *first)
    got1 = t.perturb(*first)
    assert got1[r1].any(1).all()
    got2 = t.perturb(*second)
    r2 = _rows(nu, *second)
    gone = np.setdiff1d(r1, r2)
    assert gone.size and C.bits_zero(got2[gone])
    want = M.perturb(E, M.perturb(E, np.zeros(E.shape), nu, *first, C.REG_ADV, C.EPS), nu, *second, C.REG_ADV, C.EPS)
    _check_delta("APR perturb, second of two calls (5 after 64 triplets)", got2, want, d, r2, None)
    empty = np.zeros(0, np.int32)
    assert C.bits_zero(t.perturb(empty, empty, empty))
    got3 = t.perturb(*first)                              # and the list starts over
    same_bits("APR perturb after an empty batch", dict(D=got1), dict(D=got3))


def test_rows_read_by_many_groups_while_they_are_rewritten():
    """B = 2048 over 64 x 64 tables, perturbations non-zero on entry: every row is read by dozens of producer groups and rewritten
    by the walk of the same call"""
    d, ld, nu, ni = C.HAZARD[:4]
    E, a, b = C.hazard_case()
    runs = []
    for _ in range(2):
        t = Tables(E, nu, ld)
        first = t.perturb(*a)
        runs.append(dict(first=first, second=t.perturb(*b)))
    w1 = M.perturb(E, np.zeros(E.shape), nu, *a, C.REG_ADV, C.EPS)
    w2 = M.perturb(E, w1, nu, *b, C.REG_ADV, C.EPS)
    assert w1.any(1).all() and w2.any(1).all()
    _check_delta("APR perturb B = 2048, first call", runs[0]["first"], w1, d, _rows(nu, *a), None)
    _check_delta("APR perturb B = 2048, second call on the first call's perturbations", runs[0]["second"], w2, d, _rows(nu, *b), None)
    same_bits("APR perturb B = 2048", runs[0], runs[1])


# ---- the step kernel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.sweep(), ids=C.case_id)
def test_step_kernel_matches_the_float64_mirror(case):
    d, ld, B, nu, ni = case
    E, a, b = C.kernel_case(d, B, nu, ni)
    D = M.perturb(E, np.zeros(E.shape), nu, *b, C.REG_ADV, C.EPS).astype(np.float32)
    t = Tables(E, nu, ld)
    t.set_delta(D)
    for with_delta in (False, True):
        wL, wg = M.step(E, D if with_delta else None, nu, *a, C.REG, C.REG_ADV)
        L, g = t.step(*a, with_delta, ordered=True)
        L2, g2 = t.step(*a, with_delta, ordered=True)
        La, ga = t.step(*a, with_delta, ordered=False)
        tag = "with" if with_delta else "without"
        for k, name in enumerate(("sum softplus(-x)", "batch L2", "regAdv sum softplus(-x')")):
            if wL[k] == 0:
                assert L[k] == 0 and La[k] == 0
                continue
            check(f"APR step {tag} perturbations: {name} vs the mirror", abs(L[k] - wL[k]) / abs(wL[k]), C.TOL, ctx=case)
            check(f"APR step {tag} perturbations, atomics: {name} vs the mirror", abs(La[k] - wL[k]) / abs(wL[k]), C.TOL, ctx=case)
        check(f"APR step {tag} perturbations: dE vs the mirror", C.err(g[:, :d], wg), C.TOL, ctx=case)
        check(f"APR step {tag} perturbations: dE, atomics vs ordered", C.err(ga, g), C.TOL, ctx=case)
        assert C.bits_zero(g[:, d:]) and C.bits_zero(ga[:, d:])
        same_bits(f"APR step {tag} perturbations", dict(L=L, g=g), dict(L=L2, g=g2))


def test_step_kernel_is_finite_at_scores_of_plus_and_minus_90():
    d, ld, nu, ni = 8, 32, 1, 2
    E = np.zeros((nu + ni, d), np.float32)
    E[0], E[1] = 3.0, 3.75                                # x = 8 * 3 * 3.75 = 90 one way round, -90 the other
    u, i, j = np.array([0, 0], np.int32), np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    t = Tables(E, nu, ld)
    for with_delta in (False, True):
        for ordered in (True, False):
            L, g = t.step(u, i, j, with_delta, ordered, reg=0.0)
            wL, wg = M.step(E, np.zeros(E.shape) if with_delta else None, nu, u, i, j, 0.0, C.REG_ADV)
            assert np.isfinite(L).all() and np.isfinite(g).all()
            check("APR step at x = +-90: sum softplus(-x) vs the mirror", abs(L[0] - wL[0]) / wL[0], C.TOL, ctx=(with_delta, ordered))
            check("APR step at x = +-90: dE vs the mirror", C.err(g[:, :d], wg), C.TOL, ctx=(with_delta, ordered))
    t.set_delta(np.zeros(E.shape))
    assert np.isfinite(t.perturb(u, i, j)).all()


# ---- refused arguments --------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_on_the_host_with_a_message():
    from qrec_amd import capi
    from qrec_amd.capi import DeviceBuffer as DB
    L = capi.load()
    T, G, idx, loss = DB.zeros((100, 64), np.float32), DB.zeros((100, 64), np.float32), DB.zeros(16, np.int32), DB.zeros(3, np.float64)
    touched, ws = DB.zeros(1 + 48, np.int32), DB.zeros(1 << 20, np.uint8)
    p = lambda b: CT.c_void_p(b.ptr) if b is not None else None

    def perturb(E=T, D=G, d=50, ld=64, B=16, cap=48, w=ws, wb=None):
        return L.qrec_apr_perturb(p(E), p(D), 40, 100, d, ld, p(idx), p(idx), p(idx), B, 2.0, 0.5, p(touched), cap, p(w),
                                  (w.nbytes if w is not None else 0) if wb is None else wb, None, None)

    def step(E=T, dE=G, d=50, ld=64, B=16, w=ws, wb=None):
        return L.qrec_apr_batch_loss_grad(p(E), None, 40, 100, d, ld, p(idx), p(idx), p(idx), B, 0.01, 2.0, p(dE), p(loss), p(w),
                                          (w.nbytes if w is not None else 0) if wb is None else wb, None)

    def refused(code, *words):
        msg = L.qrec_last_error().decode()
        assert code < 0, code
        assert all(w in msg for w in words), msg

    assert perturb() == 0 and step() == 0                # the same calls with good arguments pass
    refused(perturb(ld=48), "qrec_apr_perturb", "row stride", "48")
    refused(perturb(ld=256), "qrec_apr_perturb", "row stride", "256")
    refused(perturb(d=65), "qrec_apr_perturb", "65 columns")
    refused(perturb(d=0), "qrec_apr_perturb", "columns")
    refused(perturb(wb=1024), "workspace", "needed")
    refused(perturb(w=None), "qrec_apr_perturb", "workspace")
    refused(perturb(B=-1), "qrec_apr_perturb", "negative")
    refused(perturb(E=None), "qrec_apr_perturb", "null table")
    refused(perturb(D=None), "qrec_apr_perturb", "null table")
    refused(perturb(cap=47), "qrec_apr_perturb", "touched-row list", "48")
    refused(step(ld=48), "qrec_apr_batch_loss_grad", "row stride", "48")
    refused(step(d=65), "qrec_apr_batch_loss_grad", "65 columns")
    refused(step(wb=1024), "qrec_apr_batch_loss_grad", "workspace", "needed")
    refused(step(B=-1), "qrec_apr_batch_loss_grad", "negative")
    refused(step(E=None), "qrec_apr_batch_loss_grad", "null")
    refused(step(dE=None), "qrec_apr_batch_loss_grad", "null")
    out = CT.c_int64(0)
    refused(L.qrec_apr_perturb_workspace_bytes(16, 48, CT.byref(out)), "row stride")
    refused(L.qrec_apr_step_workspace_bytes(16, 256, CT.byref(out)), "row stride")
    refused(L.qrec_apr_step_workspace_bytes(-1, 64, CT.byref(out)), "bad argument")
    assert capi.apr_step_workspace_bytes(16, 64) > capi.apr_perturb_workspace_bytes(16, 64) > 0


# ---- the trainer on the recorded runs -------------------------------------------------------------------------------------------------
def _train_recorded(mode):
    """the recorded batches through AprTrainer from the recorded initial tables, ordered reductions; what the fixture holds, as the
    trainer has it"""
    from qrec_amd.graph import AprTrainer, ordered_reductions
    z, h = C.load(mode), C.hyper(mode)
    nu = z["init_U"].shape[0]
    with ordered_reductions():
        tr = AprTrainer(z["init_U"], z["init_V"], h["lr"], h["reg"], h["reg_adv"], h["eps"], max_batch=64)
    out = dict(losses=[])
    zero = True
    for k, (u, i, j) in enumerate(C.batches(mode)):
        du, di, dj = _idx(u), _idx(i), _idx(j)
        if k < h["n_pretrain"]:
            tr.pretrain_step_async(du, di, dj, len(u))
            if k == 0:
                out["grad0"] = np.concatenate(tr.gradients())
        else:
            feeds = dict(reference=(du, dj, dj), paper=(du, di, dj))[mode]
            if k == h["n_pretrain"]:
                out["pre1"] = np.concatenate(tr.tables())
            tr.perturb_async(*feeds, len(u))
            if k in (h["n_pretrain"], len(C.batches(mode)) - 1):
                out["delta_first" if k == h["n_pretrain"] else "delta_last"] = tr.D.numpy()
            elif mode == "reference":
                zero = zero and C.bits_zero(tr.D.numpy())
            tr.adversarial_step_async(du, di, dj, len(u))
            if k == h["n_pretrain"]:
                out["grad1"] = np.concatenate(tr.gradients())
        out["losses"].append(tr.loss())
    out["losses"] = np.array(out["losses"])
    out["final"] = np.concatenate(tr.tables())
    return out, zero


@pytest.mark.parametrize("mode", MODES)
def test_trainer_follows_the_recorded_run_and_repeats_its_bits(mode):
    z, h = C.load(mode), C.hyper(mode)
    nu, d = z["init_U"].shape
    a, zero = _train_recorded(mode)
    b, _ = _train_recorded(mode)
    same_bits(f"APR trainer, {mode} feed", a, b)
    check(f"APR {mode}: losses of every step vs the reference run", C.err(a["losses"], z["losses"]), C.TOL)
    check(f"APR {mode}: first pretraining gradient vs the reference run", C.err(a["grad0"], C.joint(z, "grad0")), C.TOL)
    # the first adversarial step starts from the trainer's own tables, a rounding-level distance from the recorded ones
    check(f"APR {mode}: tables at the first adversarial step vs the reference run", C.err(a["pre1"][:nu], z["pre1_U"]), C.trained_bound(mode, "pre1_U"), kind="floor")
    check(f"APR {mode}: item tables at the first adversarial step vs the reference run", C.err(a["pre1"][nu:], z["pre1_V"]), C.trained_bound(mode, "pre1_V"), kind="floor")
    for k, rows in (("U", slice(0, nu)), ("V", slice(nu, None))):
        check(f"APR {mode}: final_{k} vs the reference run", C.err(a["final"][rows], z["final_" + k]), C.trained_bound(mode, "final_" + k), kind="floor")
        check(f"APR {mode}: final_{k} vs the float64 run", C.err(a["final"][rows], C.yard(mode)["final_" + k]), C.trained_bound(mode, "final_" + k), kind="floor")
    if mode == "reference":
        assert zero and C.bits_zero(a["delta_first"]) and C.bits_zero(a["delta_last"])
    else:
        for tag in ("first", "last"):
            want = C.dense_delta(z, tag, a["final"].shape[0])
            got = a["delta_" + tag]
            assert C.bits_zero(got[:, d:]) and np.array_equal(np.flatnonzero(got.any(1)), z[f"delta_{tag}_rows"])
            check(f"APR paper: perturbations after the {tag} update vs the reference run", C.err(got[:, :d], want), C.trained_bound(mode, f"delta_{tag}_val"), kind="floor")


@pytest.mark.parametrize("mode", MODES)
def test_trainer_first_adversarial_gradient_from_the_recorded_tables(mode):
    """the first adversarial step from the RECORDED tables it started from (pre1_*): update, then gradient, both against the fixture at
    the parity bar; the Adam slots do not enter the gradient"""
    from qrec_amd.graph import AprTrainer, ordered_reductions
    z, h = C.load(mode), C.hyper(mode)
    nu, d = z["init_U"].shape
    u, i, j = C.batches(mode)[h["n_pretrain"]]
    du, di, dj = _idx(u), _idx(i), _idx(j)
    with ordered_reductions():
        tr = AprTrainer(z["pre1_U"], z["pre1_V"], h["lr"], h["reg"], h["reg_adv"], h["eps"])
    tr.perturb_async(*dict(reference=(du, dj, dj), paper=(du, di, dj))[mode], len(u))
    if mode == "paper":
        check("APR paper: first perturbations from the recorded tables", C.err(tr.D.numpy()[:, :d], C.dense_delta(z, "first", nu + z["init_V"].shape[0])), C.TOL)
    tr.adversarial_step_async(du, di, dj, len(u))
    check(f"APR {mode}: first adversarial gradient vs the reference run", C.err(np.concatenate(tr.gradients()), C.joint(z, "grad1")), C.TOL)
    check(f"APR {mode}: first loss_adv vs the reference run", abs(tr.loss() - z["losses"][h["n_pretrain"]]) / z["losses"][h["n_pretrain"]], C.TOL)


# ---- the drop-in class --------------------------------------------------------------------------------------------------------------------
def _class_run(mode, monkeypatch, tmp_path):
    from qrec_amd import capi
    from qrec_amd.QRec import resolve_model
    monkeypatch.chdir(tmp_path)                    # the log and the measure file are written under the working directory
    monkeypatch.setenv("QREC_APR_PERTURB", mode)
    monkeypatch.delenv("QREC_MODE", raising=False); monkeypatch.delenv("QREC_QUIET", raising=False); monkeypatch.delenv("QREC_REDUCTIONS", raising=False)
    m, z = C.META[C.NAMES[mode]], C.load(mode)
    train, test = C.train_test_lists(mode)
    model = resolve_model("APR")(conf_from_text(m["conf"]), train, test)
    drawn = []
    inner = model.sample_epoch_pairwise

    def sample_epoch_pairwise():
        e = inner()
        drawn.append(e)
        return e
    model.sample_epoch_pairwise = sample_epoch_pairwise
    buf = io.StringIO()
    with redirect_stdout(buf):
        model.readConfiguration(); model.initializing_log(); model.initModel()
        model.user_embeddings, model.item_embeddings = z["init_U"], z["init_V"]
        random.setstate(capi.state_to_python(z["py_state0"], None))
        model.trainModel()
    return model, m, z, drawn, buf.getvalue()


@pytest.mark.parametrize("mode", MODES)
def test_class_replays_the_recorded_stream_and_reaches_the_recorded_measure(mode, monkeypatch, tmp_path):
    model, m, z, drawn, text = _class_run(mode, monkeypatch, tmp_path)
    assert len(drawn) == m["n_epochs"]
    for key, col in (("batch_u", 0), ("batch_i", 1), ("batch_j", 2)):
        assert np.array_equal(np.concatenate([e[col] for e in drawn]), z[key]), key
    lines = [l for l in text.splitlines() if " training: " in l and " loss: " in l]
    n_adv = m["n_steps"] - m["n_pretrain_steps"]
    assert len(lines) == n_adv and "pretraining..." in text and "adversarial training..." in text
    printed = np.array([float(l.split("loss:")[1]) for l in lines])
    check(f"APR class, {mode} feed: printed loss_adv of every adversarial batch vs the reference run", C.err(printed, z["losses"][m["n_pretrain_steps"]:]), C.TOL)
    for k, got in (("U", model.P), ("V", model.Q)):
        check(f"APR class, {mode} feed: final_{k} vs the reference run", C.err(got, z["final_" + k]), C.trained_bound(mode, "final_" + k), kind="floor")
    zero = C.bits_zero(model.trainer.D.numpy())
    assert zero == (mode == "reference")
    with redirect_stdout(io.StringIO()):
        model.evalRanking()
    recall = lambda lines: float(next(s for s in lines if s.startswith("Recall:")).split(":")[1])
    check(f"APR class, {mode} feed: Recall vs the recorded one", abs(recall(model.measure) - recall(m["measure"])), 0.002, inclusive=True, kind="statistical")
    # the ranker on the RECORDED score tables gives the recorded measure strings
    model.P, model.Q = z["score_U"], z["score_V"]
    with redirect_stdout(io.StringIO()):
        model.evalRanking()
    assert [s.strip() for s in model.measure] == [s.strip() for s in m["measure"]]


def _paired_run(mode, conf, train, test, seed):
    """the class on the device stream of ``seed`` (throughput) or on its host replay (exact), ordered reductions in both"""
    import device_stream as S
    from qrec_amd.QRec import resolve_model
    cls = resolve_model("APR")
    replay = S.replay_on_host(cls, seed) if mode == "exact" else contextlib.nullcontext()
    with S._environ(QREC_MODE=mode, QREC_SEED=seed, QREC_REDUCTIONS="ordered", QREC_QUIET=1, QREC_APR_PERTURB="paper"), replay, redirect_stdout(io.StringIO()):
        state = random.getstate()
        np.random.seed(3)
        m = cls(conf, train, test)
        m.readConfiguration(); m.initializing_log(); m.initModel()
        m.trainModel()
        assert m.throughput_mode() == (mode == "throughput") and random.getstate() == state
    return dict(P=np.ascontiguousarray(m.P), Q=np.ascontiguousarray(m.Q), D=m.trainer.D.numpy())


def test_throughput_mode_and_exact_mode_agree_byte_for_byte_on_one_stream(monkeypatch, tmp_path):
    """QREC_MODE=throughput draws the epochs on the device; the exact class fed the same stream from the host ends with the same bytes
    under ordered reductions.  Batch 64 over a row count that is no multiple of it: the tail batch and the pointer offsets into the
    epoch buffers are exercised, across the pretraining / adversarial hand-over of the one epoch stream."""
    monkeypatch.chdir(tmp_path)
    meta = C.META[C.NAMES["paper"]]
    train, test = C.train_test_lists("paper")
    conf = conf_from_text(meta["conf"]); conf["num.max.epoch"] = "4"
    assert len(train) % 64 not in (0,) and int(conf["batch_size"]) == 64
    thr = _paired_run("throughput", conf, train, test, 11)
    exact = _paired_run("exact", conf, train, test, 11)
    assert thr["D"].any()
    same_bits("APR class: throughput mode vs the exact class on the replayed device stream", thr, exact)
    other = _paired_run("throughput", conf, train, test, 12)
    assert not np.array_equal(other["P"], thr["P"])       # the comparison can fail: another seed is another stream
