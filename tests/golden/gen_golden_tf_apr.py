#!/usr/bin/env python3
"""Golden vectors for the reference's APR (model/ranking/APR.py), produced by running the reference's OWN class with
``tests/golden/tf1shim.py`` standing in for ``tensorflow`` -- the harness of ``gen_golden_tf.py`` (run_tf_model, base_conf,
make_subset), imported from there; nothing of the reference's text is stored here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tf_apr.py

Needs the reference tree (build container only).  Writes, next to this file:
  tf_apr_filmtrust.npz         the unmodified class on the first N_USERS users of FilmTrust: batch 64, 6 epochs (3 of pretraining, 3
                               adversarial), d = 8, ``-regA 2 -eps 0.5``.  The initial tables, every training step's (u, i, j) with
                               offsets, per-step losses (``total_loss`` in pretraining, ``loss_adv`` after), the gradients of the first
                               pretraining step (grad0_*) and of the first adversarial step (grad1_*) with the tables that step started
                               from (pre1_*), the final tables, the score tables the class ranks with, the training triplets in id form
                               the test pairs and ``py_state0``, CPython's
                               generator when the first epoch is drawn.  The file feeds the NEGATIVES as ``v_idx`` of the perturbation update
                               (APR.py:116-117), so both perturbation tables stay exactly zero: ASSERTED here after every update.
  tf_apr_paper_filmtrust.npz   the same run with the fed ``v_idx`` of that one Session.run replaced by the batch's positives (a wrapper
                               around Session.run, in memory; the class's file is not touched) -- the update of the paper.  The same
                               arrays, plus the perturbations after the first and after the last update as touched joint rows
                               (``delta_*_rows``: user u = row u, item i = row n_users + i) and their values (``delta_*_val``); every
                               other row is asserted zero.
  golden_tf_apr.json           sizes, hyper-parameters, the measures, the conf text, what the first adversarial batch holds
  tf_apr_f64_yardstick.npz     both runs with the stand-in's arithmetic in float64 (TF1SHIM_DTYPE=float64, a child process; same
                               seeds, every fed array asserted identical): the moving arrays under ``<name>/<key>``, float64.

What the stand-in lacks for this model is closed HERE, at run time, and tf1shim.py stays as it is: ``tf.zeros``, ``tf.constant``,
``tf.nn.softplus`` and ``tf.gradients`` (torch.autograd.grad of the evaluated loss with respect to the variables' values, all
requested variables in one call, so that both perturbation updates of one Session.run see the perturbations the run started with).
The files are written with fixed zip time stamps: regeneration is byte-identical."""
import io
import json
import os
import random
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G              # noqa: E402
import gen_golden_tf as T           # noqa: E402
import tf1shim                      # noqa: E402

NAME, PAPER = "tf_apr_filmtrust", "tf_apr_paper_filmtrust"
YARD = "tf_apr_f64_yardstick"
SEED = 211
N_USERS = 80
N_EPOCHS = 6
OPTIONS = "-eps 0.5 -regA 2 -advEpoch 3"
MOVING = ("final_", "grad0_", "grad1_", "pre1_", "score_", "losses", "delta_first_val", "delta_last_val")


def close_shim_gaps():
    import torch
    tf1shim.zeros = lambda shape, dtype=None, name=None: np.zeros(tuple(int(s) for s in shape), tf1shim.NPDT)
    if not hasattr(tf1shim, "constant"):
        tf1shim.constant = lambda value, dtype=None, shape=None, name=None: tf1shim._const(value)
    tf1shim.nn.softplus = tf1shim._unary(torch.nn.functional.softplus)

    def gradients(ys, xs, name=None, **kw):
        xs = list(xs)
        assert all(isinstance(x, tf1shim.Variable) for x in xs)
        whole = tf1shim.Tensor(lambda ctx, y: tuple(torch.autograd.grad(y, [x.value for x in xs], retain_graph=True)), [tf1shim._t(ys)])
        return [tf1shim.Tensor(lambda ctx, p, k=k: p[k], [whole]) for k in range(len(xs))]
    tf1shim.gradients = gradients


def save_npz(path, arrays):
    """np.savez_compressed with fixed member time stamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o600 << 16
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zf.writestr(zi, buf.getvalue())


def touched(D_u, D_v, u, items):
    """(joint rows, values) of a pair of perturbation tables that may be non-zero at the batch's rows only"""
    nu = D_u.shape[0]
    J = np.concatenate([D_u, D_v])
    rows = np.concatenate([np.unique(u), nu + np.unique(items)]).astype(np.int32)
    rest = np.ones(J.shape[0], bool); rest[rows] = False
    assert not J[rest].any(), "a perturbation row outside the batch is not zero"
    return rows, J[rows]


def run_case(tmp, out_dir, name, paper):
    import importlib
    F = tf1shim.NPDT                  # the moving arrays keep the run's own precision (float64 in the yardstick child)
    T.N_SUBSET_USERS = N_USERS
    ratings, n_rows = T.make_subset(tmp)
    conf = T.base_conf(tmp, ratings, model__name="APR", batch_size="64", num__max__epoch=str(N_EPOCHS), APR=OPTIONS)
    cls = importlib.import_module("model.ranking.APR").APR
    state, updates = {}, []
    inner_batches, inner_run = cls.next_batch_pairwise, tf1shim.Session.run

    def next_batch_pairwise(self):            # the batch the loop body is working on: the update's run does not see its positives
        state["model"] = self
        state.setdefault("py_state0", random.getstate())       # CPython's generator when the first epoch is drawn
        for batch in inner_batches(self):
            state["batch"] = [np.array(x, np.int64) for x in batch]
            yield batch
    cls.next_batch_pairwise = next_batch_pairwise

    def run(self, fetches, feed_dict=None, **kw):
        m = state.get("model")
        fl = fetches if isinstance(fetches, (list, tuple)) else [fetches]
        if m is None or len(fl) != 2 or fl[0] is not m.update_U or fl[1] is not m.update_V:
            return inner_run(self, fetches, feed_dict, **kw)
        u, i, j = state["batch"]
        fed = {k: np.array(feed_dict[getattr(m, k)], np.int64) for k in ("u_idx", "v_idx", "neg_idx")}
        assert np.array_equal(fed["u_idx"], u) and np.array_equal(fed["v_idx"], j) and np.array_equal(fed["neg_idx"], j)
        if paper:
            feed_dict = dict(feed_dict); feed_dict[m.v_idx] = i.tolist()
        out = inner_run(self, [m.update_U, m.update_V, m.grad_U_dense, m.grad_V_dense], feed_dict, **kw)
        val = lambda v: v.value.detach().numpy().copy()
        updates.append(dict(u=u, i=i, j=j, D_u=val(m.adv_U), D_v=val(m.adv_V), G_u=np.array(out[2]), G_v=np.array(out[3])))
        return out[:2]
    tf1shim.Session.run = run
    try:
        def after(m):
            te_u, te_i = [], []
            for user, items in m.data.testSet_u.items():
                for item in items:
                    te_u.append(m.data.user.get(user, -1)); te_i.append(m.data.item.get(item, -1))
            return dict(test_uid=np.array(te_u, np.int32), test_iid=np.array(te_i, np.int32),
                        score_U=np.asarray(m.P, F), score_V=np.asarray(m.Q, F))
        rec = T.run_tf_model(conf, SEED, "model.ranking.APR", "APR", after=after)
    finally:
        tf1shim.Session.run = inner_run
        cls.next_batch_pairwise = inner_batches
    m = rec["model"]
    steps = rec["steps"]
    n_adv = len(updates)
    n_pre = len(steps) - n_adv
    assert n_adv > 0 and n_pre == n_adv and N_EPOCHS // 2 * (n_pre // (N_EPOCHS // 2)) == n_pre
    order0 = np.array(rec["order0"], dtype=np.int32)
    arrays = dict(train_uid=order0[:, 0], train_iid=order0[:, 1], train_r=np.array(rec["rating0"], np.float32))
    arrays.update(rec["extra"])
    arrays["py_state0"] = np.array(state["py_state0"][1], dtype=np.uint32)
    U, V = m.user_embeddings, m.item_embeddings
    fs_pre, fs_adv = rec["first_steps"]
    assert (fs_pre["step"], fs_adv["step"]) == (0, n_pre)
    for vn, v in (("U", U), ("V", V)):
        arrays[f"init_{vn}"] = v.initial.astype(np.float32)
        arrays[f"final_{vn}"] = v.value.detach().numpy().astype(F)
        arrays[f"grad0_{vn}"] = fs_pre["grads"][v.index].astype(F)
        arrays[f"grad1_{vn}"] = fs_adv["grads"][v.index].astype(F)
        arrays[f"pre1_{vn}"] = fs_adv["before"][v.index].astype(F)
    feeds = lambda key: [s["feeds"][key].astype(np.int32) for s in steps]
    arrays["batch_offsets"] = np.concatenate([[0], np.cumsum([x.size for x in feeds("u_idx")])]).astype(np.int64)
    arrays["batch_u"], arrays["batch_i"], arrays["batch_j"] = (np.concatenate(feeds(k)) for k in ("u_idx", "v_idx", "n_idx"))
    for k, up in enumerate(updates):          # the update of an adversarial batch precedes that batch's step
        s = steps[n_pre + k]["feeds"]
        assert np.array_equal(s["u_idx"], up["u"]) and np.array_equal(s["v_idx"], up["i"]) and np.array_equal(s["n_idx"], up["j"])
    arrays["losses"] = np.array([float(s["out"][0]) for s in steps], np.float64)
    zero = [not up["D_u"].any() and not up["D_v"].any() for up in updates]
    first = updates[0]
    info = dict(perturbations_zero_after_every_update=bool(all(zero)), n_updates=n_adv)
    if paper:
        assert not any(zero)
        for tag, up in (("first", updates[0]), ("last", updates[-1])):
            arrays[f"delta_{tag}_rows"], val = touched(up["D_u"], up["D_v"], up["u"], np.concatenate([up["i"], up["j"]]))
            arrays[f"delta_{tag}_val"] = val.astype(F)
        rows = arrays["delta_first_rows"]
        gsq = (np.concatenate([first["G_u"], first["G_v"]]).astype(np.float64)[rows] ** 2).sum(1)
        both = np.intersect1d(first["i"], first["j"])
        slots = int(np.bincount(first["u"]).max())
        assert both.size >= 1, "no item of the first adversarial batch is a positive of one triplet and a negative of another"
        assert slots >= 4, "no user of the first adversarial batch holds four slots"
        assert gsq.min() > 1e-6, "a touched row of the first adversarial batch sits at the l2_normalize clamp"
        nu = len(m.data.user)
        info.update(first_batch=dict(items_positive_and_negative=int(both.size), max_user_slots=slots, min_gamma_sq=float(gsq.min()),
                                     user_rows=int((rows < nu).sum()), item_rows=int((rows >= nu).sum()),
                                     max_abs_delta=float(np.abs(arrays["delta_first_val"]).max())))
    else:
        assert all(zero), "the reference feed left a non-zero perturbation"
        assert all(not up["G_u"].any() and not up["G_v"].any() for up in updates)
    save_npz(os.path.join(out_dir, name + ".npz"), arrays)
    return dict(name=name, seed=SEED, shim_dtype=str(tf1shim.DT), perturb="paper" if paper else "reference", n_users=len(m.data.user),
                n_items=len(m.data.item), n_train=int(order0.shape[0]), n_epochs=N_EPOCHS, n_steps=len(steps), n_pretrain_steps=n_pre,
                batch_size=m.batch_size, emb_size=m.emb_size, lr=m.lRate, regU=m.regU, regA=2.0, eps=0.5, measure=rec["measure"],
                conf=open(conf).read(), subset=dict(source="dataset/FilmTrust/ratings.txt", first_users=N_USERS, rows=n_rows), **info)


def run_cases(out_dir):
    G.install_stubs()
    sys.modules["tensorflow"] = tf1shim
    close_shim_gaps()
    metas = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.symlink(os.path.join(T.REF, "dataset"), os.path.join(tmp, "dataset"))
        cwd = os.getcwd(); os.chdir(tmp)
        try:
            for name, paper in ((NAME, False), (PAPER, True)):
                meta = metas[name] = run_case(tmp, out_dir, name, paper)
                print(name, "steps", meta["n_steps"], "users", meta["n_users"], "items", meta["n_items"], meta.get("first_batch", ""), flush=True)
        finally:
            os.chdir(cwd)
    return metas


def main():
    if "--float64-child" in sys.argv:     # started below with TF1SHIM_DTYPE=float64: the same runs, written to a scratch directory
        assert os.environ.get("TF1SHIM_DTYPE") == "float64" and str(tf1shim.DT).endswith("float64")
        run_cases(sys.argv[sys.argv.index("--float64-child") + 1])
        return
    metas = run_cases(HERE)
    with open(os.path.join(HERE, "golden_tf_apr.json"), "w") as f:
        json.dump(metas, f, indent=1, sort_keys=True, default=str)
    out = {}
    err = lambda x, y: float(np.abs(x.astype(np.float64) - y).max() / np.abs(y).max())
    with tempfile.TemporaryDirectory() as scratch:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--float64-child", scratch], check=True,
                       env=dict(os.environ, TF1SHIM_DTYPE="float64", PYTHONDONTWRITEBYTECODE="1"))
        for name in (NAME, PAPER):
            a, b = np.load(os.path.join(HERE, name + ".npz")), np.load(os.path.join(scratch, name + ".npz"))
            assert a.files == b.files
            for k in a.files:
                if k.startswith(MOVING):
                    out[f"{name}/{k}"] = b[k].astype(np.float64)
                else:
                    assert np.array_equal(a[k], b[k]), (name, k, "the float64 run left the float32 run's inputs")
            print(name, "float32 run vs float64 run:", {k: err(a[k], b[k]) for k in a.files if k.startswith(MOVING) and np.abs(b[k]).max() > 0})
    save_npz(os.path.join(HERE, YARD + ".npz"), out)
    for f in (NAME + ".npz", PAPER + ".npz", YARD + ".npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
