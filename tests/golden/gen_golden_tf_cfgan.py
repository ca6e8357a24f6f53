#!/usr/bin/env python3
"""Golden vectors for the reference's CFGAN (model/ranking/CFGAN.py), produced by running the reference's OWN class unmodified
with ``tests/golden/tf1shim.py`` standing in for ``tensorflow`` -- the harness of ``gen_golden_tf.py`` (run_tf_model, base_conf,
make_subset), imported from there; nothing of the reference's text is stored here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tf_cfgan.py

Needs the reference tree (build container only).  Writes, next to this file:
  tf_cfgan_filmtrust.npz       CFGAN on the first N_USERS users of FilmTrust: batch 64, 12 epochs = 48 train-op runs in the pattern
                               D, G, G, G, the four runs of an epoch on identical feeds (asserted).  ``S_zr = S_pm = 0.05`` are set on
                               the instance by a wrapper around ``initModel``: at the class's 0.001 a catalogue of a few hundred items
                               draws int(0.3) = 0 negatives.  Per epoch ``mask`` and ``N_zr`` as packed bits (np.packbits over
                               [epochs, batch, n_items]) and ``batch_uid`` [epochs, batch]: the smallest user whose training row equals
                               the fed ``C[n]`` (one exists for every row, asserted; ``C`` is not stored).  The four variables before
                               and after (D_W1 flat [2 n_items]), the gradients of the first D step and of the first G step, ``d_losses``
                               [12], ``g_losses`` [12, 3], the training triplets in id form and the test pairs.
                               ``final_G_W1`` and ``grad0_G_W1`` are stored sparsely (``*_idx`` flat int32 index, ``*_val``): the final
                               table where its bits differ from ``init_G_W1`` (an entry that never receives gradient keeps m = v = 0 and
                               Adam leaves it bit-unchanged), the gradient where it is non-zero.
  golden_tf_cfgan.json         sizes, hyper-parameters, the measure, the conf text
  tf_cfgan_f64_yardstick.npz   the same run with the stand-in's arithmetic in float64 (TF1SHIM_DTYPE=float64, a child process; same
                               seeds, every fed array asserted identical): trained variables, first-step gradients and losses, the two
                               sparse ones as values at the float32 run's indices (every entry outside them is asserted unchanged / zero).

What the stand-in lacks for this model is closed HERE, at run time, and tf1shim.py stays as it is:
  * ``tf.get_variable(name=, initializer=, regularizer=)`` with an initializer that is already a value (the result of calling an
    initializer on a shape, or ``tf.zeros``): a Variable of that value; the regularizer only feeds a collection nobody reads;
  * ``tf.variable_scope`` (a no-op context), ``tf.zeros``, ``tf.contrib.layers.l2_regularizer``;
  * rank-1 xavier as gen_golden_tf_cdae.py closes it (not reached by this model: its two biases are zeros);
  * the placeholders ``mask`` and ``N_zr`` carry the same name, so the feeds are recorded by identity against the model's attributes."""
import contextlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G              # noqa: E402
import gen_golden_tf as T           # noqa: E402
import gen_golden_tf_cdae as CD     # noqa: E402
import tf1shim                      # noqa: E402

NAME = "tf_cfgan_filmtrust"
SEED = 137
N_USERS = 60
S_ZR = S_PM = 0.05
VARS = ("G_W1", "G_b1", "D_W1", "D_b1")
SPARSE = ("final_G_W1", "grad0_G_W1")
FEEDS = ("C", "mask", "N_zr")


def close_shim_gaps():
    CD.close_shim_gaps()

    def get_variable(name=None, shape=None, dtype=None, initializer=None, regularizer=None, trainable=True, **kw):
        assert initializer is not None and shape is None
        return tf1shim.Variable(initializer, name=name, trainable=trainable)
    tf1shim.get_variable = get_variable
    tf1shim.variable_scope = lambda *a, **kw: contextlib.nullcontext()
    tf1shim.zeros = lambda shape, dtype=None, name=None: np.zeros(tuple(shape), tf1shim.NPDT)
    tf1shim.contrib.layers.l2_regularizer = lambda scale, scope=None: (lambda w: None)


def sparse_of(a, changed):
    idx = np.flatnonzero(changed.ravel()).astype(np.int32)
    return idx, a.ravel()[idx].astype(np.float32)


def run_case(tmp, out_dir):
    import importlib
    T.N_SUBSET_USERS = N_USERS
    ratings, n_rows = T.make_subset(tmp)
    conf = T.base_conf(tmp, ratings, model__name="CFGAN", batch_size="64", num__max__epoch="12", learnRate="-init 0.002 -max 1")
    cls = importlib.import_module("model.ranking.CFGAN").CFGAN
    inner_init = cls.initModel

    def initModel(self):              # the instance attributes, before the first batch is drawn
        self.S_zr, self.S_pm = S_ZR, S_PM
        inner_init(self)
    cls.initModel = initModel
    fed = []                          # per Session.run that carries a train op: (the op, [(placeholder, array)])
    inner_run = tf1shim.Session.run

    def run(self, fetches, feed_dict=None, **kw):
        fl = fetches if isinstance(fetches, (list, tuple)) else [fetches]
        ops = [t for t in fl if isinstance(t, tf1shim._TrainOp)]
        if ops:
            fed.append((ops[0], [(k, np.array(v)) for k, v in (feed_dict or {}).items()]))
        return inner_run(self, fetches, feed_dict, **kw)
    tf1shim.Session.run = run
    try:
        def after(m):
            te_u, te_i = [], []
            for user, items in m.data.testSet_u.items():
                for item in items:
                    te_u.append(m.data.user.get(user, -1)); te_i.append(m.data.item.get(item, -1))
            return dict(test_uid=np.array(te_u, np.int32), test_iid=np.array(te_i, np.int32))
        rec = T.run_tf_model(conf, SEED, "model.ranking.CFGAN", "CFGAN", after=after)
    finally:
        tf1shim.Session.run = inner_run
        cls.initModel = inner_init
    m = rec["model"]
    assert (m.S_zr, m.S_pm, m.alpha) == (S_ZR, S_PM, 0.01)
    holders = {id(getattr(m, a)): a for a in FEEDS}
    steps = [(op, {holders[id(k)]: v for k, v in feeds}) for op, feeds in fed]
    n_epochs, B, ni = 12, m.batch_size, m.num_items
    assert len(steps) == 4 * n_epochs and all(sorted(s) == sorted(FEEDS) for _, s in steps)
    for e in range(n_epochs):         # D, G, G, G on identical feeds
        ops = [steps[4 * e + k][0] for k in range(4)]
        assert ops[0] is m.D_solver and all(o is m.G_solver for o in ops[1:])
        for k in range(1, 4):
            assert all(np.array_equal(steps[4 * e][1][f], steps[4 * e + k][1][f]) for f in FEEDS)
    epochs = [steps[4 * e][1] for e in range(n_epochs)]
    order0 = np.array(rec["order0"], dtype=np.int32)
    arrays = dict(train_uid=order0[:, 0], train_iid=order0[:, 1], train_r=np.array(rec["rating0"], np.float32))
    arrays.update(rec["extra"])
    R = np.zeros((len(m.data.user), ni))
    R[order0[:, 0], order0[:, 1]] = rec["rating0"]
    uid = np.zeros((n_epochs, B), np.int32)
    for e, s in enumerate(epochs):
        for n in range(B):            # C is the training rows of the drawn users and nothing else
            match = np.flatnonzero((R == s["C"][n]).all(1))
            assert match.size, (e, n)
            uid[e, n] = match[0]
        assert np.array_equal(s["C"], R[uid[e]])
        assert set(np.unique(s["mask"])) <= {0, 1} and set(np.unique(s["N_zr"])) <= {0, 1}
        assert (s["mask"] >= (s["C"] != 0)).all() and not (s["N_zr"] * (s["C"] != 0)).any()
    both = (epochs[0]["mask"] * epochs[0]["N_zr"]).sum(1)
    assert (both > 0).sum() >= B // 2, "N_zr and mask coincide in too few rows of the first step: the alpha term would go untested"
    arrays["batch_uid"] = uid
    for key in ("mask", "N_zr"):
        arrays[key + "_bits"] = np.packbits(np.stack([s[key] for s in epochs]).astype(bool), axis=None)
    by_name = {v.name: v for v in tf1shim.all_variables() if v.name in VARS}
    assert sorted(by_name) == sorted(VARS)
    assert [by_name[v].index for v in VARS] == sorted(by_name[v].index for v in VARS)         # the reference's creation order
    fs_d, fs_g = rec["first_steps"]
    assert (fs_d["step"], fs_g["step"]) == (0, 1)
    used = []
    for vn in VARS:
        v = by_name[vn]
        fs = fs_d if vn.startswith("D_") else fs_g
        arrays[f"init_{vn}"] = v.initial.astype(np.float32).reshape(-1) if vn == "D_W1" else v.initial.astype(np.float32)
        arrays[f"final_{vn}"] = v.value.detach().numpy().astype(np.float32).reshape(arrays[f"init_{vn}"].shape)
        arrays[f"grad0_{vn}"] = fs["grads"][v.index].astype(np.float32).reshape(arrays[f"init_{vn}"].shape)
        used.append(dict(name=vn, index=v.index, init=[v.init_spec[0], list(v.init_spec[1]), v.init_spec[2]]))
    # the generator's first step starts from the initial G variables (the D step before it does not touch them)
    assert np.array_equal(fs_g["before"][by_name["G_W1"].index], by_name["G_W1"].initial)
    full = {k: arrays.pop(k) for k in SPARSE}
    changed = dict(final_G_W1=full["final_G_W1"].view(np.uint32) != arrays["init_G_W1"].view(np.uint32), grad0_G_W1=full["grad0_G_W1"] != 0)
    for k in SPARSE:
        arrays[k + "_idx"], arrays[k + "_val"] = sparse_of(full[k], changed[k])
    losses = [float(s["out"][0]) for s in rec["steps"]]
    arrays["d_losses"] = np.array(losses[0::4], np.float64)
    arrays["g_losses"] = np.array(losses, np.float64).reshape(n_epochs, 4)[:, 1:].copy()
    if str(tf1shim.DT).endswith("float64"):      # the child run: dense, the parent cuts it at the float32 run's indices
        arrays.update({k + "_dense": full[k] for k in SPARSE})
    np.savez_compressed(os.path.join(out_dir, NAME + ".npz"), **arrays)
    return dict(name=NAME, seed=SEED, shim_dtype=str(tf1shim.DT), n_users=len(m.data.user), n_items=ni, n_train=int(order0.shape[0]),
                n_epochs=n_epochs, batch_size=B, S_zr=m.S_zr, S_pm=m.S_pm, alpha=m.alpha, lr=m.lRate, variables=used,
                rows_with_zr_and_mask_first_step=int((both > 0).sum()), measure=rec["measure"], conf=open(conf).read(),
                subset=dict(source="dataset/FilmTrust/ratings.txt", first_users=N_USERS, rows=n_rows))


def run_cases(out_dir):
    G.install_stubs()
    sys.modules["tensorflow"] = tf1shim
    close_shim_gaps()
    T.HERE = out_dir
    with tempfile.TemporaryDirectory() as tmp:
        os.symlink(os.path.join(T.REF, "dataset"), os.path.join(tmp, "dataset"))
        cwd = os.getcwd(); os.chdir(tmp)
        try:
            meta = run_case(tmp, out_dir)
            print(meta["name"], "epochs", meta["n_epochs"], "users", meta["n_users"], "items", meta["n_items"], flush=True)
        finally:
            os.chdir(cwd)
    return meta


def main():
    if "--float64-child" in sys.argv:     # started below with TF1SHIM_DTYPE=float64: the same run, written to a scratch directory
        assert os.environ.get("TF1SHIM_DTYPE") == "float64" and str(tf1shim.DT).endswith("float64")
        run_cases(sys.argv[sys.argv.index("--float64-child") + 1])
        return
    meta = run_cases(HERE)
    with open(os.path.join(HERE, "golden_tf_cfgan.json"), "w") as f:
        json.dump({NAME: meta}, f, indent=1, sort_keys=True, default=str)
    out = {}
    moving = lambda k: k.startswith(("final_", "grad0_")) or k in ("d_losses", "g_losses")
    with tempfile.TemporaryDirectory() as scratch:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--float64-child", scratch], check=True,
                       env=dict(os.environ, TF1SHIM_DTYPE="float64", PYTHONDONTWRITEBYTECODE="1"))
        a, b = np.load(os.path.join(HERE, NAME + ".npz")), np.load(os.path.join(scratch, NAME + ".npz"))
        for k in a.files:
            if not moving(k):
                assert np.array_equal(a[k], b[k]), (k, "the float64 run left the float32 run's inputs")
        for k in SPARSE:                  # outside the float32 run's indices the float64 run is unchanged / zero as well
            dense, idx = b[k + "_dense"], a[k + "_idx"]
            rest = np.ones(dense.size, bool); rest[idx] = False
            base = b["init_G_W1"].ravel() if k == "final_G_W1" else np.zeros(dense.size, np.float32)
            assert np.array_equal(dense.ravel()[rest], base[rest]), k
            out[f"{NAME}/{k}_val"] = dense.ravel()[idx].astype(np.float32)
        rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y))
        for k in b.files:
            if moving(k) and not k.startswith(SPARSE):
                out[f"{NAME}/{k}"] = b[k].astype(np.float64 if k.endswith("losses") else np.float32)
        print(NAME, "float32 run vs float64 run:", {k.split("/")[1]: rel(a[k.split("/")[1]], v) for k, v in out.items()})
    np.savez_compressed(os.path.join(HERE, "tf_cfgan_f64_yardstick.npz"), **out)
    for f in (NAME + ".npz", "tf_cfgan_f64_yardstick.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
