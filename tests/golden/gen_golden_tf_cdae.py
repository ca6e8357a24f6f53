#!/usr/bin/env python3
"""Golden vectors for the reference's CDAE (model/ranking/CDAE.py), produced by running the reference's OWN class unmodified
with ``tests/golden/tf1shim.py`` standing in for ``tensorflow`` -- the harness of ``gen_golden_tf.py`` (run_tf_model, base_conf,
make_subset), imported from there; nothing of the reference's text is stored here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tf_cdae.py

Needs the reference tree (build container only).  Writes, next to this file:
  tf_cdae_filmtrust.npz       CDAE on the first 300 users of FilmTrust (the subset of the other TF fixtures): batch 64, -nh 24,
                              -co 0.9, 12 steps (one batch per ``num.max.epoch``).  Per step the users fed (``u_idx``) and the three
                              dense 0/1 feeds ``positive``, ``negative``, ``mask_corruption`` as packed bits (np.packbits over
                              [steps, batch, n_items]); ``X`` is not stored, it is the training ratings of the step's users.  The five
                              variables (W_enc, W_dec [nh, n_items], b_enc, b_dec, V) before and after, the first step's gradients,
                              the losses, the training triplets in id form and the test pairs.
  golden_tf_cdae.json         sizes, hyper-parameters, the measure, the conf text
  tf_cdae_f64_yardstick.npz   the same run with the stand-in's arithmetic in float64 (TF1SHIM_DTYPE=float64, a child process; same
                              seeds, and every fed array is asserted identical): trained variables, first-step gradients and losses.
                              |fixture - yardstick| is the distance of the reference's own float32 run from exact arithmetic.

What the stand-in lacks for this model is closed HERE, at run time, and tf1shim.py stays as it is:
  * ``tf.maximum`` (CDAE.py:75): out = where(y >= x, y, x) for maximum(x, y) -- the gradient goes to y where y >= x, to x elsewhere;
  * ``xavier_initializer`` on a rank-1 shape (the two biases): contrib's variance_scaling takes fan_in = fan_out = shape[-1] there,
    so the limit is sqrt(3 / n);
  * the placeholders ``X``, ``positive``, ``negative``, ``mask_corruption`` carry no name, so run_tf_model's by-name feed log keeps one
    of them: the feeds are recorded here by identity against the model's attributes."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402
import gen_golden_tf as T       # noqa: E402
import tf1shim                  # noqa: E402

NAME = "tf_cdae_filmtrust"
SEED = 131
VARS = ("W_enc", "W_dec", "b_enc", "b_dec", "V")
FEEDS = ("X", "positive", "negative", "mask_corruption", "u_idx")


def close_shim_gaps():
    def maximum(x, y, name=None):
        return tf1shim.Tensor(lambda ctx, a, b: torch.where(b >= a, b, a), [tf1shim._t(x), tf1shim._t(y)], name=name)
    tf1shim.maximum = maximum
    rank2 = tf1shim._xavier_initializer

    def xavier_initializer(uniform=True, seed=None, dtype=tf1shim.float32):
        inner = rank2(uniform, seed, dtype)

        def init(shape, dtype=None, partition_info=None):
            if len(shape) == 1:     # contrib/layers/python/layers/initializers.py: fan_in = shape[-1] when the rank is 1
                return tf1shim._Init("xavier_uniform", shape, np.sqrt(3.0 / shape[0]))
            return inner(shape, dtype, partition_info)
        return init
    tf1shim.contrib.layers.xavier_initializer = xavier_initializer


def run_case(tmp, out_dir):
    T.N_SUBSET_USERS = 300
    ratings, n_rows = T.make_subset(tmp)
    conf = T.base_conf(tmp, ratings, model__name="CDAE", CDAE="-co 0.9 -nh 24", batch_size="64", num__max__epoch="12")
    fed = []                                           # per Session.run that carries a train op: [(placeholder, array)]
    inner_run = tf1shim.Session.run

    def run(self, fetches, feed_dict=None, **kw):
        fl = fetches if isinstance(fetches, (list, tuple)) else [fetches]
        if any(isinstance(t, tf1shim._TrainOp) for t in fl):
            fed.append([(k, np.array(v)) for k, v in (feed_dict or {}).items()])
        return inner_run(self, fetches, feed_dict, **kw)
    tf1shim.Session.run = run
    try:
        def after(m):
            te_u, te_i = [], []
            for user, items in m.data.testSet_u.items():
                for item in items:
                    te_u.append(m.data.user.get(user, -1)); te_i.append(m.data.item.get(item, -1))
            return dict(test_uid=np.array(te_u, np.int32), test_iid=np.array(te_i, np.int32))
        rec = T.run_tf_model(conf, SEED, "model.ranking.CDAE", "CDAE", after=after)
    finally:
        tf1shim.Session.run = inner_run
    m = rec["model"]
    holders = {id(getattr(m, a)): a for a in FEEDS}
    steps = [{holders[id(k)]: v for k, v in step} for step in fed]
    assert len(steps) == 12 and all(sorted(s) == sorted(FEEDS) for s in steps), [sorted(s) for s in steps]
    order0 = np.array(rec["order0"], dtype=np.int32)
    arrays = dict(train_uid=order0[:, 0], train_iid=order0[:, 1], train_r=np.array(rec["rating0"], np.float32))
    arrays.update(rec["extra"])
    # X is the dense rating rows of the step's users and nothing else (CDAE.py:31,42): asserted, not stored
    R = np.zeros((len(m.data.user), len(m.data.item)))
    R[order0[:, 0], order0[:, 1]] = rec["rating0"]
    for s in steps:
        assert np.array_equal(s["X"], R[np.asarray(s["u_idx"])])
        assert set(np.unique(s["mask_corruption"])) <= {0, 1} and not (s["positive"] * s["negative"]).any()
        assert np.array_equal(s["positive"], (s["X"] != 0).astype(float))
    arrays["u_idx"] = np.array([s["u_idx"] for s in steps], np.int32)
    for key in ("positive", "negative", "mask_corruption"):
        arrays[key + "_bits"] = np.packbits(np.stack([s[key] for s in steps]).astype(bool), axis=None)
    model_vars = dict(W_enc=m.weights["encoder"], W_dec=m.weights["decoder"], b_enc=m.biases["encoder"], b_dec=m.biases["decoder"], V=m.V)
    fs = rec["first_steps"][0]
    assert fs["step"] == 0
    used = []
    for vn in VARS:
        v = model_vars[vn]
        arrays[f"init_{vn}"] = v.initial.astype(np.float32)
        arrays[f"final_{vn}"] = v.value.detach().numpy().astype(np.float32)
        arrays[f"grad0_{vn}"] = fs["grads"][v.index].astype(np.float32)
        used.append(dict(name=vn, index=v.index, init=[v.init_spec[0], list(v.init_spec[1]), v.init_spec[2]]))
    arrays["losses"] = np.array([[float(x) for x in s["out"]] for s in rec["steps"]], dtype=np.float64)
    np.savez_compressed(os.path.join(out_dir, NAME + ".npz"), **arrays)
    return dict(name=NAME, seed=SEED, shim_dtype=str(tf1shim.DT), n_users=len(m.data.user), n_items=len(m.data.item),
                n_train=int(order0.shape[0]), n_steps=len(steps), batch_size=m.batch_size, n_hidden=m.n_hidden,
                corruption_level=m.corruption_level, negative_sp=m.negative_sp, lr=m.lRate, regU=m.regU, variables=used,
                measure=rec["measure"], conf=open(conf).read(),
                subset=dict(source="dataset/FilmTrust/ratings.txt", first_users=300, rows=n_rows))


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
            print(meta["name"], "steps", meta["n_steps"], "users", meta["n_users"], "items", meta["n_items"], flush=True)
        finally:
            os.chdir(cwd)
    return meta


def main():
    if "--float64-child" in sys.argv:     # started below with TF1SHIM_DTYPE=float64: the same run, written to a scratch directory
        assert os.environ.get("TF1SHIM_DTYPE") == "float64" and str(tf1shim.DT).endswith("float64")
        run_cases(sys.argv[sys.argv.index("--float64-child") + 1])
        return
    meta = run_cases(HERE)
    with open(os.path.join(HERE, "golden_tf_cdae.json"), "w") as f:
        json.dump({NAME: meta}, f, indent=1, sort_keys=True, default=str)
    out = {}
    with tempfile.TemporaryDirectory() as scratch:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--float64-child", scratch], check=True,
                       env=dict(os.environ, TF1SHIM_DTYPE="float64", PYTHONDONTWRITEBYTECODE="1"))
        a, b = np.load(os.path.join(HERE, NAME + ".npz")), np.load(os.path.join(scratch, NAME + ".npz"))
        for k in a.files:
            if not k.startswith(("final_", "grad0_")) and k != "losses":
                assert np.array_equal(a[k], b[k]), (k, "the float64 run left the float32 run's inputs")
        rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y))
        for k in b.files:
            if k.startswith(("final_", "grad0_")) or k == "losses":
                out[f"{NAME}/{k}"] = b[k].astype(np.float32 if k != "losses" else np.float64)
        print(NAME, "float32 run vs float64 run:", {k: rel(a[k], b[k]) for k in b.files if k.startswith(("final_", "grad0_")) or k == "losses"})
    np.savez_compressed(os.path.join(HERE, "tf_cdae_f64_yardstick.npz"), **out)


if __name__ == "__main__":
    main()
