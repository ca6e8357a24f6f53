#!/usr/bin/env python3
"""Golden vectors for the reference's IRGAN (model/ranking/IRGAN.py), produced by running the reference's OWN class unmodified with
``tests/golden/tf1shim.py`` standing in for ``tensorflow`` -- the harness of ``gen_golden_tf.py`` (run_tf_model, base_conf,
make_subset), imported from there; nothing of the reference's text is stored here.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tf_irgan.py

Needs the reference tree (build container only).  Writes, next to this file:
  tf_irgan_filmtrust.npz      IRGAN on the first 120 users of FilmTrust: num.factors 8, batch_size 128, 1 epoch, -init 0.001, -u 0.001.
                              The six variables (g_P, g_Q, g_b, d_P, d_Q, d_b) initially (init_*), after the discriminator epoch
                              (snap0_*), after each of the five generator passes (snap1_* .. snap5_*) and at the end (final_*); the
                              first-step gradients of the discriminator's train op (grad0_d_*) and of the generator's (grad1_g_*);
                              every np.random.choice call's result (draw_ptr, draw_items) and the user it was made for (draw_user):
                              first get_data's calls in trainSet_u order, then the generator's, pass by pass; the discriminator's
                              batches (dis_ptr, dis_u, dis_i, dis_label); the losses of every step (losses_d: the SUM of the batch's
                              loss vector, which is what minimize differentiates; losses_g); the training triplets in id form, the
                              users' rated items in the reference's order (pos_ptr, pos_items, per user id) and the test pairs.
  golden_tf_irgan.json        sizes, hyper-parameters, the measure, the conf text, the number of uniforms the run consumed
  tf_irgan_f64_yardstick.npz  the same run with the stand-in's arithmetic in float64 (TF1SHIM_DTYPE=float64, a child process) and
                              np.random.choice replaced by a replay of the recorded draws; every fed array is asserted identical.
                              |fixture - yardstick| is the distance of the reference's own float32 run from exact arithmetic.

What the stand-in lacks for this model is closed HERE, at run time, and tf1shim.py stays as it is:
  * ``tf.variable_scope``: a context that does nothing;
  * ``tf.random_uniform(shape, -a, a)`` handed to ``tf.Variable``: _Init("xavier_uniform", shape, a), i.e. U(+-a) drawn at creation;
  * ``tf.zeros``;
  * ``tf.nn.sigmoid_cross_entropy_with_logits``: max(x, 0) - x z + log1p(exp(-|x|)) (nn_impl.py);
  * ``minimize`` of a non-scalar loss differentiates its sum (gradients() seeds every element with 1);
  * a ``Session.run`` whose only fetch is a train op: run_tf_model expects a list, so the call is wrapped before it gets there, and the
    train op's loss is fetched next to it so that the losses are on record."""
import contextlib
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

NAME = "tf_irgan_filmtrust"
SEED = 17
VARS = ("g_P", "g_Q", "g_b", "d_P", "d_Q", "d_b")
N_USERS = 120


def close_shim_gaps():
    tf1shim.variable_scope = lambda *a, **k: contextlib.nullcontext()

    def random_uniform(shape, minval=0, maxval=None, dtype=None, seed=None, name=None):
        assert maxval is not None and minval == -maxval
        return tf1shim._Init("xavier_uniform", shape, maxval)
    tf1shim.random_uniform = random_uniform
    tf1shim.zeros = lambda shape, dtype=None, name=None: np.zeros(shape, np.float32)

    def sigmoid_cross_entropy_with_logits(_sentinel=None, labels=None, logits=None, name=None):
        def f(ctx, z, x):
            return torch.clamp(x, min=0) - x * z + torch.log1p(torch.exp(-torch.abs(x)))
        return tf1shim.Tensor(f, [tf1shim._t(labels), tf1shim._t(logits)])
    tf1shim.nn.sigmoid_cross_entropy_with_logits = sigmoid_cross_entropy_with_logits

    def minimize(self, loss, global_step=None, var_list=None, name=None):
        return tf1shim._TrainOp(self, tf1shim.reduce_sum(loss), var_list)
    tf1shim.AdamOptimizer.minimize = minimize


def run_case(tmp, out_dir, replay=None):
    T.N_SUBSET_USERS = N_USERS
    ratings, n_rows = T.make_subset(tmp)
    conf = T.base_conf(tmp, ratings, model__name="IRGAN", num__factors="8", batch_size="128", num__max__epoch="1",
                       learnRate="-init 0.001 -max 1", reg__lambda="-u 0.001 -i 0.01 -b 0.2 -s 0.2")
    calls, fed, snaps = [], [], []
    inner_run, inner_choice = tf1shim.Session.run, np.random.choice

    def model_vars():
        v = tf1shim.all_variables()          # creation order: the base class's U and V, then the generator's three, then the discriminator's
        assert len(v) == 8
        return dict(zip(VARS, v[2:]))

    def run(self, fetches, feed_dict=None, **kw):
        if not isinstance(fetches, tf1shim._TrainOp):
            return inner_run(self, fetches, feed_dict, **kw)
        out = inner_run(self, [fetches, fetches.loss], feed_dict, **kw)
        fed.append((fetches, {id(k): np.array(v) for k, v in feed_dict.items()}, len(calls)))
        snaps.append(None)
        n_train_users = fed[0][2]            # get_data made one choice call per training user before the first train step
        n_d = sum(1 for f in fed if f[0] is fed[0][0])
        if len(fed) > n_d and (len(fed) - n_d) % n_train_users == 0:          # a generator pass ended
            snaps[-1] = {k: v.value.detach().numpy().copy() for k, v in model_vars().items()}
        return out

    def choice(a, size=None, replace=True, p=None):
        if replay is not None:
            out = replay[len(calls)].copy()
            assert out.size == size
        else:
            out = inner_choice(a, size, replace, p)
        calls.append(np.asarray(out).astype(np.int32))
        return out
    tf1shim.Session.run = run
    np.random.choice = choice
    try:
        def after(m):
            te_u, te_i = [], []
            for user, items in m.data.testSet_u.items():
                for item in items:
                    te_u.append(m.data.user.get(user, -1)); te_i.append(m.data.item.get(item, -1))
            return dict(test_uid=np.array(te_u, np.int32), test_iid=np.array(te_i, np.int32))
        rec = T.run_tf_model(conf, SEED, "model.ranking.IRGAN", "IRGAN", after=after)
    finally:
        tf1shim.Session.run = inner_run
        np.random.choice = inner_choice
    m = rec["model"]
    mv = model_vars()
    # trainSet_u is a defaultdict: the evaluation's look-ups of unknown test users added empty entries after training
    train_users = [u for u in m.data.trainSet_u if u in m.data.user]
    order = [m.data.user[u] for u in train_users]
    pos = {m.data.user[u]: [m.data.item[i] for i in m.data.userRated(u)[0]] for u in train_users}
    nu_t = len(order)
    d_op, g_op = m.discriminator.d_updates, m.generator.gan_updates
    d_steps = [f for f in fed if f[0] is d_op]
    g_steps = [f for f in fed if f[0] is g_op]
    n_d = -(-m.train_size // m.batch_size)
    assert len(d_steps) == n_d and len(g_steps) == 5 * nu_t and len(calls) == 6 * nu_t and fed[:n_d] == d_steps
    order0 = np.array(rec["order0"], dtype=np.int32)
    arrays = dict(train_uid=order0[:, 0], train_iid=order0[:, 1], train_r=np.array(rec["rating0"], np.float32), user_order=np.array(order, np.int32))
    arrays.update(rec["extra"])
    arrays["pos_ptr"] = np.concatenate([[0], np.cumsum([len(pos.get(u, [])) for u in range(len(m.data.user))])]).astype(np.int64)
    arrays["pos_items"] = np.concatenate([np.array(pos.get(u, []), np.int32) for u in range(len(m.data.user))])
    arrays["draw_ptr"] = np.concatenate([[0], np.cumsum([c.size for c in calls])]).astype(np.int64)
    arrays["draw_items"] = np.concatenate(calls)
    arrays["draw_user"] = np.array(order * 6, np.int32)
    D = m.discriminator
    arrays["dis_ptr"] = np.concatenate([[0], np.cumsum([f[1][id(D.u)].size for f in d_steps])]).astype(np.int64)
    arrays["dis_u"] = np.concatenate([f[1][id(D.u)] for f in d_steps]).astype(np.int32)
    arrays["dis_i"] = np.concatenate([f[1][id(D.i)] for f in d_steps]).astype(np.int32)
    arrays["dis_label"] = np.concatenate([f[1][id(D.label)] for f in d_steps]).astype(np.float32)
    # the generator's feeds are its draws: asserted, not stored twice
    Gn = m.generator
    for k, f in enumerate(g_steps):
        assert int(f[1][id(Gn.u)]) == order[k % nu_t] and np.array_equal(f[1][id(Gn.i)], calls[nu_t + k])
    # get_data's rows: per user the positives with label 1, then the draws with label 0; the discriminator saw the first train_size
    rows_u = np.concatenate([[u] * (3 * len(pos[u])) for u in order]); rows_i = np.concatenate([pos[u] + calls[k].tolist() for k, u in enumerate(order)])
    assert np.array_equal(rows_u[:m.train_size], arrays["dis_u"]) and np.array_equal(rows_i[:m.train_size], arrays["dis_i"])
    assert arrays["dis_u"].size == m.train_size < rows_u.size
    losses = [float(s["out"][0]) for s in rec["steps"]]
    arrays["losses_d"] = np.array(losses[:n_d]); arrays["losses_g"] = np.array(losses[n_d:])
    fs = rec["first_steps"]
    assert [f["step"] for f in fs] == [0, n_d]
    used = []
    ft = tf1shim.NPDT                       # computed values keep the run's precision: the float64 child's are the yardstick
    for vn in VARS:
        v = mv[vn]
        arrays[f"init_{vn}"] = v.initial.astype(np.float32)
        arrays[f"final_{vn}"] = v.value.detach().numpy().astype(ft)
        k = 0 if vn.startswith("d_") else 1
        arrays[f"grad{k}_{vn}"] = fs[k]["grads"][v.index].astype(ft)
        arrays[f"snap0_{vn}"] = fs[1]["before"][v.index].astype(ft)          # the generator's first step starts where the discriminator epoch ended
        used.append(dict(name=vn, index=v.index, init=[v.init_spec[0], list(v.init_spec[1]), v.init_spec[2]]))
    taken = [s for s in snaps if s is not None]
    assert len(taken) == 5
    for k, s in enumerate(taken):
        for vn in VARS:
            arrays[f"snap{k + 1}_{vn}"] = s[vn].astype(ft)
    np.savez_compressed(os.path.join(out_dir, NAME + ".npz"), **arrays)
    return dict(name=NAME, seed=SEED, shim_dtype=str(tf1shim.DT), n_users=len(m.data.user), n_items=len(m.data.item), n_train=int(order0.shape[0]),
                n_train_users=nu_t, n_d_steps=n_d, n_g_steps=len(g_steps), n_uniforms=int(arrays["draw_items"].size), train_size=m.train_size,
                batch_size=m.batch_size, emb_size=m.emb_size, lr=m.lRate, regU=m.regU, variables=used, measure=rec["measure"],
                conf=open(conf).read(), subset=dict(source="dataset/FilmTrust/ratings.txt", first_users=N_USERS, rows=n_rows))


def run_cases(out_dir, replay=None):
    G.install_stubs()
    sys.modules["tensorflow"] = tf1shim
    close_shim_gaps()
    T.HERE = out_dir
    with tempfile.TemporaryDirectory() as tmp:
        os.symlink(os.path.join(T.REF, "dataset"), os.path.join(tmp, "dataset"))
        cwd = os.getcwd(); os.chdir(tmp)
        try:
            meta = run_case(tmp, out_dir, replay)
            print(meta["name"], "steps", meta["n_d_steps"], "+", meta["n_g_steps"], "users", meta["n_users"], "items", meta["n_items"], flush=True)
        finally:
            os.chdir(cwd)
    return meta


def computed(k):
    return k.startswith(("final_", "grad0_", "grad1_", "snap")) or k in ("losses_d", "losses_g")


def main():
    if "--float64-child" in sys.argv:     # started below with TF1SHIM_DTYPE=float64: the same run on the recorded draws, written to a scratch directory
        assert os.environ.get("TF1SHIM_DTYPE") == "float64" and str(tf1shim.DT).endswith("float64")
        z = np.load(os.path.join(HERE, NAME + ".npz"))
        replay = [z["draw_items"][a:b] for a, b in zip(z["draw_ptr"][:-1], z["draw_ptr"][1:])]
        run_cases(sys.argv[sys.argv.index("--float64-child") + 1], replay)
        return
    meta = run_cases(HERE)
    with open(os.path.join(HERE, "golden_tf_irgan.json"), "w") as f:
        json.dump({NAME: meta}, f, indent=1, sort_keys=True, default=str)
    out = {}
    with tempfile.TemporaryDirectory() as scratch:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--float64-child", scratch], check=True,
                       env=dict(os.environ, TF1SHIM_DTYPE="float64", PYTHONDONTWRITEBYTECODE="1"))
        a, b = np.load(os.path.join(HERE, NAME + ".npz")), np.load(os.path.join(scratch, NAME + ".npz"))
        for k in a.files:
            if not computed(k):
                assert np.array_equal(a[k], b[k]), (k, "the float64 run left the float32 run's inputs")
        rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y))
        for k in b.files:
            if computed(k):
                out[f"{NAME}/{k}"] = b[k].astype(np.float64)
        print(NAME, "float32 run vs float64 run:", {k: rel(a[k], b[k]) for k in b.files if k.startswith("final_")})
    np.savez_compressed(os.path.join(HERE, "tf_irgan_f64_yardstick.npz"), **out)


if __name__ == "__main__":
    main()
