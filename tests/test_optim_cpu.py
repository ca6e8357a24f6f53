"""qrec_amd/optim.py and the joint-table pack on the host: the TF-1.14 Adam bookkeeping every trainer shares must round exactly
as the expression the trainers carried before it was stated once, and as the float32 Adam of the CDAE / CFGAN mirrors."""
import numpy as np
import pytest

import cdae_mirror
import cfgan_mirror
from qrec_amd.graph import pack_joint, split_joint
from qrec_amd.optim import AdamClock

STEPS = 2000


@pytest.mark.parametrize("lr", [0.001, 0.002, 0.01, 0.05])
def test_adam_clock_bit_equal(lr):
    f = np.float32
    clock = AdamClock(lr)
    assert all(type(x) is np.float32 for x in (clock.lr, clock.b1, clock.b2, clock.eps, clock.b1p, clock.b2p))
    assert (clock.b1, clock.b2, clock.eps) == (f(0.9), f(0.999), f(1e-8))
    # the trainers' own statement, literally: fp32 powers, alpha evaluated in fp32, powers multiplied after the step
    b1, b2, b1p, b2p = f(0.9), f(0.999), f(0.9), f(0.999)
    # the mirrors' float32 Adam carries its alpha only inside the update: one scalar per variable, updated by the mirror and
    # by the same arithmetic around the clock's alpha
    mirrors = [(cdae_mirror.Adam(lr, np.float32), cdae_mirror.VARS), (cfgan_mirror.Adam(lr, cfgan_mirror.VARS[:1], np.float32), cfgan_mirror.VARS[:1])]
    params = [{k: np.full(1, 0.25 + 0.125 * i, f) for i, k in enumerate(keys)} for _, keys in mirrors]
    mine = [dict(p=p[keys[0]].copy(), m=np.zeros(1, f), v=np.zeros(1, f)) for p, (_, keys) in zip(params, mirrors)]
    for t in range(STEPS):
        alpha = clock.alpha()
        assert type(alpha) is float
        assert f(alpha) == f(f(lr) * np.sqrt(f(1) - b2p, dtype=f) / (f(1) - b1p)) and float(f(alpha)) == alpha, (lr, t)
        assert clock.b1p == b1p and clock.b2p == b2p, (lr, t)
        for k, ((opt, keys), own) in enumerate(zip(mirrors, mine)):
            assert opt.b1p == clock.b1p and opt.b2p == clock.b2p and type(opt.b1p) is np.float32, (lr, t)
            g = np.full(1, np.sin(0.37 * t) + 1.5 + k, f)
            params[k] = opt.step(params[k], {key: g for key in keys})
            own["m"] += (g - own["m"]) * (f(1) - clock.b1)
            own["v"] += (g * g - own["v"]) * (f(1) - clock.b2)
            own["p"] = own["p"] - (own["m"] * f(alpha)) / (np.sqrt(own["v"]) + clock.eps)
            assert params[k][keys[0]].dtype == np.float32 and params[k][keys[0]][0] == own["p"][0], (lr, t)
        clock.advance()
        b1p = f(b1p * b1); b2p = f(b2p * b2)
    assert clock.b1p == b1p and clock.b2p == b2p and type(clock.b1p) is np.float32 and type(clock.b2p) is np.float32


@pytest.mark.parametrize("nu,ni,d", [(1, 1, 1), (3, 5, 7), (33, 2, 64), (2, 33, 65)])
def test_pack_split_joint(nu, ni, d):
    from qrec_amd.engine import padded_ld
    ld = padded_ld(d, np.float32)
    rng = np.random.default_rng(nu * 1000 + ni * 10 + d)
    U0 = rng.standard_normal((nu, d)); V0 = rng.standard_normal((ni, d)).astype(np.float32)      # float64 in: converted like the assignment did
    E = pack_joint(U0, V0, ld)
    assert E.shape == (nu + ni, ld) and E.dtype == np.float32 and E.flags.c_contiguous
    assert not E[:, d:].any()
    assert np.array_equal(E[:nu, :d], U0.astype(np.float32)) and np.array_equal(E[nu:, :d], V0)
    U, V = split_joint(E, nu, d)
    for out, src in ((U, U0.astype(np.float32)), (V, V0)):
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.flags.owndata and np.array_equal(out, src)
    U[...] = 7; V[...] = 7                                   # copies: the table is untouched
    assert np.array_equal(E[:nu, :d], U0.astype(np.float32)) and np.array_equal(E[nu:, :d], V0)
