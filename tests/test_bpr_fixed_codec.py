"""The fixed-point codec of the QREC_HW_FIXED BPR epoch, on the host: the numpy restatement (tests/fixed_codec.py) that the device tests
of tests/test_gpu_bpr_fixed.py compare the kernels with, held to the codec's contract."""
import numpy as np

import fixed_codec as FX


def test_round_trip_is_within_half_a_quantum():
    x = FX.edge_values()
    back = FX.round_trip(x)
    assert np.abs(x.astype(np.float64) - back.astype(np.float64)).max() <= 2.0 ** -27
    rng = np.random.default_rng(0)
    y = np.concatenate([rng.random(100_000, dtype=np.float32) / 3, (rng.random(100_000, dtype=np.float32) - 0.5) * 31.9]).astype(np.float32)
    assert np.abs(y.astype(np.float64) - FX.round_trip(y).astype(np.float64)).max() <= 2.0 ** -27
    big = y[np.abs(y) >= 0.25]                       # from 0.25 up the fp32 ulp is a whole number of quanta: nothing is lost
    assert np.array_equal(FX.round_trip(big), big)


def test_ties_go_to_even_and_zero_and_quanta_are_exact():
    q = FX.QUANTUM
    assert FX.encode([0.0, -0.0, q, -q, 0.5 * q, -0.5 * q, 1.5 * q, -1.5 * q, 2.5 * q, -2.5 * q]).tolist() == [0, 0, 1, -1, 0, 0, 2, -2, 2, -2]
    top = np.nextafter(np.float32(FX.LIMIT), np.float32(0))
    assert FX.encode([top])[0] == 2 ** 30 - 2 ** 6 and FX.round_trip([top])[0] == top


def test_out_of_range_saturates_and_never_changes_sign():
    x = np.array([16.0, -16.0, 31.9, -31.9, 32.0, -32.0, 1e9, -1e9, np.inf, -np.inf], dtype=np.float32)
    back = FX.round_trip(x)
    assert np.array_equal(np.sign(back), np.sign(x)) and np.isfinite(back).all() and (np.abs(back) <= 32.0).all()
    assert back[0] == 16.0 and back[1] == -16.0      # headroom: the range itself is +-32
    assert FX.encode([np.nan])[0] == FX.INT_LO


def test_accum_switch_is_parsed_from_the_argument_or_the_environment(monkeypatch):
    import pytest
    from qrec_amd.engine import resolve_accum
    monkeypatch.delenv("QREC_BPR_ACCUM", raising=False)
    assert resolve_accum() == "auto" and resolve_accum("f32") == "f32" and resolve_accum("i32") == "i32"
    for v in ("auto", "f32", "i32"):
        monkeypatch.setenv("QREC_BPR_ACCUM", v)
        assert resolve_accum() == v and resolve_accum("f32") == "f32"          # the object's own choice goes first
    monkeypatch.setenv("QREC_BPR_ACCUM", "int32")
    with pytest.raises(ValueError):
        resolve_accum()
    with pytest.raises(ValueError):
        resolve_accum("fp32")
