"""The fixed-point table codec of the QREC_HW_FIXED BPR epoch (csrc/common.h: fx_from_float, fx_to_float), restated in numpy.

int32 = rint(x * 2^26), round half to even, saturating; back = float32(q) * 2^-26.  Both scalings are by a power of two, hence exact
in fp32: the only roundings are the rint and, for |q| >= 2^24, the int -> fp32 conversion (round to nearest even, as numpy's)."""
import numpy as np

SCALE = np.float32(2.0 ** 26)
QUANTUM = 2.0 ** -26
LIMIT = 16.0                              # |x| >= LIMIT, or a NaN, fails the run
INT_LO, INT_HI = -2 ** 31, 2 ** 31 - 128  # the clamp: -2147483648.f and 2147483520.f, the largest fp32 below 2^31


def encode(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x * SCALE).astype(np.float64)
    y = np.where(np.isnan(y), INT_LO, np.clip(y, INT_LO, INT_HI))       # a NaN comes out of the clamp as its lower bound
    return np.rint(y).astype(np.int64).astype(np.int32)


def decode(q):
    return np.asarray(q, dtype=np.int32).astype(np.float32) * np.float32(QUANTUM)


def round_trip(x):
    return decode(encode(x))


def edge_values():
    """0, +-one quantum, half-way cases (ties to even, both parities, both signs, small and just below 2^24 quanta), values between, and
    the largest value in range"""
    q = QUANTUM
    half = [0.5 * q, -0.5 * q, 1.5 * q, -1.5 * q, 2.5 * q, -2.5 * q, (2 ** 22 + 0.5) * q, -(2 ** 22 + 1.5) * q, (2 ** 23 - 0.5) * q]
    mid = [0.25 * q, 0.75 * q, -0.75 * q, 1.25 * q, 1e-3, -1e-3, 1.0 / 3, -1.0 / 3, 0.25, 0.5, 1.0, -7.3, 15.5]
    top = np.nextafter(np.float32(LIMIT), np.float32(0))
    v = np.array([0.0, -0.0, q, -q, 2 * q, -2 * q] + half + mid + [top, -top], dtype=np.float32)
    assert all(float(np.float32(h)) == h for h in half)           # the ties are ties in fp32 as well
    return v
