"""The deterministic input set that pins include/mog_math.h (shared by
tests/test_math_spec.py, the accuracy pin on the CPU oracle, and
tests/test_gpu_math_spec.py, device bits == host bits).

* every one of the 255 finite exponent fields x 64 mantissas x both signs:
  mantissas 0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff and 56
  seeded random ones;
* +-0, +-inf, NaN, the smallest and the largest subnormal, FLT_MIN;
* every branch constant of the header, -2 .. +2 ulps around it;
* a 400 001-point linspace over [-110, 90];
* the worst inputs recorded by earlier sweeps (RECORDED_WORST).
"""
import ctypes

import numpy as np

from oracle import air_oracle as ao

EXP, LOG, EXPM1, TANH, SIGMOID, SOFTPLUS, LOG1P = range(7)
NAMES = ("exp", "log", "expm1", "tanh", "sigmoid", "softplus", "log1p")

# mog_math.h's branch constants
EXP_HI = np.float32(88.72283935546875)
EXP_LO = np.float32(-103.972084045410156)
LN2_HALF = np.float32(0.3465735912322998)
TANH_SAT = np.float32(9.1)
SOFTPLUS_T = np.float32(13.9423847198486328)
SQRT2 = np.float32(1.41421353816986083984375)
FLT_MIN = np.float32(1.17549435e-38)
BRANCH_CONSTANTS = (EXP_HI, EXP_LO, LN2_HALF, -LN2_HALF, np.float32(-17.0), TANH_SAT, -TANH_SAT,
                    np.float32(4.55), np.float32(-4.55), SOFTPLUS_T, -SOFTPLUS_T, SQRT2, FLT_MIN)

# inputs at which an earlier sweep (other random mantissas) measured more than
# this set's random mantissas reach: log1p 3.24 ulp
RECORDED_WORST = (np.float32(0.029860657),)


def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def spec_inputs() -> np.ndarray:
    rng = np.random.default_rng(20240521)
    mant = np.concatenate([np.array([0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff]),
                           rng.integers(0, 1 << 23, 56)]).astype(np.uint32)
    expo = np.arange(255, dtype=np.uint32)
    grid = ((expo[:, None] << np.uint32(23)) | mant[None, :]).ravel()
    grid = np.concatenate([grid, grid | np.uint32(0x80000000)])
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x00000001,
                        0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000], np.uint32)
    near = []
    for c in BRANCH_CONSTANTS:
        b = np.float32(c).view(np.uint32).astype(np.int64)
        near.extend(int(b) + d for d in range(-2, 3))  # +-2 ulps (sign-magnitude neighbours)
    lin = np.linspace(-110.0, 90.0, 400001).astype(np.float32)
    return np.concatenate([_bits(grid), _bits(special), _bits(np.array(near, np.uint32)), lin,
                           np.array(RECORDED_WORST, np.float32)])


def oracle_math(fn: int, x: np.ndarray) -> np.ndarray:
    """mog_math.h function `fn` over x, as gcc compiles it (oracle_math_vec)."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    ao._load().oracle_math_vec(ctypes.c_int(fn), x.ctypes.data_as(ao._FP),
                               y.ctypes.data_as(ao._FP), ctypes.c_int(x.size))
    return y


def logistic_noise(u: np.ndarray) -> np.ndarray:
    """csrc/step_math.h logistic_noise restated: log(u + 1e-9) - log((1 - u) + 1e-9)."""
    u = np.asarray(u, np.float32)
    eps = np.float32(1e-9)
    return oracle_math(LOG, u + eps) - oracle_math(LOG, (np.float32(1) - u) + eps)


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Element-wise: equal uint32 views, or both NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
