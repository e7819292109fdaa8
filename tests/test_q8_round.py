"""q8_round (csrc/kernels_decode.hip.h) restated in numpy float32: (int)(x + copysign(0x3EFFFFFF, x)), the sum rounded to nearest-even as v_add_f32 rounds it and
the conversion truncating, equals (int)roundf(x) -- trunc(x + copysign(0.5, x)) taken in double, where that sum is exact for every float below 2^29.

Checked: every float with 2^-3 <= |x| < 2^9 (12 binades of 2^23 values, both signs: 201 M values; the Q8 quotients lie in |x| <= 127 (1 + 2^-22)); +-0, the
denormals' ends, the two neighbours of every k + 0.5 for |k| <= 128, and 2^16 values of every binade below 2^-3.  The naive x + 0.5f is shown wrong at
0x3EFFFFFF, the value the addend is chosen for.  (The device runs all 2^32 patterns: tests/test_gpu_ln_q8_forms.py.)"""
import numpy as np

F32 = np.float32
ADDEND = np.array([0x3EFFFFFF], dtype=np.uint32).view(F32)[0]      # the float below 0.5


def q8_round(x):
    x = np.asarray(x, dtype=F32)
    s = x + np.copysign(ADDEND, x)
    assert s.dtype == F32
    return np.trunc(s).astype(np.int64)


def roundf(x):
    t = np.asarray(x, dtype=F32).astype(np.float64)
    return np.trunc(t + np.copysign(0.5, t)).astype(np.int64)


def _check(x, what):
    got, want = q8_round(x), roundf(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "%d mismatches" % bad.size, "first", hex(int(np.asarray(x, dtype=F32).view(np.uint32)[bad[0]])), int(got[bad[0]]), int(want[bad[0]]))


def test_the_addend_is_the_float_below_one_half():
    assert ADDEND == F32(0.49999997) and np.nextafter(ADDEND, F32(1)) == F32(0.5)
    x = ADDEND
    assert roundf(x) == 0 and q8_round(x) == 0
    assert int(np.trunc(F32(x + F32(0.5)))) == 1, "x + 0.5f rounds the float below one half up to 1: the form this addend avoids"


def test_every_float_of_the_quotients_binades():
    mant = np.arange(1 << 23, dtype=np.uint32)
    for e in range(127 - 3, 127 + 9):
        for sign in (0, 0x80000000):
            _check((mant | np.uint32(e << 23) | np.uint32(sign)).view(F32), ("binade", e - 127, sign != 0))


def test_zeros_denormals_ties_and_small_binades():
    edge = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000], dtype=np.uint32).view(F32)
    _check(edge, "zeros and denormals")
    assert (q8_round(edge) == 0).all()
    k = np.arange(-128, 129, dtype=np.float64)
    ties = np.concatenate([k + 0.5, k - 0.5]).astype(F32)
    around = np.concatenate([ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf))])
    _check(around, "k + 0.5 and its neighbours")
    assert (roundf(F32(2.5)), roundf(F32(-2.5)), roundf(np.nextafter(F32(2.5), F32(0)))) == (3, -3, 2)       # half away from zero
    g = np.random.default_rng(0x51)
    for e in range(0, 127 - 3):
        mant = g.integers(0, 1 << 23, 1 << 16, dtype=np.uint32)
        for sign in (0, 0x80000000):
            _check((mant | np.uint32(e << 23) | np.uint32(sign)).view(F32), ("binade", e - 127, sign != 0))
