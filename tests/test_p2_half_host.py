"""CPU tests of the MSD sort's half regions (option p2_half): the high half P3 gives the keys of a
16-bit segment, through the host entry point that calls the kernels' own function
(grs_debug_p2_half_hi -> grs::msd_half_hi), and the option's binding.

Setting option 18 on a sorter needs a device: tests/test_gpu_p2_half.py round-trips it."""
import ctypes

import numpy as np
import pytest


def hi_of(L, or_keys, shift, seg):
    return int(L.grs_debug_p2_half_hi(int(or_keys), int(shift), int(seg)))


def segment_of(keys, shift):
    """bucket * 256 + digit2: key bits [shift - 8, shift + 8)."""
    return (keys >> np.uint64(shift - 8)) & np.uint64(0xFFFF)


@pytest.mark.parametrize("shift", range(8, 25))
def test_hi_matches_the_keys(shift):
    """Random constant tops above the two digits, random bits below: for every key, the hi of its
    segment is the key's bits 16..31 (the OR word carries the constant bits, set low bits of the
    OR must not leak in)."""
    from gpuradixsort_amd import _lib

    L = _lib.lib()
    rng = np.random.default_rng(shift)
    vb = shift + 8   # bits that vary
    for trial in range(8):
        top = (int(rng.integers(0, 1 << 32)) >> vb) << vb if vb < 32 else 0
        if trial == 0:
            top = (0xFFFFFFFF >> vb) << vb if vb < 32 else 0   # every constant bit set
        if trial == 1:
            top = 0
        low = rng.integers(0, 1 << vb, 2000, dtype=np.uint64)
        low[0], low[1] = 0, (1 << vb) - 1   # the keys fill [top, top + 2^vb) exactly
        keys = np.uint64(top) | low
        or_keys = int(np.bitwise_or.reduce(keys))
        seg = segment_of(keys, shift)
        for k, b in zip(keys[:400].tolist(), seg[:400].tolist()):
            assert hi_of(L, or_keys, shift, b) == (k & 0xFFFF0000), (shift, hex(top), hex(k), b)


def test_hi_written_out():
    """The issue's own examples, by hand."""
    from gpuradixsort_amd import _lib

    L = _lib.lib()
    # 0xA5000000 | 24 bits, shift 16: b = key bits [8, 24)
    assert hi_of(L, 0xA5FFFFFF, 16, 0x1234) == 0xA5120000
    # 0xC0000000 | 30 bits, shift 22: b = key bits [14, 30)
    assert hi_of(L, 0xFFFFFFFF, 22, 0xFFFF) == 0xFFFF0000
    assert hi_of(L, 0xFFFFFFFF, 22, 0x0001) == 0xC0000000
    assert hi_of(L, 0xFFFFFFFF, 22, 0x0004) == 0xC0010000
    # full keys, shift 24: b is the high half
    assert hi_of(L, 0xFFFFFFFF, 24, 0xBEEF) == 0xBEEF0000
    assert hi_of(L, 0x00000000, 24, 0xBEEF) == 0xBEEF0000
    # 0xDEAD0000 | 16 bits, shift 8 (the clamp): b lies wholly below bit 16
    assert hi_of(L, 0xDEADFFFF, 8, 0xFFFF) == 0xDEAD0000
    assert hi_of(L, 0xDEADFFFF, 8, 0) == 0xDEAD0000


def test_hi_rejects_arguments_out_of_range():
    from gpuradixsort_amd import _lib

    L = _lib.lib()
    for shift, seg in ((7, 0), (25, 0), (-1, 0), (16, 0x10000)):
        assert hi_of(L, 0, shift, seg) == 0xFFFFFFFF


def test_option_is_bound():
    """p2_half is option 18 with values auto / never; a NULL sorter is GRS_EINVAL before anything
    else is looked at."""
    from gpuradixsort_amd import _lib

    opt, names = _lib.OPTIONS["p2_half"]
    assert opt == 18 and names == {"auto": 0, "never": 1}
    L = _lib.lib()
    v = ctypes.c_int()
    assert L.grs_set_option(None, 18, 0) == _lib.GRS_EINVAL
    assert L.grs_get_option(None, 18, ctypes.byref(v)) == _lib.GRS_EINVAL
