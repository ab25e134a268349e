"""CPU test of the MSD sort's P3 kernel table (grs_debug_p3_kernel; no device).

The MSD schedule's last step sorts every 16-bit segment in LDS with one of eleven kernel
instantiations, chosen from n alone (msd_local_shape / msd_p3_kernel in csrc/grs_capi.hip).
grs_debug_p3_kernel reads the selection the launch reads, so this table pins which kernel a
sort of n keys runs: a changed threshold or a re-ordered branch shows here, not as a slower
benchmark line.  tests/test_gpu_p3_shapes.py runs every one of them at small n through the
p3_shape hook.
"""
import pytest

from gpuradixsort_amd import _lib

U32, U64 = _lib.GRS_KEY_U32, _lib.GRS_KEY_U64
P3 = _lib.OPTIONS["p3"][1]
SHAPE = _lib.OPTIONS["p3_shape"][1]
KEYS, PAIRS, KEYS64 = (U32, 0), (U32, 1), (U64, 0)
ANY = (KEYS, PAIRS, KEYS64)

# shape letter -> <BLOCK,I> of its whole-key kernel (the shape holds BLOCK * I keys)
DIMS = {"S": "256,8", "M": "256,12", "A": "256,20", "W": "1024,5", "B": "512,20", "C2": "768,23",
        "C": "768,24", "D": "1024,36"}


def kernel(ktype, n, p3="per_segment", shape="size"):
    name = _lib.lib().grs_debug_p3_kernel(ktype[0], ktype[1], int(n), P3[p3], SHAPE[shape])
    return name.decode() if name else None


def whole(shape):
    return f"grs_msd_local<{DIMS[shape]}>"


BY_SIZE = [
    # n, types, the shape (its whole-key kernel) or the kernel's name
    (1 << 20, ANY, "S"),
    ((1 << 26) + 12345, ANY, "S"),
    ((1 << 27) + 77, ANY, "M"),
    (1 << 28, (KEYS, PAIRS), "A"),
    (1 << 28, (KEYS64,), "W"),
    (1 << 29, ANY, "B"),
    (700_000_000, (KEYS,), "grs_msd_local16<512,34>"),
    (1 << 30, (KEYS,), "grs_msd_local16<512,34>"),
    (1_100_000_000, (KEYS,), "C"),
    (1_500_000_000, (KEYS,), "grs_msd_local16<1024,34>"),
    ((1 << 31) + 12345, (KEYS,), "grs_msd_local16<1024,34>"),
    (2_300_000_000, (KEYS,), "D"),
    (2_400_000_000, (KEYS,), None),
    (_lib.GRS_MAX_N, (KEYS,), None),
    (700_000_000, (PAIRS, KEYS64), None),
]


@pytest.mark.parametrize("n,types,want", BY_SIZE)
def test_p3_kernel_by_size(n, types, want):
    """p3_shape = 0: the kernel chosen from n, per type."""
    if want in DIMS:
        want = whole(want)
    for t in types:
        assert kernel(t, n) == want, (n, t)


def test_p3_whole_keys_at_2_30():
    assert kernel(KEYS, 1 << 30, "whole_keys") == "grs_msd_local<768,23>"
    assert kernel(KEYS, 1_500_000_000, "whole_keys") == "grs_msd_local<1024,36>"


@pytest.mark.parametrize("n,t,shape", [
    (1 << 20, KEYS, "S"), ((1 << 27) + 77, PAIRS, "M"), (1 << 28, KEYS, "A"), (1 << 28, PAIRS, "A"),
    (1 << 29, KEYS, "B"), (1 << 29, PAIRS, "B"), (1 << 30, KEYS, "C2"), (1_100_000_000, KEYS, "C"),
    (1_500_000_000, KEYS, "D"), (2_300_000_000, KEYS, "D"),
])
def test_p3_persistent_reports_the_pf_kernel_of_the_same_shape(n, t, shape):
    assert kernel(t, n, "persistent") == f"grs_msd_local_pf<{DIMS[shape]}>"


def test_p3_persistent_is_for_u32_only():
    """u64 keys have no persistent kernel (their run finish may reload the keys): p3 does not
    change what they launch."""
    for mode in P3:
        assert kernel(KEYS64, 1 << 28, mode) == whole("W")


def test_p3_shape_pin_names_the_pinned_kernel_at_any_n():
    """A pinned shape replaces the choice by size (and only that): the hook's names at a small n."""
    n = 1 << 20
    for t, shapes in ((KEYS, "SMABC"), (PAIRS, "SMAB"), (KEYS64, "SMWB")):
        for sh in shapes:
            for mode in ("per_segment", "whole_keys"):
                assert kernel(t, n, mode, sh) == whole(sh), (t, sh, mode)
    assert kernel(KEYS, n, "per_segment", "C2") == "grs_msd_local16<512,34>"
    assert kernel(KEYS, n, "whole_keys", "C2") == whole("C2")
    # D's low-halves kernel holds 34816 keys: it runs while msd_segment_need(n) fits it
    assert kernel(KEYS, n, "per_segment", "D") == "grs_msd_local16<1024,34>"
    assert kernel(KEYS, 2_300_000_000, "per_segment", "D") == whole("D")
    assert kernel(KEYS, n, "whole_keys", "D") == whole("D")
    # code 1 is A for 4-byte keys and W for u64 keys, under either name
    assert kernel(KEYS64, n, shape="A") == whole("W") and kernel(KEYS, n, shape="W") == whole("A")


def test_p3_shape_without_an_instantiation_has_no_kernel():
    """C2 / C / D exist for u32 keys without payload only; u64 pairs take the LSD passes."""
    n = 1 << 20
    for sh in ("C2", "C", "D"):
        assert kernel(PAIRS, n, shape=sh) is None and kernel(KEYS64, n, shape=sh) is None
    for sh in SHAPE:
        assert kernel((U64, 1), n, shape=sh) is None
    L = _lib.lib()
    assert L.grs_debug_p3_kernel(U32, 0, n, 0, 8) is None        # no such shape code
    assert L.grs_debug_p3_kernel(U32, 0, n, 3, 0) is None        # no such p3 mode
    assert L.grs_debug_p3_kernel(U32, 0, 0, 0, 0) is None
    assert L.grs_debug_p3_kernel(U32, 0, _lib.GRS_MAX_N + 1, 0, 4) is None
