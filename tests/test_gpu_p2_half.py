"""GPU tests of the MSD sort's half regions (option p2_half): for u32 keys whose P3 is
grs_msd_local16, P2 writes only the low 16 bits of each key into its sampled regions and P3
rebuilds the rest from the segment's index and the keys' span.

The sampled-region path starts at 2^26 keys, so every case sorts n = 2^26 + 12345 keys (the size
test_p3_shape_reads_sampled_regions uses; its helpers are imported), once, with the shape pinned
to C2 (grs_msd_local16<512,34>) or D (<1024,34>).  Expected output: the LSD schedule's on a
second sorter (msd = never; pinned to the oracle by test_gpu_parity.py), and
oracle.stable_argsort on the planted segments.  Every case asserts that the path it is about
ran: msd_flags (p2_half, no P1 redo, no exact P2, the top shift), no error word, no guard word
touched."""
import numpy as np
import pytest
import torch

import oracle
import test_gpu_p3_shapes as p3

pytestmark = pytest.mark.gpu

N = (1 << 26) + 12345
SHAPES = ("C2", "D")
KERNEL = {"C2": "grs_msd_local16<512,34>", "D": "grs_msd_local16<1024,34>"}
TILEF = p3.TILEF["u32"]


@pytest.fixture(scope="module", autouse=True)
def _close_sorters():
    yield
    for key in list(p3._S):
        p3._S.pop(key).close()
    _LISTED.clear()


def half_sorter(shape, p2_half="auto", msd="always"):
    """The pinned u32 sorter (p3.pinned asserts the kernel's name) with option p2_half set."""
    s = p3.sorter("u32", N, msd)
    s.set_option("p3", "per_segment")
    s.set_option("p3_shape", shape)
    s.set_option("p2_half", p2_half)
    assert s.p3_kernel(N) == KERNEL[shape]
    return s


def sort_with(s, keys, gpu):
    k = torch.from_numpy(keys).to(gpu)
    s.sort(k)
    torch.cuda.synchronize()
    s.check_error()
    assert s.check_guards() == 0, "a kernel wrote past a scratch array (guard band)"
    return k, s.msd_flags(p2_half=True)


def lsd_sorted(keys, gpu):
    """The LSD schedule's output for keys (a second sorter, msd = never)."""
    ref = p3.sorter("u32", N, "never")
    rk = torch.from_numpy(keys).to(gpu)
    ref.sort(rk)
    torch.cuda.synchronize()
    ref.check_error()
    return rk


def assert_same(k, rk, what):
    if not torch.equal(k, rk):
        a, b = k.view(torch.int32), rk.view(torch.int32)
        bad = torch.nonzero(a != b).flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {k.numel()} keys differ, first at {i}: "
                             f"{int(a[i]) & 0xFFFFFFFF:#x} != {int(b[i]) & 0xFFFFFFFF:#x}")


def bounded_keys(top, bits, seed):
    """N keys top | uniform low part of `bits` bits, the low parts 0 and 2^bits - 1 among them, so
    that the keys fill [top, top + 2^bits) exactly."""
    rng = np.random.default_rng([bits, seed])
    keys = rng.integers(0, 1 << bits, N, dtype=np.uint64).astype(np.uint32)
    keys[N // 3] = 0
    keys[N // 2] = (1 << bits) - 1
    keys |= np.uint32(top)
    return keys


# (top, varying bits, top shift)
SPAN = [(0xA5000000, 24, 16), (0xC0000000, 30, 22), (0x90000000, 28, 20), (0, 32, 24),
        (0xDEAD0000, 16, 8), (0, 26, 18)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("top,bits,shift", SPAN, ids=[f"{t:#x}+{b}b" for t, b, _ in SPAN])
def test_half_regions_span(gpu, shape, top, bits, shift):
    """Uniform low parts under a constant top: bits 16..31 of every key come from the OR word
    (the constant top and nothing below bit shift + 8) and from the segment's index shifted to
    its place; at shift 8 the index lies wholly below bit 16.  Keys that fill [top, top + 2^bits)
    exactly, [0, 2^32) and [0, 2^26) among them."""
    keys = bounded_keys(top, bits, 1)
    s = half_sorter(shape)
    k, f = sort_with(s, keys, gpu)
    assert f == {"p1_redo": False, "p2_exact": False, "top_shift": shift, "p2_half": True}, f
    assert_same(k, lsd_sorted(keys, gpu), f"{shape} {top:#x} | {bits} bits")


_LISTED = {}


def listed_input(shape):
    """Keys 0xC0000000 | 30 uniform bits (top shift 22: 16-bit segment = key bits [14, 30)) with
    planted segments: one key (the widening copy), the mid list (C2: SMAX + 3; D, whose mid list
    is empty, SMAX and SMAX + 3), and the big list without and with a histogram row (MID + 3,
    2 TILEF + 1); spread evenly so that H2's sample sees its share.  -> keys, {prefix: positions}"""
    if shape in _LISTED:
        return _LISTED[shape]
    _, smax, mid = p3.expect("u32", shape, "per_segment")
    wants = [1, smax + 3, mid + 3, 2 * TILEF + 1] if mid != smax else [1, smax, smax + 3, 2 * TILEF + 1]
    prefixes = [0x0042, 0x1234, 0x8001, 0xC0DE]
    keys = bounded_keys(0xC0000000, 30, 2)
    dt = np.uint32
    for p in prefixes:   # the uniform keys of these prefixes move to the next prefix
        keys[((keys >> dt(14)) & dt(0xFFFF)) == dt(p)] += dt(1 << 14)
    rng = np.random.default_rng(smax)
    planted = {}
    for j, (p, want) in enumerate(zip(prefixes, wants)):
        at = 4 * ((np.arange(want, dtype=np.int64) * (N // 4)) // want) + j
        low = rng.integers(0, 1 << 14, want, dtype=np.uint64)
        keys[at] = (np.uint64(0xC0000000) | (np.uint64(p) << np.uint64(14)) | low).astype(dt)
        planted[p] = at
    for p, want in zip(prefixes, wants):
        assert int(np.count_nonzero(((keys >> dt(14)) & dt(0xFFFF)) == dt(p))) == want
    assert int(keys.min()) == 0xC0000000 and int(keys.max()) == 0xFFFFFFFF
    _LISTED[shape] = (keys, planted)
    return _LISTED[shape]


def check_planted(k, keys, planted):
    """The planted segments of the output k against the stable sort of their own keys."""
    for p, at in planted.items():
        order = at[oracle.stable_argsort(keys[at])]
        first = np.uint32(0xC0000000 | (p << 14))
        lo = int(np.count_nonzero(keys < first))
        assert np.array_equal(k[lo:lo + at.size].cpu().numpy(), keys[order]), hex(p)


@pytest.mark.parametrize("shape", SHAPES)
def test_half_regions_listed_segments(gpu, shape):
    """One-key, mid-list and big-list segments read from a half region at a narrow shift: each
    widened with its own hi (carried by the list entry), then sorted by the larger LDS shape or
    moved to its place for the fallback."""
    keys, planted = listed_input(shape)
    s = half_sorter(shape)
    k, f = sort_with(s, keys, gpu)
    assert f == {"p1_redo": False, "p2_exact": False, "top_shift": 22, "p2_half": True}, f
    assert_same(k, lsd_sorted(keys, gpu), f"{shape} listed")
    check_planted(k, keys, planted)


@pytest.mark.parametrize("shape", SHAPES)
def test_half_regions_spill(gpu, shape):
    """The forced exact P2 (msd = 2: no region buffer): P3 must take the whole-key, in-place
    branch, with hi from the segment's first key."""
    keys, planted = listed_input(shape)
    s = half_sorter(shape, msd="exact_p2")
    k, f = sort_with(s, keys, gpu)
    assert f == {"p1_redo": False, "p2_exact": True, "top_shift": 22, "p2_half": False}, f
    assert_same(k, lsd_sorted(keys, gpu), f"{shape} spill")
    check_planted(k, keys, planted)


def test_half_regions_switch(gpu):
    """p2_half = 1 keeps whole keys in the regions: the flag is off and the output identical."""
    keys, _ = listed_input("C2")
    k1, f1 = sort_with(half_sorter("C2", "never"), keys, gpu)
    assert f1 == {"p1_redo": False, "p2_exact": False, "top_shift": 22, "p2_half": False}, f1
    k0, f0 = sort_with(half_sorter("C2", "auto"), keys, gpu)
    assert f0["p2_half"] and not f0["p2_exact"], f0
    assert torch.equal(k0, k1)


def test_half_option_round_trip(gpu):
    """Option 18 round-trips; values outside 0..1 are GRS_EINVAL and leave it unchanged.  Types
    without a low-halves kernel accept it and keep whole keys (the flag stays off)."""
    import gpuradixsort_amd as grs

    s = grs.RadixSorter(1 << 16, key_bits=32, pairs=False, radix_bits=8)
    try:
        assert s.get_option("p2_half") == 0
        s.set_option("p2_half", "never")
        assert s.get_option("p2_half") == 1
        for bad in (-1, 2, 18):
            with pytest.raises(grs.GrsError) as e:
                s.set_option("p2_half", bad)
            assert e.value.status == 1
            assert s.get_option("p2_half") == 1
        s.set_option("p2_half", "auto")
        assert s.get_option("p2_half") == 0
        # a small sort on the MSD schedule: no sampled regions, so no halves
        s.set_option("msd", "always")
        k = torch.from_numpy(np.random.default_rng(0).integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
                             .astype(np.uint32)).to(gpu)
        s.sort(k)
        assert s.msd_flags(p2_half=True)["p2_half"] is False
        assert "p2_half" not in s.msd_flags()   # (the three-key form other tests compare whole)
    finally:
        s.close()
