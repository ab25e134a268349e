"""GPU tests of every P3 kernel instantiation of the MSD sort at small n (option p3_shape).

P3 sorts each 16-bit segment in LDS with a kernel chosen from n alone, so most instantiations
used to run only in sorts of 2^27 .. 2^31 keys, checked by order and checksums on two benign
distributions.  The p3_shape hook pins the shape while the rest of the schedule keeps going by
n; every case here first asserts (p3_kernel) that the instantiation it is meant to run is the
one a sort launches, then compares bit-exactly with the stable sort (oracle.stable_argsort):
the keys and, for pairs, the payload, which is the stable permutation.

Inputs are built per case from the running kernel's capacity SMAX (17408 / 34816 for the
low-halves kernels) and the mid list's bound MID it passes:
  segment lengths 1, 2, 3, 63, 64, 65, SMAX-1, SMAX, SMAX+1, MID, MID+1 and two fallback tiles
  + 1, with absent prefixes in between, the capacity-edge segments placed at every 16-B
  misalignment of their destination (fillers of 1, 2, 3 keys before them).
"""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

# shape letter -> (BLOCK, I): the shape holds BLOCK * I keys
DIMS = {"S": (256, 8), "M": (256, 12), "A": (256, 20), "W": (1024, 5), "B": (512, 20),
        "C2": (768, 23), "C": (768, 24), "D": (1024, 36)}
# the fallback's tile (the big tile of the type: csrc/grs_capi.hip BigTile)
TILEF = {"u32": 36864, "pairs": 17408, "u64": 17408}
KEY_BITS = {"u32": 32, "pairs": 32, "u64": 64}


def expect(typ, shape, mode):
    """(kernel name, SMAX, MID) of a case, written down from DESIGN §4.1 / run_msd: the mid
    list is shape C's for u32 keys (18432) and B's (10240) for the other types; the low-halves
    kernels hold 512 x 34 and 1024 x 34 keys, and the second has no mid list."""
    b, i = DIMS[shape]
    mid = max(b * i, 18432 if typ == "u32" else 10240)
    if mode == "persistent":
        return f"grs_msd_local_pf<{b},{i}>", b * i, mid
    if typ == "u32" and mode == "per_segment" and shape == "C2":
        return "grs_msd_local16<512,34>", 17408, mid
    if typ == "u32" and mode == "per_segment" and shape == "D":
        return "grs_msd_local16<1024,34>", 34816, 34816
    return f"grs_msd_local<{b},{i}>", b * i, mid


CASES = ([("u32", s, m) for m in ("per_segment", "whole_keys") for s in ("S", "M", "A", "B", "C2", "C", "D")]
         + [("pairs", s, "per_segment") for s in ("S", "M", "A", "B")]
         + [("u64", s, "per_segment") for s in ("S", "M", "W", "B")]
         + [("u32", "A", "persistent"), ("u32", "C", "persistent"), ("u32", "D", "persistent"),
            ("pairs", "B", "persistent")])
IDS = ["-".join(c) for c in CASES]

_S = {}


@pytest.fixture(scope="module", autouse=True)
def _close_sorters():
    yield
    for key in list(_S):
        _S.pop(key).close()
    _UNIFORM.clear()


def sorter(typ, n, msd="always"):
    """One sorter per (type, schedule), grown on demand; the large ones one at a time (HBM)."""
    import gpuradixsort_amd as grs

    key = (typ, msd)
    s = _S.get(key)
    if s is None or s.capacity < n:
        for other in list(_S):
            if other == key or n >= (1 << 26) or _S[other].capacity >= (1 << 26):
                _S.pop(other).close()
        s = grs.RadixSorter(max(n, 1 << 21), key_bits=KEY_BITS[typ], pairs=typ == "pairs", radix_bits=8)
        s.set_option("msd", msd)
        _S[key] = s
    return s


def pinned(typ, shape, mode, n):
    """The type's MSD sorter with the case's shape and p3 mode -- after asserting that a sort of
    n items launches the instantiation the case is about (a hook that was silently ignored would
    pass every case on shape S)."""
    name = expect(typ, shape, mode)[0]
    s = sorter(typ, n)
    s.set_option("p3", mode)
    s.set_option("p3_shape", shape)
    assert s.p3_kernel(n) == name, (typ, shape, mode, n)
    return s


def sort_and_check(s, keys, dev, what):
    """keys (and, for a pairs sorter, the payload 0..n-1) == the stable sort, bit for bit; no
    error word, no guard word touched."""
    k = torch.from_numpy(keys).to(dev)
    v = torch.arange(keys.size, dtype=torch.int32, device=dev).view(torch.uint32) if s.pairs else None
    s.sort(k, v)
    torch.cuda.synchronize()
    s.check_error()
    assert s.check_guards() == 0, f"{what}: a kernel wrote past a scratch array (guard band)"
    perm = oracle.stable_argsort(keys)
    got = k.cpu().numpy()
    want = keys[perm]
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {keys.size} keys differ, first at {bad[0]}: "
                             f"{got[bad[0]]:#x} != {want[bad[0]]:#x}")
    if s.pairs:
        gv = v.cpu().numpy()
        if not np.array_equal(gv, perm):
            bad = np.flatnonzero(gv != perm)
            raise AssertionError(f"{what}: {bad.size} payload words differ (stability), first at {bad[0]}")


# ---- inputs ------------------------------------------------------------------------------

def rev8(d):
    d = ((d & 0xF0) >> 4) | ((d & 0x0F) << 4)
    d = ((d & 0xCC) >> 2) | ((d & 0x33) << 2)
    return ((d & 0xAA) >> 1) | ((d & 0x55) << 1)


def low_part(pattern, rng, c, bits):
    """c low parts of `bits` bits (the bits P3 sorts), as uint64."""
    mask = (1 << bits) - 1
    if bits == 0:
        return np.zeros(c, np.uint64)
    if pattern == "uniform":
        return rng.integers(0, 1 << bits, c, dtype=np.uint64)
    if pattern == "five":   # heavy ties: the stability check of the pairs
        vals = rng.integers(0, 1 << bits, 5, dtype=np.uint64)
        return vals[rng.integers(0, 5, c)]
    if pattern == "runs64":
        # every value of every 8-bit digit 64 times (and a tail): each round's scatter sends a
        # wave's keys to run starts 64 apart, the case the XOR swizzle of the LDS positions is
        # for; byte b holds the run index, bit-reversed in the odd bytes so that a round reorders
        d = (np.arange(c, dtype=np.uint64) // np.uint64(64)) & np.uint64(255)
        r = rev8(d)
        low = np.zeros(c, np.uint64)
        for b in range((bits + 7) // 8):
            low |= (r if b & 1 else d) << np.uint64(8 * b)
        return low & np.uint64(mask)
    if pattern == "equal":
        return np.full(c, 0x5A5A5A5A5A5A5A5A & mask, np.uint64)
    raise ValueError(pattern)


def edge_lengths(smax, mid, tilef, vec):
    """The case's segment lengths in output order: the small ones, then SMAX-1 / SMAX / SMAX+1 /
    MID / MID+1 each at every destination offset mod vec (fillers of 1..3 keys in front), then
    two fallback tiles + 1 (vec: keys in 16 B)."""
    lens, at, seen = [], 0, set()

    def put(c):
        nonlocal at
        lens.append(c)
        at += c

    for c in (1, 2, 3, 63, 64, 65):
        put(c)
    edges = [smax - 1, smax, smax + 1] + ([mid, mid + 1] if mid != smax else [])
    for r in range(vec):
        for e in edges:
            while at % vec != r:
                put(min(3, (r - at) % vec))
            seen.add((e, at % vec))
            put(e)
    put(2 * tilef + 1)
    assert seen == {(e, r) for e in edges for r in range(vec)}
    return lens


def segment_keys(rng, dtype, lengths, pattern, shift):
    """Keys whose 16-bit prefixes (bits [shift - 8, shift + 8)) hold exactly lengths[i] keys, in
    ascending prefix order with absent prefixes in between, low parts by `pattern`, shuffled; one
    key of all ones below bit shift + 8 at the end, so that (with the first prefixes' clear top
    bit) the highest varying bit is shift + 7 and the top digit's shift is `shift`."""
    lb = shift - 8
    stride = 0x7000 // len(lengths)
    assert stride >= 2   # absent prefixes between any two segments
    parts = []
    for i, c in enumerate(lengths):
        prefix = np.uint64(3 + i * stride) << np.uint64(lb)
        parts.append(prefix | low_part(pattern, rng, c, lb))
    keys = np.concatenate(parts)
    rng.shuffle(keys)
    keys = np.append(keys, np.uint64((1 << (shift + 8)) - 1))
    return keys.astype(dtype)


def top_shift_of_bound(bits, key_bits):
    """DESIGN §4.1's span rule: the top digit is the byte whose top bit is the highest varying
    bit (bits - 1 for keys that fill [0, 2^bits)), kept between bits [8, 16) and the top byte."""
    return min(max(bits - 8, 8), key_bits - 8)


# ---- the tests ---------------------------------------------------------------------------

@pytest.mark.parametrize("typ,shape,mode", CASES, ids=IDS)
def test_p3_shape_segment_edges(gpu, typ, shape, mode):
    """Every instantiation at its capacity edges, every destination misalignment, four low-part
    patterns (uniform, five values, 64-long digit runs, all equal)."""
    _, smax, mid = expect(typ, shape, mode)
    kb = KEY_BITS[typ]
    dt = np.uint32 if kb == 32 else np.uint64
    lengths = edge_lengths(smax, mid, TILEF[typ], 16 // (kb // 8))
    n = sum(lengths) + 1
    assert n <= 2_100_000
    s = pinned(typ, shape, mode, n)
    for j, pattern in enumerate(("uniform", "five", "runs64", "equal")):
        rng = np.random.default_rng([smax, mid, kb, j])
        keys = segment_keys(rng, dt, lengths, pattern, kb - 8)
        sort_and_check(s, keys, gpu, f"{typ} {shape} {mode} {pattern}")
        f = s.msd_flags()
        assert f["top_shift"] == kb - 8, f


NARROW = {32: (28, 24, 20, 16), 64: (56, 40, 32, 24)}


@pytest.mark.parametrize("typ,shape,mode", CASES, ids=IDS)
def test_p3_shape_narrow_keys(gpu, typ, shape, mode):
    """Keys bounded by 2^b: the top digit follows the span, so P3 sorts fewer bits (u32: 2 rounds
    at b = 28, 1 round over 8, 4 and 0 varying bits at b = 24, 20, 16; u64: 5, 3, 2, 1 rounds) --
    every round count msd_p3_rounds returns, with a segment at SMAX and one past it."""
    _, smax, mid = expect(typ, shape, mode)
    kb = KEY_BITS[typ]
    dt = np.uint32 if kb == 32 else np.uint64
    lengths = [1, 2, 3, 65, smax - 1, 1, smax, 2, smax + 1, mid + 1]
    n = sum(lengths) + 1
    s = pinned(typ, shape, mode, n)
    for bits in NARROW[kb]:
        shift = top_shift_of_bound(bits, kb)
        rng = np.random.default_rng([smax, kb, bits])
        keys = segment_keys(rng, dt, lengths, "uniform", shift)
        assert int(keys.max()) == (1 << bits) - 1
        sort_and_check(s, keys, gpu, f"{typ} {shape} {mode} keys < 2^{bits}")
        f = s.msd_flags()
        assert f["top_shift"] == shift, (bits, f)


def run_segment(rng, prefix, runs):
    """u64 keys of one 16-bit prefix made of runs: run j holds runs[j] keys that agree in bits
    [32, 48) -- the two bytes P3's two rounds sort -- and differ below."""
    parts = []
    mids = rng.choice(1 << 16, len(runs), replace=False).astype(np.uint64)
    for m, c in zip(mids, runs):
        low = np.unique(rng.integers(0, 1 << 32, c + c // 2 + 8, dtype=np.uint64))[:c]
        assert low.size == c   # distinct low halves
        parts.append((np.uint64(prefix) << np.uint64(48)) | (m << np.uint64(32)) | low)
    return np.concatenate(parts)


@pytest.mark.parametrize("shape", ["S", "M", "W", "B"])
def test_p3_u64_run_finish(gpu, shape):
    """u64 keys: two LDS rounds on bits [32, 48), then every run of keys equal in them is
    insertion-sorted on the bits below -- up to kRunMax = 48 keys; a run of 49 sends the whole
    segment through all six rounds.  Runs of 1, 2, 47, 48, 49 and 200 keys whose members stand
    in descending order in the input (the insertion sort moves every one): segments with runs
    of at most 48 only, with a single 49-run among short ones, one that is a single run, and the
    same at the shape's capacity."""
    smax = DIMS[shape][0] * DIMS[shape][1]
    rng = np.random.default_rng(smax)
    short = [1, 2, 47, 48, 3, 48, 1, 47, 2, 48]
    fill48 = [48] * (smax // 48) + ([smax % 48] if smax % 48 else [])
    segs = [short,                                # runs <= 48 only
            short + [49],                         # a single 49-run among short ones
            [200] + short,                        # a long run first
            [1500],                               # a single run of the whole segment
            [1, 2, 47, 48, 49, 200],              # the issue's run lengths side by side
            fill48,                               # at capacity, runs <= 48 only
            [49] + fill48[:-2] + [smax - 49 - 48 * (len(fill48) - 2)],   # at capacity, one 49-run
            [smax]]                               # at capacity, a single run
    assert all(sum(r) <= smax for r in segs) and sum(segs[6]) == smax and sum(segs[5]) == smax
    keys = np.concatenate([run_segment(rng, 5 + 1000 * i, r) for i, r in enumerate(segs)])
    keys = np.append(keys, np.uint64(0xFFFFFFFFFFFFFFFF))
    rng.shuffle(keys)
    # the members of every run in descending order of their low bits, at the run's positions
    hi = keys >> np.uint64(32)
    where = np.lexsort((np.arange(keys.size), hi))          # positions grouped by run, ascending
    desc = np.lexsort((~keys, hi))                          # keys grouped by run, descending
    out = np.empty_like(keys)
    out[where] = keys[desc]
    for a in (5, 5 + 3000):   # (spot check of the construction)
        m = out[(out >> np.uint64(48)) == np.uint64(a)]
        g = m[(m >> np.uint64(32)) == (m[0] >> np.uint64(32))]
        assert np.all(g[:-1] > g[1:])
    s = pinned("u64", shape, "per_segment", out.size)
    sort_and_check(s, out, gpu, f"u64 {shape} run finish")
    assert s.msd_flags()["top_shift"] == 56


# the sampled-region path: one case per kernel family
REGION = [("u32", "C", "per_segment"), ("u32", "C2", "per_segment"), ("u32", "D", "per_segment"),
          ("pairs", "B", "per_segment"), ("u64", "W", "per_segment")]
_UNIFORM = {}


def uniform_keys(kb, n):
    if kb not in _UNIFORM:
        _UNIFORM.clear()
        rng = np.random.default_rng(kb)
        _UNIFORM[kb] = rng.integers(0, 1 << kb, n, dtype=np.uint64).astype(np.uint32 if kb == 32 else np.uint64)
    return _UNIFORM[kb]


@pytest.mark.parametrize("typ,shape,mode", REGION, ids=["-".join(c) for c in REGION])
def test_p3_shape_reads_sampled_regions(gpu, typ, shape, mode):
    """From 2^26 keys P2 scatters into regions sized from a sample and P3 reads the region
    buffer (below, it sorts in place).  Uniform keys plus two planted prefixes -- one a little
    past the kernel's SMAX (the mid list, read from the regions), one past MID (the big list:
    moved to its place, then the fallback) -- spread evenly so that H2's sample sees its share.
    Expected: the LSD schedule's output on a second sorter (pinned to the oracle by
    test_gpu_parity.py), and numpy for the planted segments."""
    _, smax, mid = expect(typ, shape, mode)
    kb = KEY_BITS[typ]
    n = (1 << 26) + 12345
    keys = uniform_keys(kb, n).copy()
    dt = keys.dtype.type
    pshift = kb - 16
    targets = {0x1234: smax + 3, 0xC0DE: mid + 3} if mid != smax else {0x1234: smax, 0xC0DE: smax + 3}
    rng = np.random.default_rng(smax)
    planted = {}
    for p in targets:   # the uniform keys of these prefixes move to the next prefix
        keys[(keys >> dt(pshift)) == dt(p)] += dt(1 << pshift)
    for j, (p, want) in enumerate(targets.items()):
        # evenly spread over the input, on the even positions for one prefix and the odd for the other
        at = 2 * ((np.arange(want, dtype=np.int64) * (n // 2)) // want) + j
        low = rng.integers(0, 1 << pshift, want, dtype=np.uint64)
        keys[at] = ((np.uint64(p) << np.uint64(pshift)) | low).astype(dt)
        planted[p] = at
    for p, want in targets.items():
        assert int(np.count_nonzero((keys >> dt(pshift)) == dt(p))) == want

    s = pinned(typ, shape, mode, n)
    k = torch.from_numpy(keys).to(gpu)
    v = torch.arange(n, dtype=torch.int32, device=gpu).view(torch.uint32) if s.pairs else None
    s.sort(k, v)
    torch.cuda.synchronize()
    s.check_error()
    assert s.check_guards() == 0
    f = s.msd_flags()
    assert not f["p1_redo"] and not f["p2_exact"], f   # else P3 sorted in place: nothing shown
    assert f["top_shift"] == kb - 8

    pairs = s.pairs
    ref = sorter(typ, n, "never")
    rk = torch.from_numpy(keys).to(gpu)
    rv = torch.arange(n, dtype=torch.int32, device=gpu).view(torch.uint32) if pairs else None
    ref.sort(rk, rv)
    torch.cuda.synchronize()
    ref.check_error()
    assert torch.equal(k, rk)
    if pairs:
        assert torch.equal(v, rv)
    # the planted segments against numpy
    for p, want in targets.items():
        at = planted[p]
        order = at[oracle.stable_argsort(keys[at])]
        lo = int(np.count_nonzero(keys < dt(p << pshift)))
        assert np.array_equal(k[lo:lo + want].cpu().numpy(), keys[order]), hex(p)
        if pairs:
            assert np.array_equal(v[lo:lo + want].cpu().numpy(), order.astype(np.uint32)), hex(p)


def test_p3_shape_option_range(gpu):
    """A shape with no instantiation for the sorter's type is GRS_EINVAL; 0 restores the choice
    by size."""
    import gpuradixsort_amd as grs

    for typ, bad in (("pairs", ("C2", "C", "D")), ("u64", ("C2", "C", "D"))):
        s = sorter(typ, 1 << 20)
        for sh in bad:
            with pytest.raises(grs.GrsError) as e:
                s.set_option("p3_shape", sh)
            assert e.value.status == 1
        s.set_option("p3_shape", "B")
        assert s.get_option("p3_shape") == 2
        s.set_option("p3_shape", "size")
        s.set_option("p3", "per_segment")
        assert s.p3_kernel(1 << 20) == "grs_msd_local<256,8>"
    s = sorter("u32", 1 << 20)
    with pytest.raises(grs.GrsError):
        s.set_option("p3_shape", 8)
    s.set_option("p3_shape", "size")
    s.set_option("p3", "per_segment")
    assert s.p3_kernel(1 << 30) == "grs_msd_local16<512,34>"
