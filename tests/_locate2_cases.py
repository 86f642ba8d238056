"""Shared cases of tests/test_locate2.py (host buffers, CPU engine) and
tests/test_gpu_locate2.py (device buffers, ec_locate2_n): geometries,
avail_masks, corruptions and the expected loc[] of ec_method_locate2[_device].

Expected values come from the oracle and the definition in include/
ec_method.h, never from the library (helpers from tests/_locate_cases.py).
loc[t] is 0 when avail is consistent; else 1 << i for the one brick whose
removal leaves the rest consistent (at most one: asserted); else the two bits
of the one pair whose removal does (at most one: asserted); else MANY.  That
is evaluated for the stripes a case corrupts; every other stripe is 0 because
the clean fragments are checked once, whole, against one prediction.  Beside
the oracle's value the MDS rule is asserted where it applies: damaged chunks
in one or two bricks give exactly those bits.

Every case also runs ec_method_locate on the same input: where it gives 0 or a
single bit locate2 must give the same value, and where it gives MANY locate2
must give two bits or MANY.
"""
import hashlib
import itertools

import numpy as np

import _locate_cases
from _locate_cases import (CHUNK, GUARD, MANY, SENTINEL, assert_clean, bits,  # noqa: F401
                           consistent, flipped, fragments, geom_id, plane_flips)

# (k, n, avail_mask), the smallest that reach each path: 5+4 is the narrowest
# volume with a - k = 4 (odd k, K = 8 bucket), 4+4 the K = 4 bucket, 0x3BFFFD
# is 16+6 with bricks 1 and 18 missing (non-contiguous basis, a - k = 4).
GEOMS = [
    (5, 9, 0x1FF),
    (4, 8, 0xFF),
    (8, 12, 0xFFF),
    (16, 20, 0xFFFFF),
    (16, 22, 0x3BFFFD),
]
GEOM_LARGEST = (16, 31, 0x7FFFFFFF)     # r = 15: 152 candidates per tile (on the GPU)
SIZES = [1, 3, 4, 5, 67]

_want_cache = {}


def drop_fragments(key):
    """Forget the shared fragments of (k, n, nst): for the one large size."""
    _locate_cases._frag_cache.pop(key, None)


def expected_loc2(O, k, n, avail, frags, t):
    """loc[t] by the definition, from the stored fragments `frags` (by brick).
    Remembered by content: the CPU generations and the GPU see the same cases."""
    chunk = {b: frags[b][t * CHUNK:(t + 1) * CHUNK] for b in avail}
    h = hashlib.blake2b(digest_size=16)
    for b in avail:
        h.update(chunk[b].tobytes())
    key = (k, n, tuple(avail), h.digest())
    if key not in _want_cache:
        _want_cache[key] = _by_definition(O, k, n, avail, chunk)
    return _want_cache[key]


def _by_definition(O, k, n, avail, chunk):
    if consistent(O, k, n, avail, chunk):
        return 0
    hits = [i for i in avail if consistent(O, k, n, [b for b in avail if b != i], chunk)]
    assert len(hits) <= 1, hits
    if hits:
        return 1 << hits[0]
    pairs = [(i, j) for i, j in itertools.combinations(avail, 2)
             if consistent(O, k, n, [b for b in avail if b not in (i, j)], chunk)]
    assert len(pairs) <= 1, pairs
    return (1 << pairs[0][0] | 1 << pairs[0][1]) if pairs else MANY


def check_against_locate(loc2, loc1, what):
    """The consequences the header states of ec_method_locate's answer."""
    loc1 = np.asarray(loc1, np.uint32)
    single = ((loc1 & (loc1 - np.uint32(1))) == 0) & (loc1 != MANY)    # 0 or a brick's bit
    assert np.array_equal(loc2[single], loc1[single]), (what, loc2[:8], loc1[:8])
    for v in loc2[~single].tolist():
        assert v == MANY or bin(v).count("1") == 2, (what, hex(v))
    assert (loc1[~single] == MANY).all(), (what, loc1[:8])


def damaged(clean, rng, t, bricks, how):
    """{brick: corrupted copy}: the chunks of `bricks` in stripe t damaged at
    different symbols, at the same symbol, at the same symbol in different
    planes, or replaced by random bytes."""
    out = {}
    for j, b in enumerate(bricks):
        if how == "symbols":
            out[b] = flipped(clean[b], t, 200 + j, 3)
        elif how == "symbol":
            out[b] = flipped(clean[b], t, 300, 2)
        elif how == "planes":
            out[b] = flipped(clean[b], t, 300 + 64 * j, 2)
        else:
            buf = clean[b].copy()
            buf[t * CHUNK:(t + 1) * CHUNK] = rng.integers(0, 256, CHUNK, dtype=np.uint8)
            out[b] = buf
    return out


WAYS = ("symbols", "symbol", "planes", "random")


def pair_kinds(basis, checks):
    k, r = len(basis), len(checks)
    return [
        (basis[0], basis[k - 1]), (basis[1], basis[2]),                 # basis + basis
        (basis[1], checks[0]), (basis[k // 2], checks[1]), (basis[0], checks[r - 1]),
        (checks[0], checks[1]), (checks[0], checks[r - 1]),             # check + check
    ]


def run_geometry(run, O, k, n, avail_mask, nst):
    """Every corruption case of one geometry and size.  run(frags) -> (loc[0..
    nst) of locate2 as uint32, nbad or None, loc[0..nst) of locate on the same
    input) with frags a list by brick (None outside avail_mask; an entry that
    is not the clean fragment object is a corrupted copy); the runner checks
    its own sentinel and guard words."""
    clean = fragments(O, k, n, nst)
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    r = len(checks)
    assert r >= 4
    assert_clean(O, k, n, avail, clean, nst)
    base = [clean[b] if b in avail else None for b in range(n)]
    rng = np.random.default_rng(11 * k + n + nst)

    def locate2(changes, what, rule=None):
        """changes: {brick: corrupted fragment}; the stripes that differ from
        the clean fragments are the ones evaluated by the definition."""
        fr = list(base)
        stripes = set()
        for b, buf in changes.items():
            fr[b] = buf
            d = (buf.reshape(nst, CHUNK) != clean[b].reshape(nst, CHUNK)).any(axis=1)
            stripes.update(np.flatnonzero(d).tolist())
        want = np.zeros(nst, np.uint32)
        for t in stripes:
            want[t] = expected_loc2(O, k, n, avail, fr, t)
        if rule is not None:
            assert want.tolist() == rule.tolist(), (what, want, rule)
        loc, nbad, loc1 = run(fr)
        assert np.array_equal(loc, want), (what, np.flatnonzero(loc != want)[:8],
                                           loc[:8], want[:8])
        if nbad is not None:
            assert nbad == int(np.count_nonzero(want)), (what, nbad)
        check_against_locate(loc, loc1, what)

    def one(t, v):
        rule = np.zeros(nst, np.uint32)
        rule[t] = v
        return rule

    def merged(*changes):
        """Corruptions of several stripes in one set of fragments."""
        out = {}
        for ch in changes:
            for b, buf in ch.items():
                if b in out:
                    d = buf != clean[b]
                    out[b] = out[b].copy()
                    out[b][d] = buf[d]
                else:
                    out[b] = buf
        return out

    locate2({}, "clean", np.zeros(nst, np.uint32))

    # the single-brick cases of _locate_cases.run_geometry: locate's answers
    for b in (basis[0], basis[k - 1], checks[0], checks[r - 1]):
        for t, byte, bit in plane_flips(nst):
            locate2({b: flipped(clean[b], t, byte, bit)}, ("flip", b, t, byte, bit),
                    one(t, 1 << b))
    for b in (basis[k // 2], checks[r // 2]):
        locate2(damaged(clean, rng, nst // 2, [b], "random"), ("random chunk", b),
                one(nst // 2, 1 << b))

    # pairs of every kind, damaged in four ways, walking over the stripes
    i = 0
    for b1, b2 in pair_kinds(basis, checks):
        for how in WAYS:
            t = (nst - 1 - i) % nst
            i += 1
            locate2(damaged(clean, rng, t, [b1, b2], how), ("pair", b1, b2, how, t),
                    one(t, 1 << b1 | 1 << b2))

    # three bricks at one symbol: the oracle decides (with a - k = 4 they can
    # imitate a pair); with a - k >= 5 the distance makes it MANY
    for trio in ((basis[0], basis[1], checks[0]), (basis[2], checks[1], checks[r - 1]),
                 (basis[0], basis[k // 2], basis[k - 1])):
        locate2(damaged(clean, rng, 0, trio, "symbol"), ("three bricks, one symbol", trio),
                one(0, MANY) if r >= 5 else None)

    # one 4-stripe tile: clean, a single, a pair of basis bricks, and three
    # bricks damaged at three symbols (each symbol has one error, so the stored
    # chunks are within one position of the original codeword per symbol and
    # no other codeword is within two: MANY)
    if nst >= 4:
        bb, cb = basis[k - 2], checks[1]
        ch = merged({bb: flipped(clean[bb], 1, 77, 5)},
                    damaged(clean, rng, 2, [basis[0], basis[k - 1]], "random"),
                    damaged(clean, rng, 3, [bb, basis[0], cb], "symbols"))
        rule = np.zeros(nst, np.uint32)
        rule[1], rule[2], rule[3] = 1 << bb, 1 << basis[0] | 1 << basis[k - 1], MANY
        if nst >= 5:                          # and a pair of check bricks in the next tile
            ch = merged(ch, damaged(clean, rng, 4, [checks[0], checks[2]], "planes"))
            rule[4] = 1 << checks[0] | 1 << checks[2]
        locate2(ch, "mixed tile", rule)

    # a pair in the ragged last tile while the first tile is clean
    if nst >= 5:
        t = nst - 1
        for b1, b2 in ((basis[2], checks[0]), (basis[0], basis[3])):
            locate2(damaged(clean, rng, t, [b1, b2], "symbols"), ("last tile", b1, b2),
                    one(t, 1 << b1 | 1 << b2))
