"""Shared cases of tests/test_locate.py (host buffers, CPU engine) and
tests/test_gpu_locate.py (device buffers, ec_locate_n): geometries,
avail_masks, corruptions and the expected loc[] of ec_method_locate[_device].

Expected values come from the oracle and the definition in include/
ec_method.h, never from the library.  A set of bricks is mutually consistent
when the oracle's encode of the oracle's decode of its k lowest chunks
reproduces every chunk of the set.  loc[t] is 0 when avail is consistent,
1 << i when avail without brick i is (at most one i can qualify: asserted),
MANY otherwise.  That is evaluated for the stripes a case corrupts; every
other stripe is 0 because the clean fragments are checked once, whole, against
one prediction.  Beside the oracle's value the MDS rule is asserted where it
applies: one damaged chunk in brick i gives exactly 1 << i.
"""
import numpy as np

CHUNK = 512
GUARD = 8                       # words after loc[nstripes) that must not change
SENTINEL = 0xFFFFFFFF
MANY = 0x80000000

# (k, n, avail_mask).  0xF6F: 10 of 12 bricks with bricks 4 and 7 missing, so
# the basis is non-contiguous; 0xBFFFD: 18 of 20 with bricks 1 and 18 missing.
GEOMS = [
    (4, 6, 0x3F),
    (8, 12, 0xFFF),
    (8, 12, 0xF6F),
    (16, 20, 0xFFFFF),
    (16, 20, 0xBFFFD),
]
GEOM_LARGEST = (16, 31, 0x7FFFFFFF)     # 31 inputs, r = 15 (on the GPU)
SIZES = [1, 3, 4, 5, 67]


def geom_id(g):
    return "%d+%d-%x" % (g[0], g[1] - g[0], g[2])


def bits(mask):
    return [i for i in range(64) if (mask >> i) & 1]


_frag_cache = {}


def fragments(O, k, n, nst):
    """The n oracle-encoded fragments of nst stripes of random data (shared,
    read-only)."""
    key = (k, n, nst)
    if key not in _frag_cache:
        data = np.random.default_rng(2000 * k + 10 * n + nst).integers(
            0, 256, size=CHUNK * k * nst, dtype=np.uint8)
        frags = O.encode(k, n, data, nthreads=8 if nst > 4096 else 1)
        for f in frags:
            f.setflags(write=False)
        _frag_cache[key] = frags
    return _frag_cache[key]


def consistent(O, k, n, bricks, chunk):
    """Do the chunks chunk[b] (b in bricks, >= k of them) lie on one codeword?"""
    basis = bricks[:k]
    data = O.decode(k, [b + 1 for b in basis], [np.ascontiguousarray(chunk[b]) for b in basis])
    enc = O.encode(k, n, data)
    return all(np.array_equal(enc[b], chunk[b]) for b in bricks)


def expected_loc(O, k, n, avail, frags, t):
    """loc[t] by the definition, from the stored fragments `frags` (by brick)."""
    chunk = {b: frags[b][t * CHUNK:(t + 1) * CHUNK] for b in avail}
    if consistent(O, k, n, avail, chunk):
        return 0
    hits = [i for i in avail if consistent(O, k, n, [b for b in avail if b != i], chunk)]
    assert len(hits) <= 1, hits
    return (1 << hits[0]) if hits else MANY


def assert_clean(O, k, n, avail, frags, nst):
    """Every stripe of the clean fragments is consistent: one whole-fragment
    prediction from the k lowest bricks of avail."""
    basis = avail[:k]
    enc = O.encode(k, n, O.decode(k, [b + 1 for b in basis], [frags[b] for b in basis]))
    for b in avail:
        assert np.array_equal(enc[b], frags[b])


def flipped(buf, stripe, byte, bit):
    c = buf.copy()
    c[stripe * CHUNK + byte] ^= np.uint8(1 << bit)
    return c


def plane_flips(nst):
    """Eight single-bit flips, one per plane (plane b = bytes [64b, 64b + 64)
    of a chunk; flip j also flips bit j of its byte): the first byte of a
    chunk (plane 0) and the last (plane 7), stripe 0 and the last stripe
    alternating.  (stripe, byte in chunk, bit)."""
    out = []
    for j in range(8):
        byte = 0 if j == 0 else 511 if j == 7 else 64 * j + (13 * j + 5) % 64
        assert byte // 64 == j
        out.append((0 if j % 2 == 0 else nst - 1, byte, j))
    return out


def run_geometry(run, O, k, n, avail_mask, nst):
    """Every corruption case of one geometry and size.  run(frags) -> (loc[0..
    nst) as uint32, nbad or None) with frags a list by brick (None outside
    avail_mask; an entry that is not the clean fragment object is a corrupted
    copy); the runner checks its own sentinel and guard words."""
    clean = fragments(O, k, n, nst)
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    r = len(checks)
    assert r >= 2
    assert_clean(O, k, n, avail, clean, nst)
    base = [clean[b] if b in avail else None for b in range(n)]
    rng = np.random.default_rng(7 * k + n + nst)

    def locate(changes, what, rule=None):
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
            want[t] = expected_loc(O, k, n, avail, fr, t)
        if rule is not None:
            assert want.tolist() == rule.tolist(), (what, want, rule)
        loc, nbad = run(fr)
        assert np.array_equal(loc, want), (what, np.flatnonzero(loc != want)[:8],
                                           loc[:8], want[:8])
        if nbad is not None:
            assert nbad == int(np.count_nonzero(want)), (what, nbad)

    def one(t, v):
        rule = np.zeros(nst, np.uint32)
        rule[t] = v
        return rule

    locate({}, "clean", np.zeros(nst, np.uint32))

    # single-bit flips: first and last basis brick (position k - 1 is the last
    # byte of the last coefficient word), c0 and the last check brick
    for b in (basis[0], basis[k - 1], checks[0], checks[r - 1]):
        for t, byte, bit in plane_flips(nst):
            locate({b: flipped(clean[b], t, byte, bit)}, ("flip", b, t, byte, bit),
                   one(t, 1 << b))

    # a whole chunk replaced by random bytes
    for b in (basis[k // 2], checks[r // 2]):
        t = nst // 2
        buf = clean[b].copy()
        buf[t * CHUNK:(t + 1) * CHUNK] = rng.integers(0, 256, CHUNK, dtype=np.uint8)
        locate({b: buf}, ("random chunk", b, t), one(t, 1 << b))

    # two bricks damaged in one stripe at different bit positions of a plane:
    # two symbols, each with its own single error, so no one brick explains it
    t = nst - 1
    for b1, b2 in ((basis[1], checks[0]), (basis[0], basis[k - 1]), (checks[0], checks[r - 1])):
        locate({b1: flipped(clean[b1], t, 200, 3), b2: flipped(clean[b2], t, 201, 3)},
               ("two bricks, two symbols", b1, b2), one(t, MANY))
        locate({b1: flipped(clean[b1], t, 70, 1), b2: flipped(clean[b2], t, 70, 6)},
               ("two bricks, two bits of a byte", b1, b2), one(t, MANY))

    # two bricks damaged at the same symbol: the oracle decides (with r = 2
    # it may be a third brick's bit); with r >= 3 the distance makes it MANY
    for b1, b2 in ((basis[1], checks[0]), (basis[0], basis[k - 1]), (checks[0], checks[r - 1])):
        locate({b1: flipped(clean[b1], 0, 300, 2), b2: flipped(clean[b2], 0, 300, 2)},
               ("two bricks, one symbol", b1, b2), one(0, MANY) if r >= 3 else None)
        locate({b1: flipped(clean[b1], 0, 300, 2), b2: flipped(clean[b2], 0, 300 + 64, 2)},
               ("two bricks, one symbol, two planes", b1, b2), one(0, MANY) if r >= 3 else None)

    # one 4-stripe tile: clean, bad basis brick, bad check brick, MANY
    if nst >= 4:
        bb, cb = basis[k - 2], checks[1]
        ch = {bb: flipped(clean[bb], 1, 77, 5), cb: flipped(clean[cb], 2, 433, 0)}
        ch[bb] = flipped(ch[bb], 3, 10, 4)
        ch[cb] = flipped(ch[cb], 3, 11, 4)
        rule = np.zeros(nst, np.uint32)
        rule[1], rule[2], rule[3] = 1 << bb, 1 << cb, MANY
        locate(ch, "mixed tile", rule)

    # a dirty stripe in the ragged last tile while the first tile is clean
    if nst >= 5:
        t = nst - 1
        for b in (basis[2], checks[0]):
            locate({b: flipped(clean[b], t, 129, 7)}, ("last tile", b), one(t, 1 << b))
