"""Shared cases of tests/test_repair.py (host buffers, CPU engine) and
tests/test_gpu_repair.py (device buffers, ec_repair_n): geometries,
avail_masks, corruptions, loc[] arrays and the expected fragments of
ec_method_repair[_device].

Every expected byte comes from the oracle: the clean fragments, and for a
hand-made loc[] the oracle's encode of the oracle's decode of the chunks of
B_i (the k lowest bricks of avail other than i) as they are stored, row i.
Every case compares every fragment of avail_mask over its whole length plus
one guard chunk behind it, and loc[] itself, which the call only reads.
"""
import numpy as np

from _locate_cases import CHUNK, MANY, bits, flipped, fragments, plane_flips

GUARD_BYTE = 0xC3               # fills the chunk after each fragment

# (k, n, avail_mask).  0x1F: a = k + 1, too few for locate, enough for repair;
# 0xF6F: bricks 4 and 7 missing (non-contiguous basis); 0xBFFFD: 1 and 18.
GEOMS = [
    (4, 6, 0x3F),
    (4, 6, 0x1F),
    (8, 12, 0xF6F),
    (16, 20, 0xBFFFD),
]
GEOM_LARGEST = (16, 31, 0x7FFFFFFF)     # every brick of 16+15 (on the GPU)
SIZES = [1, 3, 4, 5, 67]


def geom_id(g):
    return "%d+%d-%x" % (g[0], g[1] - g[0], g[2])


def basis_without(avail, k, i):
    """B_i: the k lowest bricks of avail other than i."""
    return [b for b in avail if b != i][:k]


def predicted(O, k, n, avail, frags, i, t):
    """Chunk t of brick i as the oracle predicts it from the stored chunks of
    B_i."""
    bi = basis_without(avail, k, i)
    data = O.decode(k, [b + 1 for b in bi],
                    [np.ascontiguousarray(frags[b][t * CHUNK:(t + 1) * CHUNK]) for b in bi])
    return O.encode(k, n, data)[i]


def with_guard(buf):
    return np.concatenate([buf, np.full(CHUNK, GUARD_BYTE, np.uint8)])


def check_frags(what, avail, nst, got, want):
    """got[b]: brick b's buffer after the call, guard chunk included."""
    for b in avail:
        g = got[b]
        assert g.size == (nst + 1) * CHUNK
        assert (g[nst * CHUNK:] == GUARD_BYTE).all(), (what, "guard chunk of brick", b)
        if not np.array_equal(g[:nst * CHUNK], want[b]):
            bad = np.flatnonzero(g[:nst * CHUNK] != want[b])
            raise AssertionError((what, "brick", b, "stripes",
                                  sorted(set((bad // CHUNK).tolist()))[:8], "bytes", bad[:8]))


def run_geometry(ops, O, k, n, avail_mask, nst, counters=True):
    """Every case of one geometry and size.

    ops.scrub(frags) -> (loc, out, loc2, counts): locate, repair with that
    loc[], locate again; ops.repair(frags, loc) -> (out, loc_after, counts).
    frags is a list by brick (None outside avail_mask) of nst * 512 bytes;
    out has the same shape with the guard chunk appended; counts is
    (nrepaired, nskipped) or None where the engine counts nothing."""
    clean = fragments(O, k, n, nst)
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    c0, r = checks[0], len(checks)
    can_locate = r >= 2
    base = [clean[b] if b in avail else None for b in range(n)]
    rng = np.random.default_rng(11 * k + n + nst)

    def stored(changes):
        fr = list(base)
        for b, buf in changes.items():
            fr[b] = buf
        return fr

    def counts_are(what, counts, rep, skip):
        if counters and counts is not None:
            assert counts == (rep, skip), (what, counts, (rep, skip))

    def one(t, v):
        loc = np.zeros(nst, np.uint32)
        loc[t] = v
        return loc

    def handmade(what, fr, loc, want, rep, skip):
        out, after, counts = ops.repair(fr, loc.copy())
        check_frags(what, avail, nst, out, want)
        assert np.array_equal(after, loc), (what, "loc[] written")
        counts_are(what, counts, rep, skip)

    # 1. one damaged chunk: locate names it (with k + 1 bricks the caller
    # does), repair restores the clean fragments, a second locate is all zero
    def single(what, b, buf, t):
        fr = stored({b: buf})
        if can_locate:
            loc, out, loc2, counts = ops.scrub(fr)
            assert loc.tolist() == one(t, 1 << b).tolist(), (what, loc[:8])
            assert not loc2.any(), (what, "second locate", loc2[:8])
            check_frags(what, avail, nst, out, base)
            counts_are(what, counts, 1, 0)
        else:
            handmade(what, fr, one(t, 1 << b), base, 1, 0)

    for b in dict.fromkeys((basis[0], basis[k - 1], c0, checks[r - 1])):
        for t, byte, bit in plane_flips(nst):
            single(("flip", b, t, byte, bit), b, flipped(clean[b], t, byte, bit), t)
    for b in dict.fromkeys((basis[k // 2], checks[r // 2])):
        t = nst // 2
        buf = clean[b].copy()
        buf[t * CHUNK:(t + 1) * CHUNK] = rng.integers(0, 256, CHUNK, dtype=np.uint8)
        single(("random chunk", b, t), b, buf, t)

    # 2. two bricks damaged at different symbols: MANY, left as corrupted
    t = nst - 1
    for b1, b2 in ((basis[1], c0), (basis[0], basis[k - 1])):
        fr = stored({b1: flipped(clean[b1], t, 200, 3), b2: flipped(clean[b2], t, 201, 3)})
        if can_locate:
            loc, out, loc2, counts = ops.scrub(fr)
            assert loc.tolist() == one(t, MANY).tolist(), loc[:8]
            assert np.array_equal(loc2, loc)
            check_frags(("many", b1, b2), avail, nst, out, fr)
            counts_are("many", counts, 0, 1)
        else:
            handmade(("many", b1, b2), fr, one(t, MANY), fr, 0, 1)

    # 3. the basis rule: naming a brick that is not the damaged one writes the
    # prediction from the k lowest other bricks, damaged chunk included; on a
    # clean stripe the same bytes are written again
    bad_b, t = basis[1], nst // 2
    fr = stored({bad_b: flipped(clean[bad_b], t, 321, 6)})
    for i in dict.fromkeys((basis[0], basis[k - 1], c0, checks[r - 1])):
        assert bad_b in basis_without(avail, k, i)
        chunk = predicted(O, k, n, avail, fr, i, t)
        assert not np.array_equal(chunk, clean[i][t * CHUNK:(t + 1) * CHUNK])
        want = list(fr)
        want[i] = clean[i].copy()
        want[i][t * CHUNK:(t + 1) * CHUNK] = chunk
        loc = one(t, 1 << i)
        rep = 1
        if nst > 1:
            loc[(t + 1) % nst] = 1 << i         # a clean stripe
            rep = 2
        handmade(("basis rule", i), fr, loc, want, rep, 0)

    # 4. values that are not one brick of avail_mask: nothing changes
    fr = stored({basis[0]: flipped(clean[basis[0]], 0, 17, 2)})
    ignored = [0x3, MANY | 1, MANY | (1 << basis[0]), (1 << basis[0]) | (1 << c0)]
    ignored += [1 << b for b in range(n) if b not in avail][:1]
    if n < 31:
        ignored.append(1 << n)
    for v in ignored:
        handmade(("ignored", hex(v)), fr, np.full(nst, v, np.uint32), fr, 0, nst)

    # 5. what the wave logic of the kernel can get wrong (the host engine runs
    # the same cases).  Only named chunks are damaged, so the clean fragments
    # are the expectation.
    def damage(named):
        """named[t] = brick whose chunk t is damaged (-1: none)."""
        ch = {}
        for b in set(named.tolist()) - {-1}:
            ts = np.flatnonzero(named == b)
            buf = clean[b].copy()
            buf[ts * CHUNK + (ts * 37 + 5) % CHUNK] ^= np.uint8(0x10)
            ch[b] = buf
        return stored(ch)

    def named_loc(named):
        return np.where(named >= 0, np.uint32(1) << np.maximum(named, 0).astype(np.uint32),
                        np.uint32(0)).astype(np.uint32)

    ts = np.arange(nst)
    cyc = np.array(avail)[ts % len(avail)]                   # many bricks in one wave
    handmade("every stripe, bricks in turn", damage(cyc), named_loc(cyc), base, nst, 0)
    first = np.full(nst, avail[0])                           # groups of four, ragged end
    handmade("every stripe, first brick", damage(first), named_loc(first), base, nst, 0)
    if nst > 64:
        edge = np.full(nst, -1)
        edge[63], edge[64] = basis[k - 1], c0                # lane 63, lane 0 of the next wave
        handmade("wave edge", damage(edge), named_loc(edge), base, 2, 0)
