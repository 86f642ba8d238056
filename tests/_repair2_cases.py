"""Shared cases of tests/test_repair2.py (host buffers, CPU engine) and
tests/test_gpu_repair2.py (device buffers, ec_repair2_n): geometries,
avail_masks, corruptions, loc[] arrays and the expected fragments of
ec_method_repair2[_device].

Every expected byte comes from the oracle: the clean fragments, and for a
hand-made loc[] the oracle's encode of the oracle's decode of the chunks of
B_ij (the k lowest bricks of avail other than the named ones) as they are
stored, rows i and j; for a single bit that is _repair_cases.predicted.  Every
case compares every fragment of avail_mask over its whole length plus one
guard chunk behind it, and loc[] itself, which the call only reads.
"""
import numpy as np

from _locate_cases import CHUNK, MANY, bits, flipped, fragments, plane_flips
from _locate2_cases import WAYS, damaged, pair_kinds
from _repair_cases import check_frags, geom_id, predicted, with_guard  # noqa: F401

# (k, n, avail_mask) with a = k + 2: too few for locate2, enough for repair2,
# so loc[] is hand-made.  0xF6F: bricks 4 and 7 missing (non-contiguous basis).
GEOMS_HAND = [
    (4, 6, 0x3F),
    (8, 12, 0xF6F),
]
# a >= k + 4: the geometries of _locate2_cases, locate2 -> repair2 -> locate2
GEOMS_ROUND = [
    (5, 9, 0x1FF),
    (4, 8, 0xFF),
    (8, 12, 0xFFF),
    (16, 20, 0xFFFFF),
    (16, 22, 0x3BFFFD),
]
GEOMS = GEOMS_HAND + GEOMS_ROUND
GEOM_LARGEST = (16, 31, 0x7FFFFFFF)     # every brick of 16+15 (on the GPU)
SIZE_LARGEST = 9
SIZES = [1, 3, 4, 5, 67]


def pair_bits(pair):
    v = 0
    for b in pair:
        v |= 1 << b
    return v


def predicted_set(O, k, n, avail, frags, named, t):
    """{brick: chunk t} of the bricks `named` as the oracle predicts them from
    the stored chunks of the k lowest bricks of avail outside `named`."""
    if len(named) == 1:
        return {named[0]: predicted(O, k, n, avail, frags, named[0], t)}
    bij = [b for b in avail if b not in named][:k]
    data = O.decode(k, [b + 1 for b in bij],
                    [np.ascontiguousarray(frags[b][t * CHUNK:(t + 1) * CHUNK]) for b in bij])
    enc = O.encode(k, n, data)
    return {b: enc[b] for b in named}


def kinds_of(basis, checks):
    """The seven kinds of pair of _locate2_cases, without repeats (with two
    check bricks c1 is the last one)."""
    return list(dict.fromkeys(tuple(sorted(p)) for p in pair_kinds(basis, checks)))


def run_geometry(ops, O, k, n, avail_mask, nst, counters=True):
    """Every case of one geometry and size.

    ops.scrub2(frags) -> (loc, out, loc2, counts): locate2, repair2 with that
    loc[], locate2 again (only called with a >= k + 4);
    ops.repair2(frags, loc) -> (out, loc_after, counts);
    ops.repair(frags, loc) -> the same of ec_method_repair.
    frags is a list by brick (None outside avail_mask) of nst * 512 bytes;
    out has the same shape with the guard chunk appended; counts is
    (nrepaired, nskipped) or None where the engine counts nothing."""
    clean = fragments(O, k, n, nst)
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    c0, r = checks[0], len(checks)
    assert r >= 2
    can_locate = r >= 4
    base = [clean[b] if b in avail else None for b in range(n)]
    rng = np.random.default_rng(13 * k + n + nst)
    kinds = kinds_of(basis, checks)

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
        out, after, counts = ops.repair2(fr, loc.copy())
        check_frags(what, avail, nst, out, want)
        assert np.array_equal(after, loc), (what, "loc[] written")
        counts_are(what, counts, rep, skip)

    # 1. the round trip: locate2 names the damaged chunks (with k + 2 bricks
    # the caller does), repair2 restores the clean fragments, a second locate2
    # is all zero
    def trip(what, changes, t, v):
        fr = stored(changes)
        if can_locate:
            loc, out, loc2, counts = ops.scrub2(fr)
            assert loc.tolist() == one(t, v).tolist(), (what, loc[:8])
            assert not loc2.any(), (what, "second locate2", loc2[:8])
            check_frags(what, avail, nst, out, base)
            counts_are(what, counts, 1, 0)
        else:
            handmade(what, fr, one(t, v), base, 1, 0)

    i = 0
    for pair in kinds:
        for how in WAYS:
            t = (nst - 1 - i) % nst
            i += 1
            trip(("pair", pair, how, t), damaged(clean, rng, t, list(pair), how), t,
                 pair_bits(pair))
    # first byte of the first stripe, last byte of the last stripe
    for pair in (kinds[0], kinds[-1]):
        for t, byte in ((0, 0), (nst - 1, CHUNK - 1)):
            trip(("pair edge", pair, t, byte),
                 {b: flipped(clean[b], t, byte, 1 + j) for j, b in enumerate(pair)}, t,
                 pair_bits(pair))
    for b in dict.fromkeys((basis[0], basis[k - 1], c0, checks[r - 1])):
        for t, byte, bit in plane_flips(nst):
            trip(("flip", b, t, byte, bit), {b: flipped(clean[b], t, byte, bit)}, t, 1 << b)
    for b in dict.fromkeys((basis[k // 2], checks[r // 2])):
        trip(("random chunk", b), damaged(clean, rng, nst // 2, [b], "random"), nst // 2, 1 << b)

    # three bricks damaged at three symbols: MANY, left as corrupted
    t = nst - 1
    trio = [basis[k - 2], basis[0], checks[1]]
    fr = stored(damaged(clean, rng, t, trio, "symbols"))
    if can_locate:
        loc, out, loc2, counts = ops.scrub2(fr)
        assert loc.tolist() == one(t, MANY).tolist(), loc[:8]
        assert np.array_equal(loc2, loc)
        check_frags(("many", trio), avail, nst, out, fr)
        counts_are("many", counts, 0, 1)
    else:
        handmade(("many", trio), fr, one(t, MANY), fr, 0, 1)

    # 2. the basis rule: naming a pair that is not the damaged brick writes
    # the prediction from the k lowest other bricks, damaged chunk included;
    # on a clean stripe the same bytes are written again
    t = nst // 2
    for pair in kinds:
        bad_b = [b for b in avail if b not in pair][0]      # the lowest brick of B_ij
        fr = stored({bad_b: flipped(clean[bad_b], t, 321, 6)})
        chunks = predicted_set(O, k, n, avail, fr, pair, t)
        want = list(fr)
        for b in pair:
            assert not np.array_equal(chunks[b], clean[b][t * CHUNK:(t + 1) * CHUNK])
            want[b] = clean[b].copy()
            want[b][t * CHUNK:(t + 1) * CHUNK] = chunks[b]
        loc = one(t, pair_bits(pair))
        rep = 1
        if nst > 1:
            loc[(t + 1) % nst] = pair_bits(pair)            # a clean stripe
            rep = 2
        handmade(("basis rule", pair), fr, loc, want, rep, 0)

    # 3. single bits: repair2 and repair give identical fragments
    ts = np.arange(nst)
    cyc = np.array(avail)[ts % len(avail)]
    fr = stored({basis[1]: flipped(clean[basis[1]], nst // 2, 99, 4),
                 c0: flipped(clean[c0], 0, 7, 0)})
    loc = (np.uint32(1) << cyc.astype(np.uint32)).astype(np.uint32)
    if nst > 2:
        loc[1] = 0
    out2, after2, counts2 = ops.repair2(fr, loc.copy())
    out1, after1, counts1 = ops.repair(fr, loc.copy())
    check_frags("repair2 against repair", avail, nst, out2,
                [None if o is None else o[:nst * CHUNK] for o in out1])
    assert np.array_equal(after2, loc) and np.array_equal(after1, loc)
    assert counts1 == counts2

    # 4. values that are not one or two bricks of avail_mask: nothing changes
    fr = stored({basis[0]: flipped(clean[basis[0]], 0, 17, 2)})
    ignored = [1 << basis[0] | 1 << basis[1] | 1 << c0, 0x7FFFFFFF, MANY, MANY | 1,
               MANY | 1 << basis[0] | 1 << c0]
    ignored += [1 << basis[0] | 1 << b for b in range(n) if b not in avail][:1]
    ignored += [1 << b | 1 << checks[r - 1] for b in range(n) if b not in avail][-1:]
    if n < 31:
        ignored += [1 << basis[0] | 1 << n, 1 << c0 | 1 << n]
    for v in ignored:
        handmade(("ignored", hex(v)), fr, np.full(nst, v, np.uint32), fr, 0, nst)
    handmade("all zero", fr, np.zeros(nst, np.uint32), fr, 0, 0)

    # 5. what the wave logic of the kernel can get wrong (the host engine runs
    # the same cases).  named[t] is the tuple of bricks loc[t] names, None
    # for 0 and an integer for a value that must be ignored; the named chunks
    # are damaged, so the clean fragments are the expectation, except that a
    # stripe with an ignored value keeps the damage of its first basis brick.
    def dense(what, named):
        bufs, loc, rep, skip = {}, np.zeros(nst, np.uint32), 0, 0
        for t, s in enumerate(named):
            if s is None:
                continue
            ign = not isinstance(s, tuple)
            for b in (basis[0],) if ign else s:
                if b not in bufs:
                    bufs[b] = clean[b].copy()
                bufs[b][t * CHUNK + (t * 37 + 5 + 64 * b) % CHUNK] ^= np.uint8(0x10)
            loc[t] = s if ign else pair_bits(s)
            rep, skip = rep + (not ign), skip + ign
        fr = stored(bufs)
        want = list(base)
        keep = [t for t, s in enumerate(named) if s is not None and not isinstance(s, tuple)]
        if keep:
            want[basis[0]] = clean[basis[0]].copy()
            for t in keep:
                want[basis[0]][t * CHUNK:(t + 1) * CHUNK] = fr[basis[0]][t * CHUNK:(t + 1) * CHUNK]
        handmade(what, fr, loc, want, rep, skip)

    dense("every stripe, pairs in turn", [kinds[t % len(kinds)] for t in range(nst)])
    dense("every stripe, one pair", [kinds[2]] * nst)       # groups of four, ragged end
    mix = []
    for t in range(nst):
        mix.append(((avail[t % len(avail)],), kinds[t % len(kinds)], MANY,
                    kinds[(t + 3) % len(kinds)], None, 1 << basis[0] | 1 << basis[1] | 1 << c0,
                    kinds[0])[t % 7])
    dense("singles, pairs and ignored values", mix)
    last = [None] * nst
    last[nst - 1] = kinds[1]
    dense("a pair in the last stripe", last)
    if nst > 64:
        edge = [None] * nst
        edge[63], edge[64] = kinds[0], kinds[-1]            # lane 63, lane 0 of the next wave
        dense("wave edge", edge)
