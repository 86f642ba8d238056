"""Shared cases of tests/test_heal_checked2.py (host buffers, CPU engine) and
tests/test_gpu_heal_checked2.py (device buffers, ec_heal_checked2_n): the
sizes and corruption helpers of tests/_locate_cases.py, tests/_locate2_cases.py
and tests/_decode_checked2_cases.py, geometries with holes in avail_mask for
the targets as in tests/_heal_checked_cases.py, and the expected loc[] and
out[j] of ec_method_heal_checked2[_device].

Every expected byte comes from the oracle and the contract in include/
ec_method.h, never from the library.  loc[t] is expected_loc2 of the locate2
cases for the stripes a case corrupts and 0 elsewhere.  With B the k lowest
bricks of avail and B_S the k lowest outside S, chunk t of out[j] is row
`target j` of the oracle's encode of the oracle's decode of the stored chunks
of B, or of B_S when loc[t] names the one or two bricks of S (MANY: B as
stored).

Five cross-checks on every case: loc[] equals what ec_method_locate2[_device]
returns on the same buffers; wherever ec_method_heal_checked[_device] gives 0
or one bit its loc[t] and its target chunks equal the new call's; the MDS
rule: wherever the chunks of at most two bricks of a stripe were damaged, every
target chunk is the clean fragment's (the expectation itself is asserted to
obey it first); the stripes with loc == 0 equal ec_method_heal[_device] with
mask B; and the correction matters: for a stripe that names a basis brick the
plain heal of B as stored -- the oracle's, and the library's -- differs from
the clean chunk.  With one named basis brick (alone or beside a check brick)
that is every target, because no entry of the heal matrix of an MDS code is
zero; with two named basis bricks it is every target when some symbol is
damaged in one of them only, and at least one target when both are damaged at
exactly the same symbols (the two terms can cancel in one target, not in all:
the inputs are checked for this, it is no tolerance).  So a call that forwards
to ec_method_heal_checked, or to ec_method_heal, fails the pair cases.
"""
import numpy as np

from _decode_checked_cases import FILL, mask_of  # noqa: F401
from _decode_checked2_cases import merged, named
from _heal_checked_cases import geom_id  # noqa: F401
from _locate_cases import (CHUNK, GUARD, MANY, SENTINEL, _frag_cache, assert_clean,  # noqa: F401
                           bits, flipped, fragments, plane_flips)
from _locate2_cases import SIZES, WAYS, damaged, expected_loc2, pair_kinds  # noqa: F401

# (k, n, avail_mask, targets); the targets are holes in avail_mask and a >= k +
# 4.  0x3F6F: bricks 4 and 7 missing, healed both or 7 alone; 0x3BFFFD: 16+6
# with bricks 1 and 18; 0x1F7 of a 4+5 volume: the basis 0, 1, 2, 4 is
# non-contiguous around the target (K bucket 4); 5+5: k below its bucket;
# 0x3FF3: the targets lie below every check brick; 0xFDF of a 6+6 volume: a - k
# = 5, so three damaged chunks are asserted MANY.
GEOMS = [
    (8, 14, 0x3F6F, (4, 7)),
    (8, 14, 0x3F6F, (7,)),
    (16, 22, 0x3BFFFD, (1, 18)),
    (4, 9, 0x1F7, (3,)),
    (5, 10, 0x3FB, (2,)),
    (8, 14, 0x3FF3, (2, 3)),
    (6, 12, 0xFDF, (5,)),
]
# 16+15 on the GPU: the most rows (20 bricks at hand, the other 11 healed: 44
# words of T) and the largest tile (29 staged inputs, bricks 5 and 30 healed)
_ODD11 = tuple(range(1, 22, 2))
GEOM_MOST_ROWS = (16, 31, 0x7FFFFFFF & ~mask_of(_ODD11), _ODD11)
GEOM_LARGEST = (16, 31, 0x7FFFFFFF & ~mask_of((5, 30)), (5, 30))


def damaged_set(clean, rng, t, bricks, how, basis):
    """damaged() of _locate2_cases; for two basis bricks at one symbol the
    second brick's symbol gets a second bit (the next plane), so that the two
    errors differ: equal errors cancel in a target whose two heal coefficients
    are equal, as 5+5 with 0x3FB has one for bricks 0 and 5 in target 2."""
    ch = damaged(clean, rng, t, bricks, how)
    if how == "symbol" and len(bricks) == 2 and all(b in basis for b in bricks):
        ch[bricks[1]] = flipped(ch[bricks[1]], t, 300 + 64, 2)
    return ch


def symbols(x):
    """The symbols of a chunk that are not zero, as 64 bytes of bits: symbol
    (byte, bit) has one bit in each of the chunk's 8 planes of 64 bytes."""
    return np.bitwise_or.reduce(x.reshape(8, 64), axis=0)


def heal_of(O, k, n, bricks, frags, targets, t=None):
    """The oracle's heal of the targets from the k bricks given, of stripe t
    only if given: the encode of the decode."""
    src = [np.ascontiguousarray(frags[b] if t is None else frags[b][t * CHUNK:(t + 1) * CHUNK])
           for b in bricks]
    enc = O.encode(k, n, O.decode(k, [b + 1 for b in bricks], src))
    return [enc[j] for j in targets]


def expected_out2(O, k, n, avail, targets, frags, want_loc, nst):
    """(out[j] by the contract, the heal of B as stored): the oracle's heal
    with mask B of the stored fragments, and for every stripe whose loc names
    a set S with a basis brick that stripe's heal with B_S."""
    basis = avail[:k]
    stored = heal_of(O, k, n, basis, frags, targets)
    out = [s.copy() for s in stored]
    for t in np.flatnonzero(want_loc).tolist():
        S = named(int(want_loc[t]))
        if not set(S) & set(basis):
            continue
        bs = [b for b in avail if b not in S][:k]
        for o, e in zip(out, heal_of(O, k, n, bs, frags, targets, t)):
            o[t * CHUNK:(t + 1) * CHUNK] = e
    return out, stored


def check_case(O, k, n, avail, targets, clean, fr, res, nst, what, rule=None, expect_wrong=()):
    """One call's results against the contract.  fr: the stored fragments by
    brick; res: the runner's dict (run_geometry); expect_wrong: stripes that,
    where they are MANY, must be the heal of B as stored and differ from the
    clean fragments in every target."""
    basis = avail[:k]
    ndam = np.zeros(nst, np.int64)
    for b in avail:
        if fr[b] is not clean[b]:
            ndam += (fr[b].reshape(nst, CHUNK) != clean[b].reshape(nst, CHUNK)).any(axis=1)
    want_loc = np.zeros(nst, np.uint32)
    for t in np.flatnonzero(ndam).tolist():
        want_loc[t] = expected_loc2(O, k, n, avail, fr, t)
    if rule is not None:
        assert want_loc.tolist() == rule.tolist(), (what, want_loc, rule)
    want, stored = expected_out2(O, k, n, avail, targets, fr, want_loc, nst)
    want = [w.reshape(nst, CHUNK) for w in want]
    stored = [s.reshape(nst, CHUNK) for s in stored]
    good = [clean[j].reshape(nst, CHUNK) for j in targets]
    two = ndam <= 2
    hit = (ndam >= 1) & two
    assert (want_loc[hit] != 0).all() and (want_loc[hit] != MANY).all(), what
    for t in np.flatnonzero(hit).tolist():
        assert len(named(want_loc[t])) == ndam[t], (what, t)

    # cross-check 5 on the inputs: which stripes the plain heal of B must get
    # wrong in every target, and which in at least one
    every, some = np.zeros(nst, bool), np.zeros(nst, bool)
    for t in np.flatnonzero(want_loc).tolist():
        nb = [b for b in named(int(want_loc[t])) if b in basis]
        if len(nb) == 2:
            ep, eq = (symbols(fr[b][t * CHUNK:(t + 1) * CHUNK] ^ clean[b][t * CHUNK:(t + 1) * CHUNK])
                      for b in nb)
            same = np.array_equal(ep, eq)
            every[t], some[t] = not same, same
        elif len(nb) == 1:
            every[t] = True
    wrong = np.stack([(s != g).any(axis=1) for s, g in zip(stored, good)])      # by the oracle
    assert wrong[:, every].all(), (what, "the oracle's plain heal of B is right in a target")
    assert wrong[:, some].any(axis=0).all(), (what, "the two errors cancel in every target")

    loc = res["loc"]
    assert np.array_equal(loc, want_loc), (what, np.flatnonzero(loc != want_loc)[:8], loc[:8],
                                           want_loc[:8])
    # cross-check 1: the library's own locate2 on the same buffers
    assert np.array_equal(loc, res["loc2_ref"]), (what, "loc differs from ec_method_locate2")
    # cross-check 2 (loc): heal_checked where it gives 0 or one bit
    loc1 = res["loc1_ref"]
    single = ((loc1 & (loc1 - np.uint32(1))) == 0) & (loc1 != MANY)
    assert np.array_equal(loc[single], loc1[single]), (what, "loc differs from heal_checked")
    assert (loc1[~single] == MANY).all(), (what, loc1[:8])
    z = loc == 0
    hwrong = []
    for j, w, s, g, o, o1, h in zip(targets, want, stored, good, res["out"], res["out1_ref"],
                                    res["heal_ref"]):
        o, o1, h = (x.reshape(nst, CHUNK) for x in (o, o1, h))
        # the expectation itself obeys the MDS rule
        assert np.array_equal(w[two], g[two]), (what, j)
        for t in expect_wrong:
            if want_loc[t] == MANY:
                assert np.array_equal(w[t], s[t]) and not np.array_equal(w[t], g[t]), (what, j, t)
        bad = np.flatnonzero((o != w).any(axis=1))
        assert bad.size == 0, (what, "chunks of target %d that differ" % j, bad[:8],
                               want_loc[bad[:8]])
        # cross-check 2 (bytes)
        assert np.array_equal(o[single], o1[single]), (what, j, "differs from heal_checked")
        # cross-check 3: the MDS rule
        assert np.array_equal(o[two], g[two]), (what, j, "one or two damaged chunks reached out")
        # cross-check 4: a plain heal from B where the stripe is consistent
        assert np.array_equal(o[z], h[z]), (what, j, "clean stripes differ from ec_method_heal")
        hwrong.append((h != g).any(axis=1))
    # cross-check 5: without the correction these chunks would be wrong
    hwrong = np.stack(hwrong)
    assert hwrong[:, every].all(), (what, "a plain heal of B is right in a target")
    assert hwrong[:, some].any(axis=0).all(), (what, "a plain heal of B is right in every target")
    if res.get("nbad") is not None:
        assert res["nbad"] == int(np.count_nonzero(want_loc)), (what, res["nbad"])
        assert res["nmany"] == int(np.count_nonzero(want_loc == MANY)), (what, res["nmany"])


def run_geometry(run, O, k, n, avail_mask, targets, nst):
    """Every corruption case of one geometry and size.  run(frags) -> dict
    with loc (uint32[nst]), out (a uint8[nst * 512] per target), loc2_ref (the
    library's locate2 on the same buffers), loc1_ref and out1_ref (its
    heal_checked), heal_ref (its heal with mask B, per target), and nbad /
    nmany or None; frags is a list by brick (None outside avail_mask).  The
    runner pre-fills out and loc, checks its guards, that no fragment was
    written and that the buffers of bricks outside avail_mask are untouched."""
    clean = fragments(O, k, n, nst)
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    r = len(checks)
    assert r >= 4 and not set(targets) & set(avail) and max(targets) < n
    assert_clean(O, k, n, avail, clean, nst)
    base = [clean[b] if b in avail else None for b in range(n)]
    rng = np.random.default_rng(17 * k + n + nst)

    def case(changes, what, rule=None, expect_wrong=()):
        fr = list(base)
        for b, buf in changes.items():
            fr[b] = buf
        check_case(O, k, n, avail, targets, clean, fr, run(fr), nst, what, rule, expect_wrong)

    def one(t, v):
        rule = np.zeros(nst, np.uint32)
        rule[t] = v
        return rule

    def pbits(*bricks):
        return mask_of(bricks)

    case({}, "clean", np.zeros(nst, np.uint32))

    # the single-brick classes of _heal_checked_cases.run_geometry
    for b in (basis[0], basis[k - 1], checks[0], checks[r - 1]):
        for t, byte, bit in plane_flips(nst):
            case({b: flipped(clean[b], t, byte, bit)}, ("flip", b, t, byte, bit), one(t, 1 << b))
    for b in (basis[k // 2], checks[r // 2]):
        t = nst // 2
        case(damaged(clean, rng, t, [b], "random"), ("random chunk", b, t), one(t, 1 << b))

    # pairs of every kind, damaged in four ways, walking over the stripes.
    # Among them (basis[1], checks[0]) and (basis[k - 1], checks[0]): the check
    # brick is row 0, so the error comes from s_1 (ref = 1); and (basis[0],
    # basis[k - 1]): the first and the last LDS basis slot.
    i = 0
    for b1, b2 in pair_kinds(basis, checks) + [(basis[k - 1], checks[0])]:
        for how in WAYS:
            t = (nst - 1 - i) % nst
            i += 1
            case(damaged_set(clean, rng, t, [b1, b2], how, basis), ("pair", b1, b2, how, t),
                 one(t, pbits(b1, b2)))

    # three bricks at one symbol: the oracle decides (with a - k = 4 they can
    # imitate a pair); with a - k >= 5 the distance makes it MANY, and the
    # targets are then the heal of B as stored: wrong, a basis brick is among
    # them
    for trio in ((basis[0], basis[1], checks[0]), (basis[2], checks[1], checks[r - 1]),
                 (basis[0], basis[k // 2], basis[k - 1])):
        case(damaged(clean, rng, 0, trio, "symbol"), ("three bricks, one symbol", trio),
             one(0, MANY) if r >= 5 else None, expect_wrong=(0,))

    # one 4-stripe tile: clean, a single basis brick, a pair of basis bricks
    # and three bricks damaged at three symbols (MANY: see _locate2_cases), with
    # a basis + check pair in the next tile
    if nst >= 4:
        bb, cb = basis[k - 2], checks[1]
        ch = merged(clean, {bb: flipped(clean[bb], 1, 77, 5)},
                    damaged(clean, rng, 2, [basis[0], basis[k - 1]], "random"),
                    damaged(clean, rng, 3, [bb, basis[0], cb], "symbols"))
        rule = np.zeros(nst, np.uint32)
        rule[1], rule[2], rule[3] = 1 << bb, pbits(basis[0], basis[k - 1]), MANY
        if nst >= 5:
            ch = merged(clean, ch, damaged(clean, rng, 4, [basis[1], checks[2]], "planes"))
            rule[4] = pbits(basis[1], checks[2])
        case(ch, "mixed tile", rule, expect_wrong=(3,))

    # two pair-dirty stripes of one tile that name different pairs
    if nst >= 3:
        p0, p2 = (basis[0], basis[1]), (basis[k - 1], checks[1])
        rule = np.zeros(nst, np.uint32)
        rule[0], rule[2] = pbits(*p0), pbits(*p2)
        case(merged(clean, damaged(clean, rng, 0, p0, "planes"),
                    damaged(clean, rng, 2, p2, "symbols")),
             "two pairs in one tile", rule)

    # a pair in the ragged last tile while the first tile is clean
    if nst >= 5:
        t = nst - 1
        for b1, b2 in ((basis[2], checks[0]), (basis[0], basis[3]), (checks[1], checks[3])):
            case(damaged(clean, rng, t, [b1, b2], "symbols"), ("last tile", b1, b2),
                 one(t, pbits(b1, b2)))

    # every stripe dirty: the seven kinds of pair and the single bricks taking
    # turns
    if nst == 67:
        kinds = pair_kinds(basis, checks)
        chs, rule = [], np.zeros(nst, np.uint32)
        for t in range(nst):
            j = t % (len(kinds) + 1)
            S = kinds[j] if j < len(kinds) else (avail[t % len(avail)],)
            chs.append(damaged_set(clean, rng, t, list(S), WAYS[t % len(WAYS)], basis))
            rule[t] = pbits(*S)
        case(merged(clean, *chs), "every stripe dirty", rule)
