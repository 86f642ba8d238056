"""Shared cases of tests/test_heal_checked.py (host buffers, CPU engine) and
tests/test_gpu_heal_checked.py (device buffers, ec_heal_checked_n): the sizes
and corruption helpers of tests/_locate_cases.py and tests/
_decode_checked_cases.py, geometries with holes in avail_mask for the
targets, and the expected loc[] and out[j] of ec_method_heal_checked[_device].

Every expected byte comes from the oracle and the contract in include/
ec_method.h, never from the library.  loc[t] is expected_loc of the locate
cases for the stripes a case corrupts and 0 elsewhere.  With B the k lowest
bricks of avail and B_i the k lowest other than i, chunk t of out[j] is row
`target j` of the oracle's encode of the oracle's decode of the stored chunks
of B, or of B_i when loc[t] names basis brick i (for a check brick B_i = B).

Four independent cross-checks on every case: loc[] equals what
ec_method_locate[_device] returns on the same buffers; the stripes with
loc == 0 equal ec_method_heal[_device] with mask B and the same target_mask;
the MDS rule: wherever the chunk of at most one brick of a stripe was damaged,
every target chunk is the clean fragment's; and for every stripe that names a
basis brick the plain heal with mask B differs from the clean chunk in every
target, so the correction matters and a call that merely forwards to
ec_method_heal fails.
"""
import numpy as np

from _decode_checked_cases import FILL, mask_of  # noqa: F401
from _locate_cases import (CHUNK, GUARD, MANY, SENTINEL, SIZES,  # noqa: F401
                           _frag_cache, assert_clean, bits, expected_loc, flipped, fragments,
                           plane_flips)

# (k, n, avail_mask, targets).  0xF6F: bricks 4 and 7 missing, healed both or
# 7 alone (brick 4 then belongs to neither set); 0xBFFFD: bricks 1 and 18;
# 0x77 of a 4+3 volume: the basis 0, 1, 2, 4 is non-contiguous around the
# target; 0xFF3: the targets lie below every check brick.
GEOMS = [
    (8, 12, 0xF6F, (4, 7)),
    (8, 12, 0xF6F, (7,)),
    (16, 20, 0xBFFFD, (1, 18)),
    (4, 7, 0x77, (3,)),
    (8, 12, 0xFF3, (2, 3)),
]
# 16+15 on the GPU: the most rows (18 bricks at hand, the 13 odd bricks below
# 26 healed) and the largest tile (29 staged inputs, bricks 5 and 30 healed)
_ODD13 = tuple(range(1, 26, 2))
GEOM_MOST_ROWS = (16, 31, 0x7FFFFFFF & ~mask_of(_ODD13), _ODD13)
GEOM_LARGEST = (16, 31, 0x7FFFFFFF & ~mask_of((5, 30)), (5, 30))


def geom_id(g):
    return "%d+%d-%x-%s" % (g[0], g[1] - g[0], g[2], ".".join(str(b) for b in g[3]))


def expected_out(O, k, n, avail, targets, frags, want_loc, nst):
    """out[j] by the contract: the oracle's encode of its decode with mask B
    of the stored fragments, and for every stripe whose loc names a basis
    brick i that stripe's encode of the decode with mask B_i."""
    basis = avail[:k]
    enc = O.encode(k, n, O.decode(k, [b + 1 for b in basis], [frags[b] for b in basis]))
    out = [enc[j].copy() for j in targets]
    for t in np.flatnonzero(want_loc).tolist():
        w = int(want_loc[t])
        if w == MANY or not (w & mask_of(basis)):
            continue
        i = w.bit_length() - 1
        bi = [b for b in avail if b != i][:k]
        enc = O.encode(k, n, O.decode(
            k, [b + 1 for b in bi],
            [np.ascontiguousarray(frags[b][t * CHUNK:(t + 1) * CHUNK]) for b in bi]))
        for o, j in zip(out, targets):
            o[t * CHUNK:(t + 1) * CHUNK] = enc[j]
    return out


def check_case(O, k, n, avail, targets, clean, fr, res, nst, what, rule=None, expect_wrong=()):
    """One call's results against the contract.  fr: the stored fragments by
    brick; res: the runner's dict (below); expect_wrong: stripes whose targets
    must differ from the clean fragments (MANY with a damaged basis chunk)."""
    basis = avail[:k]
    damaged = np.zeros(nst, np.int64)
    for b in avail:
        if fr[b] is not clean[b]:
            damaged += (fr[b].reshape(nst, CHUNK) != clean[b].reshape(nst, CHUNK)).any(axis=1)
    want_loc = np.zeros(nst, np.uint32)
    for t in np.flatnonzero(damaged).tolist():
        want_loc[t] = expected_loc(O, k, n, avail, fr, t)
    if rule is not None:
        assert want_loc.tolist() == rule.tolist(), (what, want_loc, rule)
    want = [w.reshape(nst, CHUNK)
            for w in expected_out(O, k, n, avail, targets, fr, want_loc, nst)]
    good = [clean[j].reshape(nst, CHUNK) for j in targets]
    one = damaged <= 1
    basis_dirty = np.array([w != MANY and (int(w) & mask_of(basis)) != 0 for w in want_loc])
    assert (want_loc[damaged == 1] != 0).all() and (want_loc[damaged == 1] != MANY).all(), what

    loc, loc_ref = res["loc"], res["loc_ref"]
    assert np.array_equal(loc, want_loc), (what, np.flatnonzero(loc != want_loc)[:8], loc[:8],
                                           want_loc[:8])
    # cross-check 1: the library's own locate on the same buffers
    assert np.array_equal(loc, loc_ref), (what, "loc differs from ec_method_locate")
    z = loc == 0
    for j, w, g, o, h in zip(targets, want, good, res["out"], res["heal_ref"]):
        o, h = o.reshape(nst, CHUNK), h.reshape(nst, CHUNK)
        # the expectation itself obeys the MDS rule
        assert np.array_equal(w[one], g[one]), (what, j)
        for t in expect_wrong:
            assert want_loc[t] == MANY and not np.array_equal(w[t], g[t]), (what, j, t)
        bad = np.flatnonzero((o != w).any(axis=1))
        assert bad.size == 0, (what, "chunks of target %d that differ" % j, bad[:8],
                               want_loc[bad[:8]])
        # cross-check 2: a plain heal from B where the stripe is consistent
        assert np.array_equal(o[z], h[z]), (what, j, "clean stripes differ from ec_method_heal")
        # cross-check 3: the MDS rule
        assert np.array_equal(o[one], g[one]), (what, j, "a single damaged chunk reached out")
        # cross-check 4: without the correction these chunks would be wrong
        same = np.flatnonzero(basis_dirty & ~(h != g).any(axis=1))
        assert same.size == 0, (what, j, "a plain heal of B is right here", same[:8])
    if res.get("nbad") is not None:
        assert res["nbad"] == int(np.count_nonzero(want_loc)), (what, res["nbad"])
        assert res["nmany"] == int(np.count_nonzero(want_loc == MANY)), (what, res["nmany"])


def run_geometry(run, O, k, n, avail_mask, targets, nst):
    """The corruption cases of _decode_checked_cases.run_geometry for one
    geometry and size.  run(frags) -> dict with loc (uint32[nst]), out (a
    uint8[nst * 512] per target), loc_ref (the library's locate on the same
    buffers), heal_ref (the library's heal with mask B, per target), and nbad /
    nmany or None; frags is a list by brick (None outside avail_mask).  The
    runner pre-fills out and loc, checks its guards, that no fragment was
    written and that the buffers of bricks outside target_mask are untouched."""
    clean = fragments(O, k, n, nst)
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    r = len(checks)
    assert r >= 2 and not set(targets) & set(avail) and max(targets) < n
    assert_clean(O, k, n, avail, clean, nst)
    base = [clean[b] if b in avail else None for b in range(n)]
    rng = np.random.default_rng(13 * k + n + nst)

    def case(changes, what, rule=None, expect_wrong=()):
        fr = list(base)
        for b, buf in changes.items():
            fr[b] = buf
        check_case(O, k, n, avail, targets, clean, fr, run(fr), nst, what, rule, expect_wrong)

    def one(t, v):
        rule = np.zeros(nst, np.uint32)
        rule[t] = v
        return rule

    case({}, "clean", np.zeros(nst, np.uint32))

    # single-bit flips in every plane: the first and the last basis brick (its
    # correction touches the last LDS basis slot), c0 and the last check brick
    for b in (basis[0], basis[k - 1], checks[0], checks[r - 1]):
        for t, byte, bit in plane_flips(nst):
            case({b: flipped(clean[b], t, byte, bit)}, ("flip", b, t, byte, bit), one(t, 1 << b))

    # a whole chunk replaced by random bytes
    for b in (basis[k // 2], checks[r // 2]):
        t = nst // 2
        buf = clean[b].copy()
        buf[t * CHUNK:(t + 1) * CHUNK] = rng.integers(0, 256, CHUNK, dtype=np.uint8)
        case({b: buf}, ("random chunk", b, t), one(t, 1 << b))

    # two bricks damaged at different symbols: MANY, and the targets are the
    # heal of B as stored -- wrong chunks when a basis brick is among them
    t = nst - 1
    for b1, b2 in ((basis[1], checks[0]), (basis[0], basis[k - 1]), (checks[0], checks[r - 1])):
        case({b1: flipped(clean[b1], t, 200, 3), b2: flipped(clean[b2], t, 201, 3)},
             ("two bricks, two symbols", b1, b2), one(t, MANY),
             expect_wrong=(t,) if b1 in basis else ())

    # one 4-stripe tile: clean, bad basis brick, bad check brick, MANY
    if nst >= 4:
        bb, cb = basis[k - 2], checks[1]
        ch = {bb: flipped(clean[bb], 1, 77, 5), cb: flipped(clean[cb], 2, 433, 0)}
        ch[bb] = flipped(ch[bb], 3, 10, 4)
        ch[cb] = flipped(ch[cb], 3, 11, 4)
        rule = np.zeros(nst, np.uint32)
        rule[1], rule[2], rule[3] = 1 << bb, 1 << cb, MANY
        case(ch, "mixed tile", rule, expect_wrong=(3,))

    # two basis-dirty stripes of one tile that name different bricks
    if nst >= 3:
        b1, b2 = basis[0], basis[k - 1]
        rule = np.zeros(nst, np.uint32)
        rule[0], rule[2] = 1 << b1, 1 << b2
        case({b1: flipped(clean[b1], 0, 321, 6), b2: flipped(clean[b2], 2, 5, 0)},
             "two basis bricks in one tile", rule)

    # a dirty stripe in the ragged last tile while the first tile is clean
    if nst >= 5:
        t = nst - 1
        for b in (basis[2], checks[0]):
            case({b: flipped(clean[b], t, 129, 7)}, ("last tile", b), one(t, 1 << b))

    # every stripe dirty, the bricks taking turns
    if nst == 67:
        ch, rule = {}, np.zeros(nst, np.uint32)
        for t in range(nst):
            b = avail[t % len(avail)]
            ch[b] = flipped(ch.get(b, clean[b]), t, (37 * t + 3) % CHUNK, t % 8)
            rule[t] = 1 << b
        case(ch, "every stripe dirty", rule)
