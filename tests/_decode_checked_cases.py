"""Shared cases of tests/test_decode_checked.py (host buffers, CPU engine) and
tests/test_gpu_decode_checked.py (device buffers, ec_decode_checked_n): the
geometries, sizes and corruption helpers of tests/_locate_cases.py, and the
expected loc[] and out of ec_method_decode_checked[_device].

Every expected byte comes from the oracle and the contract in include/
ec_method.h, never from the library.  loc[t] is expected_loc of the locate
cases for the stripes a case corrupts and 0 elsewhere.  With B the k lowest
bricks of avail and B_i the k lowest other than i, stripe t of out is the
oracle's decode of the stored chunks of B, or of B_i when loc[t] names brick
i (for a check brick B_i = B).

Three independent cross-checks on every case: loc[] equals what
ec_method_locate[_device] returns on the same buffers; the stripes with
loc == 0 equal ec_method_decode_batch with mask B; and the MDS rule: wherever
the chunk of at most one brick of a stripe was damaged, out is the user data
the fragments were encoded from, byte for byte.
"""
import numpy as np

from _locate_cases import (CHUNK, GEOM_LARGEST, GEOMS, GUARD, MANY, SENTINEL, SIZES,  # noqa: F401
                           _frag_cache, assert_clean, bits, consistent, expected_loc, flipped,
                           fragments, geom_id, plane_flips)

FILL = 0xA5                     # out is pre-filled with it; one guard chunk follows


def mask_of(bricks):
    return sum(1 << b for b in bricks)


_data_cache = {}


def user_data(O, k, n, nst):
    """The data fragments(O, k, n, nst) were encoded from (its seed), checked
    once against the oracle's decode of the clean basis fragments."""
    key = (k, n, nst)
    if key not in _data_cache:
        data = np.random.default_rng(2000 * k + 10 * n + nst).integers(
            0, 256, size=CHUNK * k * nst, dtype=np.uint8)
        fr = fragments(O, k, n, nst)
        assert np.array_equal(O.decode(k, list(range(1, k + 1)), [fr[b] for b in range(k)],
                                       nthreads=8 if nst > 4096 else 1), data)
        data.setflags(write=False)
        _data_cache[key] = data
    return _data_cache[key]


def expected_out(O, k, avail, frags, want_loc, nst):
    """out by the contract: the oracle's decode with mask B of the stored
    fragments, and for every stripe whose loc names a basis brick i the
    oracle's decode of that stripe with mask B_i."""
    basis = avail[:k]
    out = O.decode(k, [b + 1 for b in basis], [frags[b] for b in basis]).copy()
    for t in np.flatnonzero(want_loc).tolist():
        w = int(want_loc[t])
        if w == MANY or not (w & mask_of(basis)):
            continue
        i = w.bit_length() - 1
        bi = [b for b in avail if b != i][:k]
        out[t * k * CHUNK:(t + 1) * k * CHUNK] = O.decode(
            k, [b + 1 for b in bi],
            [np.ascontiguousarray(frags[b][t * CHUNK:(t + 1) * CHUNK]) for b in bi])
    return out


def check_case(O, k, n, avail, clean, data, fr, res, nst, what, rule=None, expect_wrong=()):
    """One call's results against the contract.  fr: the stored fragments by
    brick; res: the runner's dict (below); expect_wrong: stripes whose out
    must differ from the user data (MANY with a damaged basis chunk)."""
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
    want_out = expected_out(O, k, avail, fr, want_loc, nst).reshape(nst, k * CHUNK)
    user = data.reshape(nst, k * CHUNK)
    # the expectation itself obeys the MDS rule
    one = damaged <= 1
    assert np.array_equal(want_out[one], user[one]), what
    assert (want_loc[damaged == 1] != 0).all() and (want_loc[damaged == 1] != MANY).all(), what
    for t in expect_wrong:
        assert want_loc[t] == MANY and not np.array_equal(want_out[t], user[t]), (what, t)

    loc, out = res["loc"], res["out"].reshape(nst, k * CHUNK)
    assert np.array_equal(loc, want_loc), (what, np.flatnonzero(loc != want_loc)[:8], loc[:8],
                                           want_loc[:8])
    bad = np.flatnonzero((out != want_out).any(axis=1))
    assert bad.size == 0, (what, "stripes of out that differ", bad[:8], want_loc[bad[:8]])
    # cross-check 1: the library's own locate on the same buffers
    assert np.array_equal(loc, res["loc_ref"]), (what, "loc differs from ec_method_locate")
    # cross-check 2: a plain decode of B where the stripe is consistent
    dec = res["dec_ref"].reshape(nst, k * CHUNK)
    z = loc == 0
    assert np.array_equal(out[z], dec[z]), (what, "clean stripes differ from decode_batch")
    # cross-check 3: the MDS rule
    assert np.array_equal(out[one], user[one]), (what, "a single damaged chunk reached out")
    if res.get("nbad") is not None:
        assert res["nbad"] == int(np.count_nonzero(want_loc)), (what, res["nbad"])
        assert res["nmany"] == int(np.count_nonzero(want_loc == MANY)), (what, res["nmany"])


def run_geometry(run, O, k, n, avail_mask, nst):
    """Every corruption case of one geometry and size.  run(frags) -> dict
    with loc (uint32[nst]), out (uint8[nst * k * 512]), loc_ref (the library's
    locate on the same buffers), dec_ref (decode_batch with mask B), and nbad
    / nmany or None; frags is a list by brick (None outside avail_mask).  The
    runner pre-fills out and loc, checks its guards and that no fragment was
    written."""
    clean = fragments(O, k, n, nst)
    data = user_data(O, k, n, nst)
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    r = len(checks)
    assert r >= 2
    assert_clean(O, k, n, avail, clean, nst)
    base = [clean[b] if b in avail else None for b in range(n)]
    rng = np.random.default_rng(11 * k + n + nst)

    def case(changes, what, rule=None, expect_wrong=()):
        fr = list(base)
        for b, buf in changes.items():
            fr[b] = buf
        check_case(O, k, n, avail, clean, data, fr, run(fr), nst, what, rule, expect_wrong)

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

    # two bricks damaged at different symbols: MANY, and out is the decode of
    # B as stored -- wrong data when a basis brick is among them
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
