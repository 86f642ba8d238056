"""Shared cases of tests/test_decode_checked2.py (host buffers, CPU engine) and
tests/test_gpu_decode_checked2.py (device buffers, ec_decode_checked2_n): the
geometries, sizes and corruption helpers of tests/_locate2_cases.py, and the
expected loc[] and out of ec_method_decode_checked2[_device].

Every expected byte comes from the oracle and the contract in include/
ec_method.h, never from the library.  loc[t] is expected_loc2 of the locate2
cases for the stripes a case corrupts and 0 elsewhere.  With B the k lowest
bricks of avail and B_S the k lowest outside S, stripe t of out is the
oracle's decode of the stored chunks of B, or of B_S when loc[t] names the one
or two bricks of S (MANY: B as stored).

Four cross-checks on every case: loc[] equals what ec_method_locate2[_device]
returns on the same buffers; wherever ec_method_decode_checked[_device] gives
0 or one bit its loc[t] and its stripe of out equal the new call's; the MDS
rule: wherever the chunks of at most two bricks of a stripe were damaged, out
is the user data the fragments were encoded from, byte for byte (the
expectation itself is asserted to obey it first); and the stripes with
loc == 0 equal ec_method_decode_batch with mask B.
"""
import numpy as np

from _locate_cases import (CHUNK, GUARD, MANY, SENTINEL, _frag_cache, assert_clean,  # noqa: F401
                           bits, flipped, fragments, geom_id, plane_flips)
from _locate2_cases import (GEOM_LARGEST, GEOMS, SIZES, WAYS, damaged,  # noqa: F401
                            expected_loc2, pair_kinds)
from _decode_checked_cases import FILL, _data_cache, mask_of, user_data  # noqa: F401


def named(w):
    """The bricks loc word w names: none for 0 and MANY."""
    return [] if w == MANY else bits(int(w))


def expected_out2(O, k, avail, frags, want_loc, nst):
    """(out by the contract, the decode of B as stored): the oracle's decode
    with mask B of the stored fragments, and for every stripe whose loc names a
    set S with a basis brick the oracle's decode of that stripe with B_S."""
    basis = avail[:k]
    stored = O.decode(k, [b + 1 for b in basis], [frags[b] for b in basis])
    out = stored.copy()
    for t in np.flatnonzero(want_loc).tolist():
        S = named(int(want_loc[t]))
        if not set(S) & set(basis):
            continue
        bs = [b for b in avail if b not in S][:k]
        out[t * k * CHUNK:(t + 1) * k * CHUNK] = O.decode(
            k, [b + 1 for b in bs],
            [np.ascontiguousarray(frags[b][t * CHUNK:(t + 1) * CHUNK]) for b in bs])
    return out, stored


def check_case(O, k, n, avail, clean, data, fr, res, nst, what, rule=None, expect_wrong=(),
               matters=()):
    """One call's results against the contract.  fr: the stored fragments by
    brick; res: the runner's dict (below); expect_wrong: stripes that, where
    they are MANY, must differ from the user data in out; matters: stripes
    where the decode of B as stored must differ from the user data (a named
    basis brick: the correction is what makes out right)."""
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
    want_out, stored = expected_out2(O, k, avail, fr, want_loc, nst)
    want_out, stored = want_out.reshape(nst, k * CHUNK), stored.reshape(nst, k * CHUNK)
    user = data.reshape(nst, k * CHUNK)
    # the expectation itself obeys the MDS rule
    two = ndam <= 2
    assert np.array_equal(want_out[two], user[two]), what
    hit = (ndam >= 1) & two
    assert (want_loc[hit] != 0).all() and (want_loc[hit] != MANY).all(), what
    for t in np.flatnonzero(hit).tolist():
        assert len(named(want_loc[t])) == ndam[t], (what, t)
    for t in matters:
        assert set(named(want_loc[t])) & set(basis), (what, t)
        assert not np.array_equal(stored[t], user[t]), (what, t, "the correction is a no-op")
    for t in expect_wrong:
        if want_loc[t] == MANY:
            assert np.array_equal(want_out[t], stored[t]), (what, t)
            assert not np.array_equal(want_out[t], user[t]), (what, t)

    loc, out = res["loc"], res["out"].reshape(nst, k * CHUNK)
    assert np.array_equal(loc, want_loc), (what, np.flatnonzero(loc != want_loc)[:8], loc[:8],
                                           want_loc[:8])
    bad = np.flatnonzero((out != want_out).any(axis=1))
    assert bad.size == 0, (what, "stripes of out that differ", bad[:8], want_loc[bad[:8]])
    # cross-check 1: the library's own locate2 on the same buffers
    assert np.array_equal(loc, res["loc2_ref"]), (what, "loc differs from ec_method_locate2")
    # cross-check 2: decode_checked where it gives 0 or one bit
    loc1, out1 = res["loc1_ref"], res["out1_ref"].reshape(nst, k * CHUNK)
    single = ((loc1 & (loc1 - np.uint32(1))) == 0) & (loc1 != MANY)
    assert np.array_equal(loc[single], loc1[single]), (what, "loc differs from decode_checked")
    assert np.array_equal(out[single], out1[single]), (what, "out differs from decode_checked")
    assert (loc1[~single] == MANY).all(), (what, loc1[:8])
    # cross-check 3: the MDS rule
    assert np.array_equal(out[two], user[two]), (what, "one or two damaged chunks reached out")
    # cross-check 4: a plain decode of B where the stripe is consistent
    dec = res["dec_ref"].reshape(nst, k * CHUNK)
    z = loc == 0
    assert np.array_equal(out[z], dec[z]), (what, "clean stripes differ from decode_batch")
    if res.get("nbad") is not None:
        assert res["nbad"] == int(np.count_nonzero(want_loc)), (what, res["nbad"])
        assert res["nmany"] == int(np.count_nonzero(want_loc == MANY)), (what, res["nmany"])


def merged(clean, *changes):
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


def run_geometry(run, O, k, n, avail_mask, nst):
    """Every corruption case of one geometry and size.  run(frags) -> dict
    with loc (uint32[nst]), out (uint8[nst * k * 512]), loc2_ref (the
    library's locate2 on the same buffers), loc1_ref and out1_ref (its
    decode_checked), dec_ref (decode_batch with mask B), and nbad / nmany or
    None; frags is a list by brick (None outside avail_mask).  The runner
    pre-fills out and loc, checks its guards and that no fragment was
    written."""
    clean = fragments(O, k, n, nst)
    data = user_data(O, k, n, nst)
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    r = len(checks)
    assert r >= 4
    assert_clean(O, k, n, avail, clean, nst)
    base = [clean[b] if b in avail else None for b in range(n)]
    rng = np.random.default_rng(11 * k + n + nst)

    def case(changes, what, rule=None, expect_wrong=(), matters=()):
        fr = list(base)
        for b, buf in changes.items():
            fr[b] = buf
        check_case(O, k, n, avail, clean, data, fr, run(fr), nst, what, rule, expect_wrong,
                   matters)

    def one(t, v):
        rule = np.zeros(nst, np.uint32)
        rule[t] = v
        return rule

    def pbits(*bricks):
        return mask_of(bricks)

    case({}, "clean", np.zeros(nst, np.uint32))

    # the single-brick classes of _decode_checked_cases.run_geometry
    for b in (basis[0], basis[k - 1], checks[0], checks[r - 1]):
        for t, byte, bit in plane_flips(nst):
            case({b: flipped(clean[b], t, byte, bit)}, ("flip", b, t, byte, bit), one(t, 1 << b),
                 matters=(t,) if b in basis else ())
    for b in (basis[k // 2], checks[r // 2]):
        t = nst // 2
        case(damaged(clean, rng, t, [b], "random"), ("random chunk", b, t), one(t, 1 << b),
             matters=(t,) if b in basis else ())

    # pairs of every kind, damaged in four ways, walking over the stripes.
    # Among them (basis[1], checks[0]): the check brick is row 0, so the error
    # comes from s_1 (ref = 1); and (basis[0], basis[k - 1]): the first and
    # the last LDS basis slot.
    i = 0
    for b1, b2 in pair_kinds(basis, checks) + [(basis[k - 1], checks[0])]:
        for how in WAYS:
            t = (nst - 1 - i) % nst
            i += 1
            case(damaged(clean, rng, t, [b1, b2], how), ("pair", b1, b2, how, t),
                 one(t, pbits(b1, b2)), matters=(t,) if b1 in basis else ())

    # three bricks at one symbol: the oracle decides (with a - k = 4 they can
    # imitate a pair); with a - k >= 5 the distance makes it MANY, and out is
    # then B as stored: wrong data, a basis brick is among them
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
        case(ch, "mixed tile", rule, expect_wrong=(3,),
             matters=(1, 2, 4) if nst >= 5 else (1, 2))

    # two pair-dirty stripes of one tile that name different pairs
    if nst >= 3:
        p0, p2 = (basis[0], basis[1]), (basis[k - 1], checks[1])
        rule = np.zeros(nst, np.uint32)
        rule[0], rule[2] = pbits(*p0), pbits(*p2)
        case(merged(clean, damaged(clean, rng, 0, p0, "planes"),
                    damaged(clean, rng, 2, p2, "symbols")),
             "two pairs in one tile", rule, matters=(0, 2))

    # a pair in the ragged last tile while the first tile is clean
    if nst >= 5:
        t = nst - 1
        for b1, b2 in ((basis[2], checks[0]), (basis[0], basis[3]), (checks[1], checks[3])):
            case(damaged(clean, rng, t, [b1, b2], "symbols"), ("last tile", b1, b2),
                 one(t, pbits(b1, b2)), matters=(t,) if b1 in basis else ())

    # every stripe dirty: the seven kinds of pair and the single bricks taking
    # turns
    if nst == 67:
        kinds = pair_kinds(basis, checks)
        chs, rule = [], np.zeros(nst, np.uint32)
        for t in range(nst):
            j = t % (len(kinds) + 1)
            S = kinds[j] if j < len(kinds) else (avail[t % len(avail)],)
            chs.append(damaged(clean, rng, t, list(S), WAYS[t % len(WAYS)]))
            rule[t] = pbits(*S)
        case(merged(clean, *chs), "every stripe dirty", rule)
