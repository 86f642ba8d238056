"""Shared cases of tests/test_verified.py (host buffers, CPU engine) and
tests/test_gpu_verified.py (device buffers, ec_decode_verified_n and
ec_heal_verified_n): geometries with a >= k + 1 bricks at hand, corruptions,
and the expected bad[] and outputs of ec_method_decode_verified[_device] and
ec_method_heal_verified[_device].

Every expected byte comes from the oracle and the rule in include/
ec_method.h, never from the library.  With B the k lowest bricks of
avail_mask and C the others, bad[] is _verify_cases.expected_flags of the
oracle's prediction from the stored chunks of B against the stored chunks of
C; out is the oracle's decode with rows(B) of the fragments as stored; out[j]
is row `target j` of the oracle's encode of that decode.  Nothing is
corrected.

Cross-checks on every case: bad[] equals ec_method_verify[_device] with B and
C on the same buffers; the output equals ec_method_decode_batch /
ec_method_decode_device (or ec_method_heal[_device]) with mask B over every
stripe; and the MDS rules: a stripe whose damage lies in check bricks alone
has exactly their bits and the original output, a stripe with a damaged basis
chunk has every bit of C and an output that differs from the original (in
every target, for the heal), so the flag is what protects the caller.
"""
import numpy as np

from _decode_checked_cases import FILL, mask_of  # noqa: F401
from _locate_cases import (CHUNK, GUARD, SENTINEL, _frag_cache, bits, flipped,  # noqa: F401
                           fragments, plane_flips)
from _verify_cases import expected_flags, predict

# (k, n, avail_mask, targets); targets is None for decode_verified
DECODE_GEOMS = [
    (2, 3, 0x7, None),          # k = 2, one row, four waves
    (4, 6, 0x1F, None),
    (4, 6, 0x3D, None),         # non-leading basis
    (4, 6, 0x3F, None),         # two rows
    (5, 7, 0x3F, None),         # low end of the K = 8 bucket
    (8, 12, 0x1FF, None),
    (8, 12, 0xFFF, None),
    (9, 11, 0x3FF, None),       # kw = 3
    (16, 20, 0x1FFFF, None),
    (16, 20, 0xFFFFE, None),
]
HEAL_GEOMS = [
    (4, 6, 0x1F, (5,)),
    (4, 6, 0x37, (3,)),         # target below the check brick
    (4, 6, 0x2F, (4,)),
    (8, 12, 0x2FF, (8, 10, 11)),
    (16, 20, 0x1FFFF, (17, 18, 19)),
]
# 16+15 on the GPU: the 62 KiB tile, the most output rows, the largest heal tile
GEOM_ALL_31 = (16, 31, 0x7FFFFFFF, None)
GEOM_MOST_ROWS = (16, 31, 0x1FFFF, tuple(range(17, 31)))
GEOM_29 = (16, 31, 0x1FFFFFFF, (29, 30))
SIZES = [1, 3, 4, 5, 67]


def geom_id(g):
    return "%d+%d-%x%s" % (g[0], g[1] - g[0], g[2],
                           "" if g[3] is None else "-" + ".".join(str(b) for b in g[3]))


def split(k, avail_mask):
    """(basis bricks, check bricks, B as a mask, C as a mask)"""
    avail = bits(avail_mask)
    basis, checks = avail[:k], avail[k:]
    return basis, checks, mask_of(basis), mask_of(checks)


_clean_cache = {}


def clean_state(O, k, n, avail_mask, nst):
    """The clean fragments, the data they decode to from B and the prediction
    of all n fragments from B: computed once per geometry and size, read-only."""
    key = (k, n, avail_mask, nst)
    if key not in _clean_cache:
        clean = fragments(O, k, n, nst)
        basis, checks, bmask, cmask = split(k, avail_mask)
        data = O.decode(k, [b + 1 for b in basis], [clean[b] for b in basis])
        pred = O.encode(k, n, data)
        for b in range(n):
            assert np.array_equal(pred[b], clean[b])
        data.setflags(write=False)
        _clean_cache[key] = (clean, data)
    return _clean_cache[key]


def check_case(O, k, n, avail_mask, targets, clean, data, fr, res, nst, what):
    """One call's results against the rule.  fr: the stored fragments by brick
    (None outside avail_mask); res: the runner's dict (run_geometry)."""
    basis, checks, bmask, cmask = split(k, avail_mask)
    rows = [b + 1 for b in basis]
    nb = np.zeros(nst, np.int64)            # damaged basis chunks per stripe
    cbits = np.zeros(nst, np.uint32)        # the damaged check bricks' bits
    for b in basis + checks:
        if fr[b] is not clean[b]:
            d = (fr[b].reshape(nst, CHUNK) != clean[b].reshape(nst, CHUNK)).any(axis=1)
            if b in basis:
                nb += d
            else:
                cbits |= d.astype(np.uint32) << np.uint32(b)

    # the expectation: the oracle on the fragments as stored.  Stripes are
    # independent, so only those with a damaged basis chunk are decoded again.
    want_data = data.reshape(nst, k * CHUNK).copy()
    pred = [clean[b].copy() for b in range(n)]
    for t in np.flatnonzero(nb).tolist():
        sl = [np.ascontiguousarray(fr[b][t * CHUNK:(t + 1) * CHUNK]) for b in basis]
        d = O.decode(k, rows, sl)
        want_data[t] = d
        for b, chunk in enumerate(O.encode(k, n, d)):
            pred[b][t * CHUNK:(t + 1) * CHUNK] = chunk
    want_bad = expected_flags(pred, cmask, [fr[b] for b in checks], nst)
    if targets is None:
        want_out, orig, per = [want_data], [data.reshape(nst, k * CHUNK)], k * CHUNK
    else:
        want_out = [pred[j].reshape(nst, CHUNK) for j in targets]
        orig, per = [clean[j].reshape(nst, CHUNK) for j in targets], CHUNK

    # the expectation itself obeys the MDS rules
    rule = np.where(nb > 0, np.uint32(cmask), cbits).astype(np.uint32)
    assert np.array_equal(want_bad, rule), (what, want_bad, rule)
    for w, g in zip(want_out, orig):
        assert np.array_equal(w[nb == 0], g[nb == 0]), what
        assert (w[nb > 0] != g[nb > 0]).any(axis=1).all(), what

    bad = res["bad"]
    assert np.array_equal(bad, want_bad), (what, np.flatnonzero(bad != want_bad)[:8], bad[:8],
                                           want_bad[:8])
    assert np.array_equal(bad, res["bad_ref"]), (what, "bad differs from ec_method_verify")
    assert len(res["out"]) == len(want_out)
    for i, (w, g, o, h) in enumerate(zip(want_out, orig, res["out"], res["out_ref"])):
        o, h = o.reshape(nst, per), h.reshape(nst, per)
        diff = np.flatnonzero((o != w).any(axis=1))
        assert diff.size == 0, (what, "output %d: stripes that differ" % i, diff[:8])
        assert np.array_equal(o, h), (what, i, "differs from the plain call with mask B")
        assert np.array_equal(o[nb == 0], g[nb == 0]), (what, i, "a check brick reached out")
        assert (o[nb > 0] != g[nb > 0]).any(axis=1).all(), (what, i)
    if res.get("nbad") is not None:
        assert res["nbad"] == int(np.count_nonzero(want_bad)), (what, res["nbad"])


def column_flip(buf, stripe, plane, col, bit):
    """A flipped bit confined to dword column `col` (bytes 4 col .. 4 col + 3
    of a 64-byte plane): the lane that holds it is lane 16 s + col."""
    return flipped(buf, stripe, 64 * plane + 4 * col + (bit & 3), bit)


def run_geometry(run, O, k, n, avail_mask, targets, nst):
    """Every corruption case of one geometry and size.  run(frags) -> dict
    with bad (uint32[nst]), out (a list: the decoded data, or a uint8[nst *
    512] per target), bad_ref (the library's verify with B and C on the same
    buffers), out_ref (the library's decode or heal with mask B) and nbad or
    None; frags is a list by brick (None outside avail_mask).  The runner
    pre-fills its outputs and bad[], checks its guards, that no fragment was
    written and that the buffers of bricks outside avail_mask are untouched."""
    clean, data = clean_state(O, k, n, avail_mask, nst)
    basis, checks, bmask, cmask = split(k, avail_mask)
    r = len(checks)
    assert r >= 1
    if targets is not None:
        assert not set(targets) & set(basis + checks) and max(targets) < n
    base = [clean[b] if (avail_mask >> b) & 1 else None for b in range(n)]
    rng = np.random.default_rng(17 * k + n + nst)

    def case(changes, what):
        fr = list(base)
        for b, buf in changes.items():
            fr[b] = buf
        check_case(O, k, n, avail_mask, targets, clean, data, fr, run(fr), nst, what)

    case({}, "clean")

    # one flipped bit in each of the 8 planes: the first and the last basis
    # brick, and each check brick
    for b in [basis[0], basis[k - 1]] + checks:
        for t, byte, bit in plane_flips(nst):
            case({b: flipped(clean[b], t, byte, bit)}, ("flip", b, t, byte, bit))

    # stripe 3 of a tile, dword column 0 and dword column 15: the vote is per
    # 16 lanes and one lane writes the flag
    if nst >= 4:
        for b in (checks[r - 1], basis[k // 2]):
            for plane, col in ((2, 0), (5, 15)):
                case({b: column_flip(clean[b], 3, plane, col, plane)},
                     ("column", b, plane, col))

    # a whole chunk replaced by random bytes
    for b in (basis[k // 2], checks[r // 2]):
        t = nst // 2
        buf = clean[b].copy()
        buf[t * CHUNK:(t + 1) * CHUNK] = rng.integers(0, 256, CHUNK, dtype=np.uint8)
        case({b: buf}, ("random chunk", b, t))

    # two bricks damaged in one stripe, at different symbols
    t = nst - 1
    pairs = [(basis[1], checks[0]), (basis[0], basis[k - 1])]
    if r >= 2:
        pairs.append((checks[0], checks[r - 1]))
    for b1, b2 in pairs:
        case({b1: flipped(clean[b1], t, 200, 3), b2: flipped(clean[b2], t, 201, 3)},
             ("two bricks", b1, b2))

    # one 4-stripe tile: clean, check-dirty, basis-dirty, both
    if nst >= 4:
        bb, cb = basis[k - 2], checks[r - 1]
        ch = {bb: flipped(clean[bb], 2, 77, 5), cb: flipped(clean[cb], 1, 433, 0)}
        ch[bb] = flipped(ch[bb], 3, 10, 4)
        ch[cb] = flipped(ch[cb], 3, 11, 4)
        case(ch, "mixed tile")

    # a dirty stripe in the ragged last tile while the first tile is clean
    if nst >= 5:
        t = nst - 1
        for b in (basis[k - 1], checks[0]):
            case({b: flipped(clean[b], t, 129, 7)}, ("last tile", b))

    # every stripe dirty, the bricks taking turns
    if nst == 67:
        ch = {}
        avail = basis + checks
        for t in range(nst):
            b = avail[t % len(avail)]
            ch[b] = flipped(ch.get(b, clean[b]), t, (37 * t + 3) % CHUNK, t % 8)
        case(ch, "every stripe dirty")
