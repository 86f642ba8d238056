"""The table that the tests of ec_method_heal_extents[_device] share: the
geometries, the patterns, the calls (lists of extents) and the expected bytes.

A call is laid out in one arena of bytes: every fragment of every extent lies
between guards of 0xA5, extents in a shuffled address order, and the arena
that the call must leave (`want`) is compared whole, so a byte written
anywhere but in a target chunk fails.  The expected bytes never come from the
library: for every pattern the oracle decodes the k source chunks of the
pattern's extents and encodes them again, and the target rows are what the
call must leave (stripes are independent, so extents with one pattern share one
oracle call).  In the family "codeword" the fragments are the oracle's encode
of a file with the target chunks scribbled over; in the family "arbitrary"
every fragment holds independent random bytes that form no codeword.

The module asserts its own clauses at import (the end of the file).
"""
import collections
import functools

import numpy as np

import _heal_mixed_cases as M
from _heal_mixed_cases import CHUNK, FILL, SCRIBBLE, bits, geom_id, to_mask  # noqa: F401

TILE = 4
RECORD = 272                                   # sizeof(ec_method_extent_t)
FAMILIES = ["codeword", "arbitrary"]
GEOMS = [(2, 3), (4, 6), (5, 7), (8, 12), (16, 20)]
WIDE_GEOMS = [(3, 31), (7, 31), (13, 31)]      # one k per K bucket of the kernel, n = 31
BUCKET_GEOMS = [(4, 6), (8, 12), (16, 20)]
RAGGED = [1, 2, 3, 4, 5, 7, 8, 9]
EXTENT_COUNTS = [1, 2, 63, 64, 65, 257, 4097]  # the sides of a 64-way and a binary lookup
MAX_PATTERNS = 256

# The kernel arguments of ec_heal_extents_n (HealExtentsArgs, ec_kernels_impl.h):
# the table and the pattern-table pointers and six 32-bit scalars in front of
# the pattern words, 2 KiB in all.  A pattern is packed as for ec_heal_mixed_n.
ARG_BYTES = 2048
ARG_HEADER = 2 * 8 + 6 * 4
ARG_WORDS = (ARG_BYTES - ARG_HEADER) // 4


def patterns(k, n):
    """The (mask, target mask) pairs of a geometry.  Below n = 31 those of the
    mixed heal (three masks, every target count from both ends).  On n = 31 a
    target set may not be everything outside the mask (15 at the most), so the
    pairs are picked: sources and targets at brick 24 and above, sources low
    and targets high, and an empty target."""
    if n < 31:
        return M.patterns(k, n)
    top = [b for b in range(n - 1, -1, -1) if b not in (25, 29)][:k]
    mid = [b for b in range(n - 1, -1, -1) if b not in (24, 30)][:k]
    low = list(range(k))
    return [(to_mask(top), to_mask([25, 29])), (to_mask(low), to_mask([24, 30])),
            (to_mask(top), 0), (to_mask(mid), to_mask([30])), (to_mask(top), to_mask([29])),
            (to_mask(mid), to_mask([24, 30, 0] if k > 3 else [24, 30])),
            (to_mask(low), to_mask([k, 27, 28]))]


def arg_fit(k, n):
    """The largest number of patterns of M.pattern_list(k, n, ...) that travel
    in the kernel arguments."""
    c = 0
    while c < MAX_PATTERNS:
        pairs = M.pattern_list(k, n, c + 1)
        if (c + 1) * M.pattern_words(k, M.mmax(pairs)) > ARG_WORDS:
            break
        c += 1
    return c


def pattern_counts(k, n):
    fit = arg_fit(k, n)
    return sorted({1, fit, min(fit + 1, MAX_PATTERNS), MAX_PATTERNS})


# extents: (nstripes, pattern id) in table order; order: the extents in address
# order; shared: (a, b) -- extent b reads the source buffers of extent a;
# full: every brick of an extent has a fragment, named or not
Call = collections.namedtuple("Call", "k n pairs extents order shared full what")


def tiles(nstripes):
    return (nstripes + TILE - 1) // TILE


def firsts(extents):
    out, s = [], 0
    for ns, _ in extents:
        out.append(s)
        s += tiles(ns)
    return out, s


def shuffled(count, seed):
    return [int(i) for i in np.random.RandomState(seed).permutation(count)]


def walk(pairs, count, salt=0):
    """A pattern id per extent in which neighbours differ in pattern and, where
    the pairs allow it, in the number of targets."""
    with_t = [u for u, p in enumerate(pairs) if p[1]]
    by_m = sorted(with_t, key=lambda u: (len(bits(pairs[u][1])), u))
    out = []
    for i in range(count):
        # alternate between the patterns with few and with many targets
        j = (i // 2 + salt) % len(by_m)
        out.append(by_m[j] if i % 2 == 0 else by_m[len(by_m) - 1 - j])
    return out


def ragged_call(k, n):
    """Extents of 1, 2, 3, 4, 5, 7, 8 and 9 stripes: every ragged last tile,
    extents shorter than a tile, tile boundaries between extents; an extent
    without targets and without fragments between two others; a last extent
    that reads the source buffers of the 3-stripe one with another target."""
    pairs = patterns(k, n)
    ids = walk(pairs, len(RAGGED), k)
    extents = list(zip(RAGGED, ids))
    empty = next(u for u, p in enumerate(pairs) if not p[1])
    extents.insert(3, (6, empty))
    # the sharer: the mask of extent 2, a target of its own where there is one
    mask, target = pairs[extents[2][1]]
    other = [u for u, p in enumerate(pairs) if p[0] == mask and p[1] and p[1] != target]
    extents.append((3, other[0] if other else extents[2][1]))
    shared = [(2, len(extents) - 1)] if other else []
    return Call(k, n, pairs, extents, shuffled(len(extents), 5 * k + n), shared, False, "ragged")


def full_call(k, n):
    """Every brick of every extent has a fragment: the bricks that a pattern
    does not name stay as they are."""
    pairs = patterns(k, n)
    ids = walk(pairs, 5, 1)
    return Call(k, n, pairs, list(zip([5, 1, 8, 2, 6], ids)), shuffled(5, 3), [], True, "full")


def count_call(k, n, count):
    """`count` extents of one or two stripes."""
    pairs = patterns(k, n)
    ids = walk(pairs, count, 2)
    extents = [(1 + (e * 7 // 3) % 2, ids[e]) for e in range(count)]
    return Call(k, n, pairs, extents, shuffled(count, count), [], False, "%d extents" % count)


def pattern_call(k, n, count):
    """`count` patterns, the extents on ids all over the list."""
    pairs = M.pattern_list(k, n, count) if count > 1 else [p for p in patterns(k, n) if p[1]][:1]
    ids = [(count - 1 - e * ((1 + count // 11) | 1)) % count for e in range(11)]
    extents = [(1 + (3 * e) % 6, ids[e]) for e in range(11)]
    assert ids[0] == count - 1 and sum(1 for u in ids if pairs[u][1]) >= 3
    return Call(k, n, pairs, extents, shuffled(11, 11 + count), [], False,
                "%d patterns" % count)


def table(k, n):
    """The calls of one geometry."""
    out = [ragged_call(k, n), full_call(k, n)]
    if (k, n) in BUCKET_GEOMS:
        out += [count_call(k, n, c) for c in EXTENT_COUNTS if c < 4097 or (k, n) == (4, 6)]
    if n < 31:
        out += [pattern_call(k, n, c) for c in pattern_counts(k, n)]
    return out


# arena, want: the bytes before and after; frag[e][b]: the offset of extent e's
# fragment of brick b in the arena, None for none
Built = collections.namedtuple("Built", "arena want frag")


def rotating(i):
    return i % 16


def one_off(i):
    return 1


def aligned(i):
    return 0


def needed(call, e):
    mask, target = call.pairs[call.extents[e][1]]
    return (mask | target) if target else 0


@functools.lru_cache(maxsize=None)
def pool(oracle, k, n, nstripes, family):
    """n fragments of `nstripes` stripes that the extents of a call cut their
    content from."""
    if family == "codeword":
        data = oracle.fill_xorshift(CHUNK * k * nstripes, seed=oracle.SEED + 137 * k + n)
        frags = oracle.encode(k, n, data)
    else:
        frags = [np.random.RandomState(1000 * k + 32 * n + i).randint(0, 256, CHUNK * nstripes)
                 .astype(np.uint8) for i in range(n)]
    for f in frags:
        f.setflags(write=False)
    return tuple(frags)


def build(oracle, call, family, guard, offset=aligned):
    k, n, pairs, extents = call.k, call.n, call.pairs, call.extents
    start, total = [], 0
    for ns, _ in extents:
        start.append(total)
        total += ns
    content = pool(oracle, k, n, total, family)
    frag = [[None] * n for _ in extents]
    alias = {b: a for a, b in call.shared}
    at, i = 0, 0
    for e in call.order:
        ns = extents[e][0]
        need = needed(call, e)
        for b in range(n):
            if not (call.full and need) and not (need >> b) & 1:
                continue
            if e in alias and (pairs[extents[e][1]][0] >> b) & 1:
                continue                       # filled in below
            at += guard + offset(i)
            frag[e][b] = at
            at += ns * CHUNK
            at += -at % 16
            i += 1
    for e, a in alias.items():
        assert extents[a][0] >= extents[e][0]
        written = pairs[extents[a][1]][1] | pairs[extents[e][1]][1]
        for b in bits(pairs[extents[e][1]][0]):
            assert frag[a][b] is not None and not (written >> b) & 1
            frag[e][b] = frag[a][b]
    arena = np.full(at + guard, FILL, np.uint8)
    for e, (ns, u) in enumerate(extents):
        for b in range(n):
            if frag[e][b] is not None and not (e in alias and (pairs[u][0] >> b) & 1):
                lo = frag[e][b]
                arena[lo:lo + ns * CHUNK] = content[b][start[e] * CHUNK:(start[e] + ns) * CHUNK]
    if family == "codeword":
        for e, (ns, u) in enumerate(extents):
            for b in bits(pairs[u][1]):
                arena[frag[e][b]:frag[e][b] + ns * CHUNK] = SCRIBBLE
    want = arena.copy()
    for u, (mask, target) in enumerate(pairs):
        mine = [e for e, x in enumerate(extents) if x[1] == u]
        if not target or not mine:
            continue
        rows = oracle.mask_rows(mask)
        src = [np.concatenate([arena[frag[e][r - 1]:frag[e][r - 1] + extents[e][0] * CHUNK]
                               for e in mine]) for r in rows]
        enc = oracle.encode(k, n, oracle.decode(k, rows, src))
        lo = 0
        for e in mine:
            size = extents[e][0] * CHUNK
            for b in bits(target):
                want[frag[e][b]:frag[e][b] + size] = enc[b][lo:lo + size]
            lo += size
    return Built(arena, want, frag)


def records(call, built, base):
    """(frags, nstripes, pattern) per extent with the arena at address `base`,
    as glusterfs_amd.ec_method.extent_table takes them."""
    return [([0 if o is None else base + o for o in built.frag[e]], ns, u)
            for e, (ns, u) in enumerate(call.extents)]


# ------------------------------------------------------------ the clauses
def _clauses():
    assert ARG_WORDS == 502
    for k, n in GEOMS + WIDE_GEOMS:
        pairs = patterns(k, n)
        assert all(len(bits(m)) == k and m >> n == 0 and t >> n == 0 and not m & t and
                   len(bits(t)) <= 15 for m, t in pairs), (k, n)
        assert any(not t for _, t in pairs)
        c = ragged_call(k, n)
        sizes = [ns for ns, _ in c.extents]
        assert all(s in sizes for s in RAGGED)
        assert {s % TILE for s in sizes} == {0, 1, 2, 3} and min(sizes) < TILE
        f, total = firsts(c.extents)
        assert total == sum(tiles(s) for s in sizes) and f[1] == 1     # a boundary after 1 stripe
        m = [len(bits(pairs[u][1])) for _, u in c.extents]
        assert any(c.extents[e][1] != c.extents[e + 1][1] for e in range(len(m) - 1))
        if n - k >= 2:
            assert any(m[e] and m[e + 1] and m[e] != m[e + 1] for e in range(len(m) - 1))
        assert m[3] == 0 and m[2] and m[4]                             # empty between two others
        assert c.order != sorted(c.order)
        if n - k >= 2:
            assert c.shared
        if n == 31:
            assert any(max(bits(mk)) >= 24 and t and max(bits(t)) >= 24 for mk, t in pairs)
            assert k > 3 or any(min(bits(mk) + bits(t)) >= 24 for mk, t in pairs if t)
    assert sorted(k for k, n in WIDE_GEOMS) == [3, 7, 13]              # K buckets 4, 8 and 16
    for k, n in GEOMS:
        fit = arg_fit(k, n)
        assert 2 < fit < MAX_PATTERNS and fit >= M.arg_fit(k, n)
        assert {1, fit, fit + 1, 256} == set(pattern_counts(k, n))
    assert any(count_call(4, 6, c).extents for c in EXTENT_COUNTS)
    big = count_call(4, 6, 4097)
    assert {ns for ns, _ in big.extents} == {1, 2}
    assert sum(ns for ns, _ in big.extents) * 6 * CHUNK + 4097 * RECORD < 20 << 20


_clauses()
