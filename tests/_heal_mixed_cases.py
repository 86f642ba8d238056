"""The table that the tests of ec_method_heal_mixed[_device] share: the
geometries, the (mask, target mask) patterns, the shapes, the pattern counts
and the expected fragments.

The expected bytes never come from the library.  For every group the oracle
decodes the k source chunks of the group's stripes and encodes them again, and
the rows of the group's targets are what the call must leave in the target
fragments; every other byte of every fragment must stay as it was.  In the
family "codeword" the fragments are the oracle's encode of a file with the
target chunks scribbled over (a call that does nothing fails); in the family
"arbitrary" every fragment holds arbitrary bytes that form no codeword, so a
wrong inverse, brick order or src[] shows.
"""
import collections
import functools
import itertools

import numpy as np

CHUNK = 512
FILL = 0xA5
SCRIBBLE = 0x3C
GEOMS = [(2, 3), (3, 5), (4, 6), (5, 7), (8, 12), (16, 20)]
BUCKET_GEOMS = [(4, 6), (8, 12), (16, 20)]     # one per K bucket of the kernel
NSTRIPES = [4, 5, 7, 8, 37, 67]
GROUPS = [4, 8, 16]
FAMILIES = ["codeword", "arbitrary"]
MAX_PATTERNS = 256

# The kernel arguments of ec_heal_mixed_n (HealMixedArgs, ec_kernels_impl.h):
# 32 brick pointers, nstripes, two table pointers and six 32-bit scalars in
# front of the pattern words, 2 KiB in all.  A pattern is the k source bytes
# in kw = ceil(k / 4) words, a word for m, the target bytes in ceil(mmax / 4)
# words and mmax rows of kw words.
ARG_BYTES = 2048
ARG_HEADER = 32 * 8 + 3 * 8 + 6 * 4
ARG_WORDS = (ARG_BYTES - ARG_HEADER) // 4


def geom_id(g):
    return "%d+%d" % (g[0], g[1] - g[0])


def bits(mask):
    return [i for i in range(64) if (mask >> i) & 1]


def to_mask(bricks):
    m = 0
    for b in bricks:
        m |= 1 << b
    return m


def masks(k, n):
    """The k lowest bricks, the k highest, and one with a gap at brick 1."""
    low = (1 << k) - 1
    return [low, low << (n - k), (low & ~2) | (1 << k)]


def patterns(k, n):
    """The (mask, target mask) pairs of the table.  For each mask, target sets
    of every size 0 .. n - k taken from the low end of the bricks outside the
    mask and from the high end: targets above the sources (low mask), below
    them (high mask) and between them (the gap mask's brick 1); pairs with one
    mask and different targets; pairs with one target and different masks
    where n - k >= 2 allows them; m from 0 to n - k inside one list."""
    out = []
    for mask in masks(k, n):
        rest = [b for b in range(n) if not (mask >> b) & 1]
        for m in range(n - k + 1):
            for pick in (rest[:m], rest[len(rest) - m:]):
                p = (mask, to_mask(pick))
                if p not in out:
                    out.append(p)
    return out


def all_pairs(k, n):
    """Every valid pair of the geometry, the table's first."""
    seen = set(patterns(k, n))
    yield from patterns(k, n)
    for src in itertools.combinations(range(n), k):
        mask = to_mask(src)
        rest = [b for b in range(n) if not (mask >> b) & 1]
        for m in range(len(rest), -1, -1):
            for pick in itertools.combinations(rest, m):
                p = (mask, to_mask(pick))
                if p not in seen:
                    seen.add(p)
                    yield p


def pattern_list(k, n, count, distinct=False):
    """`count` pairs: the table's, then further pairs of the geometry, then (a
    small geometry has fewer than 256) the same again unless distinct."""
    pairs = list(itertools.islice(all_pairs(k, n), count))
    assert not distinct or len(pairs) == count
    return [pairs[i % len(pairs)] for i in range(count)]


def mmax(pairs):
    return max(len(bits(t)) for _, t in pairs)


def pattern_words(k, m):
    kw = (k + 3) // 4
    return kw + 1 + (m + 3) // 4 + m * kw


def arg_fit(k, n):
    """The largest number of patterns of pattern_list(k, n, ...) that travel in
    the kernel arguments."""
    c = 0
    while c < MAX_PATTERNS:
        pairs = pattern_list(k, n, c + 1)
        if (c + 1) * pattern_words(k, mmax(pairs)) > ARG_WORDS:
            break
        c += 1
    return c


def counts(k, n):
    fit = arg_fit(k, n)
    return sorted({1, 2, fit, min(fit + 1, MAX_PATTERNS), MAX_PATTERNS})


def group_ids(ngroups, npat, salt=0):
    """A pattern id per group: the last pattern, the first, then a walk that
    reaches patterns all over the list and repeats some in adjacent groups."""
    ids = [(npat - 1 - (g // 2) * (1 + npat // 7) - salt) % npat for g in range(ngroups)]
    if ngroups > 1:
        ids[1] = 0
    return ids


def ngroups(nstripes, gs):
    return (nstripes + gs - 1) // gs


Case = collections.namedtuple("Case", "frags want")


@functools.lru_cache(maxsize=None)
def base(oracle, k, n, nstripes, family):
    if family == "codeword":
        data = oracle.fill_xorshift(CHUNK * k * nstripes, seed=oracle.SEED + 131 * k + n)
        frags = oracle.encode(k, n, data)
    else:
        frags = [oracle.fill_xorshift(CHUNK * nstripes, seed=oracle.SEED + 977 * k + 31 * n + i)
                 for i in range(n)]
    for f in frags:
        f.setflags(write=False)
    return tuple(frags)


def case(oracle, k, n, pairs, ids, nstripes, gs, family):
    """frags: what the call is given (writable copies); want: what it must
    leave.  ids[g] indexes pairs (already clamped)."""
    frags = [f.copy() for f in base(oracle, k, n, nstripes, family)]
    if family == "codeword":
        for g, u in enumerate(ids):
            for b in bits(pairs[u][1]):
                frags[b][g * gs * CHUNK:min((g + 1) * gs, nstripes) * CHUNK] = SCRIBBLE
    want = [f.copy() for f in frags]
    for g, u in enumerate(ids):
        mask, target = pairs[u]
        if not target:
            continue
        lo, hi = g * gs * CHUNK, min((g + 1) * gs, nstripes) * CHUNK
        rows = oracle.mask_rows(mask)
        data = oracle.decode(k, rows, [frags[r - 1][lo:hi] for r in rows])
        enc = oracle.encode(k, n, data)
        for b in bits(target):
            want[b][lo:hi] = enc[b]
    return Case(frags, want)


def table(k, n):
    """(nstripes, group_stripes, pairs, ids) of every shape, with the table's
    patterns."""
    pairs = patterns(k, n)
    for i, (ns, gs) in enumerate(itertools.product(NSTRIPES, GROUPS)):
        yield ns, gs, pairs, group_ids(ngroups(ns, gs), len(pairs), i)


def needed(pairs, ids, n):
    """The bricks that a call with these groups reads or writes."""
    m = 0
    for u in set(ids):
        if pairs[u][1]:
            m |= pairs[u][0] | pairs[u][1]
    return [bool((m >> b) & 1) for b in range(n)]
