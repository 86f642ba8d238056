"""Shared cases of tests/test_scrub_report.py (host arrays) and
tests/test_gpu_scrub_report.py (device tensors): sizes, fills, dirty values
and caps of ec_method_scrub_report[_device], and what the call must give.

Expected values come from numpy (np.flatnonzero, np.count_nonzero, per-bit
sums) and the definition in include/ec_method.h, never from the library.
"""
import numpy as np

MANY = 0x80000000
NODES = 31
REPORT_BYTES = 272
REPORT_WORDS = REPORT_BYTES // 8        # nbad, nmany, listed, brick[31]
GUARD = 16                              # words behind every output that must not change
SENTINEL8 = 0xA5                        # every byte of an output before the call

# What the device kernels are built around: a block counts and
# ranks a tile of TILE stripes, and the one scan block takes SCAN tiles per
# round.  Both are powers of two, so the sizes 2^p - 1, 2^p, 2^p + 1 below sit
# on each side of them: TILE = 2^12, and SCAN tiles are 2^20 stripes, past the
# table (the large case of the GPU test is there for that).
TILE = 4096
SCAN = 256

SIZES = list(range(1, 131)) + [(1 << p) + d for p in range(7, 17) for d in (-1, 0, 1)]

FILLS = ("clean", "all dirty", "stripe 0", "last stripe", "tile edge", "1 in 64", "1 in 2")


def value_pool():
    """The dirty values: every single bit 0..30, pairs of bits, MANY alone,
    MANY with other bits, and all 32 bits.  The rare kinds are repeated so
    that small fills draw them too."""
    single = [1 << b for b in range(NODES)]
    pairs = [1 << b | 1 << (b * 7 + 3) % NODES for b in range(NODES) if (b * 7 + 3) % NODES != b]
    many_bits = [MANY | 1, MANY | 1 << 30, MANY | 0x6, MANY | 1 << 13 | 1 << 14,
                 MANY | 0x7FFFFFFF, MANY | 1 << 17, MANY | 0x10001, MANY | 1 << 29 | 1]
    pool = single + pairs + [MANY] * 8 + many_bits + [0xFFFFFFFF] * 4
    return np.array(pool, dtype=np.uint32)


POOL = value_pool()

_fill_cache = {}


def fill(nst, kind):
    """loc[0..nst) of one fill (shared, read-only; fixed seeds)."""
    key = (nst, kind)
    if key in _fill_cache:
        return _fill_cache[key]
    rng = np.random.default_rng(1000003 * FILLS.index(kind) + nst)
    loc = np.zeros(nst, np.uint32)
    if kind == "clean":
        dirty = np.zeros(0, np.int64)
    elif kind == "all dirty":
        dirty = np.arange(nst)
    elif kind == "stripe 0":
        dirty = np.array([0])
    elif kind == "last stripe":
        dirty = np.array([nst - 1])
    elif kind == "tile edge":
        # the last stripe of the first tile and the first of the second (of a
        # tile that is not whole: its last stripe; no second tile: none)
        dirty = np.array(sorted({min(TILE, nst) - 1} | ({TILE} if nst > TILE else set())))
    else:
        p = 1 / 64 if kind == "1 in 64" else 1 / 2
        dirty = np.flatnonzero(rng.random(nst) < p)
    loc[dirty] = rng.choice(POOL, size=len(dirty))
    assert np.count_nonzero(loc) == len(dirty)
    loc.setflags(write=False)
    _fill_cache[key] = loc
    return loc


def caps(loc):
    """The values of cap for one fill: 0, 1, nbad - 1, nbad, nbad + 7, and the
    cumulative dirty count at the end of the first tile that has any (the cut
    then falls on a tile boundary), that count - 1 and + 1."""
    nbad = int(np.count_nonzero(loc))
    per_tile = [int(np.count_nonzero(loc[t:t + TILE])) for t in range(0, len(loc), TILE)]
    edge = next((c for c in per_tile if c), 0)      # the tiles before it are empty
    return sorted({c for c in (0, 1, nbad - 1, nbad, nbad + 7, edge - 1, edge, edge + 1)
                   if c >= 0})


_summary_cache = {}


def summary(loc):
    """(indices of the non-zero words, nmany, the 31 brick counts) by numpy;
    remembered for the shared read-only fills, which live as long as the
    process."""
    key = None if loc.flags.writeable else id(loc)
    if key in _summary_cache:
        return _summary_cache[key]
    where = np.flatnonzero(loc).astype(np.uint64)
    nmany = np.count_nonzero(loc >> np.uint32(31))
    brick = [np.count_nonzero((loc >> np.uint32(i)) & np.uint32(1)) for i in range(NODES)]
    if key is not None:
        _summary_cache[key] = (where, nmany, brick)
    return where, nmany, brick


def expected(loc, cap):
    """(the 34 words of the report, idx[0..listed), val[0..listed)) by numpy."""
    where, nmany, brick = summary(loc)
    rep = np.array([len(where), nmany, min(len(where), cap)] + brick, dtype=np.uint64)
    idx = where[:cap]
    return rep, idx, loc[idx.astype(np.int64)]


class Outputs:
    """One byte arena that holds report, idx[cap] and val[cap], each followed
    by GUARD words, all filled with SENTINEL8: one fill before the call and one
    look (or one copy back from the device) after it.  Offsets in bytes."""

    def __init__(self, cap, extra=0):
        self.cap = cap
        self.report = 0
        self.idx = self.report + REPORT_BYTES + 8 * GUARD
        self.val = self.idx + 8 * cap + 8 * GUARD
        self.extra = self.val + 4 * cap + 4 * GUARD     # 8-byte aligned: cap + GUARD words
        self.extra += -self.extra % 8
        self.nbytes = self.extra + extra

    def check(self, got, loc, with_val=True, what=None):
        """got: the arena after the call, as a numpy uint8 array."""
        want_rep, want_idx, want_val = expected(loc, self.cap)
        listed = len(want_idx)
        rep = got[self.report:self.idx].view(np.uint64)
        assert np.array_equal(rep[:REPORT_WORDS], want_rep), (what, rep[:6], want_rep[:6])
        idx = got[self.idx:self.val].view(np.uint64)
        assert np.array_equal(idx[:listed], want_idx), (what, idx[:8], want_idx[:8])
        val = got[self.val:self.val + 4 * (self.cap + GUARD)].view(np.uint32)
        if with_val:
            assert np.array_equal(val[:listed], want_val), (what, val[:8], want_val[:8])
        else:
            assert (got[self.val:self.val + 4 * listed] == SENTINEL8).all(), (what, "val written")
        # the guards, and every entry at or past `listed`
        assert (got[self.report + REPORT_BYTES:self.idx] == SENTINEL8).all(), (what, "report guard")
        assert (got[self.idx + 8 * listed:self.val] == SENTINEL8).all(), (what, "idx past listed")
        assert (got[self.val + 4 * listed:self.extra] == SENTINEL8).all(), (what, "val past listed")

