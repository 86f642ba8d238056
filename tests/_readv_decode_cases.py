"""The table that the tests of ec_method_readv_decode[_device] share: the
geometries, three masks for each, the ranges (head, size) and the expected
bytes.

The expected bytes never come from the library: a file of NSTRIPES stripes is
encoded by the oracle once per geometry and decoded by the oracle once per
mask, and a case is a slice of that decode.  A case reads a window of the
fragments that starts `win` chunks in (the chunk of the stripe that holds the
first user byte) and is exactly ns * 512 bytes long.
"""
import functools

import numpy as np

CHUNK = 512
FILL = 0xA5

# every K bucket of the edge kernel (4, 8, 16), with the run-time k below the
# bucket for 3 and 5
GEOMS = [(2, 3), (3, 5), (4, 6), (5, 7), (8, 12), (16, 20)]
# one geometry per bucket: the cases that run at every destination offset,
# and with fragments 1 byte off alignment
BUCKET_GEOMS = [(3, 5), (8, 12), (16, 20)]


def masks(k, n):
    """The k lowest bricks, the k highest, and the k + 1 lowest without brick
    1: a mask with a gap."""
    low = (1 << k) - 1
    return [low, low << (n - k), ((1 << (k + 1)) - 1) & ~2]


def ranges(k):
    S = CHUNK * k
    return [
        # aligned: the whole-stripe decode
        (0, S), (0, 3 * S),
        # inside one stripe, clipped at both ends
        (0, 1), (S - 1, 1), (1, S - 2), (3, 1), (2, 4), (4, 4), (63, 2), (64, 1), (65, 3),
        (511, 2), (512, 1), (513, 510),
        # and ends just before and on a plane and a chunk boundary inside the stripe
        (10, 53), (60, 4), (10, 501), (500, 12),
        # two stripes, no interior
        (S - 1, 2), (1, S - 1), (5, 2 * S - 5), (0, S + 1), (0, 2 * S - 3),
        # with an interior
        (7, 2 * S), (S - 1, S + 2), (100, 5 * S + 33), (S // 2, 7 * S), (333, 40 * S + 4095),
    ]


def offset_ranges(k):
    """The ranges that run at all 16 destination offsets."""
    return [(65, 3), (100, 5 * CHUNK * k + 33)]


def stripes(k, head, size):
    return -(-(head + size) // (CHUNK * k))


def interior(k, head, size):
    """(first, count) of the stripes that lie wholly inside the range."""
    S = CHUNK * k
    first = 1 if head else 0
    return first, max((head + size) // S - first, 0)


def clips(k, head, size):
    """The (lo, hi) of the one or two stripes that the range covers in part."""
    S = CHUNK * k
    end = head + size
    out = []
    if head or end < S:
        out.append((head, min(end, S)))
    if end // S >= 1 and end % S:
        out.append((0, end % S))
    return out


def cuts(k, head, size):
    """Two places at which the range is cut into three segments of odd
    lengths.  Where there is an interior, the first cut falls inside its
    first stripe, an odd number of bytes in."""
    S = CHUNK * k
    first, count = interior(k, head, size)
    c1 = first * S - head + S // 2 + 1 if count else size // 3
    c2 = c1 + (size - c1) // 2
    return c1, c2


# the longest window is that of (333, 40 S + 4095) with k = 2: 45 stripes
NSTRIPES = 48


@functools.lru_cache(maxsize=None)
def _fragments(oracle, k, n):
    data = oracle.fill_xorshift(CHUNK * k * NSTRIPES, seed=oracle.SEED + 131 * k + n)
    frags = oracle.encode(k, n, data)
    for f in frags:
        f.setflags(write=False)
    return tuple(frags)


@functools.lru_cache(maxsize=None)
def _decoded(oracle, k, n, mask):
    rows = oracle.mask_rows(mask)
    assert len(rows) == k and rows[-1] <= n
    d = oracle.decode(k, rows, [_fragments(oracle, k, n)[r - 1] for r in rows])
    d.setflags(write=False)
    return d


def case(oracle, k, n, mask, head, size, win=0):
    """(the k fragments of the mask, each exactly ns * 512 bytes and a copy of
    its own; the size bytes expected)."""
    ns = stripes(k, head, size)
    assert win + ns <= NSTRIPES
    frags = _fragments(oracle, k, n)
    ins = [frags[r - 1][win * CHUNK:(win + ns) * CHUNK].copy()
           for r in oracle.mask_rows(mask)]
    want = _decoded(oracle, k, n, mask)[win * CHUNK * k + head:win * CHUNK * k + head + size]
    assert want.size == size
    return ins, want


def window(k, head, size, i):
    """Where case i starts in the file: it rotates through the first stripes
    that leave the window inside the file."""
    return i % (NSTRIPES - stripes(k, head, size) + 1) % 3
