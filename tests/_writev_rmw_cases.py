"""The table that the tests of ec_method_writev_rmw[_device] share: the
geometries, masks and ranges of tests/_readv_decode_cases.py, the user bytes,
the old chunks and the expected fragments.

The expected bytes never come from the library.  A file D of NSTRIPES stripes
is encoded by the oracle once per geometry.  A case replaces [win * S + head,
+ size) of D with fresh xorshift bytes; its old chunks are the stored chunks
of the first and the last stripe of the window on the bricks of the mask, each
a 512-byte array of its own, and the expectation is the oracle's encode of the
ns stripes of the window.  In the second family the old chunks are arbitrary
bytes, no codeword: the expectation is then the oracle's decode of those k
chunks for that mask, merged as ec_writev_start merges, and encoded, so a
wrong inverse or brick order shows.  `drop` names the old arrays that are not
given ("head", "tail"): their stripes read as zeros.
"""
import collections
import functools

import numpy as np

import _readv_decode_cases as R

CHUNK = R.CHUNK
FILL = R.FILL
GEOMS = R.GEOMS
BUCKET_GEOMS = R.BUCKET_GEOMS
NSTRIPES = R.NSTRIPES
masks = R.masks
ranges = R.ranges
offset_ranges = R.offset_ranges
stripes = R.stripes
interior = R.interior
clips = R.clips
cuts = R.cuts
window = R.window

FAMILIES = ["file", "arbitrary"]
DROPS = [("head",), ("tail",), ("head", "tail")]

Case = collections.namedtuple("Case", "user old_head old_tail want merged")


@functools.lru_cache(maxsize=None)
def file(oracle, k, n):
    """(D, its n fragments), read-only."""
    data = oracle.fill_xorshift(CHUNK * k * NSTRIPES, seed=oracle.SEED + 977 * k + n)
    frags = oracle.encode(k, n, data)
    for a in [data] + frags:
        a.setflags(write=False)
    return data, tuple(frags)


def user_bytes(oracle, size, i):
    return oracle.fill_xorshift(size, seed=oracle.SEED + 7919 * (i + 1) + size)


def case(oracle, k, n, mask, head, size, win=0, i=0, family="file", drop=()):
    S = CHUNK * k
    ns = stripes(k, head, size)
    assert win + ns <= NSTRIPES
    data, frags = file(oracle, k, n)
    rows = oracle.mask_rows(mask)
    assert len(rows) == k and rows[-1] <= n
    user = user_bytes(oracle, size, i)
    if family == "file":
        last = win + ns - 1
        old_head = [frags[r - 1][win * CHUNK:(win + 1) * CHUNK].copy() for r in rows]
        old_tail = [frags[r - 1][last * CHUNK:(last + 1) * CHUNK].copy() for r in rows]
    else:
        old_head = [oracle.fill_xorshift(CHUNK, seed=oracle.SEED + 31 * i + p) for p in range(k)]
        old_tail = [oracle.fill_xorshift(CHUNK, seed=oracle.SEED + 37 * i + p + 64)
                    for p in range(k)]
    if "head" in drop:
        old_head = None
    if "tail" in drop:
        old_tail = None
    if family == "file" and not drop:
        merged = data[win * S:(win + ns) * S].copy()
        merged[head:head + size] = user
    else:
        o0 = None if old_head is None else oracle.decode(k, rows, old_head)
        o1 = None if old_tail is None else oracle.decode(k, rows, old_tail)
        merged = oracle.writev_merge(k, head, user, o0, o1)
    want = oracle.encode(k, n, merged)
    assert all(w.size == ns * CHUNK for w in want)
    return Case(user, old_head, old_tail, want, merged)


def decoded_olds(oracle, k, mask, c):
    """The S-byte stripes that ec_method_writev_encode wants for case c."""
    rows = oracle.mask_rows(mask)
    return (None if c.old_head is None else oracle.decode(k, rows, c.old_head),
            None if c.old_tail is None else oracle.decode(k, rows, c.old_tail))


def in_place(oracle, k, n, mask, head, size, win, i=0):
    """The in-place form: (user, the n fragments of the whole file as writable
    copies, the fragments of the file after the write)."""
    S = CHUNK * k
    data, frags = file(oracle, k, n)
    user = user_bytes(oracle, size, i)
    after = data.copy()
    after[win * S + head:win * S + head + size] = user
    return user, [f.copy() for f in frags], oracle.encode(k, n, after)
