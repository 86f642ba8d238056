"""Shared case table of tests/test_combine_sweep.py (host buffers, CPU engine)
and tests/test_gpu_combine_sweep.py (device buffers: every call that goes
through ecdk_combine / combine_any<true> in glusterfs_amd/csrc/ec_kernels.hip):
decode, heal, mixed decode, encode and row-masked encode for every k from 1 to
16, with the run-time k at every value of each K bucket (1...4, 5...8,
9...16), row counts on both sides of the wave count, and every launch branch
of launch_narrow_k / launch_combine_k: single pattern, tile-mixed and sorted,
each with its masks in the kernel arguments and in a device table.

Nothing here calls the library.  All fragments are random bytes, so a check
covers the whole linear map and not a round trip of codewords, and the
expected values are the oracle's: decode = oracle.decode of the k fragments,
heal of brick b = oracle.encode(k, n, that decode)[b], encode = oracle.encode.
A mixed call gives each group its mask's decode; an id past the mask list
means the last mask (include/ec_method.h).

k = 1: ec_method_init accepts one data brick, so it is swept too.  The
translator never has it (2 * redundancy < bricks), and the oracle's inverse,
which restates ec-method.c:38-72, writes past a 1 x 1 matrix, so
oracle.decode is never called with k = 1.  There the encode matrix is a column
of ones (oracle.encode_matrix) and every fragment is the data (oracle.encode,
checked in build()): the decode of a fragment is that fragment.

Single-pattern calls take 13 stripes: three 4-stripe tiles and a ragged one,
or one 8-stripe tile and a ragged one.  A mixed call has one partial last
group with a mask of its own (id 0: a sorted run of 1 to 3 stripes), a stripe
count that is no multiple of 8, every other mask in use and one id past the
list.
"""
import functools
import itertools
import math
from types import SimpleNamespace

import numpy as np

CHUNK = 512
FILL = 0xA5
NST = 13                        # stripes of a single-pattern call
ARG_WORDS = 512                 # kPatWords: the pattern words a launch carries
MAX_PAT_WORDS = 128             # kMaxPatWords: one pattern
MAX_MASKS = 256
TILE_ENCODER = {(2, 3), (4, 6), (8, 12), (16, 20)}    # ecdk_has_vander


def bits(mask):
    return [b for b in range(32) if (mask >> b) & 1]


def mask_of(bricks):
    return sum(1 << int(b) for b in bricks)


def rows_of(mask):
    return [b + 1 for b in bits(mask)]


def bucket(k):
    """The K the combine kernels are compiled for (launch_combine_k)."""
    return 4 if k <= 4 else 8 if k <= 8 else 16


def inside(k):
    """Strictly inside its bucket: the run-time k is below the compiled K."""
    return k != bucket(k)


def pwords(k, rows=None):
    """Words of one pattern: src[] and one row of ceil(k / 4) words per output
    (mixed decode: rows = k)."""
    return (k + 3) // 4 * (1 + (k if rows is None else rows))


def fit(k):
    """The masks of a mixed decode that travel in the kernel arguments."""
    return ARG_WORDS // pwords(k)


def sort_below(k):
    """Groups below a tile (4 stripes for k <= 8, else 8) are sorted first."""
    return 4 if k <= 8 else 8


# Every k with 31 bricks, the most the library takes for any k, and with a
# small volume: k + 2 bricks, 4+8 for a heal of 8 bricks from 4, 1+2.  None
# has a tile encoder, so every encode here is the combine with rows = n.
GEOMS = [(k, n) for k in range(1, 17) for n in ({1: 3, 4: 12}.get(k, k + 2), 31)]
OFFSET_GEOMS = [(3, 31), (6, 31), (11, 31)]     # and groups of 1 stripe
TABLE_K = (4, 6, 8, 11, 16)                     # fit(k) + 3 masks: a device table
EDGE_K = (3, 7, 15)                             # pwords divides 512: fit(k), fit(k) + 1


def geom_id(g):
    return "%d+%d" % (g[0], g[1] - g[0])


def _rng(k, n, salt):
    return np.random.default_rng((k * 64 + n) * 100 + salt)


def _draw_mask(rng, k, n, must=None):
    pool = [b for b in range(n) if b != must]
    pick = rng.choice(pool, size=k - (must is not None), replace=False).tolist()
    return mask_of(pick + ([must] if must is not None else []))


def draw_masks(k, n, count, salt):
    """`count` distinct masks of k bricks out of n (all of them when there are
    no more): the k lowest, the k highest, one with a brick >= 24 where n
    allows, the others drawn."""
    total = math.comb(n, k)
    if total <= count:
        return [mask_of(c) for c in itertools.combinations(range(n), k)]
    rng = _rng(k, n, salt)
    out = [mask_of(range(k)), mask_of(range(n - k, n))]
    if n > 24:
        out.append(_draw_mask(rng, k, n, must=int(rng.integers(24, n))))
    while len(out) < count:
        m = _draw_mask(rng, k, n)
        if m not in out:
            out.append(m)
    return out


def _heals(k, n):
    """(source mask, target mask): for the k lowest bricks and a drawn mask,
    one brick, two bricks, every brick outside the mask and a drawn set in
    between."""
    rng = _rng(k, n, 2)
    out = []
    for m in dict.fromkeys([mask_of(range(k)), draw_masks(k, n, 6, 1)[-1]]):
        outside = [b for b in range(n) if not (m >> b) & 1]
        sizes = [1, 2, len(outside)]
        if len(outside) > 3:
            sizes.append(int(rng.integers(3, len(outside))))
        for s in dict.fromkeys(sizes):
            t = outside if s == len(outside) else rng.choice(outside, size=s, replace=False)
            out.append((m, mask_of(t)))
    return out


def _row_masks(k, n):
    rng = _rng(k, n, 3)
    drawn = mask_of(rng.choice(n, size=int(rng.integers(2, n)), replace=False))
    return [1 << int(rng.integers(0, n)), drawn, (1 << n) - 1]


def _mixed(k, n, group, nmasks, salt):
    """One mixed decode: see the module's docstring."""
    rng = _rng(k, n, salt)
    masks = draw_masks(k, n, nmasks, salt)
    M = len(masks)
    assert M >= 3, (k, n)
    last = {1: 1, 2: 1, 4: 3}.get(group, 5)     # stripes of the partial last group
    full = max(M + 3, 6)
    while (full * group + last) % 8 == 0:
        full += 1
    ids = list(range(1, M)) + rng.integers(1, M, full - M).tolist() + \
        [int(rng.integers(M, 256))]
    ids = [ids[i] for i in rng.permutation(full)] + [0]
    return SimpleNamespace(group=group, masks=masks, ids=np.array(ids, np.uint8),
                           nst=full * group + last, last=last,
                           table=M * pwords(k) > ARG_WORDS, sorted=group < sort_below(k))


def _mixed_cases(k, n):
    groups = [2, 4] if k <= 8 else [4, 8]
    out = [_mixed(k, n, g, 5, 10 + g) for g in groups]
    if (k, n) in OFFSET_GEOMS:
        out.append(_mixed(k, n, 1, 5, 11))
    if n == 31 and k in TABLE_K:
        out += [_mixed(k, n, g, fit(k) + 3, 20 + g) for g in groups]
    if n == 31 and k in EDGE_K:
        out += [_mixed(k, n, g, fit(k) + past, 30 + g + past) for g in groups for past in (0, 1)]
    return out


@functools.lru_cache(maxsize=None)
def cases(geom):
    """The calls of one geometry; no data yet."""
    k, n = geom
    return SimpleNamespace(k=k, n=n, decode=draw_masks(k, n, 6, 1), heal=_heals(k, n),
                           row_masks=_row_masks(k, n), mixed=_mixed_cases(k, n))


def shape(k, mx):
    return ("sorted" if mx.sorted else "tile") + ("-table" if mx.table else "-args")


# what a later edit (or a change of seed) must not lose
assert {k for k, _ in GEOMS} == set(range(1, 17))
assert all(31 in {n for kk, n in GEOMS if kk == k} and
           len({n for kk, n in GEOMS if kk == k}) >= 2 for k in range(1, 17))
assert not set(GEOMS) & TILE_ENCODER
assert all(inside(k) and n >= 20 for k, n in OFFSET_GEOMS)
assert [bucket(k) for k, _ in OFFSET_GEOMS] == [4, 8, 16]
for _g in GEOMS:
    _c = cases(_g)
    _k, _n = _g
    assert len(_c.decode) == min(6, math.comb(_n, _k)) == len(set(_c.decode)), _g
    assert mask_of(range(_k)) in _c.decode and mask_of(range(_n - _k, _n)) in _c.decode, _g
    assert _n < 25 or any(bits(m)[-1] >= 24 and m != mask_of(range(_n - _k, _n))
                          for m in _c.decode), _g
    assert all(len(bits(m)) == _k and m >> _n == 0 for m in _c.decode), _g
    assert len({m for m, _ in _c.heal}) >= 2, _g
    for _m, _t in _c.heal:
        assert len(bits(_m)) == _k and _t and not _m & _t and (_m | _t) >> _n == 0, _g
    for _m in {m for m, _ in _c.heal}:
        assert {1, 2, _n - _k} <= {len(bits(t)) for m, t in _c.heal if m == _m}, _g
    assert [len(bits(r)) for r in _c.row_masks][::2] == [1, _n], _g
    assert pwords(_k, _n) <= MAX_PAT_WORDS, _g
    for _x in _c.mixed:
        assert _x.nst % 8 and len(_x.ids) == -(-_x.nst // _x.group), _g
        assert len(_x.masks) == len(set(_x.masks)) <= MAX_MASKS, _g
        assert set(range(len(_x.masks))) <= set(_x.ids.tolist()), _g
        assert sum(i >= len(_x.masks) for i in _x.ids.tolist()) == 1, _g
        assert _x.ids.tolist().count(0) == 1 and _x.ids[-1] == 0 and 1 <= _x.last <= 5, _g
        assert not _x.sorted or _x.last <= 3, _g
    assert {x.group for x in _c.mixed if not x.table} >= {sort_below(_k) // 2, sort_below(_k)}, _g
for _K in (4, 8, 16):
    _in = [g for g in GEOMS if bucket(g[0]) == _K and inside(g[0])]
    # a k strictly inside the bucket for each of the five launch shapes
    assert _in and all(cases(g).decode for g in _in), _K
    assert {shape(g[0], x) for g in _in for x in cases(g).mixed} == \
        {"tile-args", "tile-table", "sorted-args", "sorted-table"}, _K
    assert any(x.group == 1 for g in _in for x in cases(g).mixed), _K
    # ...and the bucket's top through a table too
    assert {shape(_K, x) for x in cases((_K, 31)).mixed} >= {"tile-table", "sorted-table"}, _K
    # rows below and above the wave count (K waves per block up to 2^17
    # stripes; rows go to waves round robin), rows > k, rows = 31
    _rows = {(g[0], len(bits(t))) for g in _in for _, t in cases(g).heal}
    assert any(r < _K for _, r in _rows) and any(r > _K for _, r in _rows), _K
    # a third pass over the waves (K = 16 has 16 waves and at most 22 rows)
    assert _K == 16 or any(r > 2 * _K for _, r in _rows), _K
    assert any(r > k for k, r in _rows), _K
    assert any(g[1] == 31 for g in _in), _K                     # encode: rows = n
    # the exact 512-word fit, and one mask past it
    _edge = [(len(x.masks) * pwords(g[0]), x.table, x.sorted)
             for g in _in for x in cases(g).mixed]
    for _s in (False, True):
        assert (ARG_WORDS, False, _s) in _edge, _K
        assert any(w > ARG_WORDS and w - ARG_WORDS <= MAX_PAT_WORDS and t and s == _s
                   for w, t, s in _edge), _K
assert (mask_of(range(4)), mask_of(range(4, 12))) in cases((4, 12)).heal   # 8 bricks from 4
assert any(len(bits(t)) == 15 for _, t in cases((16, 31)).heal)             # 15 from 16
assert pwords(16, 31) == MAX_PAT_WORDS                                      # a 16+15 encode
assert [len(x.masks) for x in cases((15, 31)).mixed if len(x.masks) > 5] == [8, 9, 8, 9]


def decode(O, k, mask, frags):
    """The data the k fragments of `mask` (frags is indexed by brick) decode
    to; for k = 1 see the module's docstring."""
    src = [np.ascontiguousarray(frags[b]) for b in bits(mask)]
    if k == 1:
        return src[0].copy()
    return O.decode(k, rows_of(mask), src)


def build(O, geom):
    """The buffers and expected values of cases(geom)."""
    k, n = geom
    C = cases(geom)
    rng = _rng(k, n, 0)
    frags = [rng.integers(0, 256, CHUNK * NST, dtype=np.uint8) for _ in range(n)]
    data = rng.integers(0, 256, CHUNK * k * NST, dtype=np.uint8)
    enc = O.encode(k, n, data)
    if k == 1:
        assert O.encode_matrix(1, n).tolist() == [[1]] * n
        assert all(np.array_equal(f, data) for f in enc)
    dec = {m: decode(O, k, m, frags) for m in C.decode}
    heal = {}
    for m, t in C.heal:
        full = O.encode(k, n, decode(O, k, m, frags))
        heal[m, t] = [full[b] for b in bits(t)]
    big = max(x.nst for x in C.mixed)
    mfr = [rng.integers(0, 256, CHUNK * big, dtype=np.uint8) for _ in range(n)]
    mixed = []
    for x in C.mixed:
        out = np.empty(CHUNK * k * x.nst, np.uint8)
        for g, i in enumerate(x.ids.tolist()):
            a0, a1 = g * x.group * CHUNK, min(x.nst, (g + 1) * x.group) * CHUNK
            m = x.masks[min(i, len(x.masks) - 1)]
            out[a0 * k:a1 * k] = decode(O, k, m, [f[a0:a1] for f in mfr])
        mixed.append(out)
    for a in frags + [data] + enc + list(dec.values()) + mfr + mixed + \
            [f for v in heal.values() for f in v]:
        a.setflags(write=False)
    return SimpleNamespace(k=k, n=n, C=C, frags=frags, data=data, enc=enc, dec=dec, heal=heal,
                           mfr=mfr, mixed=mixed)


@functools.lru_cache(maxsize=2)
def built(geom):
    """build() of a geometry of GEOMS: shared, read-only, the last two kept."""
    import oracle as O
    O.lib()
    return build(O, geom)
