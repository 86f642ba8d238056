"""Shared case table of tests/test_encode_sweep.py (host buffers, CPU engine)
and tests/test_gpu_encode_sweep.py (device buffers): the third kernel family
of glusterfs_amd/csrc/ec_kernels.hip, the compile-time encoders of 2+1, 4+2,
8+4 and 16+4 (ec_encode_tile_t, ec_encode_tile_rb, ec_encode_vander) and the
partial-stripe write (ec_rmw_gather, the same encoders with the edge stripes
gathered, ec_encode_vander_rmw, and for 5+2 and 10+3 the gather of the whole
padded buffer followed by the generic combine).

Nothing here calls the library.  The data is random bytes and the expected
fragments are the oracle's: oracle.encode(k, n, data) for a plain encode and
oracle.encode(k, n, oracle.writev_merge(k, head, user, old_head, old_tail))
for a write (absent old content means zeros, and a one-stripe write takes both
ends from whichever old stripe is given: ec-inode-write.c:1886-1895 as the
oracle restates it).

What the table holds, and the assertion at the end of the module that proves
each clause (a later edit or another seed must not lose one):

plain encodes (ENC_GEOMS)                                          [P1]...[P5]
  P1  every stripe count from 1 to 9, B - 1, B and B + 1 for the register
      encoder's block of B = 256 / (16 / W) stripes, and BIG = 259 (3 mod 4),
      all buffers aligned; so every residue mod 4 of the stripe count;
  P2  at 9, 6 and 7 stripes (a ragged tile of 1, 2 and 3 stripes) the input
      at every address modulo 16, so every byte shift 0...15;
  P3  each shift mod 4 != 0 together with each ragged-tile size 1, 2 and 3
      (stage_tile_shift: a lane whose next piece is past nstripes);
  P4  in those cases fragment i sits at (off + i) mod 16, so every fragment
      at an address of its own and, over the case list, at every offset;
  P5  one case per count with a shifted input and every output aligned.

partial writes (WRITE_GEOMS)                                       [W1]...[W10]
  W1  merged stripe counts 1, 2, 3, 4, 5, 6 and 9, so the tail stripe in
      every slot 0...3 of its tile, and alone in a ragged tile;
  W2  for each count every head of {0, 1, 15, 16, 17, S / 2, S - 1} and every
      end b2 mod S of {0, 1, 16, S - 1}, the pairs drawn by seed;
  W3  one stripe with the user range strictly inside;
  W4  one stripe with head + size == S;
  W5  head == 0 and b2 % S == 0: nothing merged;
  W6  b2 % S == 0 with old_tail given and more than one stripe (the tail
      pointer is one past old_tail and no byte of it is wanted);
  W7  a user range of 1 byte, and one of <= 15 bytes inside one 16-byte piece
      of ec_rmw_gather; a range across a piece boundary; heads on both sides
      of one (15, 16, 17);
  W8  two stripes with one user byte in each;
  W9  all four presence combinations of old_head / old_tail, for one-stripe
      and for multi-stripe writes;
  W10 at 6 merged stripes the interior address (user - head) mod 16 at every
      value 0...15.

Buffers.  Every output of a call is a slice of one allocation, pre-filled with
0xA5: per output a guard of GUARD = 2 KiB (one tile's row run: a tile encoder
writes a row's 4 chunks as one run), the payload at its offset, and a guard of
at least 2 KiB, so a tile's worth of stray writes stays inside memory the test
owns.  check_outputs() compares payloads and guards and says which differs.
Every input sits between FLANK = 64 random bytes and the whole input buffer is
compared with what was uploaded after the call.
"""
import functools
from types import SimpleNamespace

import numpy as np

CHUNK = 512
FILL = 0xA5
GUARD = 2048
FLANK = 64
TILE = 4
ENC_GEOMS = [(2, 3), (4, 6), (8, 12), (16, 20)]         # ecdk_has_vander
GENERIC_GEOMS = [(5, 7), (10, 13)]                      # writes: gather + combine
WRITE_GEOMS = ENC_GEOMS + GENERIC_GEOMS
BLOCK = {2: 64, 4: 32, 8: 16, 16: 16}                   # 256 / (16 / W) stripes
BIG = 259
ALIGN_NST = {9: 2, 6: 7, 7: 13}     # count: the shifted input of its aligned-output case
W_NST = (1, 2, 3, 4, 5, 6, 9)
SHIFT_NST = 6
PRESENCE = ((True, True), (True, False), (False, True), (False, False))


def geom_id(g):
    return "%d+%d" % (g[0], g[1] - g[0])


def heads(S):
    return (0, 1, 15, 16, 17, S // 2, S - 1)


def ends(S):
    return (0, 1, 16, S - 1)


def _rng(k, n, salt):
    return np.random.default_rng((k * 64 + n) * 100 + salt)


# --- the cases ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plain_cases(geom):
    """nst stripes, the input at address `off` mod 16, fragment i at outs[i]."""
    k, n = geom
    B = BLOCK[k]
    out = [SimpleNamespace(nst=nst, off=0, outs=(0,) * n, kind="count")
           for nst in sorted(set(range(1, 10)) | {B - 1, B, B + 1, BIG})]
    for nst, shifted in ALIGN_NST.items():
        out += [SimpleNamespace(nst=nst, off=off, outs=tuple((off + i) % 16 for i in range(n)),
                                kind="align") for off in range(16)]
        out.append(SimpleNamespace(nst=nst, off=shifted, outs=(0,) * n, kind="aligned-out"))
    return out


def plain_id(c):
    return "encode %s: %d stripes, input at +%d, outputs at +%s" % (
        c.kind, c.nst, c.off, sorted(set(c.outs)))


@functools.lru_cache(maxsize=None)
def write_cases(geom):
    """A write of `size` user bytes at `head`; the user buffer at address `mis`
    mod 16; oh / ot: old_head / old_tail given."""
    k, n = geom
    S = CHUNK * k
    rng = _rng(k, n, 1)
    out = []

    def add(head, size, oh, ot, mis=None):
        head, size = int(head), int(size)
        assert 0 <= head < S and size > 0
        out.append(SimpleNamespace(
            head=head, size=size, oh=oh, ot=ot, b2=head + size, nst=-(-(head + size) // S),
            mis=int(rng.integers(0, 16)) if mis is None else mis))

    def b2(nst, end):
        return (nst - 1) * S + (end or S)

    add(1, 1, True, True)                       # one byte, strictly inside
    add(17, 9, True, False)                     # inside the piece [16, 32)
    add(15, 2, False, True)                     # across a piece boundary
    add(S // 2, 100, False, False)
    add(16, S - 16, True, True)                 # head + size == S
    add(S - 1, 1, False, True)
    add(0, S, True, True)                       # nothing merged
    add(0, 3 * S, False, False)
    add(1, 2 * S - 1, False, True)              # ends on a boundary, old_tail given
    add(0, 4 * S, True, True)
    for oh, ot in PRESENCE:
        add(S - 1, 2, oh, ot)                   # two stripes, one user byte in each
    p = 0
    for nst in W_NST:
        for h in rng.permutation(heads(S)):
            e = rng.choice([e for e in ends(S) if b2(nst, e) > h])
            add(h, b2(nst, e) - h, *PRESENCE[p % 4])
            p += 1
        for e in ends(S):
            h = rng.choice([h for h in heads(S) if b2(nst, e) > h])
            add(h, b2(nst, e) - h, *PRESENCE[p % 4])
            p += 1
    for sh in range(16):                        # (user - head) mod 16 == sh
        h = int(rng.choice(heads(S)))
        e = int(rng.choice(ends(S)))
        add(h, b2(SHIFT_NST, e) - h, *PRESENCE[sh % 4], mis=(sh + h) % 16)
    return out


def write_id(c):
    return "write: head %d, %d bytes (%d stripes, end %d), old_head %s, old_tail %s, user at +%d" % (
        c.head, c.size, c.nst, c.b2, c.oh, c.ot, c.mis)


def interior_shift(c):
    """(user - head) mod 16: where the interior stripes are read in place."""
    return (c.mis - c.head) % 16


# --- the guard and checking helper (pure numpy) ------------------------------

def aligned(nbytes, fill=None):
    """A 64-byte aligned uint8 array."""
    raw = np.empty(nbytes + 64, np.uint8)
    v = raw[(-raw.ctypes.data) % 64:][:nbytes]
    if fill is not None:
        v[:] = fill
    return v


def layout(sizes, offs):
    """Where the outputs of a call lie in their one allocation (16-byte
    aligned): seg[i] = (lo, start, size, hi), the payload at [start, start +
    size) with start mod 16 == offs[i], its guards [lo, start) and [start +
    size, hi), both of GUARD bytes or more."""
    seg, pos = [], 0
    for size, off in zip(sizes, offs):
        assert 0 <= off < 16 and size > 0
        hi = pos + GUARD + 16 + -(-size // 16) * 16 + GUARD
        seg.append((pos, pos + GUARD + off, size, hi))
        pos = hi
    return SimpleNamespace(total=pos, seg=seg)


def new_outputs(lay):
    return aligned(lay.total, FILL)


def check_outputs(buf, lay, wants):
    """Compare the allocation `buf` of layout `lay` with the expected payloads:
    a list of (output, "front guard" | "back guard" | "payload", detail), empty
    when every payload is right and every guard byte is still FILL."""
    buf = np.asarray(buf)
    assert buf.size == lay.total and len(wants) == len(lay.seg)
    errs = []
    for i, ((lo, start, size, hi), want) in enumerate(zip(lay.seg, wants)):
        assert want.size == size
        front = np.flatnonzero(buf[lo:start] != FILL)
        if front.size:
            errs.append((i, "front guard", "%d bytes written, the farthest %d before the payload"
                         % (front.size, start - lo - int(front[0]))))
        back = np.flatnonzero(buf[start + size:hi] != FILL)
        if back.size:
            errs.append((i, "back guard", "%d bytes written, the farthest %d past the payload"
                         % (back.size, int(back[-1]) + 1)))
        d = np.flatnonzero(buf[start:start + size] != want)
        if d.size:
            errs.append((i, "payload", "%d bytes differ, first at %d (stripe %d)"
                         % (d.size, int(d[0]), int(d[0]) // CHUNK)))
    return errs


def pack_inputs(arrs, offs, seed):
    """One buffer (to be placed 16-byte aligned) with every array of `arrs`
    between FLANK random bytes, array i at an address of offs[i] mod 16:
    (buffer, [start of array i])."""
    starts, pos = [], 0
    for a, off in zip(arrs, offs):
        assert 0 <= off < 16
        starts.append(pos + FLANK + off)
        pos += FLANK + 16 + -(-a.size // 16) * 16 + FLANK
    buf = np.random.default_rng(seed).integers(0, 256, pos, dtype=np.uint8)
    for a, s in zip(arrs, starts):
        buf[s:s + a.size] = a
    return buf, starts


# --- what a later edit (or a change of seed) must not lose -------------------

for _g in ENC_GEOMS:
    _P = plain_cases(_g)
    _B = BLOCK[_g[0]]
    _cnt = [c for c in _P if c.kind == "count"]
    # P1
    assert {c.nst for c in _cnt} >= set(range(1, 10)) | {_B - 1, _B, _B + 1}, _g
    assert all(c.off == 0 and not any(c.outs) for c in _cnt), _g
    assert any(c.nst >= 200 and c.nst % 4 == 3 for c in _cnt), _g
    assert {c.nst % TILE for c in _cnt} == {0, 1, 2, 3}, _g
    _al = [c for c in _P if c.kind == "align"]
    # P2
    assert {(c.nst, c.off) for c in _al} == {(s, o) for s in (9, 6, 7) for o in range(16)}, _g
    assert {c.off for c in _al} == set(range(16)), _g
    # P3
    assert {(c.off % 4, c.nst % TILE) for c in _al if c.off % 4 and c.nst > TILE} == \
        {(sh, rag) for sh in (1, 2, 3) for rag in (1, 2, 3)}, _g
    # P4
    assert all(c.outs == tuple((c.off + i) % 16 for i in range(_g[1])) for c in _al), _g
    assert all(len(set(c.outs)) == min(16, _g[1]) for c in _al), _g
    assert {o for c in _al for o in c.outs} == set(range(16)), _g
    # P5
    assert {c.nst for c in _P if c.kind == "aligned-out" and c.off % 4 and not any(c.outs)} == \
        {9, 6, 7}, _g
for _g in WRITE_GEOMS:
    _C = write_cases(_g)
    _S = CHUNK * _g[0]
    _one = [c for c in _C if c.nst == 1]
    _multi = [c for c in _C if c.nst > 1]
    # W1
    assert {c.nst for c in _C} >= set(W_NST), _g
    assert {(c.nst - 1) % TILE for c in _multi} == {0, 1, 2, 3} and _one, _g
    # W2
    for _n in W_NST:
        assert {c.head for c in _C if c.nst == _n} >= set(heads(_S)), (_g, _n)
        assert {c.b2 % _S for c in _C if c.nst == _n} >= set(ends(_S)), (_g, _n)
    # W3, W4, W5
    assert any(c.head > 0 and c.b2 < _S for c in _one), _g
    assert any(c.head > 0 and c.b2 == _S for c in _one), _g
    assert any(c.head == 0 and c.b2 % _S == 0 for c in _one), _g
    assert any(c.head == 0 and c.b2 % _S == 0 for c in _multi), _g
    # W6
    assert any(c.b2 % _S == 0 and c.ot and c.head for c in _multi), _g
    # W7
    assert any(c.size == 1 and 0 < c.head and c.b2 < _S for c in _one), _g
    assert any(1 < c.size <= 15 and c.head // 16 == (c.b2 - 1) // 16 for c in _one), _g
    assert any(c.size <= 15 and c.head // 16 != (c.b2 - 1) // 16 for c in _one), _g
    # W8
    assert any(c.head == _S - 1 and c.size == 2 for c in _multi), _g
    # W9
    assert {(c.oh, c.ot) for c in _one} == set(PRESENCE) == {(c.oh, c.ot) for c in _multi}, _g
    assert {(c.oh, c.ot) for c in _C if c.head == _S - 1 and c.size == 2} == set(PRESENCE), _g
    # W10
    assert {interior_shift(c) for c in _C if c.nst == SHIFT_NST} == set(range(16)), _g
    assert all(c.nst == -(-c.b2 // _S) and c.head < _S and 0 <= c.mis < 16 for c in _C), _g


# --- data and expected values ------------------------------------------------

def build(O, geom):
    """The buffers and expected values of a geometry's cases: every case gets
    its packed input buffer (`ibuf`; `iseg` = the start of the encode input,
    or of user / old_head / old_tail), the layout of its outputs (`lay`) and
    the expected fragments (`want`)."""
    k, n = geom
    S = CHUNK * k
    rng = _rng(k, n, 0)
    plain = []
    if geom in ENC_GEOMS:
        data = rng.integers(0, 256, S * BIG, dtype=np.uint8)
        enc = {}
        for i, c in enumerate(plain_cases(geom)):
            if c.nst not in enc:
                enc[c.nst] = O.encode(k, n, data[:S * c.nst])
            ibuf, iseg = pack_inputs([data[:S * c.nst]], [c.off], 1000 + i)
            plain.append(SimpleNamespace(c=c, ibuf=ibuf, iseg=iseg, want=enc[c.nst],
                                         lay=layout([CHUNK * c.nst] * n, c.outs)))
    writes = []
    for i, c in enumerate(write_cases(geom)):
        user = rng.integers(0, 256, c.size, dtype=np.uint8)
        oh = rng.integers(0, 256, S, dtype=np.uint8) if c.oh else None
        ot = rng.integers(0, 256, S, dtype=np.uint8) if c.ot else None
        merged = O.writev_merge(k, c.head, user, oh, ot)
        assert merged.size == c.nst * S
        olds = [a for a in (oh, ot) if a is not None]
        ibuf, iseg = pack_inputs([user] + olds, [c.mis] + [(c.mis + 5 + 6 * j) % 16
                                                           for j in range(len(olds))], 2000 + i)
        pos = iter(iseg[1:])
        writes.append(SimpleNamespace(
            c=c, ibuf=ibuf, iseg=iseg, user=iseg[0], oh=next(pos) if c.oh else None,
            ot=next(pos) if c.ot else None, want=O.encode(k, n, merged),
            lay=layout([CHUNK * c.nst] * n, [(c.mis + 3 * b) % 16 if i % 2 else 0
                                             for b in range(n)])))
    for x in plain + writes:
        x.ibuf.setflags(write=False)
        for f in x.want:
            f.setflags(write=False)
    return SimpleNamespace(k=k, n=n, S=S, plain=plain, writes=writes)


@functools.lru_cache(maxsize=2)
def built(geom):
    """build() of a geometry: shared, read-only, the last two kept."""
    import oracle as O
    O.lib()
    return build(O, geom)
