"""Shared case table of tests/test_verified_sweep.py (host buffers, CPU engine)
and tests/test_gpu_verified_sweep.py (device buffers, ec_decode_verified_n and
ec_heal_verified_n): ec_method_decode_verified[_device] and
ec_method_heal_verified[_device] over every k from 1 to 16, every check-row
count from 1 to 15, target counts from 1 to 31 - a, bases that reach brick 24
and above and every stripe residue, one call per (geometry, heal) that meets every brick of
avail_mask.

A geometry is (k, n, avail_mask, heals): one read, and one heal per entry of
heals (a tuple of target bricks).  Stripe i of its calls is case i of a seeded
shuffle of: one clean stripe, one stripe per brick of avail_mask with that
brick's chunk damaged, one per pair of check bricks, one (basis, check) pair
per check brick and one pair of basis bricks.  So a four-stripe tile mixes the
kinds; the count depends on k and a alone and needs no padding to meet every
residue mod 4 (clause V6 asserts that).
The damage is one symbol, one bit or the whole chunk, by t % 3; the bricks of
a pair are damaged in different symbols, so that two errors cannot cancel in
a check row.

Nothing here calls the library.  With B the k lowest bricks of avail_mask and
C the others, bad[] is _verify_cases.expected_flags of the oracle's prediction
from the stored chunks of B against the stored chunks of C, out is the
oracle's decode of the chunks of B as stored, and out[j] is row `target j` of
the oracle's encode of that decode.  Before anything is compared with the
library, build() asserts that this expectation obeys the MDS rules: damage in
check bricks alone gives exactly their bits and the original output, a
damaged basis chunk gives every bit of C and an output that differs from the
original, in every target.

k = 1: the oracle's inverse writes past a 1 x 1 matrix (tests/
_combine_sweep.py), so oracle.decode is never called with k = 1.  The encode
matrix is a column of ones and every fragment is the data: the decode of the
one basis fragment is that fragment.

The launcher (launch_scrub_tile, ec_kernels.hip) is restated below in plain
Python -- bucket, waves, kw, items -- and clauses V1...V7 are asserted on the
table at import, so that a change of SEED cannot lose what the sweep is for.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np

import _locate_cases as LC
from _verify_cases import expected_flags

CHUNK = LC.CHUNK
GUARD = LC.GUARD
SENTINEL = LC.SENTINEL
FILL = 0xA5
ALL31 = 0x7FFFFFFF
MAX_STRIPES = 497
SEED = 1825

bits = LC.bits


def mask_of(bricks):
    return sum(1 << b for b in bricks)


def rows_of(bricks):
    return [b + 1 for b in bricks]


# --- the launcher, restated ---------------------------------------------------

def bucket(k):
    """The K the two kernels are compiled for (launch_scrub_tile)."""
    return 4 if k <= 4 else 8 if k <= 8 else 16


def waves(k, nst=1):
    """NW: the waves of a block, which share the items of its tile."""
    return 4 if k <= 4 or (k <= 8 and nst > 1 << 17) else 8


def kw(k):
    """Words per row of the coefficient table (pack_rows)."""
    return (k + 3) // 4


def split(g):
    """(basis bricks, check bricks) of a geometry: B and C."""
    avail = bits(g[2])
    return avail[:g[0]], avail[g[0]:]


def nrows(g):
    """The check rows, a - k: where scrub_verified's items change kind."""
    return len(bits(g[2])) - g[0]


def items(g, targets=None):
    """The wave items of a call: the check rows, then the k rows of inv(B)
    (read) or one row per target (heal)."""
    return nrows(g) + (g[0] if targets is None else len(targets))


def table_words(g, targets=None):
    """Words of the one coefficient table that both halves share (of 128)."""
    return items(g, targets) * kw(g[0])


def position(g, brick):
    """Where a brick outside avail_mask lies with respect to the basis."""
    basis, _ = split(g)
    return "below" if brick < basis[0] else "between" if brick < basis[-1] else "above"


def geom_id(g):
    return "%d+%d-%x" % (g[0], g[1] - g[0], g[2])


def calls(sweep):
    """(kernel, geometry, targets) of every call of a table."""
    out = []
    for g in sweep:
        out.append(("read", g, None))
        out += [("heal", g, t) for t in g[3]]
    return out


# --- the table ----------------------------------------------------------------

def _rng(seed, *salt):
    return np.random.default_rng([seed] + [int(s) for s in salt])


def _draw(rng, lo, a, ok=lambda m: True):
    """a seeded bricks out of lo...30 that satisfy ok()."""
    for _ in range(4000):
        m = mask_of(rng.choice(np.arange(lo, 31), size=a, replace=False).tolist())
        if ok(m):
            return m
    raise AssertionError("no mask of %d bricks from %d on satisfies the rule" % (a, lo))


def _outside(n, mask):
    return [b for b in range(n) if not (mask >> b) & 1]


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _standard_heals(rng, k, mask):
    """Of a drawn mask on n = 31: one drawn target; two targets, one of them
    below the highest basis brick where the mask leaves one there; and all
    31 - a remaining bricks."""
    out = _outside(31, mask)
    top = bits(mask)[k - 1]
    low = [b for b in out if b < top]
    first = _pick(rng, low or out)
    second = _pick(rng, [b for b in out if b != first])
    return ((_pick(rng, out),), tuple(sorted((first, second))), tuple(out))


def _gap(bricks):
    """A brick range with a hole in it."""
    return bricks[-1] - bricks[0] + 1 > len(bricks)


def table(seed):
    """The geometries of one seed, clauses V1...V7 asserted."""
    out = []
    for k in range(1, 17):
        rng = _rng(seed, k)
        # no brick to spare: a read alone, there is nothing to heal
        out.append((k, k + 1, (1 << (k + 1)) - 1, ()))
        # k + 3 bricks: the k + 1 lowest heal the other two, k + 2 drawn ones
        # heal the one left over
        out.append((k, k + 3, (1 << (k + 1)) - 1, ((k + 1, k + 2),)))
        miss = int(rng.integers(0, k + 3))
        out.append((k, k + 3, ((1 << (k + 3)) - 1) & ~(1 << miss), ((miss,),)))
        for extra in (3, 5):
            m = _draw(rng, 0, k + extra)
            out.append((k, 31, m, _standard_heals(rng, k, m)))

    # per K bucket, rows 4 and 6...14 among them (V3):
    for k, r in ((3, 6), (7, 8), (11, 12)):
        # a drawn mask whose lowest brick is >= 3, with bricks left out below,
        # between and above the basis bricks (V5); also run 1 byte off
        def ok(m, k=k):
            b = bits(m)[:k]
            o = _outside(31, m)
            return any(b[0] < x < b[-1] for x in o) and any(x > b[-1] for x in o)
        rng = _rng(seed, k, 100)
        m = _draw(rng, 3, k + r, ok)
        b, o = bits(m)[:k], _outside(31, m)
        below = int(rng.integers(0, 3))
        between = _pick(rng, [x for x in o if b[0] < x < b[-1]])
        above = _pick(rng, [x for x in o if x > b[-1]])
        out.append((k, 31, m, ((below,), (between, above), (below, between, above))))
    for k, r, heals in ((4, 4, ((0,), (5, 22))),
                        (6, 6, ((0, 10),)),
                        (12, 5, ((3,), (0, 7, 13), (0, 3, 7, 13)))):
        # the a highest bricks of 31: the basis reaches brick 24 and above
        a = k + r
        out.append((k, 31, ALL31 & ~((1 << (31 - a)) - 1), heals))
    for k, r in ((2, 7), (5, 9), (10, 11)):
        # check bricks that are not contiguous; a target between two of them
        rng = _rng(seed, k, 200)
        m = _draw(rng, 0, k + r, lambda m, k=k: _gap(bits(m)[k:]))
        c = bits(m)[k:]
        mid = _pick(rng, [x for x in _outside(31, m) if c[0] < x < c[-1]])
        out.append((k, 31, m, ((mid,),)))
    for k, r in ((3, 13), (7, 10), (14, 14)):
        # many check rows: 13 rows on 4 waves, 17 items at K = 8, 14 rows
        rng = _rng(seed, k, 300)
        m = _draw(rng, 0, k + r)
        o = _outside(31, m)
        out.append((k, 31, m, ((_pick(rng, o),), tuple(o[:3]))))
    # every brick of 31: the largest tables at kw = 4, 124 words; 13 has the
    # most rows with a partial last coefficient word
    out.append((13, 31, ALL31, ()))
    out.append((16, 31, ALL31, ()))
    check_clauses(out, seed)
    return out


def shuffled_cases(g, seed):
    """The stripes of a geometry's calls (see the module's docstring): a list
    of tuples of damaged bricks.  Needs no oracle."""
    k, n, avail_mask, heals = g
    basis, checks = split(g)
    rng = _rng(seed, k, n, avail_mask % 1000003, 1)
    cases = [()] + [(b,) for b in basis + checks] + list(itertools.combinations(checks, 2))
    cases += [(_pick(rng, basis), c) for c in checks]
    if k >= 2:
        cases.append(tuple(sorted(rng.choice(basis, size=2, replace=False).tolist())))
    return [cases[i] for i in rng.permutation(len(cases))], rng


def nstripes(g, seed=SEED):
    return len(shuffled_cases(g, seed)[0])


def check_clauses(sweep, seed):
    """V1...V7 on a table."""
    C = calls(sweep)
    assert len({geom_id(g) for g in sweep}) == len(sweep)
    for g in sweep:
        k, n, m, heals = g
        basis, checks = split(g)
        assert 1 <= k <= 16 and len(checks) >= 1 and bits(m)[-1] < n <= 31, g
        assert k + nrows(g) <= 31 and table_words(g) <= 128, g
        for t in heals:
            assert t and list(t) == sorted(set(t)) and t[-1] < n and not mask_of(t) & m, g
            assert table_words(g, t) <= 128, g
        # no heal is possible with every brick at hand, and only then is there none
        assert bool(heals) == (len(bits(m)) < n), g

    # V1: every k, for the read and for the heal
    for kernel in ("read", "heal"):
        assert {g[0] for kn, g, _ in C if kn == kernel} == set(range(1, 17)), kernel

    # V2: where the wave-item loop changes trips and kinds
    for kernel in ("read", "heal"):
        for K in (4, 8, 16):
            NW = waves(K)
            mine = [(g, t) for kn, g, t in C if kn == kernel and bucket(g[0]) == K]
            its = {items(g, t) for g, t in mine}
            if (kernel, K) == ("read", 16):
                # a >= k + 1 >= 10 items: fewer than NW = 8 cannot be, nor can
                # NW and NW + 1; the least there is, NW + 2, is in
                assert min(k + 1 for k in range(9, 17)) == 10 == NW + 2 == min(its)
            else:
                assert any(i < NW for i in its), (kernel, K)
                assert NW in its and NW + 1 in its, (kernel, K, sorted(its))
            assert any(i >= 2 * NW + 1 for i in its), (kernel, K)
            assert len({nrows(g) % NW for g, _ in mine} - {0}) >= 3, (kernel, K)
            # a wave that takes a check row on one trip and an output row on
            # the next, at a boundary that is no multiple of NW
            assert any(nrows(g) % NW and nrows(g) > NW and items(g, t) > nrows(g)
                       for g, t in mine), (kernel, K)

    # V3: check-row counts; both sides of a word of brick[] are single-damage
    # stripes in every geometry (shuffled_cases), so 9 rows or more have rows
    # 3, 4, 7 and 8
    assert {nrows(g) for g in sweep} >= set(range(1, 16))
    assert any(nrows(g) >= 9 for g in sweep)
    for g in sweep:
        cases, _ = shuffled_cases(g, seed)
        assert all((c,) in cases for c in split(g)[1]), g

    # V4: every kw; a table of more than 64 words where there can be one
    assert {kw(g[0]) for g in sweep} == {1, 2, 3, 4}
    assert max(31 * kw(k) for k in range(1, 9)) <= 64
    for kernel in ("read", "heal"):
        for w in (3, 4):
            assert any(table_words(g, t) > 64 for kn, g, t in C
                       if kn == kernel and kw(g[0]) == w), (kernel, w)
    assert max((31 - k) * kw(k) for k in range(1, 17)) == 72 == (31 - 13) * kw(13)
    assert any(kn == "heal" and g[0] == 13 and table_words(g, t) == 72 for kn, g, t in C)
    for k in (13, 16):
        assert any(kn == "read" and g[0] == k and table_words(g) == 124 for kn, g, _ in C)

    # V5: high bases; C lies above B by the rule; targets on every side of B
    for K in (4, 8, 16):
        mine = [g for g in sweep if bucket(g[0]) == K]
        assert any(split(g)[0][-1] >= 24 for g in mine), K
        assert any(bits(g[2])[0] >= 3 for g in mine), K
        assert any(_gap(split(g)[1]) for g in mine), K
        assert {position(g, b) for g in mine for t in g[3] for b in t} == \
            {"below", "between", "above"}, K
    assert all(split(g)[1][0] > split(g)[0][-1] for g in sweep)

    # V6: every stripe residue per kernel and bucket
    for kernel in ("read", "heal"):
        for K in (4, 8, 16):
            res = {nstripes(g, seed) % 4 for kn, g, _ in C if kn == kernel and bucket(g[0]) == K}
            assert res == {0, 1, 2, 3}, (kernel, K, res)

    # V7: sizes
    assert all(nstripes(g, seed) <= MAX_STRIPES for g in sweep)
    assert 1 + 31 + 30 * 29 // 2 + 30 == MAX_STRIPES         # the most there can be: 1+30
    assert len(sweep) <= 110


SWEEP = table(SEED)


def bucket_geoms(K):
    return [g for g in SWEEP if bucket(g[0]) == K]


def offset_geoms():
    """One geometry per K bucket, k below the compiled K, with three heals:
    four calls, one per dword offset of bad[] modulo 16."""
    out = [g for g in SWEEP if g[0] in (3, 7, 11) and bits(g[2])[0] >= 3 and
           [len(t) for t in g[3]] == [1, 2, 3]]
    assert [g[0] for g in out] == [3, 7, 11]
    return out


# --- the fragments and the expected values ------------------------------------

def chunk(buf, t):
    return buf[t * CHUNK:(t + 1) * CHUNK]


def damage(rng, frags, t, case):
    """Damage the chunks of case's bricks in stripe t, in the way t % 3 names.
    A symbol is one bit position of the 64-byte planes, a bit of it in each of
    the 8 planes; the bricks of a pair get different symbols."""
    cols = rng.permutation(64)[:len(case)].tolist()
    for b, col in zip(case, cols):
        c = chunk(frags[b], t)
        if t % 3 == 0:          # one symbol: a non-zero value over its 8 planes
            bit, val = int(rng.integers(0, 8)), int(rng.integers(1, 256))
            for p in range(8):
                if (val >> p) & 1:
                    c[64 * p + col] ^= np.uint8(1 << bit)
        elif t % 3 == 1:        # one bit
            c[64 * int(rng.integers(0, 8)) + col] ^= np.uint8(1 << int(rng.integers(0, 8)))
        else:                   # the whole chunk XORed with non-zero bytes
            c[:] ^= rng.integers(1, 256, CHUNK, dtype=np.uint8)


def decode(O, k, basis, frags):
    """The data that the chunks of the k bricks `basis` imply, as stored."""
    src = [np.ascontiguousarray(frags[b]) for b in basis]
    if k == 1:
        return src[0].copy()
    return O.decode(k, rows_of(basis), src)


def build(O, g, seed=SEED):
    """The stripes, fragments and expected values of one geometry."""
    k, n, avail_mask, heals = g
    basis, checks = split(g)
    cmask = mask_of(checks)
    cases, rng = shuffled_cases(g, seed)
    nst = len(cases)
    data = rng.integers(0, 256, CHUNK * k * nst, dtype=np.uint8)
    clean = O.encode(k, n, data)
    if k == 1:
        assert O.encode_matrix(1, n).tolist() == [[1]] * n
        assert all(np.array_equal(f, data) for f in clean)
    frags = [clean[b].copy() if (avail_mask >> b) & 1 else None for b in range(n)]
    for t, case in enumerate(cases):
        damage(rng, frags, t, case)

    # every case has the damaged chunks it claims, and no damage is zero
    nb = np.zeros(nst, np.int64)            # damaged basis chunks per stripe
    cbits = np.zeros(nst, np.uint32)        # the damaged check bricks' bits
    for b in basis + checks:
        d = (frags[b].reshape(nst, CHUNK) != clean[b].reshape(nst, CHUNK)).any(axis=1)
        assert d.tolist() == [b in c for c in cases], (g, b)
        if b in basis:
            nb += d
        else:
            cbits |= d.astype(np.uint32) << np.uint32(b)

    # the expectation: the oracle on the chunks of B as stored
    out = decode(O, k, basis, frags)
    enc = O.encode(k, n, out)
    bad = expected_flags(enc, cmask, [frags[b] for b in checks], nst)

    # ... which obeys the MDS rules
    rule = np.where(nb > 0, np.uint32(cmask), cbits).astype(np.uint32)
    assert np.array_equal(bad, rule), (g, np.flatnonzero(bad != rule)[:8])
    hit = nb > 0
    kc = k * CHUNK
    assert np.array_equal(out.reshape(nst, kc)[~hit], data.reshape(nst, kc)[~hit]), g
    assert (out.reshape(nst, kc)[hit] != data.reshape(nst, kc)[hit]).any(axis=1).all(), g
    for j in sorted({j for t in heals for j in t}):
        w, c = enc[j].reshape(nst, CHUNK), clean[j].reshape(nst, CHUNK)
        assert np.array_equal(w[~hit], c[~hit]), (g, j)
        assert (w[hit] != c[hit]).any(axis=1).all(), (g, j)
    for b in basis:                         # B predicts itself
        assert np.array_equal(enc[b], frags[b]), (g, b)

    for arr in [data, out, bad] + list(clean) + list(enc) + [f for f in frags if f is not None]:
        arr.setflags(write=False)
    return SimpleNamespace(
        g=g, k=k, n=n, avail_mask=avail_mask, heals=heals, basis=basis, checks=checks,
        bmask=mask_of(basis), cmask=cmask, nst=nst, cases=cases, data=data, clean=clean,
        frags=frags, bad=bad, out=out, enc=enc, nbad=int(np.count_nonzero(bad)),
        basis_hit=hit)


@functools.lru_cache(maxsize=4)
def _built(g):
    import oracle as O
    O.lib()
    return build(O, g)


def built(g):
    """build() of a geometry of SWEEP: shared, read-only, the last four kept."""
    return _built(g)


def compare(S, targets, bad, outs, nbad, what):
    """One call's results (bad[0..nst), the outputs without their guards, and
    nbad or None) against the expectation."""
    d = np.flatnonzero(bad != S.bad)
    assert d.size == 0, (what, "bad", [(t, S.cases[t], hex(bad[t]), hex(S.bad[t])) for t in d[:8]])
    if targets is None:
        want, per = [S.out], S.k * CHUNK
    else:
        want, per = [S.enc[j] for j in targets], CHUNK
    assert len(outs) == len(want)
    for i, (o, w) in enumerate(zip(outs, want)):
        d = np.flatnonzero((o.reshape(S.nst, per) != w.reshape(S.nst, per)).any(axis=1))
        assert d.size == 0, (what, "output %d" % i, [(t, S.cases[t]) for t in d[:8]])
    if nbad is not None:
        assert nbad == S.nbad, (what, nbad, S.nbad)
