"""Shared case builder of tests/test_scrub_sweep.py (host buffers, CPU engine)
and tests/test_gpu_scrub_sweep.py (device buffers, the six scrub tile kernels
and ec_repair_n / ec_repair2_n): one call per geometry that meets every brick
and every pair of bricks of avail_mask, for every k from 2 to 16.

Case i is stripe i: a seeded shuffle of one clean stripe, one stripe per brick
of avail_mask with that brick's chunk damaged, and one stripe per pair of
bricks with both chunks damaged, 1 + a + C(a, 2) stripes (at most 497).  So a
four-stripe tile mixes clean, single and pair stripes, and every entry of the
pair tables that locate2, decode_checked2 and repair2 carry is used.

Nothing here calls the library.  The expected values are the data the
fragments were encoded from, the oracle's encode and decode, and the rules
stated in include/ec_method.h:
  - one damaged chunk is always named, and decoded, healed and repaired around;
  - two damaged chunks are EC_MI355X_LOCATE_MANY for locate when a - k >= 3.
    With a - k == 2 they can imitate a single error in a third brick, so those
    stripes are evaluated by the definition (_locate_cases.expected_loc), and
    the _checked calls and repair then give what the code implies: the decode
    of B_m as stored, for the brick m the definition names;
  - with a - k >= 4 locate2 names both, decode_checked2 returns the data and
    repair2 restores the clean fragments;
  - a MANY stripe decodes and heals from B, the k lowest bricks, as stored.
"""
import functools
import itertools
from types import SimpleNamespace

import numpy as np

import _locate_cases as LC

CHUNK = LC.CHUNK
GUARD = LC.GUARD
SENTINEL = LC.SENTINEL
MANY = LC.MANY
FILL = 0xA5
ALL31 = 0x7FFFFFFF

bits = LC.bits


def mask_of(bricks):
    return sum(1 << b for b in bricks)


def rows_of(bricks):
    return [b + 1 for b in bricks]


def _drawn(k, a, lo, salt):
    """a seeded bricks out of lo...30."""
    rng = np.random.default_rng(1000 * k + 10 * a + salt)
    return mask_of(rng.choice(np.arange(lo, 31), size=a, replace=False).tolist())


def _sweep():
    out = []
    for k in range(2, 17):
        out.append((2, 4, 0xF) if k == 2 else (k, k + 2, (1 << (k + 2)) - 1))
        out.append((k, k + 3, (1 << (k + 2)) - 1))          # the last brick is healed
        out.append((k, k + 4, (1 << (k + 4)) - 1))
        out.append((k, k + 5, (1 << (k + 5)) - 1))
        out.append((k, 31, _drawn(k, k + 4, 0, 1)))
        out.append((k, 31, _drawn(k, k + 6, 0, 2)))
    out.append((16, 31, ALL31))
    # per K bucket a drawn mask whose lowest brick is >= 3, and the a highest
    # bricks of 31: the basis reaches brick 24 and above
    for k in (3, 7, 11):
        out.append((k, 31, _drawn(k, k + 4, 3, 3)))
    for k in (4, 7, 12):
        a = k + 4
        out.append((k, 31, ALL31 & ~((1 << (31 - a)) - 1)))
    assert len(set(out)) == len(out)
    return out


SWEEP = _sweep()


def bucket(k):
    """The K the scrub tile kernels are compiled for (launch_scrub_tile)."""
    return 4 if k <= 4 else 8 if k <= 8 else 16


# what a change of seed must not lose
assert {g[0] for g in SWEEP} == set(range(2, 17))
for _K in (4, 8, 16):
    assert any(bucket(g[0]) == _K and bits(g[2])[0] >= 3 for g in SWEEP), _K
assert any(max(bits(g[2])[:g[0]]) >= 24 for g in SWEEP)
assert all(len(bits(g[2])) >= g[0] + 2 and bits(g[2])[-1] < g[1] <= 31 for g in SWEEP)
assert all(1 + a + a * (a - 1) // 2 <= 497 for a in (len(bits(g[2])) for g in SWEEP))


def geom_id(g):
    return "%d+%d-%x" % (g[0], g[1] - g[0], g[2])


def seed_of(g):
    return (g[0] * 64 + g[1]) * 7 + g[2] % 1000003


def targets_of(g):
    """The bricks heal_checked regenerates: the lowest brick outside
    avail_mask (the last brick of k + 3), and the highest one too beside
    k + 6 bricks; none where the volume has no brick to spare."""
    k, n, avail_mask = g
    outside = [b for b in range(n) if not (avail_mask >> b) & 1]
    if not outside or n - k < 3:
        return []
    if len(bits(avail_mask)) == k + 6 and len(outside) >= 2:
        return [outside[0], outside[-1]]
    return [outside[0]]


def offset_geoms():
    """One geometry per K bucket that takes all eight calls."""
    out = [g for g in SWEEP if g[0] in (3, 7, 11) and g[1] == 31
           and len(bits(g[2])) == g[0] + 6]
    assert [g[0] for g in out] == [3, 7, 11]
    return out


def chunk(buf, t):
    return buf[t * CHUNK:(t + 1) * CHUNK]


def recode(O, k, n, basis, frags, t=None):
    """(data, fragments) that the chunks of the k bricks `basis` imply: the
    oracle's decode and the encode of it; of stripe t only, if given."""
    src = [np.ascontiguousarray(frags[b] if t is None else chunk(frags[b], t)) for b in basis]
    data = O.decode(k, rows_of(basis), src)
    return data, O.encode(k, n, data)


def damage(rng, frags, t, case):
    """Damage the chunks of case's bricks in stripe t, in the way t % 3 names."""
    if t % 3 == 0:          # one symbol: the same bit of the same byte in each brick
        byte, bit = int(rng.integers(0, CHUNK)), int(rng.integers(0, 8))
        for b in case:
            frags[b][t * CHUNK + byte] ^= np.uint8(1 << bit)
    elif t % 3 == 1:        # one random bit at a random byte per brick
        for b in case:
            byte, bit = int(rng.integers(0, CHUNK)), int(rng.integers(0, 8))
            frags[b][t * CHUNK + byte] ^= np.uint8(1 << bit)
    else:                   # the whole chunk XORed with non-zero bytes
        for b in case:
            chunk(frags[b], t)[:] ^= rng.integers(1, 256, CHUNK, dtype=np.uint8)


def build(O, k, n, avail_mask, seed):
    """The cases, fragments and expected values of one geometry (see the
    module's docstring)."""
    avail = bits(avail_mask)
    a = len(avail)
    assert a >= k + 2 and avail[-1] < n
    basis, checks = avail[:k], avail[k:]
    rng = np.random.default_rng(seed)
    cases = [()] + [(b,) for b in avail] + list(itertools.combinations(avail, 2))
    cases = [cases[i] for i in rng.permutation(len(cases))]
    nst = len(cases)
    data = rng.integers(0, 256, CHUNK * k * nst, dtype=np.uint8)
    clean = O.encode(k, n, data)
    frags = [clean[b].copy() if b in avail else None for b in range(n)]
    for t, case in enumerate(cases):
        damage(rng, frags, t, case)

    # every case has the damaged chunks it claims, and no damage is zero
    differs = {b: (frags[b].reshape(nst, CHUNK) != clean[b].reshape(nst, CHUNK)).any(axis=1)
               for b in avail}
    for t, case in enumerate(cases):
        assert tuple(b for b in avail if differs[b][t]) == case, (t, case)

    single = np.array([len(c) == 1 for c in cases])
    pair = np.array([len(c) == 2 for c in cases])
    rule = np.array([mask_of(c) for c in cases], np.uint32)        # the OR of the case's bits

    # locate: by rule, and by the definition where a pair can imitate a single
    loc1 = np.where(pair, np.uint32(MANY), rule).astype(np.uint32)
    implied = {}                    # stripe -> (brick m, data, fragments) of an imitation
    if a - k == 2:
        for t in np.flatnonzero(pair).tolist():
            v = LC.expected_loc(O, k, n, avail, frags, t)
            assert v != 0 and not v & int(rule[t]), (t, cases[t], hex(v))
            loc1[t] = v
            if v != MANY:
                m = bits(v)[0]
                implied[t] = (m,) + recode(O, k, n, [b for b in avail if b != m][:k], frags, t)

    # verify, directly: what B implies against what is stored
    dec_b, enc_b = recode(O, k, n, basis, frags)
    bad = np.zeros(nst, np.uint32)
    for j in checks:
        d = (enc_b[j].reshape(nst, CHUNK) != frags[j].reshape(nst, CHUNK)).any(axis=1)
        bad |= np.where(d, np.uint32(1 << j), np.uint32(0))

    # decode_checked / heal_checked: the data and the clean targets around one
    # damaged chunk, B as stored for MANY, B_m as stored for an imitation
    clean_or_single = ~pair
    kc = k * CHUNK
    assert np.array_equal(dec_b.reshape(nst, kc)[loc1 == 0], data.reshape(nst, kc)[loc1 == 0])
    out1 = dec_b.copy()
    out1.reshape(nst, kc)[clean_or_single] = data.reshape(nst, kc)[clean_or_single]
    heal1 = [f.copy() for f in enc_b]
    for f, c in zip(heal1, clean):
        f.reshape(nst, CHUNK)[clean_or_single] = c.reshape(nst, CHUNK)[clean_or_single]
    # repair with loc1: the single stripes are clean again, an imitation gets
    # the chunk the code implies, every other stripe stays as stored
    rep1 = [None if f is None else f.copy() for f in frags]
    for t in np.flatnonzero(single).tolist():
        b = cases[t][0]
        chunk(rep1[b], t)[:] = chunk(clean[b], t)
    for t, (m, d, e) in implied.items():
        out1[t * kc:(t + 1) * kc] = d
        for f, ef in zip(heal1, e):
            chunk(f, t)[:] = ef
        chunk(rep1[m], t)[:] = e[m]

    # repair2 on the k + 2 lowest bricks of avail_mask, loc by rule for the
    # cases that lie inside them: those stripes are clean again in those bricks
    sub = avail[:k + 2]
    inside = np.array([all(b in sub for b in c) for c in cases])
    loc_sub = np.where(inside, rule, np.uint32(0)).astype(np.uint32)
    rep_sub = [None if f is None else f.copy() for f in frags]
    for t in np.flatnonzero(loc_sub).tolist():
        for b in cases[t]:
            chunk(rep_sub[b], t)[:] = chunk(clean[b], t)

    for arr in [data, bad, loc1, rule, loc_sub, out1] + clean + heal1 + \
            [f for f in frags + rep1 + rep_sub if f is not None]:
        arr.setflags(write=False)
    return SimpleNamespace(
        k=k, n=n, avail_mask=avail_mask, avail=avail, a=a, basis=basis, checks=checks, nst=nst,
        cases=cases, data=data, clean=clean, frags=frags, two=a - k >= 4,
        loc1=loc1,                  # locate, and the loc of decode_checked / heal_checked
        loc2=rule,                  # locate2 (a - k >= 4), and repair2's loc by rule
        bad=bad, out1=out1, heal1=heal1, rep1=rep1,
        sub_mask=mask_of(sub), loc_sub=loc_sub, rep_sub=rep_sub,
        nbad=int(np.count_nonzero(loc1)), nmany=int(np.count_nonzero(loc1 == MANY)),
        nsingle1=int(np.count_nonzero((loc1 != 0) & (loc1 != MANY))),
        ndirty=int(np.count_nonzero(rule)))


@functools.lru_cache(maxsize=2)
def _built(k, n, avail_mask):
    import oracle as O
    O.lib()
    return build(O, k, n, avail_mask, seed_of((k, n, avail_mask)))


def built(g):
    """build() of a geometry of SWEEP: shared, read-only, the last two kept."""
    return _built(*g)


def expected_stripe(O, k, n, avail, chunks):
    """One stripe by the definitions of include/ec_method.h, from the stored
    chunks (by brick): (loc of locate, bad of verify with mask B and every
    other brick of avail checked, the data decode_checked returns, the
    fragments heal_checked regenerates from)."""
    basis = avail[:k]
    loc = LC.expected_loc(O, k, n, avail, chunks, 0)
    _, enc_b = recode(O, k, n, basis, chunks)
    bad = mask_of(j for j in avail[k:] if not np.array_equal(enc_b[j], chunks[j]))
    src = basis if loc in (0, MANY) else [b for b in avail if b != bits(loc)[0]][:k]
    d, e = recode(O, k, n, src, chunks)
    return loc, bad, d, e
