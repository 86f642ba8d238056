"""Shared case table of tests/test_heal_mixed_sweep.py (host buffers, CPU
engine) and tests/test_gpu_heal_mixed_sweep.py (device buffers,
ec_heal_mixed_n): ec_method_heal_mixed[_device] over every k from 1 to 16,
target counts on both sides of the block's wave count, one to four target
words, bricks up to 30 as sources and targets, and pattern lists on both sides
of the kernel's argument space with patterns of up to 69 words.

A call is (k, n, pairs, ids, nstripes, group_stripes): the (mask, target mask)
patterns of the device call and the pattern id of each stripe group.  Per k
there is a small call (n = k + 1 ... k + 4, mmax = n - k) and a wide one (n =
31, mmax from the plan of DW_PLAN); per K bucket, and for k = 16 too, a pair
of calls with mmax = 15 whose pattern counts are the most that the kernel
arguments hold and one more.  Pattern 0 of a call has m = mmax and its group 0,
pattern 1 is empty and has group 1, the next patterns take the target counts
around the wave count, the others are drawn; on n = 31 pattern 0 is built so
that its sources start at brick 3 or above, reach brick 24 or above and leave a
gap, with targets below them, in the gap and at brick 30.  The groups walk
through the patterns so that neighbours differ in m.

Nothing here calls the library.  The fragments and the expected bytes are
those of _heal_mixed_cases.case: the oracle's decode of each group's sources,
its encode, the rows of the group's targets.

k = 1: the oracle's inverse writes past a 1 x 1 matrix (tests/
_combine_sweep.py), so oracle.decode is never called with k = 1.  The encode
matrix is a column of ones and every fragment is the data: the decode of the
one source fragment is that fragment.  oracle_for() asserts both and hands
_heal_mixed_cases.case an oracle whose decode is that identity.

The launcher (ecdk_heal_mixed, ec_kernels.hip) is restated below in plain
Python -- bucket, waves, kw, dw, pattern words, where the patterns travel --
and clauses M1...M7 are asserted on the table at import, so that a change of
SEED cannot lose what the sweep is for.
"""
import collections
import functools

import numpy as np

import _heal_mixed_cases as C

CHUNK = C.CHUNK
SEED = 2029
MAX_STRIPES = 128
MAX_TARGETS = 15            # ECM_HEAL_MIXED_TARGETS: m is 0 ... 15
FAMILIES = C.FAMILIES

bits = C.bits
to_mask = C.to_mask

Call = collections.namedtuple("Call", "k n pairs ids ns gs kind")

# the target words of the wide call of each k: dw = 2, 3 and 4 in every bucket
DW_PLAN = {1: 2, 2: 3, 3: 4, 4: 4, 5: 2, 6: 3, 7: 4, 8: 4,
           9: 4, 10: 2, 11: 4, 12: 3, 13: 4, 14: 2, 15: 3, 16: 4}
# the k whose pattern counts cross the argument space: one per bucket below
# its K, and the largest pattern there is
FIT_K = (3, 7, 11, 16)


# --- the launcher, restated ---------------------------------------------------

def bucket(k):
    """The K that ec_heal_mixed_n is compiled for (launch_heal_mixed)."""
    return 4 if k <= 4 else 8 if k <= 8 else 16


def waves(k):
    """NW: the waves of a block, which share the m rows of its tile."""
    return 4 if k <= 4 else 8


def kw(k):
    """Words of the source bytes, and of a row of the heal matrix."""
    return (k + 3) // 4


def dw(mmax):
    """Words of the target bytes."""
    return (mmax + 3) // 4


def pwords(k, mmax):
    assert C.pattern_words(k, mmax) == kw(k) + 1 + dw(mmax) + mmax * kw(k)
    return C.pattern_words(k, mmax)


def in_table(call):
    """The patterns do not fit the kernel arguments: the device table, PG."""
    return len(call.pairs) * pwords(call.k, C.mmax(call.pairs)) > C.ARG_WORDS


def arg_fit(k, pairs):
    """The longest prefix of pairs that travels in the kernel arguments:
    _heal_mixed_cases.arg_fit with this table's patterns."""
    c = 0
    while c < len(pairs) and (c + 1) * pwords(k, C.mmax(pairs[:c + 1])) <= C.ARG_WORDS:
        c += 1
    return c


def ngroups(call):
    return C.ngroups(call.ns, call.gs)


def used(call):
    """The patterns that a group of the call names."""
    return [call.pairs[u] for u in sorted(set(call.ids))]


def count(pair):
    return len(bits(pair[1]))


def positions(pair):
    """Where the targets lie with respect to the sources."""
    src = bits(pair[0])
    return {"below" if b < src[0] else "above" if b > src[-1] else "between"
            for b in bits(pair[1])}


def call_id(c):
    return "%d+%d-%s-p%d-s%d-g%d" % (c.k, c.n - c.k, c.kind, len(c.pairs), c.ns, c.gs)


# --- the table ----------------------------------------------------------------

def _rng(seed, *salt):
    return np.random.default_rng([seed] + [int(s) for s in salt])


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _some(rng, seq, size):
    return sorted(int(x) for x in rng.choice(np.array(seq, dtype=np.int64), size=size,
                                              replace=False)) if size else []


def _drawn_pair(rng, k, n, m):
    src = _some(rng, range(n), k)
    return to_mask(src), to_mask(_some(rng, [b for b in range(n) if b not in src], m))


def _spread_pair(rng, k, m):
    """On n = 31, k >= 2, m >= 3: sources from brick 3 on that reach brick 24
    or above and leave a gap; a target below them, one in a gap, brick 30."""
    for _ in range(4000):
        src = _some(rng, range(3, 30), k)
        if src[-1] >= 24 and src[-1] - src[0] + 1 > k:
            break
    else:
        raise AssertionError("no spread sources for k = %d" % k)
    gap = [b for b in range(src[0], src[-1]) if b not in src]
    tgt = [30, int(rng.integers(0, 3)), _pick(rng, gap)]
    rest = [b for b in range(31) if b not in src and b not in tgt]
    return to_mask(src), to_mask(tgt + _some(rng, rest, m - 3))


def _pattern_list(rng, k, n, mmax, npat):
    """npat pairs: m = mmax, m = 0, the counts around the wave count that mmax
    allows, then drawn counts from 1 to mmax."""
    NW = waves(k)
    around = [v for v in (NW - 1, NW, NW + 1, 2 * NW + 1) if 0 < v < mmax]
    # the third has fewer targets than mmax wherever a pattern can
    ms = [mmax, 0] + (around or [int(rng.integers(1, max(mmax, 2)))])
    ms = (ms + [int(rng.integers(1, mmax + 1)) for _ in range(npat)])[:npat]
    out = []
    for i, m in enumerate(ms):
        if i == 0 and n == 31 and k >= 2 and m >= 3:
            out.append(_spread_pair(rng, k, m))
        else:
            out.append(_drawn_pair(rng, k, n, m))
    return out


def _group_ids(rng, pairs, groups):
    """Patterns 0, 1 (the empty one) and 2, then the others in a drawn order
    and all of them again: each group takes the pattern that has waited
    longest among those whose m is not the last group's."""
    ms = [count(p) for p in pairs]
    assert len(pairs) >= 3 and groups >= 3 and ms[0] and not ms[1] and ms[2]
    ids = [0, 1, 2]
    todo = [u for u in rng.permutation(len(pairs)).tolist() if u > 2] + ids
    while len(ids) < groups:
        u = next(u for u in todo if ms[u] != ms[ids[-1]])
        todo.remove(u)
        todo.append(u)
        ids.append(u)
    return ids


def table(seed):
    """The calls of one seed, clauses M1...M7 asserted."""
    out = []
    turn = collections.Counter()            # calls so far per bucket

    def add(k, n, pairs, salt, kind, gs=None, full=None):
        K = bucket(k)
        i = turn[K]
        turn[K] += 1
        rng = _rng(seed, k, n, salt)
        if gs is None:
            gs = C.GROUPS[i % 3]
        if full is None:
            full = int(rng.integers(*{4: (8, 32), 8: (4, 16), 16: (3, 8)}[gs]))
        ns = full * gs + i % 4              # every residue mod 4, short last groups
        out.append(Call(k, n, pairs, _group_ids(rng, pairs, C.ngroups(ns, gs)), ns, gs, kind))

    for k in range(1, 17):
        rng = _rng(seed, k)
        r = int(rng.integers(1, 5))
        add(k, k + r, _pattern_list(rng, k, k + r, r, int(rng.integers(3, 9))), 1, "small")
        lo = 4 * DW_PLAN[k] - 3
        mmax = int(rng.integers(lo, min(lo + 3, MAX_TARGETS) + 1))
        add(k, 31, _pattern_list(rng, k, 31, mmax, int(rng.integers(6, 11))), 2, "wide")
        if k in FIT_K:
            pairs = _pattern_list(rng, k, 31, MAX_TARGETS, 32)
            fit = arg_fit(k, pairs)
            assert 5 <= fit < 31
            # 31 groups of 4 and a short one: enough to name every pattern
            add(k, 31, pairs[:fit], 3, "fit", 4, 31)
            add(k, 31, pairs[:fit + 1], 4, "over", 4, 31)
    check_clauses(out)
    return out


def check_clauses(sweep):
    """M1...M7 on a table."""
    assert len({call_id(c) for c in sweep}) == len(sweep)
    for c in sweep:
        assert 1 <= c.k <= 16 and c.k < c.n <= 31 and len(c.pairs) <= C.MAX_PATTERNS, c
        assert len(c.ids) == ngroups(c) and all(0 <= u < len(c.pairs) for u in c.ids), c
        for mask, target in c.pairs:
            assert len(bits(mask)) == c.k and not mask & target, c
            assert (mask | target) >> c.n == 0 and count((mask, target)) <= MAX_TARGETS, c

    # M1: every k
    assert {c.k for c in sweep} == set(range(1, 17))

    for K in (4, 8, 16):
        mine = [c for c in sweep if bucket(c.k) == K]
        NW = {4: 4, 8: 8, 16: 8}[K]
        assert all(waves(c.k) == NW for c in mine)
        pats = [p for c in mine for p in used(c)]
        ms = {count(p) for p in pats}

        # M2: the row loop `for (j = wave; j < m; j += NW)` on every side of NW
        assert any(0 < m < NW for m in ms) and NW in ms and NW + 1 in ms, (K, sorted(ms))
        if K == 4:
            assert any(m >= 2 * NW + 1 for m in ms), (K, sorted(ms))
        else:
            # a third trip needs m >= 17 at NW = 8, and a pattern has at most
            # 15 targets (ECM_HEAL_MIXED_TARGETS): (8, 17) and (16, 17) cannot be
            assert 2 * NW + 1 > MAX_TARGETS

        # M3: every dw; beside the pattern with m = mmax a call has used
        # patterns with fewer targets (unused target bytes and rows); targets
        # are packed in ascending brick order, so a pattern of 13 targets or
        # more has one at j = 3, 4, 7, 8, 11 and 12, both sides of every word
        assert {dw(C.mmax(c.pairs)) for c in mine} == {1, 2, 3, 4}, K
        for c in mine:
            mm = C.mmax(c.pairs)
            got = {count(p) for p in used(c)}
            assert mm in got and (mm == 1 or any(0 < m < mm for m in got)), c
        assert any(m >= 13 for m in ms), K

        # M5: high bricks on both sides, a target at 30, targets on every side
        # of the sources, sources that start at brick 3 or above
        assert any(bits(p[0])[-1] >= 24 for p in pats if p[1]), K
        assert any(b >= 24 for p in pats for b in bits(p[1])), K
        assert any(30 in bits(p[1]) for p in pats), K
        assert set().union(*[positions(p) for p in pats]) == {"below", "between", "above"}, K
        assert any(bits(p[0])[0] >= 3 for p in pats if p[1]), K

        # M6: both sides of the argument space with patterns of mmax = 15
        fit = [c for c in mine if c.kind == "fit"]
        over = [c for c in mine if c.kind == "over"]
        assert fit and len(fit) == len(over), K
        for f, o in zip(fit, over):
            assert f.k == o.k and o.pairs[:-1] == f.pairs and C.mmax(f.pairs) == MAX_TARGETS
            w = pwords(f.k, MAX_TARGETS)
            assert w >= 21 and len(f.pairs) == C.ARG_WORDS // w == arg_fit(f.k, o.pairs)
            assert not in_table(f) and in_table(o)
            # every pattern of both lists is some group's
            assert len(used(f)) == len(f.pairs) and len(used(o)) == len(o.pairs)

        # M7: stripe residues, group sizes
        assert {c.ns % 4 for c in mine} == {0, 1, 2, 3}, K
        assert {c.gs for c in mine} == {4, 8, 16}, K
        assert any(c.ns % c.gs for c in mine), K            # a short last group

    # M4: every kw; in bucket 16 a ragged and a full last word of both widths
    assert {kw(c.k) for c in sweep} == {1, 2, 3, 4}
    assert [kw(k) for k in (9, 12, 13, 16)] == [3, 3, 4, 4]
    # M6: at kw >= 3 and dw >= 2 the table is reached with fewer than 16 patterns
    for w in (3, 4):
        assert any(in_table(c) and kw(c.k) == w and dw(C.mmax(c.pairs)) >= 2 and
                   len(c.pairs) < 16 for c in sweep), w
    # a pattern of 16 sources and 15 targets is 69 words: 7 of them overflow
    assert pwords(16, 15) == 69 and 6 * 69 <= C.ARG_WORDS < 7 * 69

    # M7: in every call an empty group between two that are not, neighbours
    # that differ in m, and at most 128 stripes
    for c in sweep:
        ms = [count(c.pairs[u]) for u in c.ids]
        assert len(ms) >= 3 and any(ms[g] == 0 and ms[g - 1] and ms[g + 1]
                                    for g in range(1, len(ms) - 1)), c
        assert all(a != b for a, b in zip(ms, ms[1:])), c
        assert c.ns <= MAX_STRIPES, c
    assert len(sweep) == 2 * 16 + 2 * len(FIT_K)


SWEEP = table(SEED)


def offset_calls():
    """The calls of one k per K bucket, below the compiled K: they run again
    with every fragment 1 byte off alignment."""
    out = [c for c in SWEEP if c.k in (3, 7, 11)]
    assert {c.k for c in out} == {3, 7, 11}
    return out


# --- the fragments and the expected values ------------------------------------

class _IdentityAtOne:
    """The oracle, with the decode of k = 1 that needs no inverse."""

    def __init__(self, O):
        self._O = O

    def __getattr__(self, name):
        return getattr(self._O, name)

    def decode(self, k, rows, frags):
        assert k == 1 and len(rows) == 1 and len(frags) == 1
        return np.array(frags[0], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _identity(O):
    return _IdentityAtOne(O)


@functools.lru_cache(maxsize=None)
def oracle_for(O, k, n):
    """The oracle to build the cases of k + (n - k) with: itself, or for k = 1
    the one whose decode is the identity, once the two facts that make it so
    are checked."""
    if k > 1:
        return O
    assert O.encode_matrix(1, n).tolist() == [[1]] * n
    data = O.fill_xorshift(CHUNK * 3, seed=O.SEED + n)
    assert all(np.array_equal(f, data) for f in O.encode(1, n, data))
    return _identity(O)


def case(O, c, family):
    """_heal_mixed_cases.case of a call: (frags, want)."""
    return C.case(oracle_for(O, c.k, c.n), c.k, c.n, c.pairs, c.ids, c.ns, c.gs, family)


def check_case(c, cs, family):
    """What the expectation must be before anything is compared with it: no
    byte outside the chunks of a group's targets differs from what the call is
    given, and in the family "codeword" every one of those chunks does (a call
    that does nothing fails).  The arbitrary fragments are xorshift streams of
    neighbouring seeds, which are linear in the seed, so there a heal row can
    regenerate a chunk that is already in place and nothing is asked."""
    touched = [np.zeros(c.ns, bool) for _ in range(c.n)]
    for g, u in enumerate(c.ids):
        for b in bits(c.pairs[u][1]):
            touched[b][g * c.gs:(g + 1) * c.gs] = True
    for b in range(c.n):
        d = (cs.frags[b].reshape(c.ns, CHUNK) != cs.want[b].reshape(c.ns, CHUNK)).any(axis=1)
        assert not (d & ~touched[b]).any(), (call_id(c), family, b)
        assert family != "codeword" or np.array_equal(d, touched[b]), (call_id(c), family, b)
