"""ec_method_heal_mixed on host buffers: the fused heal with a pattern per
stripe group, over the whole table of tests/_heal_mixed_cases.py.  No GPU is
needed: the host variant runs on the calling thread's CPU engine for every gen.

The expected fragments come from the oracle alone (decode of each group's
sources, encode, the target rows).  Every fragment lies between 64 guard bytes
of 0xA5 on each side, every byte that is no target chunk must stay as it was,
and the engine counters stay as they were.
"""
import errno

import numpy as np
import pytest

import _heal_mixed_cases as C

GENS = ["none", "avx"]
GUARD = 64


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def guarded(frags):
    """Each fragment in a buffer of its own between two guards: (buffers, views)."""
    bufs = []
    for f in frags:
        b = np.full(GUARD + f.size + GUARD, C.FILL, np.uint8)
        b[GUARD:GUARD + f.size] = f
        bufs.append(b)
    return bufs, [b[GUARD:b.size - GUARD] for b in bufs]


def check(bufs, want, what):
    for i, (b, w) in enumerate(zip(bufs, want)):
        assert (b[:GUARD] == C.FILL).all() and (b[b.size - GUARD:] == C.FILL).all(), \
            "%s: a guard of fragment %d was written" % (what, i)
        assert np.array_equal(b[GUARD:b.size - GUARD], w), "%s: fragment %d differs" % (what, i)


def run(L, oracle, k, n, pairs, ids, ns, gs, family, what):
    c = C.case(oracle, k, n, pairs, ids, ns, gs, family)
    bufs, views = guarded(c.frags)
    gm = [pairs[u][0] for u in ids]
    gt = [pairs[u][1] for u in ids]
    assert L.heal_mixed(ns, gs, gm, gt, views) == 0
    check(bufs, c.want, what)
    return c


def raises(L, err, text, *args):
    import glusterfs_amd.ec_method as m
    with pytest.raises(OSError) as e:
        L.heal_mixed(*args)
    assert e.value.errno == err
    assert text in m.lib.ec_method_last_error().decode(), m.lib.ec_method_last_error().decode()


def test_table_covers_what_it_promises():
    for k, n in C.GEOMS:
        pairs = C.patterns(k, n)
        low, high, gap = C.masks(k, n)
        assert len({low, high, gap}) == 3 and all(len(C.bits(m)) == k for m in (low, high, gap))
        assert all(m >> n == 0 and t >> n == 0 and not (m & t) for m, t in pairs)
        for mask in (low, high, gap):
            assert {len(C.bits(t)) for m, t in pairs if m == mask} == set(range(n - k + 1))
        assert any(m == low and t > low for m, t in pairs)            # targets above
        assert any(m == high and 0 < t < high for m, t in pairs)      # below
        assert any(m == gap and t & 2 for m, t in pairs)              # between
        if n - k >= 2:
            tm = {}
            for m, t in pairs:
                if t:
                    tm.setdefault(t, set()).add(m)
            assert any(len(v) > 1 for v in tm.values())   # one target, different masks
        fit = C.arg_fit(k, n)
        assert 2 < fit < C.MAX_PATTERNS and fit + 1 in C.counts(k, n)
        assert fit * C.pattern_words(k, n - k) <= C.ARG_WORDS < (fit + 1) * C.pattern_words(k, n - k)
    shapes = [(ns, gs) for ns in C.NSTRIPES for gs in C.GROUPS]
    assert any(ns % gs and ns > gs for ns, gs in shapes)             # a short last group
    assert any(ns % 4 for ns, gs in shapes)                          # a short last tile


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_heal_mixed_matches_oracle(ec, oracle, geom, family, gen):
    k, n = geom
    before = ec.stats()
    with ec.ECMatrixList(k, n, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        for ns, gs, pairs, ids in C.table(k, n):
            run(L, oracle, k, n, pairs, ids, ns, gs, family,
                "%s %d stripes in groups of %d, %s" % (C.geom_id(geom), ns, gs, family))
    assert ec.stats() == before


@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_pattern_counts(ec, oracle, geom):
    """1, 2, the count that fills the device kernel's arguments, one more, and
    256 patterns (the host call sees the distinct ones among them)."""
    k, n = geom
    ns, gs = 67, 4
    with ec.ECMatrixList(k, n, gen="none") as L:
        for count in C.counts(k, n):
            pairs = C.pattern_list(k, n, count)
            ids = C.group_ids(C.ngroups(ns, gs), count)
            run(L, oracle, k, n, pairs, ids, ns, gs, "arbitrary",
                "%s %d patterns" % (C.geom_id(geom), count))


@pytest.mark.parametrize("geom", [(8, 12), (16, 20)], ids=C.geom_id)
def test_256_distinct_pairs_pass_and_257_are_too_many(ec, oracle, geom):
    k, n = geom
    gs = 4
    pairs = C.pattern_list(k, n, 257, distinct=True)
    with ec.ECMatrixList(k, n, gen="none") as L:
        ids = list(range(256))
        run(L, oracle, k, n, pairs, ids, 256 * gs, gs, "arbitrary", "256 distinct pairs")
        frags = [f.copy() for f in C.base(oracle, k, n, 257 * gs, "arbitrary")]
        keep = [f.copy() for f in frags]
        with pytest.raises(OSError) as e:
            L.heal_mixed(257 * gs, gs, [p[0] for p in pairs], [p[1] for p in pairs], frags)
        assert e.value.errno == errno.E2BIG
        assert "ec_method_heal_mixed" in ec.lib.ec_method_last_error().decode()
        assert all(np.array_equal(a, b) for a, b in zip(frags, keep))


@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_each_group_equals_ec_method_heal(ec, oracle, geom):
    k, n = geom
    ns, gs = 37, 8
    pairs = C.patterns(k, n)
    ids = C.group_ids(C.ngroups(ns, gs), len(pairs), 1)
    with ec.ECMatrixList(k, n, gen="none") as L:
        c = run(L, oracle, k, n, pairs, ids, ns, gs, "arbitrary", C.geom_id(geom))
        for g, u in enumerate(ids):
            mask, target = pairs[u]
            if not target:
                continue
            lo, hi = g * gs * C.CHUNK, min((g + 1) * gs, ns) * C.CHUNK
            out = [np.empty(hi - lo, np.uint8) for _ in C.bits(target)]
            L.heal((hi - lo) // C.CHUNK, mask, [c.frags[b][lo:hi] for b in C.bits(mask)], target,
                   out)
            for b, o in zip(C.bits(target), out):
                assert np.array_equal(o, c.want[b][lo:hi]), (g, b)


@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_bricks_of_empty_target_groups_may_be_null(ec, oracle, geom):
    """Groups with an empty target are left alone and not read: a brick that
    only they name, or that no group names, may be NULL."""
    k, n = geom
    ns, gs = 37, 4
    low, high, _ = C.masks(k, n)
    target = 1 << k                            # low mask, the brick above it healed
    pairs = [(low, target), (high, 0)]
    ids = [g % 2 for g in range(C.ngroups(ns, gs))]
    c = C.case(oracle, k, n, pairs, ids, ns, gs, "arbitrary")
    used = C.needed(pairs, ids, n)
    assert all(used) == (n - k < 2)            # 2+1 has no brick to spare
    with ec.ECMatrixList(k, n, gen="none") as L:
        bufs, views = guarded(c.frags)
        given = [v if u else None for v, u in zip(views, used)]
        assert L.heal_mixed(ns, gs, [pairs[u][0] for u in ids], [pairs[u][1] for u in ids],
                            given) == 0
        check(bufs, c.want, C.geom_id(geom))
        # every group empty: nothing is read at all
        assert L.heal_mixed(ns, gs, [high] * len(ids), [0] * len(ids), [None] * n) == 0


def test_no_stripes(ec):
    with ec.ECMatrixList(4, 6, gen="none") as L:
        assert L.heal_mixed(0, 4, [0xF], [0x10], [None] * 6) == 0
        raises(L, errno.EINVAL, "group_stripes", 0, 2, [0xF], [0x10], [None] * 6)


def args(k=4, n=6, ns=8, gs=4):
    frags = [np.zeros(ns * C.CHUNK, np.uint8) for _ in range(n)]
    g = C.ngroups(ns, gs)
    return ns, gs, [(1 << k) - 1] * g, [1 << k] * g, frags


@pytest.mark.parametrize("gs", [0, 1, 2, 3, 6, 12])
def test_einval_group_stripes(ec, gs):
    with ec.ECMatrixList(4, 6, gen="none") as L:
        ns, _, gm, gt, frags = args()
        raises(L, errno.EINVAL, "group_stripes is not a power of two of at least 4", ns, gs, gm,
               gt, frags)


@pytest.mark.parametrize("mask", [0x7, 0x1F, 0x4F, 0], ids=hex)
def test_einval_mask_is_not_k_bricks(ec, mask):
    with ec.ECMatrixList(4, 6, gen="none") as L:
        ns, gs, gm, gt, frags = args()
        gm[1] = mask
        gt[1] = 0
        raises(L, errno.EINVAL, "a mask is not k bricks of the volume", ns, gs, gm, gt, frags)


def test_einval_target_outside_the_volume(ec):
    with ec.ECMatrixList(4, 6, gen="none") as L:
        ns, gs, gm, gt, frags = args()
        gt[1] = 1 << 6
        raises(L, errno.EINVAL, "a target mask names a brick outside the volume", ns, gs, gm, gt,
               frags)


def test_einval_target_overlaps_its_mask(ec):
    with ec.ECMatrixList(4, 6, gen="none") as L:
        ns, gs, gm, gt, frags = args()
        gt[0] = 0x30 | 0x2
        raises(L, errno.EINVAL, "a target mask overlaps its mask", ns, gs, gm, gt, frags)


@pytest.mark.parametrize("brick", [0, 3, 4])
def test_einval_null_fragment(ec, brick):
    with ec.ECMatrixList(4, 6, gen="none") as L:
        ns, gs, gm, gt, frags = args()
        frags[brick] = None
        raises(L, errno.EINVAL, "a fragment of a mask or a target mask is NULL", ns, gs, gm, gt,
               frags)
        frags[5] = None                       # brick 5 is named by nothing
        frags[brick] = np.zeros(ns * C.CHUNK, np.uint8)
        assert L.heal_mixed(ns, gs, gm, gt, frags) == 0


def test_einval_null_arguments(ec):
    import ctypes
    lib = ec.lib
    with ec.ECMatrixList(4, 6, gen="none") as L:
        ns, gs, gm, gt, frags = args()
        one = (ctypes.c_size_t * 2)(0xF, 0xF)
        tgt = (ctypes.c_size_t * 2)(0x10, 0x10)
        fr = ec._ptr_array(frags)
        lst = ctypes.byref(L._list)
        for a, text in (((None, ns, gs, one, tgt, fr), "no list"),
                        ((lst, ns, gs, None, tgt, fr), "array is NULL"),
                        ((lst, ns, gs, one, None, fr), "array is NULL"),
                        ((lst, ns, gs, one, tgt, None), "no fragment list")):
            assert lib.ec_method_heal_mixed(*a) == -errno.EINVAL
            assert text in ec.lib.ec_method_last_error().decode(), ec.lib.ec_method_last_error().decode()
