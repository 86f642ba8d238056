"""ec_method_heal_extents on host buffers: the fused heal of many extents, each
with fragments of its own, over the whole table of tests/_heal_extents_cases.py.
No GPU is needed: the host variant runs on the calling thread's CPU engine for
every gen.

The expected bytes come from the oracle alone.  Every fragment lies between 64
guard bytes of 0xA5 in one arena that is compared whole, and the engine
counters stay as they were.
"""
import ctypes
import errno

import numpy as np
import pytest

import _heal_extents_cases as C

GENS = ["none", "avx"]
GUARD = 64
ALL_GEOMS = C.GEOMS + C.WIDE_GEOMS


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def host_table(ec, call, built):
    t = ec.extent_table(C.records(call, built, built.arena.ctypes.data))
    assert ec.extents_layout(t) == C.firsts(call.extents)[1]
    return t


def masks_of(call):
    return [p[0] for p in call.pairs], [p[1] for p in call.pairs]


def run(ec, L, oracle, call, family, offset=C.rotating):
    b = C.build(oracle, call, family, GUARD, offset)
    t = host_table(ec, call, b)
    assert L.heal_extents(t, *masks_of(call)) == 0
    assert np.array_equal(b.arena, b.want), "%s %s %s" % (C.geom_id((call.k, call.n)), call.what,
                                                         family)
    return b


def test_record_layout(ec):
    assert ctypes.sizeof(ec.Extent) == C.RECORD == 272
    assert ec.Extent.first.offset == 256 and ec.Extent.zero.offset == 268


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("geom", ALL_GEOMS, ids=C.geom_id)
def test_heal_extents_matches_oracle(ec, oracle, geom, family, gen):
    before = ec.stats()
    with ec.ECMatrixList(*geom, gen=gen) as L:
        assert L.engine.startswith("cpu/")
        for call in C.table(*geom):
            run(ec, L, oracle, call, family)
    assert ec.stats() == before


@pytest.mark.parametrize("geom", ALL_GEOMS, ids=C.geom_id)
def test_each_extent_equals_ec_method_heal(ec, oracle, geom):
    k, n = geom
    call = C.ragged_call(k, n)
    with ec.ECMatrixList(k, n, gen="none") as L:
        b = C.build(oracle, call, "arbitrary", GUARD)
        before = b.arena.copy()
        assert L.heal_extents(host_table(ec, call, b), *masks_of(call)) == 0
        for e, (ns, u) in enumerate(call.extents):
            mask, target = call.pairs[u]
            if not target:
                continue
            size = ns * C.CHUNK
            out = [np.empty(size, np.uint8) for _ in C.bits(target)]
            L.heal(ns, mask, [before[b.frag[e][i]:b.frag[e][i] + size] for i in C.bits(mask)],
                   target, out)
            for i, o in zip(C.bits(target), out):
                assert np.array_equal(o, b.arena[b.frag[e][i]:b.frag[e][i] + size]), (e, i)


@pytest.mark.parametrize("geom", C.BUCKET_GEOMS, ids=C.geom_id)
def test_one_extent_equals_heal_mixed_with_one_group(ec, oracle, geom):
    k, n = geom
    pairs = C.patterns(k, n)
    u = max(range(len(pairs)), key=lambda i: len(C.bits(pairs[i][1])))
    ns = 37
    call = C.Call(k, n, pairs, [(ns, u)], [0], [], True, "one extent")
    with ec.ECMatrixList(k, n, gen="none") as L:
        b = C.build(oracle, call, "arbitrary", GUARD)
        frags = [b.arena[o:o + ns * C.CHUNK].copy() for o in b.frag[0]]
        assert L.heal_extents(host_table(ec, call, b), *masks_of(call)) == 0
        assert L.heal_mixed(ns, 64, [pairs[u][0]], [pairs[u][1]], frags) == 0
        for i, o in enumerate(b.frag[0]):
            assert np.array_equal(frags[i], b.arena[o:o + ns * C.CHUNK]), i
        assert np.array_equal(b.arena, b.want)


def test_extents_layout(ec):
    sizes = [1, 4, 5, 8, 9, 0xFFFFFFFF, 3]
    t = ec.extent_table([([], ns, 0) for ns in sizes])
    for r in t:
        r.first = 77
    total = ec.extents_layout(t)
    want = C.firsts([(ns, 0) for ns in sizes])
    assert total == want[1] and [r.first for r in t] == want[0]
    assert ec.extents_layout(t, 0) == 0
    assert ec.lib.ec_method_extents_layout(0, None) == 0
    assert ec.lib.ec_method_extents_layout(3, None) == -errno.EINVAL
    # two extents of 2^32 - 1 stripes are 2^31 tiles: one too many
    big = ec.extent_table([([], 0xFFFFFFFF, 0), ([], 0xFFFFFFFC, 0)])
    assert ec.extents_layout(big) == 0x7FFFFFFF
    big[1].nstripes = 0xFFFFFFFF
    big[1].first = 5
    with pytest.raises(OSError) as e:
        ec.extents_layout(big)
    assert e.value.errno == errno.EINVAL and "2^31 - 1 tiles" in str(e.value)
    assert big[1].first == 5                   # left as it was
    t[2].nstripes = 0
    with pytest.raises(OSError) as e:
        ec.extents_layout(t)
    assert e.value.errno == errno.EINVAL and "no stripes" in str(e.value)


def small(ec, oracle):
    """A valid call of 4+2: three extents on two patterns."""
    low = 0xF
    call = C.Call(4, 6, [(low, 0x10), (low, 0x30), (0x3C, 0)], [(5, 0), (2, 1), (3, 2)],
                  [0, 1, 2], [], False, "small")
    b = C.build(oracle, call, "arbitrary", GUARD)
    return call, b, host_table(ec, call, b)


def rejected(ec, err, text, fn, *args):
    with pytest.raises(OSError) as e:
        fn(*args)
    assert e.value.errno == err, e.value
    assert text in ec.lib.ec_method_last_error().decode(), ec.lib.ec_method_last_error()


def test_no_extents(ec, oracle):
    call, b, t = small(ec, oracle)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        assert L.heal_extents(t, *masks_of(call), nextents=0) == 0
        # the patterns are checked first
        rejected(ec, errno.EINVAL, "overlaps its mask", L.heal_extents, t, [0xF], [0x11], 0)
    assert np.array_equal(b.arena, C.build(oracle, call, "arbitrary", GUARD).arena)


def test_einval_null_arguments(ec, oracle):
    call, b, t = small(ec, oracle)
    m = (ctypes.c_size_t * 3)(*masks_of(call)[0])
    tg = (ctypes.c_size_t * 3)(*masks_of(call)[1])
    with ec.ECMatrixList(4, 6, gen="none") as L:
        lst = ctypes.byref(L._list)
        for a, text in (((None, 3, ec.addr(t), 3, m, tg), "no list"),
                        ((lst, 3, None, 3, m, tg), "no extent table"),
                        ((lst, 3, ec.addr(t), 3, None, tg), "array is NULL"),
                        ((lst, 3, ec.addr(t), 3, m, None), "array is NULL"),
                        ((lst, 3, ec.addr(t), 0, m, tg), "no patterns")):
            assert ec.lib.ec_method_heal_extents(*a) == -errno.EINVAL
            assert text in ec.lib.ec_method_last_error().decode()
            assert "ec_method_heal_extents: " in ec.lib.ec_method_last_error().decode()


@pytest.mark.parametrize("mask", [0x7, 0x1F, 0x4F, 0], ids=hex)
def test_einval_mask_is_not_k_bricks(ec, oracle, mask):
    call, b, t = small(ec, oracle)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        # pattern 2 has no target: it is checked all the same
        rejected(ec, errno.EINVAL, "ec_method_heal_extents: a mask is not k bricks of the volume",
                 L.heal_extents, t, [0xF, 0xF, mask], [0x10, 0x30, 0])


@pytest.mark.parametrize("target,text", [(0x40, "a target mask names a brick outside the volume"),
                                         (0x21, "a target mask overlaps its mask")])
def test_einval_target(ec, oracle, target, text):
    call, b, t = small(ec, oracle)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        rejected(ec, errno.EINVAL, text, L.heal_extents, t, [0xF, 0xF, 0x3C], [0x10, target, 0])


def test_einval_more_than_15_targets(ec):
    t = ec.extent_table([([], 1, 0)])
    ec.extents_layout(t)
    with ec.ECMatrixList(3, 31, gen="none") as L:
        rejected(ec, errno.EINVAL, "more than 15 bricks", L.heal_extents, t, [0x7], [0xFFFF << 3])


@pytest.mark.parametrize("field,value,text", [
    ("nstripes", 0, "an extent has no stripes"),
    ("zero", 1, "the zero field of an extent is not 0"),
    ("pattern", 3, "the pattern of an extent is not below npatterns"),
    ("first", 1, "the first of an extent is not the tiles before it"),
])
def test_einval_record(ec, oracle, field, value, text):
    call, b, t = small(ec, oracle)
    setattr(t[1], field, value)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        rejected(ec, errno.EINVAL, text, L.heal_extents, t, *masks_of(call))
    assert np.array_equal(b.arena, C.build(oracle, call, "arbitrary", GUARD).arena)


@pytest.mark.parametrize("brick", [0, 3, 4, 5])
def test_einval_fragment_is_zero(ec, oracle, brick):
    call, b, t = small(ec, oracle)
    keep = t[1].frag[brick]
    t[1].frag[brick] = 0
    with ec.ECMatrixList(4, 6, gen="none") as L:
        rejected(ec, errno.EINVAL, "a fragment of a mask or a target mask is 0", L.heal_extents,
                 t, *masks_of(call))
        t[1].frag[brick] = keep
        t[0].frag[5] = 0                       # brick 5 is not named by pattern 0
        assert L.heal_extents(t, *masks_of(call)) == 0
    assert np.array_equal(b.arena, b.want)


def test_e2big_257_patterns(ec, oracle):
    call, b, t = small(ec, oracle)
    with ec.ECMatrixList(4, 6, gen="none") as L:
        rejected(ec, errno.E2BIG, "ec_method_heal_extents", L.heal_extents, t, [0xF] * 257,
                 [0x10] * 257)
        assert L.heal_extents(t, [0xF, 0xF] + [0x3C] * 254, [0x10, 0x30] + [0] * 254) == 0
    assert np.array_equal(b.arena, b.want)
