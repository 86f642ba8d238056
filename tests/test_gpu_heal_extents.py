"""ec_method_heal_extents_device: the fused heal of many extents with fragments
of their own in device memory, over the whole table of
tests/_heal_extents_cases.py: every K bucket of ec_heal_extents_n with the
run-time k below the bucket, every ragged last tile, extents shorter than a
tile, extent counts on both sides of 64 and of a power of two, pattern sets in
the kernel arguments and in the device table, and an out-of-range pattern in
the device table.

The expected bytes come from the oracle alone.  Every fragment of every extent
of a call is carved from one tensor between 2 KiB guards of 0xA5, at a byte
offset that rotates through 0 .. 15, extents in a shuffled address order; the
whole tensor is compared afterwards, so a byte written anywhere but in a
target chunk fails.  The calls of a test are queued on one side stream with one
sync.  The table runs with the host copy of the extent table (checked in full)
and without it, again with every fragment 1 byte off for one geometry per
bucket, and in a child process with non-temporal staging forced
(EC_MI355X_LDSNT=1, read when the library loads) on 16-byte aligned fragments.
"""
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

import _heal_extents_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 2048
ALL_GEOMS = C.GEOMS + C.WIDE_GEOMS


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def masks_of(call):
    return [p[0] for p in call.pairs], [p[1] for p in call.pairs]


def upload(table):
    """The bytes of a host extent table in device memory."""
    import torch
    return torch.from_numpy(np.frombuffer(table, np.uint8).copy()).to(DEV)


class Held:
    """One call in device memory: the arena with every fragment, the extent
    table for its addresses on the host and on the device."""

    def __init__(self, ec, oracle, call, family, offset=C.rotating):
        import torch
        self.call = call
        self.built = C.build(oracle, call, family, GUARD, offset)
        self.t = torch.from_numpy(self.built.arena).to(DEV)
        assert self.t.data_ptr() % 16 == 0
        self.host = ec.extent_table(C.records(call, self.built, self.t.data_ptr()))
        self.ntiles = ec.extents_layout(self.host)
        assert self.ntiles == C.firsts(call.extents)[1]
        self.dev = upload(self.host)
        self.what = "%s %s %s" % (C.geom_id((call.k, call.n)), call.what, family)

    def heal(self, L, stream, checked=True):
        return L.heal_extents_device(0, stream, len(self.call.extents), self.ntiles, self.dev,
                                     self.host if checked else None, *masks_of(self.call))

    def frag(self, e, b):
        lo = self.built.frag[e][b]
        return None if lo is None else self.t[lo:lo + self.call.extents[e][0] * C.CHUNK]

    def check(self, want=None):
        got = self.t.cpu().numpy()
        want = self.built.want if want is None else want
        if np.array_equal(got, want):
            return
        for e, (ns, u) in enumerate(self.call.extents):
            for b, lo in enumerate(self.built.frag[e]):
                if lo is not None:
                    assert np.array_equal(got[lo:lo + ns * C.CHUNK], want[lo:lo + ns * C.CHUNK]), \
                        "%s: fragment %d of extent %d (%d stripes, pattern %d) differs" % (
                            self.what, b, e, ns, u)
        raise AssertionError("%s: bytes outside the fragments were written" % self.what)


def run_calls(ec, oracle, geom, calls, family, checked=True, offset=C.rotating):
    """All queued on one side stream, then one sync and the checks."""
    import torch
    held = [Held(ec, oracle, c, family, offset) for c in calls]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(*geom) as L:
        for h in held:
            assert h.heal(L, st.cuda_stream, checked) == 0
        ec.sync_device(0, st.cuda_stream)
    for h in held:
        h.check()


@pytest.mark.parametrize("checked", [True, False], ids=["ext_host", "no_ext_host"])
@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("geom", ALL_GEOMS, ids=C.geom_id)
def test_heal_extents_device_matches_oracle(ec, oracle, geom, family, checked):
    run_calls(ec, oracle, geom, C.table(*geom), family, checked)


@pytest.mark.parametrize("geom", C.BUCKET_GEOMS, ids=C.geom_id)
def test_fragments_one_byte_off(ec, oracle, geom):
    run_calls(ec, oracle, geom, C.table(*geom), "arbitrary", True, C.one_off)


@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_pattern_counts_cross_the_argument_space(ec, oracle, geom):
    """The most patterns that the kernel arguments hold, and one more (the
    device table)."""
    k, n = geom
    fit = C.arg_fit(k, n)
    words = C.M.pattern_words(k, C.M.mmax(C.M.pattern_list(k, n, fit)))
    assert fit * words <= C.ARG_WORDS < (fit + 1) * C.M.pattern_words(
        k, C.M.mmax(C.M.pattern_list(k, n, fit + 1)))
    run_calls(ec, oracle, geom, [C.pattern_call(k, n, fit), C.pattern_call(k, n, fit + 1)],
              "arbitrary", False)


@pytest.mark.parametrize("geom", C.BUCKET_GEOMS, ids=C.geom_id)
def test_pattern_past_the_table_clamps_to_the_last(ec, oracle, geom):
    """pattern = 255 in the device table only; such a table has no host copy."""
    k, n = geom
    pairs = C.patterns(k, n)
    last = len(pairs) - 1
    assert pairs[last][1] and last < 255
    call = C.Call(k, n, pairs, [(5, last), (3, 1), (9, last)], [2, 0, 1], [], False, "clamp")
    h = Held(ec, oracle, call, "arbitrary")
    for e in (0, 2):
        h.host[e].pattern = 255
    h.dev = upload(h.host)
    with ec.ECMatrixList(k, n) as L:
        assert h.heal(L, None, checked=False) == 0
        ec.sync_device(0)
    h.check()


@pytest.mark.parametrize("geom", C.BUCKET_GEOMS + C.WIDE_GEOMS, ids=C.geom_id)
def test_equals_heal_mixed_device_per_extent_and_the_host_variant(ec, oracle, geom):
    import torch
    k, n = geom
    call = C.ragged_call(k, n)
    h = Held(ec, oracle, call, "arbitrary")
    per = h.t.clone()
    gp = torch.zeros(4, dtype=torch.uint8, device=DEV)
    b = h.built
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        assert h.heal(L, None) == 0
        for e, (ns, u) in enumerate(call.extents):
            mask, target = call.pairs[u]
            if not target:
                continue
            frags = [None if lo is None else per[lo:lo + ns * C.CHUNK] for lo in b.frag[e]]
            assert L.heal_mixed_device(0, None, ns, 64, gp, [mask], [target], frags) == 0
        ec.sync_device(0)
    host = b.arena.copy()
    table = ec.extent_table(C.records(call, b, host.ctypes.data))
    ec.extents_layout(table)
    with ec.ECMatrixList(k, n, gen="none") as L:
        assert L.heal_extents(table, *masks_of(call)) == 0
    h.check()
    assert np.array_equal(host, b.want), "host variant"
    assert torch.equal(per, h.t), "one heal_mixed_device per extent"


@pytest.mark.parametrize("geom", C.BUCKET_GEOMS, ids=C.geom_id)
def test_heal_between_encode_and_verify_on_one_stream(ec, oracle, geom):
    """encode_device writes every extent's fragments into tensors of their
    own, the target fragments are scribbled over, one heal_extents_device
    restores them and verify_device checks every brick of every extent against
    the k lowest: one stream, no synchronisation in between."""
    import torch
    k, n = geom
    pairs = C.patterns(k, n)
    ids = C.walk(pairs, len(C.RAGGED), 3)
    low = (1 << k) - 1
    st = torch.cuda.Stream()
    ext, want = [], []
    for e, ns in enumerate(C.RAGGED):
        data = oracle.fill_xorshift(C.CHUNK * k * ns, seed=oracle.SEED + 7 + e)
        want.append(oracle.encode(k, n, data))
        ext.append((torch.from_numpy(data).to(DEV),
                    [torch.full((ns * C.CHUNK,), C.FILL, dtype=torch.uint8, device=DEV)
                     for _ in range(n)],
                    torch.full((ns,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)))
    table = ec.extent_table([(fr, ns, u) for (_, fr, _), ns, u in zip(ext, C.RAGGED, ids)])
    ntiles = ec.extents_layout(table)
    dev = upload(table)
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        for (din, fr, bad), ns, u in zip(ext, C.RAGGED, ids):
            L.encode_device(0, st.cuda_stream, ns, din, fr)
            with torch.cuda.stream(st):
                for b in C.bits(pairs[u][1]):
                    fr[b].fill_(C.SCRIBBLE)
        assert L.heal_extents_device(0, st.cuda_stream, len(ext), ntiles, dev, table,
                                     [p[0] for p in pairs], [p[1] for p in pairs]) == 0
        for (din, fr, bad), ns in zip(ext, C.RAGGED):
            L.verify_device(0, st.cuda_stream, ns, low, fr[:k], ((1 << n) - 1) & ~low, fr[k:],
                            bad)
        ec.sync_device(0, st.cuda_stream)
    for e, (din, fr, bad) in enumerate(ext):
        assert not bad.cpu().numpy().any(), e
        for b in range(n):
            assert np.array_equal(fr[b].cpu().numpy(), want[e][b]), (e, b)


def test_empty_targets_launch_nothing(ec, oracle):
    """A call whose patterns all have empty targets needs no fragment at all,
    and no extents is no work."""
    k, n = 4, 6
    table = ec.extent_table([([], 5, 0), ([], 1, 1)])
    ntiles = ec.extents_layout(table)
    dev = upload(table)
    with ec.ECMatrixList(k, n) as L:
        assert L.heal_extents_device(0, None, 2, ntiles, dev, table, [0xF, 0x3C], [0, 0]) == 0
        assert L.heal_extents_device(0, None, 2, ntiles, dev, None, [0xF, 0x3C], [0, 0]) == 0
        assert L.heal_extents_device(0, None, 0, 0, dev, None, [0xF], [0x10]) == 0
        ec.sync_device(0)


CHILD = r"""
import sys
sys.path[:0] = ["tests", "oracle"]
import glusterfs_amd.ec_method as ec
import oracle as O
import _heal_extents_cases as C
import test_gpu_heal_extents as T
O.lib()
for g in T.ALL_GEOMS:
    T.run_calls(ec, O, g, C.table(*g), "arbitrary", True, C.aligned)
print("ok")
"""


def test_heal_extents_device_nontemporal():
    """The kLdsDmaNT copies of the six instantiations: the whole table, both
    sides of the argument / table boundary included, on aligned fragments with
    the host copy of the table (which is what tells the call that they are)."""
    env = dict(os.environ, EC_MI355X_QUIET="1", EC_MI355X_LDSNT="1")
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=170)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


def test_heal_extents_device_argument_errors(ec, oracle):
    k, n = 4, 6
    low = 0xF
    call = C.Call(k, n, [(low, 0x10), (low, 0x30)], [(5, 0), (2, 1), (3, 0)], [0, 1, 2], [],
                  False, "errors")
    h = Held(ec, oracle, call, "arbitrary")
    masks, targets = masks_of(call)
    hostbuf = h.built.arena.copy()
    htable = ec.extent_table(C.records(call, h.built, hostbuf.ctypes.data))
    ec.extents_layout(htable)

    def rejected(text, fn, *args):
        with pytest.raises(OSError) as e:
            fn(*args)
        assert e.value.errno == errno.EINVAL, e.value
        assert text in ec.lib.ec_method_last_error().decode(), ec.lib.ec_method_last_error()

    def table(change):
        t = ec.extent_table(C.records(call, h.built, h.t.data_ptr()))
        ec.extents_layout(t)
        change(t)
        return t

    def set_field(e, name, value):
        return lambda t: setattr(t[e], name, value)

    def set_frag(e, b, value):
        def f(t):
            t[e].frag[b] = value
        return f

    with ec.ECMatrixList(k, n) as L:
        d = L.heal_extents_device
        ne, nt = 3, h.ntiles
        # host and device mixed: the table, its host copy, all or one fragment
        rejected("the extent table is not memory of the device", d, 0, None, ne, nt, h.host,
                 h.host, masks, targets)
        rejected("the host copy of the extent table is device memory", d, 0, None, ne, nt, h.dev,
                 h.dev, masks, targets)
        rejected("a fragment is not memory of the device", d, 0, None, ne, nt, h.dev, htable,
                 masks, targets)
        rejected("a fragment is not memory of the device", d, 0, None, ne, nt, h.dev,
                 table(set_frag(1, 5, htable[1].frag[5])), masks, targets)
        rejected("the extent table is device memory", L.heal_extents, h.dev, masks, targets, ne)
        rejected("a fragment is device memory", L.heal_extents, h.host, masks, targets)
        rejected("a fragment is device memory", L.heal_extents,
                 table_mixed(ec, call, h, hostbuf), masks, targets)
        rejected("the extent table is not 8-byte aligned", d, 0, None, ne, nt, h.dev[4:],
                 h.host, masks, targets)
        # the records and the total
        rejected("an extent has no stripes", d, 0, None, ne, nt, h.dev,
                 table(set_field(1, "nstripes", 0)), masks, targets)
        rejected("the zero field", d, 0, None, ne, nt, h.dev, table(set_field(2, "zero", 1)),
                 masks, targets)
        rejected("not below npatterns", d, 0, None, ne, nt, h.dev,
                 table(set_field(0, "pattern", 2)), masks, targets)
        rejected("the tiles before it", d, 0, None, ne, nt, h.dev,
                 table(set_field(2, "first", 2)), masks, targets)
        rejected("is 0", d, 0, None, ne, nt, h.dev, table(set_frag(0, 4, 0)), masks, targets)
        rejected("ntiles is not the total", d, 0, None, ne, nt + 1, h.dev, h.host, masks, targets)
        rejected("ntiles is not the total", d, 0, None, ne, ne - 1, h.dev, None, masks, targets)
        rejected("ntiles is not the total", d, 0, None, ne, 1 << 31, h.dev, None, masks, targets)
        # the patterns, with and without a host copy and before the no-extents return
        rejected("a mask is not k bricks", d, 0, None, ne, nt, h.dev, None, [low, 0x7], targets)
        rejected("overlaps its mask", d, 0, None, 0, 0, h.dev, None, masks, [0x10, 0x21])
        rejected("outside the volume", d, 0, None, ne, nt, h.dev, h.host, masks, [0x10, 0x40])
        rejected("no patterns", d, 0, None, ne, nt, h.dev, h.host, [], [])
        rejected("no extent table", d, 0, None, ne, nt, None, h.host, masks, targets)
        with pytest.raises(OSError) as e:
            d(0, None, ne, nt, h.dev, h.host, [low] * 257, [0x10] * 257)
        assert e.value.errno == errno.E2BIG
        ec.sync_device(0)
        assert np.array_equal(h.t.cpu().numpy(), h.built.arena), "a rejected call wrote"
        assert np.array_equal(hostbuf, h.built.arena)
        # and the call they all fall short of
        assert h.heal(L, None) == 0
        ec.sync_device(0)
    h.check()


def table_mixed(ec, call, h, hostbuf):
    """A host table of host fragments in which one fragment is device memory."""
    t = ec.extent_table(C.records(call, h.built, hostbuf.ctypes.data))
    ec.extents_layout(t)
    t[2].frag[0] = h.host[2].frag[0]
    return t
