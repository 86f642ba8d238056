"""ec_method_heal_mixed_device: the fused heal with a pattern per stripe group
on fragments in device memory, over the whole table of
tests/_heal_mixed_cases.py: every K bucket of ec_heal_mixed_n with the run-time
k below the bucket, short last groups and tiles, pattern sets in the kernel
arguments and in the device table, and an out-of-range id in the group map.

The expected fragments come from the oracle alone.  The n fragments of a case
are carved from one tensor, each between two 2 KiB guards of 0xA5 and at a byte
offset that rotates through 0 .. 15; the whole tensor is compared afterwards, so
a byte written anywhere but in a target chunk fails.  The calls of a test are
queued on one side stream with one sync.  The table runs again with every
fragment 1 byte off for one geometry per bucket, and in a child process with
non-temporal staging forced (EC_MI355X_LDSNT=1, read when the library loads) on
16-byte aligned fragments, which is what lets that policy through.
"""
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

import _heal_mixed_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 2048


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def rotating(i, b):
    return (i + b) % 16


def one_off(i, b):
    return 1


def aligned(i, b):
    return 0


class Held:
    """The fragments of one case in one device tensor, each between two guards."""

    def __init__(self, c, i, offset):
        import torch
        size = c.frags[0].size
        slot = GUARD + 16 + size + GUARD
        slot += -slot % 16
        self.spans = [(b * slot + GUARD + offset(i, b), size) for b in range(len(c.frags))]
        host = np.full(slot * len(c.frags), C.FILL, np.uint8)
        self.want = host.copy()
        for (lo, sz), f, w in zip(self.spans, c.frags, c.want):
            host[lo:lo + sz] = f
            self.want[lo:lo + sz] = w
        self.t = torch.from_numpy(host).to(DEV)
        assert self.t.data_ptr() % 16 == 0
        self.frags = [self.t[lo:lo + sz] for lo, sz in self.spans]

    def check(self, what):
        got = self.t.cpu().numpy()
        if np.array_equal(got, self.want):
            return
        for b, (lo, sz) in enumerate(self.spans):
            assert np.array_equal(got[lo:lo + sz], self.want[lo:lo + sz]), \
                "%s: fragment %d differs" % (what, b)
        raise AssertionError("%s: bytes outside the fragments were written" % what)


def dev_bytes(ids, offset=0):
    import torch
    t = torch.empty(len(ids) + offset, dtype=torch.uint8, device=DEV)
    t[offset:].copy_(torch.tensor(ids, dtype=torch.uint8))
    return t[offset:]


def run_cases(ec, oracle, k, n, cases, offset=rotating):
    """cases: (pairs, ids as given to the device, nstripes, group_stripes,
    family).  All queued on one side stream, then one sync and the checks."""
    import torch
    held = []
    for i, (pairs, ids, ns, gs, family) in enumerate(cases):
        clamped = [min(u, len(pairs) - 1) for u in ids]
        c = C.case(oracle, k, n, pairs, clamped, ns, gs, family)
        held.append((Held(c, i, offset), dev_bytes(ids, i % 4), pairs, ns, gs, family))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        for h, gp, pairs, ns, gs, family in held:
            assert L.heal_mixed_device(0, st.cuda_stream, ns, gs, gp, [p[0] for p in pairs],
                                       [p[1] for p in pairs], h.frags) == 0
        ec.sync_device(0, st.cuda_stream)
    for h, gp, pairs, ns, gs, family in held:
        h.check("%d+%d %d stripes in groups of %d, %d patterns, %s" % (k, n - k, ns, gs,
                                                                     len(pairs), family))


def table_cases(k, n, family):
    out = []
    for i, (ns, gs, pairs, ids) in enumerate(C.table(k, n)):
        if i % 3 == 1:
            ids = ids[:-1] + [255]         # past the patterns: clamps to the last one
        out.append((pairs, ids, ns, gs, family))
    return out


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_heal_mixed_device_matches_oracle(ec, oracle, geom, family):
    k, n = geom
    assert len(C.patterns(k, n)) < 255
    run_cases(ec, oracle, k, n, table_cases(k, n, family))


@pytest.mark.parametrize("geom", C.BUCKET_GEOMS, ids=C.geom_id)
def test_fragments_one_byte_off(ec, oracle, geom):
    k, n = geom
    run_cases(ec, oracle, k, n, table_cases(k, n, "arbitrary"), one_off)


@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_pattern_counts_cross_the_argument_space(ec, oracle, geom):
    """1 and 2 patterns, the most that the kernel arguments hold, one more (the
    device table) and 256."""
    k, n = geom
    ns, gs = 67, 4
    cases = []
    for count in C.counts(k, n):
        pairs = C.pattern_list(k, n, count)
        cases.append((pairs, C.group_ids(C.ngroups(ns, gs), count), ns, gs, "arbitrary"))
    run_cases(ec, oracle, k, n, cases)


def test_257_patterns_are_too_many(ec):
    k, n = 4, 6
    pairs = C.pattern_list(k, n, 257)
    h = Held(C.Case([np.zeros(4 * C.CHUNK, np.uint8)] * n, [np.zeros(4 * C.CHUNK, np.uint8)] * n),
             0, aligned)
    with ec.ECMatrixList(k, n) as L:
        with pytest.raises(OSError) as e:
            L.heal_mixed_device(0, None, 4, 4, dev_bytes([0]), [p[0] for p in pairs],
                                [p[1] for p in pairs], h.frags)
        assert e.value.errno == errno.E2BIG
        ec.sync_device(0)
    h.check("257 patterns")


@pytest.mark.parametrize("geom", C.GEOMS, ids=C.geom_id)
def test_equals_heal_device_per_group_and_the_host_variant(ec, oracle, geom):
    import torch
    k, n = geom
    ns, gs = 37, 8
    pairs = C.patterns(k, n)
    ids = C.group_ids(C.ngroups(ns, gs), len(pairs), 1)
    c = C.case(oracle, k, n, pairs, ids, ns, gs, "arbitrary")
    h = Held(c, 3, rotating)
    src = [torch.from_numpy(f.copy()).to(DEV) for f in c.frags]
    host = [f.copy() for f in c.frags]
    refs = []
    torch.cuda.synchronize()
    with ec.ECMatrixList(k, n) as L:
        assert L.heal_mixed_device(0, None, ns, gs, dev_bytes(ids), [p[0] for p in pairs],
                                   [p[1] for p in pairs], h.frags) == 0
        for g, u in enumerate(ids):
            mask, target = pairs[u]
            if not target:
                continue
            lo, hi = g * gs * C.CHUNK, min((g + 1) * gs, ns) * C.CHUNK
            out = [torch.full((hi - lo,), C.FILL, dtype=torch.uint8, device=DEV)
                   for _ in C.bits(target)]
            L.heal_device(0, None, (hi - lo) // C.CHUNK, mask, [src[b][lo:hi] for b in C.bits(mask)],
                          target, out)
            refs.append((lo, hi, C.bits(target), out))
        ec.sync_device(0)
    with ec.ECMatrixList(k, n, gen="none") as L:
        assert L.heal_mixed(ns, gs, [pairs[u][0] for u in ids], [pairs[u][1] for u in ids],
                            host) == 0
    h.check(C.geom_id(geom))
    for b, f in enumerate(h.frags):
        assert np.array_equal(f.cpu().numpy(), host[b]), "host variant, fragment %d" % b
    for lo, hi, bricks, out in refs:
        for b, o in zip(bricks, out):
            assert torch.equal(o, h.frags[b][lo:hi]), "heal_device, fragment %d at %d" % (b, lo)


@pytest.mark.parametrize("geom", C.BUCKET_GEOMS, ids=C.geom_id)
def test_heal_between_encode_and_verify_on_one_stream(ec, oracle, geom):
    """encode_device writes the fragments, the target chunks are scribbled
    over, heal_mixed_device restores them and verify_device checks every brick
    against the k lowest: one stream, no synchronisation in between."""
    import torch
    k, n = geom
    ns, gs = 67, 16
    pairs = C.patterns(k, n)
    ids = C.group_ids(C.ngroups(ns, gs), len(pairs), 2)
    data = oracle.fill_xorshift(C.CHUNK * k * ns, seed=oracle.SEED + 5)
    want = oracle.encode(k, n, data)
    din = torch.from_numpy(data).to(DEV)
    frags = [torch.full((ns * C.CHUNK,), C.FILL, dtype=torch.uint8, device=DEV) for _ in range(n)]
    bad = torch.full((ns,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
    gp = dev_bytes(ids)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    low = (1 << k) - 1
    with ec.ECMatrixList(k, n) as L:
        L.encode_device(0, st.cuda_stream, ns, din, frags)
        with torch.cuda.stream(st):
            for g, u in enumerate(ids):
                for b in C.bits(pairs[u][1]):
                    frags[b][g * gs * C.CHUNK:(g + 1) * gs * C.CHUNK].fill_(C.SCRIBBLE)
        assert L.heal_mixed_device(0, st.cuda_stream, ns, gs, gp, [p[0] for p in pairs],
                                   [p[1] for p in pairs], frags) == 0
        L.verify_device(0, st.cuda_stream, ns, low, frags[:k], ((1 << n) - 1) & ~low, frags[k:],
                        bad)
        ec.sync_device(0, st.cuda_stream)
    assert any(pairs[u][1] for u in ids)
    assert not bad.cpu().numpy().any()
    for b, (f, w) in enumerate(zip(frags, want)):
        assert np.array_equal(f.cpu().numpy(), w), "fragment %d" % b


def test_empty_targets_and_no_stripes_on_device(ec, oracle):
    """A brick that only groups without targets name may be NULL, a call whose
    groups all have no target reads nothing, and no stripes is no work."""
    k, n = 4, 6
    ns, gs = 37, 4
    low, high, _ = C.masks(k, n)
    pairs = [(low, 1 << k), (high, 0)]
    ids = [g % 2 for g in range(C.ngroups(ns, gs))]
    c = C.case(oracle, k, n, pairs, ids, ns, gs, "arbitrary")
    h = Held(c, 0, rotating)
    used = C.needed(pairs, ids, n)
    gp = dev_bytes(ids)
    with ec.ECMatrixList(k, n) as L:
        given = [f if u else None for f, u in zip(h.frags, used)]
        assert L.heal_mixed_device(0, None, ns, gs, gp, [low, high], [1 << k, 0], given) == 0
        assert L.heal_mixed_device(0, None, ns, gs, gp, [high, low], [0, 0], [None] * n) == 0
        assert L.heal_mixed_device(0, None, 0, gs, gp, [low, high], [1 << k, 0], given) == 0
        ec.sync_device(0)
    h.check("empty targets")


CHILD = r"""
import sys
sys.path[:0] = ["tests", "oracle"]
import glusterfs_amd.ec_method as ec
import oracle as O
import _heal_mixed_cases as C
import test_gpu_heal_mixed as T
O.lib()
for k, n in C.GEOMS:
    T.run_cases(ec, O, k, n, T.table_cases(k, n, "arbitrary"), T.aligned)
    cases = []
    for count in C.counts(k, n)[2:4]:
        pairs = C.pattern_list(k, n, count)
        cases.append((pairs, C.group_ids(C.ngroups(67, 4), count), 67, 4, "arbitrary"))
    T.run_cases(ec, O, k, n, cases, T.aligned)
print("ok")
"""


def test_heal_mixed_device_nontemporal():
    """The kLdsDmaNT copies of the six instantiations: the table and both sides
    of the argument / table boundary, on aligned fragments."""
    env = dict(os.environ, EC_MI355X_QUIET="1", EC_MI355X_LDSNT="1")
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=170)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


def test_heal_mixed_device_argument_errors(ec, oracle):
    k, n = 4, 6
    ns, gs = 8, 4
    low = (1 << k) - 1
    pairs = [(low, 0x10), (low, 0x30)]
    ids = [0, 1]
    c = C.case(oracle, k, n, pairs, ids, ns, gs, "arbitrary")
    h = Held(c, 0, rotating)
    start = Held(C.Case(c.frags, c.frags), 0, rotating)
    hfrags = [f.copy() for f in c.frags]
    gp = dev_bytes(ids)
    masks, targets = [low, low], [0x10, 0x30]

    def rejected(text, call, *args):
        with pytest.raises(OSError) as e:
            call(*args)
        assert e.value.errno == errno.EINVAL, e.value
        assert text in ec.lib.ec_method_last_error().decode(), ec.lib.ec_method_last_error()

    with ec.ECMatrixList(k, n) as L:
        d = L.heal_mixed_device
        f = start.frags
        # host pointers given to the device entry point, all or some
        rejected("not memory of the device", d, 0, None, ns, gs, gp, masks, targets, hfrags)
        rejected("not memory of the device", d, 0, None, ns, gs, gp, masks, targets,
                 f[:5] + hfrags[5:])
        rejected("not memory of the device", d, 0, None, ns, gs, np.array(ids, np.uint8), masks,
                 targets, f)
        # device pointers given to the host entry point, all or some
        rejected("device memory", L.heal_mixed, ns, gs, masks, targets, f)
        rejected("device memory", L.heal_mixed, ns, gs, masks, targets, hfrags[:2] + f[2:])
        for bad in (0, 1, 2, 3, 6):
            rejected("group_stripes", d, 0, None, ns, bad, gp, masks, targets, f)
        for bad in (0x7, 0x1F, 0x4F, 0):
            rejected("a mask is not k bricks", d, 0, None, ns, gs, gp, [low, bad], [0x10, 0], f)
        rejected("outside the volume", d, 0, None, ns, gs, gp, masks, [0x10, 0x40], f)
        rejected("overlaps its mask", d, 0, None, ns, gs, gp, masks, [0x10, 0x21], f)
        rejected("is NULL", d, 0, None, ns, gs, gp, masks, targets, f[:5] + [None])
        rejected("is NULL", d, 0, None, ns, gs, gp, masks, targets, [None] + f[1:])
        rejected("no patterns", d, 0, None, ns, gs, gp, [], [], f)
        rejected("array is NULL", d, 0, None, ns, gs, None, masks, targets, f)
        # the checks come before the zero-stripes return
        rejected("overlaps its mask", d, 0, None, 0, gs, gp, masks, [0x10, 0x21], f)
        ec.sync_device(0)
        start.check("rejected calls")
        assert all(np.array_equal(a, b) for a, b in zip(hfrags, c.frags))
        # and the call they all fall short of
        assert L.heal_mixed_device(0, None, ns, gs, gp, masks, targets, h.frags) == 0
        ec.sync_device(0)
    h.check("valid")
