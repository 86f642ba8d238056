"""ec_method_heal_mixed_device over the whole table of
tests/_heal_mixed_sweep.py: ec_heal_mixed_n with the run-time k at every value
of each K bucket (1...4, 5...8, 9...16), target counts below, at and above the
block's wave count (a second and a third trip of the row loop), one to four
target words with targets on both sides of every word, a coefficient row of
three words with the fourth unused, bricks up to 30 as sources and targets,
and pattern lists of 21 to 69 words a pattern on both sides of the kernel's
argument space.

The expected fragments come from the oracle alone.  The calls of one (k, n)
are queued on one side stream by run_cases of tests/test_gpu_heal_mixed.py:
the n fragments of a call are carved from one tensor, each between two 2 KiB
guards of 0xA5 and at a byte offset that rotates through 0 .. 15, and the whole
tensor is compared afterwards, so a byte written anywhere but in a target chunk
of its group fails.  The calls of k = 3, 7 and 11 run again with every fragment
1 byte off, and the whole table in a child process with non-temporal staging
forced (EC_MI355X_LDSNT=1, read when the library loads) on 16-byte aligned
fragments.
"""
import os
import subprocess
import sys

import pytest

import _heal_mixed_sweep as W
import test_gpu_heal_mixed as T

pytestmark = pytest.mark.gpu

ROOT = T.ROOT


@pytest.fixture(scope="module")
def ec():
    import glusterfs_amd.ec_method as m
    return m


def geoms(calls):
    """The (k, n) of the calls, in their order."""
    return list(dict.fromkeys((c.k, c.n) for c in calls))


def geom_id(g):
    return "%d+%d" % (g[0], g[1] - g[0])


def run(ec, oracle, calls, geom, family, offset):
    """The calls of one (k, n), on one stream with one sync."""
    k, n = geom
    mine = [c for c in calls if (c.k, c.n) == geom]
    assert mine
    T.run_cases(ec, W.oracle_for(oracle, k, n), k, n,
                [(c.pairs, c.ids, c.ns, c.gs, family) for c in mine], offset)


@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("geom", geoms(W.SWEEP), ids=geom_id)
def test_heal_mixed_sweep_device(ec, oracle, geom, family):
    run(ec, oracle, W.SWEEP, geom, family, T.rotating)


@pytest.mark.parametrize("geom", geoms(W.offset_calls()), ids=geom_id)
def test_heal_mixed_sweep_device_fragments_one_byte_off(ec, oracle, geom):
    run(ec, oracle, W.offset_calls(), geom, "arbitrary", T.one_off)


CHILD = r"""
import sys
sys.path[:0] = ["tests", "oracle"]
import glusterfs_amd.ec_method as ec
import oracle as O
import _heal_mixed_sweep as W
import test_gpu_heal_mixed as T
import test_gpu_heal_mixed_sweep as S
O.lib()
failed = 0
for g in S.geoms(W.SWEEP):
    try:
        S.run(ec, O, W.SWEEP, g, "arbitrary", T.aligned)
        print("geom %s ok" % S.geom_id(g), flush=True)
    except AssertionError as e:
        failed = 1
        print("geom %s FAILED %s" % (S.geom_id(g), str(e)[:300].replace("\n", " ")), flush=True)
sys.exit(failed)
"""


def test_heal_mixed_sweep_nontemporal():
    """The kLdsDmaNT copies of the six instantiations: the whole table on
    aligned fragments, one result line per (k, n)."""
    env = dict(os.environ, EC_MI355X_QUIET="1", EC_MI355X_LDSNT="1")
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=170)
    lines = r.stdout.splitlines()
    for g in geoms(W.SWEEP):
        assert "geom %s ok" % geom_id(g) in lines, \
            (geom_id(g), [x for x in lines if "FAILED" in x][:4], r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
