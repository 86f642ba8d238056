"""The host-buffer family on the GPU (tests/_host_sweep.py): every zero-copy
kernel ecdk_combine_host can launch, ec_encode_vander_zc, and the batching of
ec_device.hip, through encode_batch, encode_rows, decode_batch, decode_mixed,
heal and writev_encode on pinned, pageable, misaligned, registered and mixed
host buffers, against the oracle.

After every call: the bytes, 4 KiB of guard on both sides of every output, the
inputs with their flanks, stats()["cpu_fallbacks"] unchanged and gpu_calls
advanced by one -- a launch the runtime refuses is recoded on the CPU engine
with the right bytes, and only the counters show it.  A failure names the call,
the kernels the restated predicates say it launched, the buffer kind and the
first wrong offset.

Every call runs in a child process (tests/_host_sweep_run.py, EC_GPU_ALWAYS=1),
so the 47,000 calls, their pinned and registered arenas and the staging slots
they grow share no process with any other test.  test_host_sweep[geometry]
reads its geometry's line from one child that runs the whole table with the
defaults; a child that dies leaves the later geometries without a line, and
they fail.  The settings read once per process run in children of their own:
EC_MI355X_ZCDB=0 (ec_combine_zc<K>, one tile per
block, for every K, single and MIXED), EC_PIPE_BATCH_MB=1 (the batch edges of
clause H12, also with one copy thread) and two "devices" on one GPU
(partition's ranges with align = group, fewer units than devices, one stripe).
"""
import os
import subprocess
import sys

import pytest

import _host_sweep as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_child(mode, **env):
    e = dict(os.environ, EC_MI355X_QUIET="1", EC_GPU_ALWAYS="1", **env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_host_sweep_run.py"), mode],
                          cwd=ROOT, env=e, capture_output=True, text=True, timeout=170)


@pytest.fixture(scope="module")
def table():
    """The table's default-process calls, all geometries, in one child."""
    return run_child("table")


@pytest.mark.parametrize("geom", H.GEOMS, ids=H.geom_id)
def test_host_sweep(table, geom):
    gid = H.geom_id(geom)
    want = "GEOM %s calls=%d failures=0" % (gid, len(H.cases(geom)))
    fails = [l for l in table.stdout.splitlines() if l.startswith("FAIL %s " % gid)]
    assert want in table.stdout.splitlines(), \
        "%d failures:\n%s\n%s" % (len(fails), "\n".join(fails[:20]), table.stderr[-1500:])


def child(mode, **env):
    r = run_child(mode, **env)
    assert r.returncode == 0 and "SWEEP-OK" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
    return r.stdout


def test_host_sweep_one_tile_per_block():
    child("zcdb0", EC_MI355X_ZCDB="0")


@pytest.mark.parametrize("threads", [None, "1"], ids=["default", "one-copy-thread"])
def test_host_sweep_small_batches(threads):
    child("batches", EC_PIPE_BATCH_MB="1", **({"EC_COPY_THREADS": threads} if threads else {}))


def test_host_sweep_two_devices():
    child("split", EC_PIPE_BATCH_MB="1", EC_MI355X_HOST_DEVICES="0,0", EC_MI355X_TEST_SPLIT="1",
          EC_SPLIT_MIN_MB="0")
