"""The host variant of the extent heal under ASan + UBSan: the host layer built
around the device-layer stub, as tests/test_sanitizers.py builds it (the new
device entry is a weak reference), driving tests/c/heal_extents_check.c, a
stand-alone program whose fragments are exactly their extent's nstripes * 512
bytes, whose table is exactly nextents records and whose unnamed bricks have no
buffer.  CPU only; the build takes seconds."""
import os
import subprocess

from test_sanitizers import build


def test_heal_extents_host_variant_under_asan_ubsan(tmp_path):
    exe = build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                main="heal_extents_check")
    env = dict(os.environ, EC_MI355X_QUIET="1", ASAN_OPTIONS="detect_leaks=1")
    env.pop("EC_GPU_ALWAYS", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout + r.stderr)[-4000:]
