"""The host variant of the mixed heal under ASan + UBSan: the host layer built
around the device-layer stub, as tests/test_sanitizers.py builds it (the link
is the same: the new device entry is a weak reference), driving
tests/c/heal_mixed_check.c, a stand-alone program whose fragments are exactly
nstripes * 512 bytes, whose mask and target arrays have exactly one entry per
group and whose unused bricks are NULL.  CPU only; the build takes seconds."""
import os
import subprocess

from test_sanitizers import build


def test_heal_mixed_host_variant_under_asan_ubsan(tmp_path):
    exe = build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                main="heal_mixed_check")
    env = dict(os.environ, EC_MI355X_QUIET="1", ASAN_OPTIONS="detect_leaks=1")
    env.pop("EC_GPU_ALWAYS", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout + r.stderr)[-4000:]
