"""The host variant of ec_method_heal_checked2 under ASan + UBSan: the host
layer built around the device-layer stub, as tests/test_sanitizers.py builds
it, driving tests/c/heal_checked2_check.c, a stand-alone program whose buffers
have exactly the sizes the contract names and whose shapes sit on the edges of
the steps the call shares with its siblings (one window of the check pass, a
full one, a one-stripe tail; runs of one stripe that name different sets).
CPU only; the build takes seconds."""
import os
import subprocess

from test_sanitizers import build


def test_heal_checked2_host_variant_under_asan_ubsan(tmp_path):
    exe = build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                main="heal_checked2_check")
    env = dict(os.environ, EC_MI355X_QUIET="1", ASAN_OPTIONS="detect_leaks=1")
    env.pop("EC_GPU_ALWAYS", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout + r.stderr)[-4000:]
