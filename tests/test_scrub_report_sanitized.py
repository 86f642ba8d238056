"""The host variant of ec_method_scrub_report under ASan + UBSan: the host layer
built around the device-layer stub, as tests/test_sanitizers.py builds it,
driving tests/c/scrub_report_check.c, a stand-alone program whose loc, idx, val
and report are heap blocks of exactly the sizes the contract names.  The same
build is one without the device layer (the stub has no ecd_scrub_report), so
it also shows the device entry point's -ENODEV.  CPU only; the one build takes
seconds."""
import os
import subprocess

import pytest

from test_sanitizers import build


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("scrub_report"),
                 ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                 main="scrub_report_check")


def run(exe, *args):
    env = dict(os.environ, EC_MI355X_QUIET="1", ASAN_OPTIONS="detect_leaks=1")
    env.pop("EC_GPU_ALWAYS", None)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)


def test_scrub_report_host_variant_under_asan_ubsan(exe):
    r = run(exe)
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout + r.stderr)[-4000:]


def test_device_entry_point_without_the_device_layer_is_enodev(exe):
    """The weak reference to ecd_scrub_report is NULL in this build: an
    otherwise valid device call answers -ENODEV and writes nothing, after the
    argument checks and the zero-stripes return."""
    r = run(exe, "enodev")
    assert r.returncode == 0 and "enodev ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
