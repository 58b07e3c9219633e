"""Runs the host mirror's auto-invalidation test (stl.fusion_amd/host/test_auto.cpp) on the GPU: every scenario on
a registry with ComputedRegistry::DeviceTimers on (the timers in the engine: fgi_timers_auto_open,
fgi_timers_set_auto_delay, fgi_set_output_ex) and on one with it off (the registry's own entries, keep-the-earlier),
driven by the same fake clock. The two agree on every handler invocation, on every node's state after every step
and on what RunDueTimers returns; among the scenarios a transient-error node retries after its delay while a
sibling with AutoInvalidationDelay = max() stays.

The binary links the in-tree engine (stl.fusion_amd/lib/libfgi.so) through the host mirror
(host/build/libfusion.so); both are built by __graft_entry__.build() / `make -C stl.fusion_amd/host`.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stl.fusion_amd", "host")
BIN = os.path.join(HOST, "build", "test_auto")


def test_auto_test_builds_and_links():
    """CPU: test_auto compiles against the mirror and links libfgi.so (no GPU call)."""
    subprocess.run(["make", "-s", "-C", HOST], check=True, timeout=300)
    assert os.path.exists(BIN)
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, check=True).stdout
    assert "libfgi.so" in out and "libfusion.so" in out and "not found" not in out


@pytest.mark.gpu
def test_device_auto_invalidation_matches_host_timers(gpu_available):
    subprocess.run(["make", "-s", "-C", HOST], check=True, timeout=300)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and r.stdout.count("trace lines agree") == 7
    assert "transient_retry:" in r.stdout
