"""Runs the host mirror's state-view tests (stl.fusion_amd/host/test_view.cpp) on the GPU: every
Computed's Flags() / State() / IsConsistent() read the engine's host-memory state view
(fgi_state_view_open) and equal fgi_get_state after every wave; with no wave pending, state reads and
TryUseExisting hits make no engine call (ComputedRegistry::EngineCalls); the hit throughput on one thread
is printed, with no threshold.

The binary links the in-tree engine (stl.fusion_amd/lib/libfgi.so) through the host mirror
(host/build/libfusion.so); both are built by __graft_entry__.build() / `make -C stl.fusion_amd/host`.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stl.fusion_amd", "host")
BIN = os.path.join(HOST, "build", "test_view")


def test_view_test_builds_and_links():
    """CPU: test_view compiles against the mirror and links libfgi.so (no GPU call)."""
    subprocess.run(["make", "-s", "-C", HOST], check=True, timeout=300)
    assert os.path.exists(BIN)
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, check=True).stdout
    assert "libfgi.so" in out and "libfusion.so" in out and "not found" not in out


@pytest.mark.gpu
def test_host_view_scenarios(gpu_available):
    subprocess.run(["make", "-s", "-C", HOST], check=True, timeout=300)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and "hit throughput" in r.stdout
