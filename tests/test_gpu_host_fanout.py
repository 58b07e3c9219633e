"""Runs the host mirror's replica fan-out test (stl.fusion_amd/host/test_fanout.cpp) on the GPU: the registry
with ComputedRegistry::DeviceFanout on (subscriptions in the engine, per-peer lists from fgi_last_wave_fanout /
fgi_fanout_ids) delivers the same call ids per peer, in the same order, in the same batches, each exactly once,
as the registry with it off (the host gather) — for one scope over all hubs with the ids as a list and as a
bitmap, for a reentrant peer sink that runs a wave of its own, and for an asynchronous wave's completion.

The binary links the in-tree engine (stl.fusion_amd/lib/libfgi.so) through the host mirror
(host/build/libfusion.so); both are built by __graft_entry__.build() / `make -C stl.fusion_amd/host`.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stl.fusion_amd", "host")
BIN = os.path.join(HOST, "build", "test_fanout")


def test_fanout_test_builds_and_links():
    """CPU: test_fanout compiles against the mirror and links libfgi.so (no GPU call)."""
    subprocess.run(["make", "-s", "-C", HOST], check=True, timeout=300)
    assert os.path.exists(BIN)
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True, check=True).stdout
    assert "libfgi.so" in out and "libfusion.so" in out and "not found" not in out


@pytest.mark.gpu
def test_device_fanout_matches_host_fanout(gpu_available):
    subprocess.run(["make", "-s", "-C", HOST], check=True, timeout=300)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and r.stdout.count("same batches: yes") == 4
