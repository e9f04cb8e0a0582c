"""Device-resident Arrow batches through the gandiva:: C++ API (gandiva/device_memory.h: HipDevice, HipMemoryManager),
exercised by gandiva_amd/cxx/tests/test_device_cxx.cc the way a C++ caller would use them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "gandiva_amd", "cxx")
BIN = os.path.join(CXX, "tests", "test_device_cxx")


def _build():
    subprocess.run(["make", "-C", CXX, "all", "test_cxx"], stdout=subprocess.DEVNULL, check=True, timeout=900)


def test_hip_device_and_manager_host_only():
    """What needs no allocation holds with or without a GPU: one Equals device per number, kROCM, not a CPU device,
    a stable default_memory_manager() whose device() is the device."""
    _build()
    out = subprocess.run([BIN, "--host-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK (host-only)" in out.stdout


@pytest.mark.gpu
def test_device_resident_batches_through_the_cxx_api():
    """One process: the reference KATs, host against device evaluation of C1 / C2 / C3 / C5-shaped trees and a raising
    one at 1 .. 70001 rows with and without validity buffers, slices, caller-allocated outputs from ReserveSet, the
    three selection modes, the selection-mode projector and FilterProject, the pool, two devices, device restore."""
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stdout.strip().endswith("OK")
