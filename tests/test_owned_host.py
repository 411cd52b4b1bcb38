"""The owning handles (csrc/device/owned.hpp) where no device is visible: tests/host_harness/owned_check.cpp, a program of its own built with
hipcc, finds every create failing cleanly (hipErrorNoDevice) and checks what the handles promise then — empty after a failed create, the four
live counts at zero, moved-from handles empty, reset() twice harmless, a borrowed stream never released.  What they do WITH a device is
tests/test_gpu_ctx_lifetime.py's."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_handles_without_a_device(fg, tmp_path):
    if _has_gpu():
        pytest.skip("a GPU is visible: the creates would succeed")
    exe = str(tmp_path / "owned_check")
    subprocess.run([fg.build._hipcc(), "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror",
                    os.path.join(REPO, "tests", "host_harness", "owned_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "OK", p.stdout + p.stderr


def test_the_live_counts_are_readable_without_a_device(fg):
    if _has_gpu():
        pytest.skip("a GPU is visible: other tests' objects may be alive")
    assert fg.live_resources() == (0, 0, 0, 0)
