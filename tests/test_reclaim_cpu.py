"""The two mechanisms under the runtime's pools and deferred frees (gandiva_amd/csrc/gdv_reclaim.h: FreeList, DeferredQueue)
as a stand-alone program without HIP (tests/cxx/reclaim_test.cc): built plain and under ThreadSanitizer, each build run as a
child process of its own.  Nothing is loaded into this interpreter.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cxx", "reclaim_test.cc")
INC = os.path.join(HERE, "..", "gandiva_amd", "csrc")
OUT = os.path.join(INC, "build")
BASE = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread"]


@pytest.mark.parametrize("name,extra", [("plain", []), ("tsan", ["-fsanitize=thread", "-g"])])
def test_free_list_and_deferred_queue_keep_one_owner_per_entry(name, extra):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "reclaim_test_" + name)
    subprocess.check_call(BASE + extra + ["-I", INC, SRC, "-o", exe])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}\n{run.stderr}"
    assert "WARNING: ThreadSanitizer" not in run.stderr, run.stderr
    assert "reclaim_test: ok" in run.stdout
