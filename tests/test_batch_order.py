"""The order of a file run's batches (npore_amd/csrc/batch_order.hpp) under the thread sanitizer, without a GPU.

tests/model/batch_order_tsan.cpp drives the skeleton with fake stages: batch counts around the slot count, with and
without a serial source, and one injected failure per run in every stage -- returned or thrown -- among them a collect and
a write failure with more than n_slots batches behind them, which the pipeline used to lose.  The program is built here,
stand-alone, and run as a child process: nothing is loaded into this interpreter.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_order_under_the_thread_sanitizer(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    san = ["-fsanitize=thread", "-pthread"]
    probe = subprocess.run(["g++"] + san + ["-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the thread sanitizer's runtime is missing")
    src = os.path.join(REPO, "tests", "model", "batch_order_tsan.cpp")
    exe = str(tmp_path / "batch_order_tsan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + san + ["-o", exe, src])
    # (a deadlock of the skeleton fails here instead of hanging: 60 s for a few thousand fake batches of microseconds each)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66"))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert "ThreadSanitizer" not in out.stderr and lines[-1].endswith("all expectations held") and all(l.startswith("ok ") for l in lines[:-1])
    # the cases that name the hole: a collect and a write failure at batch 2 of 19, more than n_slots batches behind it
    for stage in ("collect", "write"):
        assert sum(f"n=19 serial={s} fail={stage:<7}@ 2 how=0" in l and "written=2" in l for l in lines for s in (0, 1)) == 6, stage
