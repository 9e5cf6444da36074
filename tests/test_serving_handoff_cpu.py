"""The host side of the serving threads -- the completion hand-off, the callers-inside guard and the guarded loop body of
the-algorithm_amd/csrc/handoff.h, and the micro-batching queue of request_queue.h with a fake runner in place of the GPU call
-- in tests/serving_handoff_host_check.cpp, a stand-alone program built three ways: under the thread sanitizer, under the
address and undefined-behaviour sanitizers, and plain with an operator new that fails the k-th allocation of a submit.  Host
code only: nothing here touches a device, and nothing of it is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread", *flags, "-I", os.path.join(ROOT, "the-algorithm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "serving_handoff_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("ok: ") and last.endswith(", 0 failures"), run.stdout[-4000:]
    return run.stdout


def test_hand_off_and_queue_under_the_thread_sanitizer(tmp_path):
    # (the runtimes linked statically: the program then starts whatever else the process environment loads first)
    _build_and_run(tmp_path, "serving_handoff_tsan", ["-fsanitize=thread", "-static-libtsan"])


def test_hand_off_and_queue_under_the_address_and_undefined_sanitizers(tmp_path):
    _build_and_run(tmp_path, "serving_handoff_asan",
                   ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])


def test_a_submit_that_finds_no_memory_leaves_the_queue_as_it_was(tmp_path):
    # no sanitizer here: a replaced operator new does not link against the static address-sanitizer runtime
    out = _build_and_run(tmp_path, "serving_handoff_faults", ["-DALLOC_FAULTS"])
    assert "failing allocation sites k=0" in out and "none under the lock" in out, out[-4000:]
