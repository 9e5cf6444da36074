"""The one heap of the HNSW code (the-algorithm_amd/csrc/hnsw_queue.h) under the address and undefined-behaviour sanitizers:
tests/hnsw_queue_host_check.cpp, a stand-alone program, holds every host instantiation of the template -- both entry types,
both orders, plain and split stores -- against java.util.PriorityQueue written out, on tie-heavy offer / poll sequences.
Host code only: nothing here touches a device."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_heap_is_java_priority_queue_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hnsw_queue_host_check")
    # (the runtimes linked statically: the program then starts whatever else the process environment loads first)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-Wall", "-Wextra", "-Wno-unused-function", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "the-algorithm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "hnsw_queue_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    last = re.fullmatch(r"ok: 100 sequences, (\d+) operations, 0 failures", run.stdout.strip().splitlines()[-1])
    assert last, run.stdout[-4000:]
    assert int(last.group(1)) >= 100 * 1400  # every sequence runs its 1400 operations and then drains
