"""The host form of the HNSW graph (the-algorithm_amd/csrc/hnsw_graph_host.h) under the address and undefined-behaviour
sanitizers: tests/hnsw_graph_host_check.cpp, a stand-alone program, round-trips random small graphs through it and feeds it
malformed ones.  Host code only: nothing here touches a device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_host_round_trip_and_refusals_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hnsw_graph_host_check")
    # (the runtimes linked statically: the program then starts whatever else the process environment loads first)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "the-algorithm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "hnsw_graph_host_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    assert run.stdout.strip().endswith("ok: 400 graphs, 0 failures"), run.stdout[-4000:]
