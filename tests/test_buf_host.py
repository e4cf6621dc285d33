"""The owning buffer of the context's allocations (csrc/cpm_buf.h) without a GPU: tests/buf_host.cc, a stand-alone host program with a
counting allocator that fails on request, built with the address and undefined-behaviour sanitizers and run as it is."""
import os
import subprocess

from conftest import ROOT


def test_owning_buffer_under_a_counting_allocator_with_sanitizers(tmp_path):
    exe = str(tmp_path / "buf_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "carparkingmaps_amd", "csrc"),
                           os.path.join(ROOT, "tests", "buf_host.cc"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buf_host: ok" in run.stdout
