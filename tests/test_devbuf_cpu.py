"""brx::DevBuf / brx::DevScratch on the host: tests/devbuf_host.cpp built with the address and undefined-behaviour
sanitizers and run as a child process.  The program replaces the block pool by malloc / free and checks growth, reuse
within capacity, the failed growth, moves and hand-overs, and that nothing leaks."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_devbuf_host_program(tmp_path):
    exe = tmp_path / "devbuf_host"
    build = subprocess.run(
        ["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-Wall", "-Wextra",
         "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, os.path.join(HERE, "devbuf_host.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "0 live blocks, 0 failed checks" in run.stdout
