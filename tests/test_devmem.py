"""The HIP-free part of csrc/devmem.h as plain C++ under the sanitizers (tests/devmem_host.cpp): the one growth rule of the grow-only buffers against the formula
the stages wrote out by hand, and the per-(device, stream) scratch registry -- the same object for the same key, one entry released exactly once, creation and
release from sixteen threads.  The registry and the buffers run under the device tests of test_scratch_lifecycle_gpu.py."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tag: str, flags: list) -> str:
    out = os.path.join(HERE, "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "devmem_host_" + tag)
    src = [os.path.join(HERE, "devmem_host.cpp"), os.path.join(HERE, "..", "bwa-mem_gpu_amd", "csrc", "devmem.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-fno-omit-frame-pointer"] + flags + [src[0], "-o", exe])
    return exe


@pytest.mark.parametrize("tag,flags", [("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), ("tsan", ["-fsanitize=thread"])])
def test_devmem_under_sanitizers(tag, flags):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([_build(tag, flags)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and r.stdout.strip() == b"ok" and "Sanitizer" not in err and "runtime error" not in err, "the sanitizers (or the driver) reported:\n" + err[-4000:]
