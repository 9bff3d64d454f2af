"""csrc/device_memory.h on the host: tests/cpp/device_memory_main.cpp fakes the four HIP allocator calls over malloc and checks
the owners' rules (scope, moves, ensure's growth and retry, exact, the drain of an abandoned capacity change) under
AddressSanitizer and UBSan.  A stand-alone program: nothing of it is loaded into this interpreter."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_the_owners_free_move_grow_and_drain_under_the_sanitizers(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "device_memory_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
                    f"-I{ROOT / 'mlvectordb_amd' / 'csrc'}", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "device_memory_main.cpp"), "-o", str(exe)],
                   capture_output=True, text=True, check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "device_memory ok" and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr


def test_the_header_stands_alone():
    """It includes the HIP runtime API and standard headers only, and the Makefile rebuilds on its changes."""
    text = (ROOT / "mlvectordb_amd" / "csrc" / "device_memory.h").read_text()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes[0] == "<hip/hip_runtime_api.h>" and all(i.startswith("<") and "/" not in i for i in includes[1:]), includes
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    hdrs = make[make.index("HDRS ="):make.index("# the filter scan's body")]
    assert "device_memory.h" in hdrs.split()
