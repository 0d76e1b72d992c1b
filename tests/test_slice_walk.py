"""The slice walk of sorted_file_io.h (walk_slice) and its open helpers, checked by a stand-alone program under the address and
undefined-behaviour sanitizers: tests/host/slice_walk_main.cpp compares the walk with the rule written out as one loop, over
block sizes of 1, 2, 3 and above the file, starts at 0 and mid-file, empty slices, slices that end on a block boundary or with
the file, thresholds below and above every key, flagged words and a caller that stops the walk. No GPU is needed."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_slice_walk_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/slice_walk_main.cpp"
    exe = tmp_path / "slice_walk_main"
    subprocess.run(
        [cxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-static-libasan", "-static-libubsan",  # (the runtimes inside the executable: it is run as it is)
         "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + os.path.join(ROOT, "kmersgwas_amd", "csrc"),
         os.path.join(ROOT, "tests", "host", "slice_walk_main.cpp"), "-o", str(exe)],
        check=True)
    work = tmp_path / "files"
    work.mkdir()
    r = subprocess.run([str(exe), str(work)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "slice walk OK"
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
