"""The host JPEG decoder reads untrusted bytes: a stand-alone program (tests/jpeg_host_driver.cpp, its own main) is built
with the host compiler and -fsanitize=address,undefined, linked with csrc/jpeg_host.cpp ONLY, and run as a subprocess over the
grid images of test_jpeg_cpu.py written to a temp directory -- each intact, with 200 seeded single-byte mutations and at
every truncation length up to 600 bytes.  It must exit 0 with no sanitizer report: corrupt input yields an error code or
"unsupported", never a crash.  Nothing loaded into Python is sanitised.  (The driver applies the mutations and truncations
to the files in memory, from the seed on its command line: 324 x 801 damaged copies are not worth writing to disk.)"""
import os
import shutil
import subprocess

import pytest

from test_jpeg_cpu import grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    pytest.fail("no host C++ compiler (c++ / g++ / clang++) to build the sanitised driver with")


def test_sanitised_decoder_survives_mutated_and_truncated_streams(tmp_path):
    exe = str(tmp_path / "jpeg_host_driver")
    cxx = _compiler()
    # the sanitizer runtime linked INTO the program (gcc's default is the shared one), so that nothing has to be preloaded
    static = []
    for flags in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):           # gcc's spelling, clang's
        probe = subprocess.run([cxx, *flags, "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                               input="int main() { return 0; }\n", capture_output=True, text=True)
        if probe.returncode == 0:
            static = flags
            break
    build = subprocess.run([cxx, "-std=c++17", *static, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "tumblr_emotions_amd", "csrc"),
                            os.path.join(ROOT, "tests", "jpeg_host_driver.cpp"),
                            os.path.join(ROOT, "tumblr_emotions_amd", "csrc", "jpeg_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    paths = []
    for i, (label, data, _) in enumerate(grid()):
        paths.append(str(tmp_path / ("%03d-%s.jpg" % (i, label))))
        with open(paths[-1], "wb") as f:
            f.write(data)
    listing = str(tmp_path / "files.txt")
    with open(listing, "w") as f:
        f.write("\n".join(paths) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    run = subprocess.run([exe, listing, "200", "600", "20261018"], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-6000:]
    files, decoded, rejected = [int(x) for x in run.stdout.split()[1::2]]
    assert files == len(paths) and decoded >= files and rejected > 0
    assert decoded + rejected >= files * (1 + 200)
