"""The restart-segment entry points read untrusted bytes: a stand-alone program (tests/jpeg_restart_driver.cpp, its own
main) is built with the host compiler and -fsanitize=address,undefined, linked with csrc/jpeg_host.cpp ONLY, and run as a
subprocess over restart-marked, plain and optimised files written to a temp directory -- each intact, with 200 seeded
single-byte mutations inside its scan and at every truncation length up to 600 bytes -- through ds_jpeg_scan,
ds_jpeg_restart_transcode and ds_jpeg_entropy_decode_segments_host.  It must exit 0 with no sanitizer report; the driver
also holds the segment decoder to ds_jpeg_entropy_decode's verdict and coefficients on every damaged copy.  Nothing loaded
into Python is sanitised."""
import os
import subprocess

from test_jpeg_cpu import encode, pixels
from test_jpeg_host_sanitized_cpu import _compiler
from test_jpeg_restart_cpu import mutation_files, restart_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitised_segment_entry_points_survive_mutated_and_truncated_streams(tmp_path):
    exe = str(tmp_path / "jpeg_restart_driver")
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
                            os.path.join(ROOT, "tests", "jpeg_restart_driver.cpp"),
                            os.path.join(ROOT, "tumblr_emotions_amd", "csrc", "jpeg_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    datas = [d for _, d in restart_grid()[::3]] + mutation_files()
    for sub in (0, 2, "L"):                    # no restart markers; optimised tables (the transcoder replaces some)
        datas += [encode(pixels(33, 17, "gradient"), sub, 30, optimize=True), encode(pixels(17, 33, "noise"), sub, 100)]
    paths = []
    for i, data in enumerate(datas):
        paths.append(str(tmp_path / ("%03d.jpg" % i)))
        with open(paths[-1], "wb") as f:
            f.write(data)
    listing = str(tmp_path / "files.txt")
    with open(listing, "w") as f:
        f.write("\n".join(paths) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    run = subprocess.run([exe, listing, "200", "600", "20261018"], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-6000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-6000:]
    files, decoded, flagged, rejected, transcoded = [int(x) for x in run.stdout.split()[1::2]]
    assert files == len(paths) and decoded >= files and flagged > 0 and rejected > 0 and transcoded >= 2 * files
    assert decoded + flagged + rejected == files + sum(200 + min(601, len(d)) for d in datas)
