"""The one builder of the host harnesses (tests/host/*.cpp): g++ with csrc/ and tests/host/ on the include
path, so a harness reaches a core header (DESIGN.md "Core headers") with #include and its stand-ins with
device_standins.hpp.  Every harness is a stand-alone program and runs as its own process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "livox-motion-compensation-sim_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
SAN = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

# every header whose text both the device and a harness compile; tests/test_core_headers.py holds each to
# compiling on its own behind the stand-ins
CORE_HEADERS = ("voxel_core.hpp", "normals_core.hpp", "relfold.hpp", "time_rule.hpp", "scan_core.hpp", "raymarch_core.hpp",
                "fmt6_core.hpp", "pcd_line_core.hpp", "csim_text_core.hpp", "ingest_token_core.hpp", "las_core.hpp",
                "unit_order.hpp")


def _command(harness, flags, sanitize):
    return ["g++", "-std=c++17", *(SAN if sanitize else ("-O2",)), *flags, "-I", CSRC, "-I", HOST, os.path.join(HOST, str(harness))]


def build(tmp, harness, *flags, sanitize=False):
    """tests/host/<harness> (or an absolute path) -> an executable under tmp: -O2, or the sanitizer set; flags
    may name further sources of csrc/."""
    exe = tmp / (os.path.splitext(os.path.basename(str(harness)))[0] + ("_san" if sanitize else ""))
    r = subprocess.run([*_command(harness, flags, sanitize), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def preprocessed(harness, *flags, sanitize=False) -> str:
    """The harness as the compiler sees it (g++ -E): what a mutation test alters and builds again as a .ii file."""
    r = subprocess.run([*_command(harness, flags, sanitize), "-E"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def run(exe, *args, timeout=300):
    """exe as its own process: exit status 0, and no sanitizer report (AddressSanitizer, LeakSanitizer) or UBSan
    runtime error on stderr."""
    r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=timeout, env=ENV)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r
