"""csrc/ctx_pool.h on the host, through tests/csrc/ctx_pool_check.cpp (a program of its own: nothing is loaded into Python) with a mock
context that counts its init / release / drain calls and asserts that nobody else is inside the same context.  The program is built twice
where the compiler's sanitizer runtimes work, once with the thread sanitizer and once with the address and undefined-behaviour
sanitizers, and plainly otherwise; every check runs under every build."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "ctx_pool_check.cpp")
INC = os.path.join(ROOT, "mpibwa_amd", "csrc")
SANITIZERS = ["thread", "address,undefined"]


def _works(d, flags):
    """does a program built with these flags build and run here?"""
    exe = str(d / "probe")
    b = subprocess.run(["g++", "-pthread", "-x", "c++", "-", "-o", exe] + flags, input="int main(){}", capture_output=True, text=True)
    return b.returncode == 0 and subprocess.run([exe], capture_output=True, timeout=60).returncode == 0


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctx_pool_host")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", INC, SRC]
    built = {}
    for san in SANITIZERS:
        flags = ["-fsanitize=" + san, "-fno-sanitize-recover=all"]
        if _works(d, flags):
            built[san] = str(d / ("check_" + san.split(",")[0]))
            subprocess.run(base + flags + ["-o", built[san]], check=True)
    if not built:
        built["plain"] = str(d / "check_plain")
        subprocess.run(base + ["-o", built["plain"]], check=True)
    return built, d


def _check(programs, what):
    for kind, exe in programs[0].items():
        r = subprocess.run([exe, what], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == "ok %s\n" % what, (kind, r.returncode, r.stdout, r.stderr[-2000:])


def test_more_threads_than_contexts_nobody_shares_one_and_everybody_is_served(programs):
    _check(programs, "crowd")


def test_a_lease_prefers_a_context_that_has_its_buffers(programs):
    _check(programs, "prefer")


def test_release_idle_beside_leases_never_takes_a_held_context_and_leaves_none_half_done(programs):
    _check(programs, "release")


def test_two_first_leases_initialise_at_the_same_time(programs):
    _check(programs, "init")


def test_sanitizers_were_used_where_they_work(programs):
    built, d = programs
    want = [s for s in SANITIZERS if _works(d, ["-fsanitize=" + s, "-fno-sanitize-recover=all"])]
    assert sorted(built) == sorted(want or ["plain"])
