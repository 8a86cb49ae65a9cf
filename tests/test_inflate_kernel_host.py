"""bgzf_inflate_kernel's arithmetic on the host (csrc/inflate_util.h through tests/csrc/inflate_host_check.cpp, a program of its own:
nothing is loaded into Python): every block of every family gives zlib's text, every malformed block is refused, and the blocks round
a malformed one are not.  The program is built with the address and undefined-behaviour sanitizers where the compiler has their
runtimes (payload, text and window are heap blocks of their exact sizes), without them otherwise."""
import os
import struct
import subprocess
import zlib

import pytest

import bgzf_in_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "inflate_host_check.cpp")
INC = os.path.join(ROOT, "mpibwa_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_host")
    exe = str(d / "inflate_host_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", INC, SRC, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.run(base, check=True)
    return exe, san.returncode == 0, d


def _fnv(t):
    h = 2166136261
    for b in t:
        h = ((h ^ b) * 16777619) & 0xffffffff
    return h


def _run(program, blks, name):
    exe, _, d = program
    path = str(d / name)
    with open(path, "wb") as f:
        for b in blks:
            f.write(struct.pack("<I", len(b)) + b)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(blks)
    return [(int(a), int(h, 16), int(n)) for a, h, n in rows]


def test_every_family_gives_zlibs_text(program):
    names, blks = [], []
    for name, (data, _) in cases.families().items():
        for _, blk in cases.split(data):
            names.append(name)
            blks.append(blk)
    got = _run(program, blks, "families.bin")
    for name, blk, (status, h, n) in zip(names, blks, got):
        want = zlib.decompress(blk[18:-8], -15)
        assert (status, n, h) == (0, len(want), _fnv(want)), name


def test_every_malformed_block_is_refused_and_its_neighbours_are_not(program):
    for name, (data, bad_off) in cases.malformed().items():
        if name in ("bsize_past_buffer", "garbage_between"):
            continue   # (the framing's errors: the block table's, tests/test_bgzf_inflate_api.py)
        parts = cases.split(data)
        got = _run(program, [b for _, b in parts], name + ".bin")
        for (off, blk), (status, h, n) in zip(parts, got):
            if off == bad_off:
                assert status != 0, name
            else:
                assert status == 0 and h == _fnv(zlib.decompress(blk[18:-8], -15)), name


def test_status_codes_name_the_edit(program):
    M = cases.malformed()
    want = {"truncated_payload": 1, "crc_one_bit": 11, "isize_too_small": 9, "isize_too_large": 10, "btype_3": 2, "stored_len_nlen": 3,
            "over_subscribed": 5, "incomplete_literal_code": 6, "distance_before_start": 8}
    for name, code in want.items():
        data, bad_off = M[name]
        blk = dict(cases.split(data))[bad_off]
        assert _run(program, [blk], "one.bin")[0][0] == code, name


def test_a_block_cut_anywhere_is_refused_without_a_read_past_its_end(program):
    """the payload of a good block cut after every 37th byte (the trailer kept): the bit reader must stop at the payload's end"""
    data, _ = cases.families()["level6"]
    blk = cases.split(data)[0][1]
    pay = blk[18:-8]
    cuts = [cases.frame(pay[:k], crc=0, isize=3000) for k in range(0, len(pay), 37)]
    for status, _, _ in _run(program, cuts, "cuts.bin"):
        assert status != 0


def test_sanitizers_were_used_where_the_compiler_has_them(program):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(program[2] / "probe")], input="int main(){}", capture_output=True, text=True)
    assert program[1] == (probe.returncode == 0)
