"""The device paths of the BAI index (csrc/bam_index_kernel.hip, csrc/bam_sort_stage.hip): mi355x_bam_index_dev gives
mi355x_bam_index's bytes, codes and reasons on bam_index_cases.py's inputs and leaves the walk to the host exactly where a record spans
blocks; mi355x_bam_sort_index_dev writes mi355x_bam_sort_dev's bytes and the index of them, the same on every call, refuses a position
beyond 2^29 and a file that does not fit with nothing written; and mpibwa_sort --index / --index-only on the example data's --bam file."""
import ctypes as C
import os
import subprocess

import pytest

import bam_index_cases as ic
import bam_index_model as mi
import bam_sort_cases as sc
import bam_sort_model as sm
from test_bam_index_cases import expected_of_the_sorts_table, index_with, libc
from test_gpu_bam import example  # noqa: F401  (the fixture: the library's SAM text of the example data's first 1 500 pairs)

pytestmark = pytest.mark.gpu
INT64_MIN = -2 ** 63
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mpibwa_amd", "mpibwa_sort")


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def counts(lib):
    c = (C.c_uint64 * 8)()
    lib.mi355x_bam_index_dev_counts(c)
    return list(c)


def dev_sort(lib, bam):
    cap = max(lib.mi355x_bam_sort_bound(bam, len(bam)), 1)
    out = C.create_string_buffer(cap)
    size = lib.mi355x_bam_sort_dev(bam, len(bam), out, cap)
    return out.raw[:size] if size > 0 else size


def sort_index(lib, bam, fill=0x5a):
    """(the sorted file or the code, the index or None, the reason, the output buffer)"""
    cap = max(lib.mi355x_bam_sort_bound(bam, len(bam)), 1)
    out = C.create_string_buffer(cap)
    C.memset(out, fill, cap)
    p, n, why = C.c_void_p(), C.c_size_t(0), C.c_int(-1)
    size = lib.mi355x_bam_sort_index_dev(bam, len(bam), out, cap, C.byref(p), C.byref(n), C.byref(why))
    if size <= 0:
        assert not p.value and n.value == 0
        return size, None, why.value, out
    bai = C.string_at(p.value, n.value)
    libc.free(p)
    return out.raw[:size], bai, why.value, out


def test_good_cases_and_who_walked(lib):
    walked = []
    for what, bam, _ in ic.good_cases() + [ic.big_case()]:
        want = index_with(lib.mi355x_bam_index, bam)
        c0 = counts(lib)
        assert index_with(lib.mi355x_bam_index_dev, bam) == want, what
        d = [a - b for a, b in zip(counts(lib), c0)]
        contigs, _ = mi.parse(want[0])
        chunks = sum(len(c) for bins, _ in contigs for b, c in bins.items() if b != mi.PSEUDO)
        windows = sum(len(io) for _, io in contigs)
        assert (d[0], d[1], d[6], d[7]) == (1, want[2], len(want[0]), 0), what
        if d[2]:
            walked.append(what)
        else:
            assert d[4] == chunks and d[5] == windows and d[3] >= chunks, (what, d)
    assert walked == ["records that span blocks", "a record that spans two blocks"]


def test_files_that_cannot_be_indexed_get_the_hosts_code_and_reason(lib):
    for what, bam, code, reason in ic.bad_cases():
        assert index_with(lib.mi355x_bam_index_dev, bam)[:2] == (code, reason), what
    for what, bam, code in sc.malformed_cases():
        assert index_with(lib.mi355x_bam_index_dev, bam)[:2] == expected_of_the_sorts_table(bam, code), what


def check_fused(lib, what, bam):
    z = dev_sort(lib, bam)
    assert isinstance(z, bytes), (what, z)
    got, bai, why, _ = sort_index(lib, bam)
    assert got == z and why == 0, what
    assert bai == index_with(lib.mi355x_bam_index, z)[0], what
    assert bai == mi.build(z), what
    assert sort_index(lib, bam)[:2] == (z, bai), what
    return z, bai


def test_the_fused_call_on_the_unsorted_forms_of_the_cases(lib):
    for what, bam, _ in ic.good_cases():
        check_fused(lib, what, ic.unsorted(bam))
    what, bam, _ = ic.big_case()
    z, bai = check_fused(lib, what, ic.unsorted(bam))
    assert index_with(lib.mi355x_bam_index_dev, z)[0] == bai


def test_the_fused_call_on_more_blocks_than_a_piece(lib):
    what, bam = sc.piece_case()
    z, bai = check_fused(lib, what, bam)
    assert len(sm.decode_sorted(z)[2]) > 512 + 2
    assert index_with(lib.mi355x_bam_index_dev, z)[0] == bai


def test_the_fused_call_refuses_a_position_beyond_2_29_with_nothing_written(lib):
    # the sort's case of 70 001 records has positions up to 2^31 - 2 on contigs: the sort takes them, a BAI index cannot
    what, bam = sc.many_case()
    assert isinstance(dev_sort(lib, bam), bytes)
    stream = sm.inflate(bam)
    at = sm.bm.decode_header(stream)[2]
    for r in sm.bm.split_records(stream, at):
        if mi.interval(r)[2] > mi.LIMIT:
            break
        at += len(r)
    got, bai, why, out = sort_index(lib, bam, fill=0x77)
    assert (got, bai, why) == (-at - 1, None, 4)
    assert out.raw == b"\x77" * len(out.raw)
    for what, bam, code, reason in ic.bad_cases():
        if reason == 4:
            assert sort_index(lib, bam)[:3] == (code, None, 4), what


def test_the_fused_call_has_the_sorts_codes(lib):
    for what, bam, code in sc.malformed_cases():
        got, bai, why, out = sort_index(lib, bam)
        block = expected_of_the_sorts_table(bam, code)[1] == 1   # (the sort does not look at the order: a record's code is reason 2)
        assert (got, bai, why) == (code, None, 1 if block else 2), what
        assert out.raw == b"\x5a" * len(out.raw), what


def test_a_file_that_does_not_fit_is_refused(lib, monkeypatch):
    what, bam, _ = ic.good_cases()[-1]
    monkeypatch.setenv("MPIBWA_BAM_SORT_MAX_BYTES", "1")
    c0 = counts(lib)
    got, bai, why, out = sort_index(lib, ic.unsorted(bam), fill=0x33)
    assert (got, bai) == (INT64_MIN, None) and out.raw == b"\x33" * len(out.raw)
    p, n = C.c_void_p(0x1234), C.c_size_t(77)
    assert lib.mi355x_bam_index_dev(bam, len(bam), C.byref(p), C.byref(n), None) == INT64_MIN
    assert (p.value, n.value) == (0x1234, 77)
    assert [a - b for a, b in zip(counts(lib), c0)] == [2, 0, 0, 0, 0, 0, 0, 2]
    monkeypatch.delenv("MPIBWA_BAM_SORT_MAX_BYTES")
    check_fused(lib, what, ic.unsorted(bam))


def test_the_stage_times_are_reported(lib):
    what, bam, _ = ic.good_cases()[-1]
    index_with(lib.mi355x_bam_index_dev, bam)
    ms = (C.c_double * 8)()
    lib.mi355x_bam_index_dev_stage_ms(ms)
    assert all(v >= 0 for v in ms) and ms[4] >= ms[2] > 0 and ms[5] > 0 and list(ms[6:]) == [0, 0]


def run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=e)


def test_the_program_on_the_example_datas_bam_file(lib, example, tmp_path):
    eng, text = example
    d = tmp_path
    (d / "in.bam").write_bytes(sc.example_bam(lib, eng.bns, text))
    for name, flags in (("dev.bam", ["--device", "--index"]), ("host.bam", ["--index"])):
        r = run(flags + ["-o", d / name, d / "in.bam"])
        assert r.returncode == 0, r.stderr[-2000:]
        z = (d / name).read_bytes()
        bai = (d / (name + ".bai")).read_bytes()
        assert bai == mi.build(z), name
        contigs, no_coor = mi.parse(bai)
        placed = sum(s[37450][1][0] + s[37450][1][1] for s, _ in contigs if 37450 in s)
        assert placed > 0 and placed + no_coor == len(sm.decode_sorted(z)[1]) >= 3000
        os.remove(d / (name + ".bai"))
        for more in ([], ["--device"]):
            r = run(["--index-only"] + more + [d / name])
            assert r.returncode == 0, r.stderr[-2000:]
            assert (d / (name + ".bai")).read_bytes() == bai, (name, more)
            os.remove(d / (name + ".bai"))
    for more in ([], ["--device"]):
        r = run(["--index-only"] + more + [d / "in.bam"])
        assert r.returncode != 0 and len(r.stderr.strip().splitlines()) == 1 and "not in coordinate order: the record at offset" in r.stderr, r.stderr
        assert not (d / "in.bam.bai").exists()
