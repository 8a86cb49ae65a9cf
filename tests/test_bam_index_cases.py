"""mi355x_bam_index (csrc/bam_index.cpp) against tests/bam_index_model.py on bam_index_cases.py's inputs: the index's bytes,
the codes and reasons of files that cannot be indexed, and — judging the model and the library against the format itself, not against
each other — a region query through the index that finds exactly the records a full scan finds.  No GPU."""
import ctypes as C
import random
import struct

import pytest

import bam_index_cases as ic
import bam_index_model as mi
import bam_model as bm
import bam_sort_cases as sc
import bam_sort_model as sm

libc = C.CDLL(None)
libc.free.argtypes = [C.c_void_p]


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def index_with(fn, bam):
    """(the index's bytes or the code, the reason, the records)"""
    p, n, why = C.c_void_p(), C.c_size_t(0), C.c_int(-1)
    r = fn(bam, len(bam), C.byref(p), C.byref(n), C.byref(why))
    if r < 0:
        assert not p.value
        return r, why.value, 0
    bai = C.string_at(p.value, n.value)
    libc.free(p)
    return bai, why.value, r


def n_records(bam):
    return len(mi.layout(bam)[1])


def test_the_model_on_a_case_small_enough_to_read():
    recs = [ic.rec("a", 0, 5, ic.M(10)), ic.rec("b", 0, ic.W - 1, ic.M(2)), ic.rec("c", 0, ic.W + 5, ic.M(3)), ic.rec("d", 2, 0, (), flag=4), ic.rec("u", -1, -1, flag=4)]
    bam = ic.file_in_blocks([recs[:2], recs[2:]])
    header_block = len(sc.block(sc.header_bytes(ic.TEXT, ic.CONTIGS)))
    second = header_block + len(sc.block(b"".join(recs[:2])))
    end = second + len(sc.block(b"".join(recs[2:])))
    v = [header_block << 16, header_block << 16 | len(recs[0]), second << 16, second << 16 | len(recs[2]), second << 16 | len(recs[2]) + len(recs[3]), end << 16]
    contigs, no_coor = mi.parse(mi.build(bam))
    assert no_coor == 1 and len(contigs) == 3
    assert contigs[0] == ({4681: [(v[0], v[1])], 585: [(v[1], v[2])], 4682: [(v[2], v[3])], 37450: [(v[0], v[3]), (3, 0)]}, [v[0], v[1]])
    assert contigs[1] == ({}, [])
    assert contigs[2] == ({4681: [(v[3], v[4])], 37450: [(v[3], v[4]), (0, 1)]}, [v[3]])


GOOD = ic.good_cases()


@pytest.mark.parametrize("k", range(len(GOOD)), ids=[w.replace(" ", "_") for w, _, _ in GOOD])
def test_good_cases(lib, k):
    what, bam, _ = GOOD[k]
    got, why, n = index_with(lib.mi355x_bam_index, bam)
    assert isinstance(got, bytes) and why == 0 and n == n_records(bam), (what, got, why)
    assert got == mi.build(bam), what


def test_the_seeded_case_of_200_000_records(lib):
    what, bam, _ = ic.big_case()
    got, why, n = index_with(lib.mi355x_bam_index, bam)
    assert why == 0 and n == 200_000
    assert got == mi.build(bam)


def test_the_join_happens_exactly_where_the_second_chunk_begins_in_the_first_ones_last_block(lib):
    by_name = {w: mi.parse(mi.build(b))[0][0][0][4681] for w, b, _ in GOOD if "run" in w}
    assert [len(by_name[w]) for w in sorted(by_name)] == [1, 1, 2], sorted(by_name)


def random_regions(rng, bam, ref, n):
    spans = [mi.interval(r) for _, r in mi.layout(bam)[1]]
    top = max([e for c, _, e, _ in spans if c == ref] or [1000]) + 2 * ic.W
    out = []
    for _ in range(n):
        beg = rng.randrange(0, top)
        out.append((ref, beg, min(beg + rng.choice((1, 2, 100, 5000, ic.W, 70000)), 1 << 29)))
    return [r for r in out if r[1] < r[2]]


def check_queries(lib, what, bam, designed):
    """through the library's index and through the model's: what a full scan finds"""
    got, why, _ = index_with(lib.mi355x_bam_index, bam)
    assert why == 0, what
    rng = random.Random(len(bam))
    regions = list(designed)
    for ref in range(len(ic.CONTIGS)):
        regions += random_regions(rng, bam, ref, 200)
    for bai in sorted({got, mi.build(bam)}):   # (one index where the two are the same bytes)
        for ref, beg, end in regions:
            assert mi.query(bam, bai, ref, beg, end) == mi.scan(bam, ref, beg, end), (what, ref, beg, end)


@pytest.mark.parametrize("k", range(len(GOOD)), ids=[w.replace(" ", "_") for w, _, _ in GOOD])
def test_a_query_through_the_index_finds_what_a_scan_finds(lib, k):
    check_queries(lib, *GOOD[k])


def test_queries_on_the_seeded_case(lib):
    check_queries(lib, *ic.big_case())


def test_a_query_finds_something(lib):
    # (so that the equality above is not one of empty lists)
    what, bam, regions = GOOD[[w for w, _, _ in GOOD].index("10M500000N10M: 31 windows and a high bin")]
    bai = mi.build(bam)
    assert [len(mi.query(bam, bai, 0, b, e)) for b, e in ((100000, 100100), (200000, 200010), (0, 1000), (0, 1001), (501019, 501020), (501065, 501066))] == [1, 2, 0, 1, 2, 0]


BAD = ic.bad_cases()


@pytest.mark.parametrize("k", range(len(BAD)), ids=[w.replace(" ", "_") for w, _, _, _ in BAD])
def test_files_that_cannot_be_indexed(lib, k):
    what, bam, code, reason = BAD[k]
    assert index_with(lib.mi355x_bam_index, bam)[:2] == (code, reason), what
    if reason in (3, 4):
        with pytest.raises(mi.Refused) as e:
            mi.build(bam)
        assert (-e.value.offset - 1, e.value.reason) == (code, reason), what


def expected_of_the_sorts_table(bam, code):
    """the sort's malformed inputs are unsorted files: bad blocks and headers keep their codes; a malformed record keeps its code unless
    a record before it already sorts before its predecessor"""
    try:
        stream = b"".join(p for _, p in bm.bgzf_blocks(bam))
    except Exception:
        return code, 1
    try:
        _, contigs, at = bm.decode_header(stream)
        assert stream[:4] == b"BAM\1"
    except Exception:
        return code, 2
    prev, bad_at = None, -code - 1
    while at < bad_at:
        size, = struct.unpack_from("<i", stream, at)
        key = sm.key(stream[at:at + 4 + size], len(contigs))
        if prev is not None and key < prev:
            return -at - 1, 3
        prev = key
        at += 4 + size
    return code, 2


def test_the_sorts_malformed_table(lib):
    for what, bam, code in sc.malformed_cases():
        want = expected_of_the_sorts_table(bam, code)
        assert index_with(lib.mi355x_bam_index, bam)[:2] == want, what
    assert index_with(lib.mi355x_bam_index, b"")[:2] == (-1, 2)


def test_reason_may_be_null(lib):
    p, n = C.c_void_p(), C.c_size_t(0)
    what, bam, _ = GOOD[3]
    assert lib.mi355x_bam_index(bam, len(bam), C.byref(p), C.byref(n), None) == n_records(bam)
    libc.free(p)
    assert lib.mi355x_bam_index(BAD[0][1], len(BAD[0][1]), C.byref(p), C.byref(n), None) == BAD[0][2]
