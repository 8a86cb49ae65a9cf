"""mi355x_bam_sort (csrc/bam_sort.cpp) against tests/bam_sort_model.py on bam_sort_cases.py's inputs: the header with the
rewritten @HD line, the records in coordinate order with ties in input order, blocks of whole records, the empty end block, the codes
of malformed inputs, and a cap that is too small.  No GPU."""
import ctypes as C

import pytest

import bam_model as bm
import bam_sort_cases as sc
import bam_sort_model as sm


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def host_sort(lib, bam, level=1, cap=None, fill=None):
    bound = lib.mi355x_bam_sort_bound(bam, len(bam))
    cap = max(bound, 1) if cap is None else cap
    out = C.create_string_buffer(max(cap, 1))
    if fill is not None:
        C.memset(out, fill, max(cap, 1))
    size = lib.mi355x_bam_sort(bam, len(bam), level, out, cap)
    return (out.raw[:size] if size > 0 else size), out


def check_sorted(got, bam, what):
    header, recs = sm.sort_bam(bam)
    assert isinstance(got, bytes), (what, got)
    g_header, g_recs, payloads = sm.decode_sorted(got)
    assert g_header == header, what
    assert g_recs == recs, what
    sm.check_blocks(header, payloads)
    n_ref = len(bm.decode_header(header)[1])
    keys = [sm.packed_key(r, n_ref) for r in g_recs]
    assert keys == sorted(keys) and all(k < 1 << sm.key_bits(n_ref) for k in keys), what


def test_the_model_orders_as_the_rule_says():
    # the model itself, on a case small enough to read: reverse behind forward at one place, unmapped last, a tie in input order
    lines = [sc.bc.line(qname=b"u", flag=4, rname=b"*", pos=0, cigar=b"*", rnext=b"*", pnext=0, tlen=0), sc.bc.line(qname=b"r", flag=16, rname=b"chr2", pos=9),
             sc.bc.line(qname=b"f1", flag=0, rname=b"chr2", pos=9), sc.bc.line(qname=b"a", flag=0, rname=b"chr1", pos=500), sc.bc.line(qname=b"f2", flag=0, rname=b"chr2", pos=9),
             sc.bc.line(qname=b"m", flag=69, rname=b"chr1", pos=3, cigar=b"*")]
    header, recs = sm.sort_bam(sc.own(lines))
    assert [r[36:r.index(b"\0", 36)] for r in recs] == [b"m", b"a", b"f1", b"f2", b"r", b"u"]
    assert bm.decode_header(header)[0] == sc.TEXT.replace(b"SO:unsorted", b"SO:coordinate")
    assert [sm.key_bits(n) for n in (0, 1, 2, 3, 255, 256, 70000)] == [33, 34, 35, 35, 41, 42, 50]


@pytest.mark.parametrize("k", range(len(sc.good_cases())), ids=[w.replace(" ", "_") for w, _ in sc.good_cases()])
def test_good_cases(lib, k):
    what, bam = sc.good_cases()[k]
    got, _ = host_sort(lib, bam)
    check_sorted(got, bam, what)


def test_more_blocks_than_a_piece(lib):
    what, bam = sc.piece_case()
    got, _ = host_sort(lib, bam)
    check_sorted(got, bam, what)
    assert len(bm.bgzf_blocks(got)) > 512 + 2


def test_the_chunks_and_merges_of_65_536_records_and_more(lib, monkeypatch):
    # the branch every real file takes: 64 chunks sorted side by side and merged pair by pair; few keys, so stability decides the order
    what, bam = sc.many_case()
    header, recs = sm.sort_bam(bam)
    assert len(recs) >= 65536 and len(recs) % 64 != 0 and len({sm.key(r, 6) for r in recs}) == 30
    for n in (None, "1", "3"):
        if n:
            monkeypatch.setenv("MPIBWA_SAMPOST_THREADS", n)
        got, _ = host_sort(lib, bam)
        check_sorted(got, bam, what)


def test_the_bytes_do_not_depend_on_the_threads(lib, monkeypatch):
    what, bam = sc.good_cases()[2]
    _, big = sc.piece_case()
    _, many = sc.many_case()
    want = [host_sort(lib, b, level=3)[0] for b in (bam, big, many)]
    for n in ("1", "3"):
        monkeypatch.setenv("MPIBWA_SAMPOST_THREADS", n)
        assert [host_sort(lib, b, level=3)[0] for b in (bam, big, many)] == want
    check_sorted(host_sort(lib, bam, level=9)[0], bam, what)


@pytest.mark.parametrize("k", range(len(sc.malformed_cases())), ids=[w.replace(" ", "_") for w, _, _ in sc.malformed_cases()])
def test_malformed_cases(lib, k):
    what, bam, code = sc.malformed_cases()[k]
    got, out = host_sort(lib, bam, cap=len(bam) * 4 + (1 << 20), fill=0x5a)
    assert got == code, what
    assert out.raw == b"\x5a" * len(out.raw), what


def test_a_cap_one_byte_short(lib):
    what, bam = sc.good_cases()[2]
    bound = lib.mi355x_bam_sort_bound(bam, len(bam))
    stream = sm.inflate(bam)
    assert len(stream) < bound < len(stream) + 4096
    got, out = host_sort(lib, bam, cap=bound - 1, fill=0xa5)
    assert got == 0 and out.raw == b"\xa5" * (bound - 1)
    got, _ = host_sort(lib, bam, cap=bound)
    check_sorted(got, bam, what)
