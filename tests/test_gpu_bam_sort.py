"""The device BAM sort (csrc/bam_sort_kernel.hip, csrc/bam_sort_stage.hip): mi355x_bam_sort_dev gives the header and the
records of tests/bam_sort_model.py on bam_sort_cases.py's inputs, blocks that inflate to the bytes of the host path's blocks one by one,
the host path's codes for malformed inputs, the counts as include/mpibwa_amd.h states them (the walk by the host exactly where a block
ends inside a record), the same bytes on every call and from four threads at once, no buffer growth on a second call, a refusal for
memory under MPIBWA_BAM_SORT_MAX_BYTES, and the sorted form of the example data's --bam file."""
import ctypes as C
import threading

import pytest

import bam_model as bm
import bam_sort_cases as sc
import bam_sort_model as sm
from test_gpu_bam import example  # noqa: F401  (the fixture: the library's SAM text of the example data's first 1 500 pairs)

pytestmark = pytest.mark.gpu
INT64_MIN = -2 ** 63


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def counts(lib):
    c = (C.c_uint64 * 8)()
    lib.mi355x_bam_sort_dev_counts(c)
    return list(c)


def dev_sort(lib, bam, cap=None, fill=None):
    bound = lib.mi355x_bam_sort_bound(bam, len(bam))
    cap = max(bound, 1) if cap is None else cap
    out = C.create_string_buffer(max(cap, 1))
    if fill is not None:
        C.memset(out, fill, max(cap, 1))
    size = lib.mi355x_bam_sort_dev(bam, len(bam), out, cap)
    return (out.raw[:size] if size > 0 else size), out


def host_sort(lib, bam, cap=None):
    bound = lib.mi355x_bam_sort_bound(bam, len(bam))
    cap = max(bound, 1) if cap is None else cap
    out = C.create_string_buffer(max(cap, 1))
    size = lib.mi355x_bam_sort(bam, len(bam), 1, out, cap)
    return out.raw[:size] if size > 0 else size


def check(lib, what, bam):
    """one good input through the device path: the model's result, the host path's blocks, the counts"""
    header, recs = sm.sort_bam(bam)
    c0 = counts(lib)
    got, _ = dev_sort(lib, bam)
    c1 = counts(lib)
    assert isinstance(got, bytes), (what, got)
    g_header, g_recs, payloads = sm.decode_sorted(got)
    assert g_header == header, what
    assert g_recs == recs, what
    sm.check_blocks(header, payloads)
    assert payloads == sm.decode_sorted(host_sort(lib, bam))[2], what
    in_blocks = bm.bgzf_blocks(bam)
    want = [1, len(recs), int(sc.needs_host_walk(bam)), sum(len(p) for _, p in in_blocks), len(in_blocks), len(payloads) + 1, len(got), 0]
    assert [a - b for a, b in zip(c1, c0)] == want, what
    return got


def test_good_cases(lib):
    walked = []
    for what, bam in sc.good_cases():
        check(lib, what, bam)
        if sc.needs_host_walk(bam):
            walked.append(what)
    # records that span blocks leave the walk to the host; the library's own layout, a header that ends mid-block, a missing end block
    # and empty blocks do not
    assert walked == ["large records", "cut every 0xff00 bytes", "cut every 1000 bytes"]


def test_more_blocks_than_a_piece_twice_and_from_four_threads(lib):
    what, bam = sc.piece_case()
    z = check(lib, what, bam)
    assert len(bm.bgzf_blocks(z)) > 512 + 2
    g0 = lib.mi355x_buffer_growths()
    assert dev_sort(lib, bam)[0] == z
    assert lib.mi355x_buffer_growths() == g0
    _, small = sc.good_cases()[2]
    want = [z, dev_sort(lib, small)[0], z, dev_sort(lib, small)[0]]
    got = [None] * 4

    def work(k):
        got[k] = dev_sort(lib, bam if k % 2 == 0 else small)[0]
    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == want
    assert lib.mi355x_buffer_growths() == g0


def test_65_536_records_and_more_in_more_than_two_inflate_groups(lib):
    # the host path's chunks and merges against the device's radix sort, and the staging buffers of the inflate used a second time
    what, bam = sc.many_case()
    assert len(bm.bgzf_blocks(bam)) > 2 * 512 + 512 and not sc.needs_host_walk(bam)
    z = check(lib, what, bam)
    assert dev_sort(lib, bam)[0] == z


def test_malformed_inputs_return_the_hosts_code(lib):
    for what, bam, code in sc.malformed_cases():
        cap = len(bam) * 4 + (1 << 20)
        assert host_sort(lib, bam, cap=cap) == code, what
        got, out = dev_sort(lib, bam, cap=cap, fill=0x5a)
        assert got == code, what
        assert out.raw == b"\x5a" * len(out.raw), what


def test_a_cap_one_byte_short(lib):
    what, bam = sc.good_cases()[2]
    bound = lib.mi355x_bam_sort_bound(bam, len(bam))
    got, out = dev_sort(lib, bam, cap=bound - 1, fill=0xa5)
    assert got == 0 and out.raw == b"\xa5" * (bound - 1)


def test_a_file_that_does_not_fit_is_refused(lib, monkeypatch):
    what, bam = sc.good_cases()[2]
    z, _ = dev_sort(lib, bam)
    for admitted in ("1", str(300 << 20)):   # below the fixed buffers; below the fixed buffers and the margin
        monkeypatch.setenv("MPIBWA_BAM_SORT_MAX_BYTES", admitted)
        c0 = counts(lib)
        got, out = dev_sort(lib, bam, fill=0x33)
        assert got == INT64_MIN and out.raw == b"\x33" * len(out.raw)
        c1 = counts(lib)
        assert [a - b for a, b in zip(c1, c0)] == [1, 0, 0, 0, 0, 0, 0, 1]
    monkeypatch.delenv("MPIBWA_BAM_SORT_MAX_BYTES")
    assert dev_sort(lib, bam)[0] == z


def test_the_example_datas_bam_file(lib, example):
    eng, text = example
    bam = sc.example_bam(lib, eng.bns, text)
    assert not sc.needs_host_walk(bam)
    z = check(lib, "the example data", bam)
    names = [eng.bns.contents.anns[i].name for i in range(eng.bns.contents.n_seqs)]
    header, recs, _ = sm.decode_sorted(z)
    assert b"@HD\tVN:1.6\tSO:coordinate\n@SQ" in header
    lines = [bm.decode_record(r, names) for r in recs]
    assert sorted(lines) == sorted(bm.normalise(ln) for ln in text.split(b"\n")[:-1]) and len(lines) >= 3000
    # mapped reads come contig by contig in rising position, the reads without a place last
    places = [(names.index(f[2]) if f[2] != b"*" else len(names), int(f[3])) for f in (ln.split(b"\t") for ln in lines)]
    assert places == sorted(places) and places[0][0] < len(names)
