"""CPU side of the degenerate-genome tests of the index builders and the FM-index kernels (tests/index_cases.py): the plain model of
tests/index_model.py is tied to the reference (it writes the reference's own hg19.small .bwt and .sa), the CPU builder equals the model on
every family, the families reach what they are meant to reach, and the oracle that judges the kernels in tests/test_gpu_fm_degenerate.py
is held against the model's suffix array and — where the reference library is built — against the reference's mem_collect_intv on the
very reads and indexes of that test.  Every comparison is exact."""
import os
import re
import tarfile

import numpy as np
import pytest

import index_cases as ic
import index_model as im
import smem_cases as sc
from oracle import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DATA = os.path.join(HERE, "golden", "mpibwa_examples", "hg19.small.tar.gz")
ROW0 = np.uint64(0xFFFFFFFFFFFFFFFF)      # bwt_sa(0): the stored sa[0] = -1 (src/bwt.c:86-96)


def test_model_writes_the_references_own_index(tmp_path):
    """the model's only tie to the reference: hg19.small.fa.bwt / .sa as the reference shipped them, from the bases of its .pac"""
    with tarfile.open(REF_DATA) as tf:
        tf.extractall(tmp_path)
    prefix = str(tmp_path / "hg19.small.fa")
    fwd = im.read_pac_file(prefix)
    assert len(fwd) == 671_250
    bwt, sa, sa_full = im.index_files(fwd)
    assert bwt == open(prefix + ".bwt", "rb").read()
    assert sa == open(prefix + ".sa", "rb").read()
    assert len(sa_full) == 2 * len(fwd) + 1 and sa_full[0] == 2 * len(fwd)


def test_doubling_equals_sorting_the_suffixes():
    """suffix_array against the definition, on every family member of up to 64 symbols and on short degenerate texts"""
    n = 0
    for c in ic.all_cases():
        T = im.text_of(c.codes)
        if len(T) <= 64:
            assert (im.suffix_array(T) == im.suffix_array_sorted(T)).all(), c.name
            n += 1
    assert n == 24        # l_pac 1 .. 19 and 28 .. 32
    for T in ([0] * 40, [3] * 40, [0, 3] * 20, [1, 2, 1] * 13, [2]):
        assert (im.suffix_array(np.array(T, np.uint8)) == im.suffix_array_sorted(T)).all()


def test_pac_packer_round_trip():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 4099):
        codes = rng.integers(0, 4, size=n, dtype=np.uint8)
        pac = im.pack_pac(codes)
        assert len(pac) == n // 4 + 1 and (im.unpack_pac(pac, n) == codes).all()
    assert im.pack_pac([0, 1, 2, 3, 3]).tolist() == [0x1B, 0xC0]


@pytest.mark.parametrize("group", ic.GROUPS)
def test_cpu_builder_equals_the_model(built, tmp_path, group):
    from mpibwa_amd import bigindex
    cases = ic.group(group)
    assert cases
    for c in cases:
        fa = sc.write_index(tmp_path, "c%d" % cases.index(c), c.names(), c.seqs())
        bwt, sa, _ = im.index_files(c.codes)
        assert open(fa + ".bwt", "rb").read() == bwt, c.name
        assert open(fa + ".sa", "rb").read() == sa, c.name
        assert (im.read_pac_file(fa) == c.codes).all(), c.name
        # what the GPU test writes beside the GPU builder's files is what the CPU builder writes
        g = str(tmp_path / "meta")
        bigindex.write_meta_files(g, im.pack_pac(c.codes), np.array(c.contigs, np.int64))
        for ext in ("pac", "ann", "amb"):
            assert open(fa + "." + ext, "rb").read() == open(g + "." + ext, "rb").read(), (c.name, ext)


def test_the_families_are_the_ones_asked_for():
    names = [c.name for c in ic.all_cases()]
    for l in list(range(1, 20)) + list(range(28, 34)) + [57, 58, 59, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1023, 1024, 1025]:
        assert "len%d" % l in names and ic.by_name("len%d" % l).l_pac == l
    assert {ic.by_name("len%d" % l).l_pac % 4 for l in range(1, 20)} == {0, 1, 2, 3}
    for n in ("homoA", "homoC", "homoG", "homoT"):
        assert ic.by_name(n).l_pac == 4099 and len(set(ic.by_name(n).codes.tolist())) == 1
    assert ic.by_name("diAT").l_pac == 4100 and ic.by_name("diAT+A").l_pac == 4101 and ic.by_name("diAT+A").codes[-1] == 0
    for n in ("diAT", "diCG"):                       # a text that is one period throughout: the reverse complement continues it
        T = im.text_of(ic.by_name(n).codes)
        assert (T[2:] == T[:-2]).all()
    for p in ic.PERIODS:
        c = ic.by_name("period%d" % p).codes
        assert len(c) == 6000 and (c[p:] == c[:-p]).all() and not any((c[q:] == c[:-q]).all() for q in range(1, p))
    s = ic.by_name("selfrc").codes
    assert (im.text_of(s)[:6000] == im.text_of(s)[6000:]).all()
    d, d1 = ic.by_name("doubled").codes, ic.by_name("doubled-1").codes
    assert (d[:3000] == d[3000:]).all() and (d != d1).sum() == 1 and d1[4500] != d[4500]
    assert set(ic.by_name("fibGT").codes.tolist()) == {2, 3} and ic.by_name("fibGT").l_pac == 6765
    assert ic.by_name("ordinary").l_pac == 200_000
    multi = [c for c in ic.all_cases() if len(c.contigs) > 1]
    assert len(multi) == 3 and all(len(c.contigs) == 3 and 1 in c.contigs for c in multi) and {c.group for c in multi} == {"lengths_b", "periods", "selfrc"}
    assert all(len(ic.group(g)) <= 28 for g in ic.GROUPS) and sum(len(ic.group(g)) for g in ic.GROUPS) == len(names)
    src = open(os.path.join(ROOT, "mpibwa_amd", "csrc", "index_gpu.hip")).read()
    assert re.search(r"#define KMER (\d+)", src).group(1) == str(ic.KMER)
    assert len(ic.kb_cases_short()) == 25 and len(ic.kb_cases_long()) == 6


def test_the_families_reach_what_they_are_meant_to():
    rs = [ic.reach(c) for c in ic.all_cases()]
    for r in rs:
        print(r)
    by = {r["name"]: r for r in rs}
    assert any(r["m"] == 0 for r in rs) and any(r["m"] >= 0.9 * r["N"] for r in rs)
    assert max(r["rounds"] for r in rs) >= 12
    assert any(r["first_block"] for r in rs) and any(r["last_block"] for r in rs)
    assert by["homoA"]["primary"] == 1 and by["homoT"]["primary"] == by["homoT"]["N"]          # the first and the last row of all
    assert by["len50-p"]["N"] <= 128 and by["len50-p"]["primary"] == 96                         # one occ block, primary on a multiple of 32
    assert by["len300-p"]["primary"] == 256                                                     # ... and of 128
    assert by["len16"]["primary"] == 32 == by["len16"]["N"] and by["len64"]["primary"] == 127  # among the uploaded ones (index_cases.LENGTH_SEEDS)
    assert {0, 2, 126} <= {r["n128"] for r in rs}
    assert {0, 2, 14, 16, 18, 30} <= {r["N"] % 32 for r in rs} and {0, 2, 14} <= {r["N"] % 16 for r in rs}
    assert by["homoA"]["absent"] == [1, 2] and by["diCG"]["absent"] == [0, 3]
    assert by["len1"]["N"] == 2 and by["len15"]["N"] < 32 <= by["len16"]["N"]                    # n_sa = 1: no sample beside row 0
    # every suffix of a self-reverse-complement text is tied with its partner on the other strand to the end of the text
    assert by["selfrc"]["m"] >= by["selfrc"]["N"] - 2 * ic.KMER and by["selfrc"]["rounds"] >= 12


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle on the indexes that are uploaded
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fm_indexes(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("fm_degenerate")
    out = {}
    for k, name in enumerate(ic.FM_CASES):
        c = ic.by_name(name)
        out[name] = (c, sc.write_index(d, "i%d" % k, c.names(), c.seqs()))
    return out


def test_oracle_sa_equals_the_models_suffix_array(fm_indexes):
    """every row of every uploaded index; and the number of LF steps is the distance to the next sampled row"""
    for name, (c, prefix) in fm_indexes.items():
        _, _, sa_full = im.index_files(c.codes)
        fm = po.OracleFM(prefix)
        assert fm.fm.seq_len == 2 * c.l_pac and len(fm.sa) == (2 * c.l_pac + 32) // 32
        got = np.array([fm.sa_lookup(r) for r in range(len(sa_full))], dtype=np.uint64)
        assert got[0] == ROW0 and (got[1:] == sa_full[1:].astype(np.uint64)).all(), name


def test_homopolymer_reads_outgrow_the_lds_lists(fm_indexes):
    """the 150- and 257-base reads on A x 4099 change their interval size at every extension: a list of more than LCAP entries"""
    c, _ = fm_indexes["homoA"]
    reads = dict(ic.fm_reads(c))
    for tag in ("150@0", "161@0", "257@0"):
        assert sc.list_entries(c.codes, reads[tag], 0) > sc.LCAP, tag
    assert sc.LCAP == 23 and sc.length_class([reads["150@0"]]) == 0 and sc.length_class([reads["161@0"]]) == 1 and sc.length_class([reads["257@0"]]) == 2


def test_reads_cover_the_lengths_and_the_strand_boundary(fm_indexes):
    for name, (c, _) in fm_indexes.items():
        reads = ic.fm_reads(c)
        N = 2 * c.l_pac
        assert len(reads) <= 120 and len({r.tobytes() for _, r in reads}) == len(reads)
        lens = {len(r) for _, r in reads}
        assert {l for l in ic.READ_LENS if l <= N} <= lens, name
        if N < 257:
            assert max(lens) > N and 300 in lens, name
        else:
            across = im.text_of(c.codes)[c.l_pac - 75:c.l_pac + 75].tobytes()     # (reads of equal bases are held once)
            assert any(r.tobytes() == across for _, r in reads), name
    for name in ("homoA", "fibGT"):
        c = fm_indexes[name][0]
        assert 1 not in c.codes and all(1 in r for _, r in ic.absent_base_reads(c))
    assert ic.reach(fm_indexes["homoA"][0])["absent"] == [1, 2] and ic.reach(fm_indexes["fibGT"][0])["absent"] == []


@pytest.mark.skipif(not po.ref_available(), reason="oracle/_ref/libbwaref.so not built")
@pytest.mark.parametrize("opts", ["default", "corner"])
def test_oracle_matches_the_reference_on_the_degenerate_indexes(fm_indexes, opts):
    """the oracle's mem_collect_intv against the reference's own, on the reads of tests/test_gpu_fm_degenerate.py (those with a base the
    text lacks included), as tests/test_smem_cases.py has it for its genomes"""
    kw = {} if opts == "default" else sc.CORNER
    args = sc.oracle_args(kw)
    n = n_zero = 0
    for name, (c, prefix) in fm_indexes.items():
        fm, ref = po.OracleFM(prefix), po.RefIndex(prefix)
        ropt = ref.opt(**kw)
        reads = [r for _, r in ic.fm_reads(c)]
        if name in ("homoA", "fibGT"):
            reads += [r for _, r in ic.absent_base_reads(c)]
        for k, r in enumerate(reads):
            b = fm.collect_intv(r, *args) if len(r) >= args[0] else np.zeros((0, 4), np.uint64)
            a = ref.collect_intv(ropt, r.copy())
            assert a.shape == b.shape, (name, k, len(r), a.shape, b.shape)
            rows = lambda x: np.array(sorted(map(tuple, x.tolist())), dtype=np.uint64).reshape(-1, 4)
            assert (rows(a) == rows(b)).all(), (name, k, a.tolist(), b.tolist())
            n += len(b)
            n_zero += int((b[:, 2] == 0).sum())
    print("intervals", n, "of size 0", n_zero)
    assert n > 1000
