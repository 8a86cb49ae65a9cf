"""The GPU index builder (csrc/index_gpu.hip) on the degenerate genomes of tests/index_cases.py: its .bwt and .sa must be the bytes of the
plain model (tests/index_model.py, tied to the reference's own index and equal to the CPU builder on the same genomes in
tests/test_index_cases.py), and the .pac / .ann / .amb written beside them those of the CPU builder.  Every family, through the composite
[group | rank] key and through the two stable passes (MPIBWA_IDX_WIDE=1), and a selection with the round-0 buckets forced onto 2, 3 and 4
leading symbols (MPIBWA_IDX_KB), where most buckets are empty and the short suffixes fall into zero-padded ones."""
import ctypes as C
import os

import numpy as np
import pytest

import index_cases as ic
import index_model as im
import smem_cases as sc

pytestmark = pytest.mark.gpu

_model = {}


def _want(case):
    """the model's files, computed once per genome for all modes"""
    if case.name not in _model:
        _model[case.name] = im.index_files(case.codes)[:2]
    return _model[case.name]


def _build_and_compare(lib, directory, case, tag):
    from mpibwa_amd import bigindex
    pac = im.pack_pac(case.codes)
    g = os.path.join(str(directory), "g%s.fa" % tag)
    bigindex.write_meta_files(g, pac, np.array(case.contigs, np.int64))
    secs = C.c_double(0)
    assert lib.mi355x_index_build_gpu(0, pac.ctypes.data, case.l_pac, g.encode(), C.byref(secs)) == 0
    bwt, sa = _want(case)
    got_bwt, got_sa = open(g + ".bwt", "rb").read(), open(g + ".sa", "rb").read()
    assert len(got_bwt) == len(bwt) and len(got_sa) == len(sa), (case.name, tag, len(got_bwt), len(bwt), len(got_sa), len(sa))
    if got_bwt != bwt:
        a, b = np.frombuffer(got_bwt, np.uint8), np.frombuffer(bwt, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        raise AssertionError((case.name, tag, ".bwt differs from byte %d on, %d bytes in all; primary" % (at, int((a != b).sum())),
                              int(np.frombuffer(got_bwt[:8], "<u8")[0]), int(np.frombuffer(bwt[:8], "<u8")[0])))
    if got_sa != sa:
        a, b = np.frombuffer(got_sa, "<u8"), np.frombuffer(sa, "<u8")
        at = int(np.flatnonzero(a != b)[0])
        raise AssertionError((case.name, tag, ".sa differs from word %d on, %d words in all" % (at, int((a != b).sum())), int(a[at]), int(b[at])))
    return g


def _lib():
    from mpibwa_amd import api
    lib = api.load_library()
    lib.mi355x_index_build_gpu.restype = C.c_int
    lib.mi355x_index_build_gpu.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_char_p, C.POINTER(C.c_double)]
    return lib


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("group", ic.GROUPS)
def test_gpu_builder_equals_the_model(built, tmp_path, monkeypatch, group, wide):
    lib = _lib()
    monkeypatch.delenv("MPIBWA_IDX_KB", raising=False)
    if wide:
        monkeypatch.setenv("MPIBWA_IDX_WIDE", "1")
    else:
        monkeypatch.delenv("MPIBWA_IDX_WIDE", raising=False)
    cases = ic.group(group)
    assert 1 <= len(cases) <= 28
    for k, c in enumerate(cases):
        g = _build_and_compare(lib, tmp_path, c, "%d" % k)
        if not wide:      # the files beside them: what the CPU builder leaves for the same FASTA
            fa = sc.write_index(tmp_path, "c%d" % k, c.names(), c.seqs())
            for ext in ("pac", "ann", "amb"):
                assert open(fa + "." + ext, "rb").read() == open(g + "." + ext, "rb").read(), (c.name, ext)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("kb", [2, 3, 4])
@pytest.mark.parametrize("which", ["short", "long"])
def test_gpu_builder_with_forced_buckets_equals_the_model(built, tmp_path, monkeypatch, which, kb, wide):
    """short: every length up to 33 (N <= 66: at kb = 4 a bucket holds a suffix or none, and the last kb - 1 suffixes are shorter than
    the bucket's prefix); long: a homopolymer (one bucket in 4^kb takes nearly everything), one-period texts, period 29, a
    self-reverse-complement text and an ordinary genome"""
    lib = _lib()
    monkeypatch.setenv("MPIBWA_IDX_KB", str(kb))
    if wide:
        monkeypatch.setenv("MPIBWA_IDX_WIDE", "1")
    else:
        monkeypatch.delenv("MPIBWA_IDX_WIDE", raising=False)
    cases = ic.kb_cases_short() if which == "short" else ic.kb_cases_long()
    for k, c in enumerate(cases):
        _build_and_compare(lib, tmp_path, c, "%d" % k)
