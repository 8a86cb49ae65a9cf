"""mi355x_bgzf_inflate_dev (csrc/bgzf_inflate_kernel.hip, csrc/bgzf_in_stage.hip): BGZF blocks inflated by the device decoder.

The cases are tests/bgzf_in_cases.py's, which the host run of the kernel's source has passed (tests/test_inflate_kernel_host.py); every
result is held against the host path's (mi355x_bgzf_inflate, zlib), the return value for malformed input included."""
import ctypes as C
import gzip
import os
import threading

import numpy as np
import pytest

import bgzf_in_cases as cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EX = os.path.join(HERE, "golden", "mpibwa_examples")


@pytest.fixture(scope="module")
def lib(built):
    from mpibwa_amd import api
    return api.load_library()


def _inflate(fn, data, cap):
    out = C.create_string_buffer(max(cap, 1))
    n = fn(data, len(data), out, cap)
    return n, out.raw[:max(n, 0)]


def _counts(lib):
    c = (C.c_uint64 * 4)()
    lib.mi355x_bgzf_inflate_dev_counts(c)
    return list(c)


def _compress_dev(lib, t):
    cap = lib.mi355x_bgzf_bound(len(t))
    out = C.create_string_buffer(max(cap, 1))
    n = lib.mi355x_bgzf_compress_dev(t, len(t), out, cap)
    return out.raw[:n]


def test_every_family_gives_the_host_paths_text_and_the_counts_move(lib):
    for name, (data, text) in cases.families().items():
        c0 = _counts(lib)
        host = _inflate(lib.mi355x_bgzf_inflate, data, len(text))
        assert host == (len(text), text), name
        assert _inflate(lib.mi355x_bgzf_inflate_dev, data, len(text)) == host, name
        c1 = _counts(lib)
        assert [b - a for a, b in zip(c0, c1)] == [len(cases.split(data)), 0, len(data), len(text)], name
    # all of them as one file, and a buffer one byte short
    data = b"".join(d for d, _ in cases.families().values())
    text = b"".join(t for _, t in cases.families().values())
    assert _inflate(lib.mi355x_bgzf_inflate_dev, data, len(text)) == (len(text), text)
    assert _inflate(lib.mi355x_bgzf_inflate_dev, data, len(text) - 1) == (0, b"")


@pytest.mark.parametrize("n_blocks", [1, 2, 511, 512, 513])
def test_launches_round_the_piece_boundary(lib, n_blocks):
    text = cases.fastq_text(100 * n_blocks + 37, seed=20)      # blocks of 100 bytes, and a last one of 37
    data = cases.blocks(text[:100 * n_blocks], 100, level=1)
    if n_blocks == 513:
        data += cases.block(text[100 * n_blocks:], level=1)
    else:
        text = text[:100 * n_blocks]
    assert len(cases.split(data)) == n_blocks + (n_blocks == 513)
    assert _inflate(lib.mi355x_bgzf_inflate_dev, data, len(text)) == (len(text), text)


@pytest.fixture(scope="module")
def ordinary():
    rng = np.random.default_rng(4)

    def record(n):
        return b"r%d\t99\tchr1\t%d\t60\t%dM\t=\t%d\t400\t" % (n, n * 7, 150, n * 7 + 250) + bytes(rng.choice(list(b"ACGT"), 150).tolist()) + b"\t" + \
            bytes((rng.integers(2, 42, 150) + 33).astype(np.uint8).tolist()) + b"\tNM:i:0\tMD:Z:150\tAS:i:150\tXS:i:0\n"
    return b"".join(record(n) for n in range(4000))   # 1.5 MB of ordinary records, as tests/test_gpu_bgzf.py builds them


@pytest.fixture(scope="module")
def real():
    with gzip.open(os.path.join(EX, "HCC1187C_R1_10K.fastq.gz"), "rb") as g:
        return g.read()                                # the example reads as they are: FASTQ text


@pytest.mark.parametrize("which", ["ordinary", "real"])
def test_what_the_device_deflates_the_device_inflates(lib, ordinary, real, which):
    t = ordinary if which == "ordinary" else real
    data = _compress_dev(lib, t)
    assert len(data) > 0 and cases.good(data) == t
    assert _inflate(lib.mi355x_bgzf_inflate_dev, data, len(t)) == (len(t), t)


def test_malformed_files_give_the_host_paths_return_value_and_a_good_call_follows(lib):
    c0 = _counts(lib)
    failed = 0
    for name, (data, off) in cases.malformed().items():
        cap = 3 * 65536
        host = _inflate(lib.mi355x_bgzf_inflate, data, cap)[0]
        assert host == -off - 1, name
        assert _inflate(lib.mi355x_bgzf_inflate_dev, data, cap)[0] == host, name
        failed += name not in ("bsize_past_buffer", "garbage_between")     # (the framing's errors: no block fails, the walk stops)
    assert _counts(lib)[1] - c0[1] == failed
    data, text = cases.families()["level6"]
    assert _inflate(lib.mi355x_bgzf_inflate_dev, data, len(text)) == (len(text), text)


def test_callers_side_by_side_and_beside_the_aligner(lib, ordinary, real, genome, reads_pe):
    from mpibwa_amd import abi, api, simulate
    texts = [ordinary, real[:1_000_000], cases.families()["size_65536"][1] * 3, ordinary[5:333_333]]
    files = [_compress_dev(lib, t) for t in texts[:2]] + [cases.blocks(t, 65536, level=6) for t in texts[2:]]
    for f, t in zip(files, texts):
        assert _inflate(lib.mi355x_bgzf_inflate_dev, f, len(t)) == (len(t), t)      # the lone call's result
    lib.mi355x_finalize()                      # no context has buffers: the first round below, four calls started together, makes four
    eng = api.Engine(genome["prefix"], device=0)
    opt, ra = eng.opt(flag=abi.MEM_F_PE), simulate.reads_to_ascii(reads_pe)
    sam = eng.process(opt, ra)
    for _ in range(2):
        assert eng.process(opt, ra) == sam
    rounds, gate, bad, marks = 4, threading.Barrier(4), [], []

    def caller(k):
        for r in range(rounds):
            i = gate.wait(timeout=600)
            if r == 1 and i == 0:
                marks.append(int(lib.mi355x_buffer_growths()))   # every context has its buffers after the first round
            if _inflate(lib.mi355x_bgzf_inflate_dev, files[k], len(texts[k])) != (len(texts[k]), texts[k]):
                bad.append((k, r))

    def aligner():
        if eng.process(opt, ra) != sam:
            bad.append("sam")
    th = [threading.Thread(target=caller, args=(k,)) for k in range(4)] + [threading.Thread(target=aligner)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not bad
    assert int(lib.mi355x_buffer_growths()) == marks[0]
    lib.mi355x_finalize()
    assert _inflate(lib.mi355x_bgzf_inflate_dev, files[2], len(texts[2])) == (len(texts[2]), texts[2])   # the contexts come back after mi355x_finalize
