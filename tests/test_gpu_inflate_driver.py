"""mpibwa_gpu on BGZF-compressed FASTQ on the GPU box: the example reads, bgzipped by the test, through --device-inflate on
one and two ranks and through the host path.  The records and the header are those of the run on the plain files, and the run reports
as many device-inflated blocks as the files' block tables give for the slice scan plus the chunk reads.  One run is compressed in and
compressed out (--device-inflate -g --device-bgzf)."""
import bisect
import gzip
import os
import re
import struct
import subprocess
import tarfile

import pytest

import bgzf_in_cases as cases
from test_gpu_bgzf_driver import EXE, EX, _bgzf_blocks, _run, _split, mpiexec

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(mpiexec() is None or not os.path.exists(EXE), reason="mpibwa_gpu or mpiexec not present")]
BASE = ["-K", "1000000", "--in-flight", "3"]
REPORT = r"BGZF input: device (\d+) blocks, (\d+) bytes -> (\d+) bytes of text; host (\d+) blocks, (\d+) bytes -> (\d+) bytes of text"


@pytest.fixture(scope="module")
def example(tmp_path_factory, built):
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()
    d = tmp_path_factory.mktemp("infdrv")
    with tarfile.open(os.path.join(EX, "hg19.small.tar.gz")) as t:
        t.extractall(d)
    fq, gz, texts = [], [], []
    for k, size in ((1, 65280), (2, 20000)):        # (the two files are cut into blocks differently)
        with gzip.open(os.path.join(EX, "HCC1187C_R%d_10K.fastq.gz" % k), "rb") as g:
            text = g.read()
        plain, packed = str(d / ("R%d.fastq" % k)), str(d / ("R%d.fastq.gz" % k))
        with open(plain, "wb") as f:
            f.write(text)
        with open(packed, "wb") as f:
            f.write(cases.blocks(text, size) + cases.EOF_BLOCK)
        fq.append(plain); gz.append(packed); texts.append(text)
    return str(d), os.path.join(str(d), "hg19.small.fa"), fq, gz, texts


@pytest.fixture(scope="module")
def plain(example):
    d, prefix, fq, _, _ = example
    out = os.path.join(d, "plain.sam")
    _run(1, BASE + ["--ordered", "-o", out, prefix] + fq, d)
    head, body = _split(open(out, "rb").read())
    assert len(body) >= 20000
    return head, body


def _covering(toff, at, n):
    """blocks that read_text inflates for n bytes of text from `at`: from the last block that starts at or before `at` to the first that
    starts at or behind the end"""
    if n <= 0:
        return 0
    b0 = bisect.bisect_right(toff, at) - 1
    b1 = b0 + 1
    while toff[b1] < at + n:
        b1 += 1
    return b1 - b0


def _expected_blocks(example, ranks):
    """device-inflated blocks of a run: every rank's slice (from the first record at or behind its byte share to the next rank's) and
    every chunk's bytes, in both files"""
    d, prefix, fq, gz, texts = example
    env = dict(os.environ)
    env.pop("LD_LIBRARY_PATH", None)
    r = subprocess.run([mpiexec(), "-n", "1", EXE, "mem", "--dry-run"] + BASE + [prefix] + fq, capture_output=True, text=True, timeout=300, env=env, cwd=d)
    assert r.returncode == 0
    table = [tuple(int(x) for x in ln.split()[1::2]) for ln in r.stdout.strip().splitlines()[1:]]
    total = 0
    for k, (path, text) in enumerate(zip(gz, texts)):
        sizes = [struct.unpack_from("<I", b, len(b) - 4)[0] for _, b in cases.split(open(path, "rb").read())]
        toff = [sum(sizes[:i]) for i in range(len(sizes) + 1)]
        recs, at, lines = [], 0, text.split(b"\n")
        for i in range(0, len(lines) - 3, 4):
            recs.append(at)
            at += sum(len(x) + 1 for x in lines[i:i + 4])
        cut = [min([o for o in recs if o >= len(text) // ranks * r] + [len(text)]) for r in range(ranks)] + [len(text)]
        total += sum(_covering(toff, cut[r], cut[r + 1] - cut[r]) for r in range(ranks))
        offs = [t[2 + k] for t in table]
        total += sum(_covering(toff, offs[c], offs[c + 1] - offs[c]) for c in range(len(offs) - 1))
    return total


@pytest.mark.parametrize("ranks", [1, 2])
def test_device_inflate_gives_the_plain_runs_records(example, plain, ranks):
    d, prefix, fq, gz, texts = example
    head, body = plain
    out = os.path.join(d, "dev%d.sam" % ranks)
    r = _run(ranks, BASE + ["--device-inflate", "-o", out, prefix] + gz, d)
    zhead, zbody = _split(open(out, "rb").read())
    assert zhead[:-1] == head[:-1] and sorted(zbody) == sorted(body)
    m = re.search(REPORT, r.stderr)
    assert m, r.stderr[-3000:]
    dev_blocks, dev_in, dev_out, host_blocks = (int(x) for x in m.groups()[:4])
    assert dev_blocks == _expected_blocks(example, ranks)
    assert dev_out >= 2 * sum(len(t) for t in texts) and dev_in < dev_out
    assert (host_blocks == 0) == (ranks == 1)        # (the probing reads of a rank that enters a file in its middle stay on the cores)


def test_the_host_path_and_a_mixed_pair(example, plain):
    d, prefix, fq, gz, texts = example
    head, body = plain
    out = os.path.join(d, "host.sam")
    r = _run(1, BASE + ["-o", out, prefix] + gz, d)
    zhead, zbody = _split(open(out, "rb").read())
    assert zhead[:-1] == head[:-1] and sorted(zbody) == sorted(body)
    m = re.search(REPORT, r.stderr)
    assert m and int(m.group(1)) == 0 and int(m.group(4)) == _expected_blocks(example, 1)
    out = os.path.join(d, "mixed.sam")
    r = _run(2, BASE + ["--device-inflate", "-o", out, prefix, fq[0], gz[1]], d)
    assert sorted(_split(open(out, "rb").read())[1]) == sorted(body)
    # plain files: the option is accepted, does nothing, and nothing is reported
    out = os.path.join(d, "noop.sam")
    r = _run(1, BASE + ["--ordered", "--device-inflate", "-o", out, prefix] + fq, d)
    assert "BGZF input" not in r.stderr and _split(open(out, "rb").read())[1] == body


def test_compressed_in_and_compressed_out(example, plain):
    d, prefix, fq, gz, _ = example
    head, body = plain
    out = os.path.join(d, "inout.gz")
    r = _run(2, BASE + ["--device-inflate", "-g", "--device-bgzf", "-o", out, prefix] + gz, d)
    text = b"".join(p for _, p in _bgzf_blocks(open(out, "rb").read()))
    zhead, zbody = _split(text)
    assert zhead[:-1] == head[:-1] and sorted(zbody) == sorted(body)
    assert re.search(REPORT, r.stderr) and "device BGZF:" in r.stderr
