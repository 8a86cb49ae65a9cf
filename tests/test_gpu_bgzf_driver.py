"""mpibwa_gpu --device-bgzf on the GPU box: the chunks' BGZF blocks come from the deflate kernel.  On the example data,
with -g and with -b on one and two ranks, with -f -b --by-chr: every file is well-formed BGZF (each block a gzip member with the
'BC' field, BSIZE, CRC32 and ISIZE), its records and header are those of the plain run, -b ends in the 28-byte empty block, and the
run reports what the device path compressed.  Without -g / -b the option is a usage error, and without the option a -g run writes
the bytes it wrote before: mi355x_bgzf_compress at level 3 over the header and over every chunk's text."""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess
import tarfile
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "mpibwa_amd", "mpibwa_gpu")
EX = os.path.join(HERE, "golden", "mpibwa_examples")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def mpiexec():
    import shutil
    for p in (shutil.which("mpiexec"), "/opt/conda/bin/mpiexec"):
        if p and os.path.exists(p):
            return p
    return None


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(mpiexec() is None or not os.path.exists(EXE), reason="mpibwa_gpu or mpiexec not present")]


def _run(ranks, args, cwd, ok=True):
    env = dict(os.environ)
    env.pop("LD_LIBRARY_PATH", None)
    r = subprocess.run([mpiexec(), "-n", str(ranks), EXE, "mem"] + args, capture_output=True, text=True, timeout=900, env=env, cwd=cwd)
    if ok:
        assert r.returncode == 0, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    return r


def _bgzf_blocks(data):
    """[(block bytes, payload)] of a BGZF stream, every header field checked (SAM spec 4.1)"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 12] == b"\x06\x00" and data[at + 12:at + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        blk = data[at:at + bsize]
        assert len(blk) == bsize
        payload = zlib.decompress(blk[18:-8], -15)
        crc, isize = struct.unpack("<II", blk[-8:])
        assert crc == zlib.crc32(payload) and isize == len(payload) and bsize <= 65536
        out.append((blk, payload))
        at += bsize
    assert at == len(data)
    return out


def _split(text):
    lines = text.splitlines(keepends=True)
    return [ln for ln in lines if ln.startswith(b"@")], [ln for ln in lines if not ln.startswith(b"@")]


@pytest.fixture(scope="module")
def example(tmp_path_factory, built):
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()
    d = tmp_path_factory.mktemp("bzdrv")
    with tarfile.open(os.path.join(EX, "hg19.small.tar.gz")) as t:
        t.extractall(d)
    fq = []
    for k in (1, 2):
        dst = str(d / ("R%d.fastq" % k))
        with gzip.open(os.path.join(EX, "HCC1187C_R%d_10K.fastq.gz" % k), "rb") as g, open(dst, "wb") as f:
            f.write(g.read())
        fq.append(dst)
    return str(d), os.path.join(str(d), "hg19.small.fa"), fq


BASE = ["-K", "1000000", "--in-flight", "3"]


@pytest.fixture(scope="module")
def plain(example):
    """the plain run: one rank, chunks in input order"""
    d, prefix, fq = example
    out = os.path.join(d, "plain.sam")
    _run(1, BASE + ["--ordered", "-o", out, prefix] + fq, d)
    head, body = _split(open(out, "rb").read())
    assert len(body) >= 20000
    return head, body


@pytest.mark.parametrize("flag,ranks", [("-g", 1), ("-g", 2), ("-b", 1), ("-b", 2)])
def test_device_blocks_hold_the_plain_runs_records(example, plain, flag, ranks):
    d, prefix, fq = example
    head, body = plain
    out = os.path.join(d, "dev%s%d.bin" % (flag[1], ranks))
    r = _run(ranks, BASE + [flag, "--device-bgzf", "-o", out, prefix] + fq, d)
    data = open(out, "rb").read()
    blocks = _bgzf_blocks(data)
    text = b"".join(p for _, p in blocks)
    assert gzip.decompress(data) == text
    zhead, zbody = _split(text)
    assert zhead[:-1] == head[:-1] and zhead[-1].startswith(b"@PG\tID:mpibwa_gpu")
    assert sorted(zbody) == sorted(body)
    assert data.endswith(EOF_BLOCK) == (flag == "-b") and (blocks[-1][1] == b"") == (flag == "-b")
    assert len(data) < 0.6 * sum(len(ln) for ln in body)
    # the run says what the device path compressed: every chunk's text, and nothing but it (the header's blocks are zlib's)
    m = re.search(r"device BGZF: (\d+) blocks \((\d+) stored\), (\d+) bytes of text -> (\d+) bytes", r.stderr)
    assert m, r.stderr[-3000:]
    n_blocks, n_stored, n_in, n_out = (int(x) for x in m.groups())
    assert n_in == sum(len(ln) for ln in body) and n_stored == 0
    hdr_blocks = 0
    while hdr_blocks < len(blocks) and b"".join(p for _, p in blocks[:hdr_blocks]) != b"".join(zhead):
        hdr_blocks += 1
    chunk_blocks = blocks[hdr_blocks:len(blocks) - (flag == "-b")]
    assert n_blocks == len(chunk_blocks) and n_out == sum(len(b) for b, _ in chunk_blocks)


def test_level_is_noted_as_without_effect_and_the_option_needs_a_compressed_format(example, plain):
    d, prefix, fq = example
    out = os.path.join(d, "lvl.gz")
    r = _run(1, BASE + ["-g", "--device-bgzf", "--level", "9", "-o", out, prefix] + fq, d)
    assert "--level has no effect" in r.stderr
    assert sorted(_split(b"".join(p for _, p in _bgzf_blocks(open(out, "rb").read())))[1]) == sorted(plain[1])
    bad = os.path.join(d, "never.sam")
    r = _run(1, BASE + ["--device-bgzf", "-o", bad, prefix] + fq, d, ok=False)
    assert r.returncode != 0 and "usage:" in r.stderr and "--device-bgzf" in r.stderr and not os.path.exists(bad)


def test_by_chromosome_files_with_fixmate(example):
    d, prefix, fq = example
    recs = {}
    for extra in ([], ["--device-bgzf"]):
        dd = os.path.join(d, "bychr%d" % len(extra))
        os.makedirs(dd)
        r = _run(2, BASE + ["-f", "-b", "--by-chr"] + extra + ["-o", os.path.join(dd, "x.bam"), prefix] + fq, d)
        assert ("device BGZF:" in r.stderr) == bool(extra)
        got = {}
        for fn in sorted(os.listdir(dd)):
            data = open(os.path.join(dd, fn), "rb").read()
            blocks = _bgzf_blocks(data)
            assert data.endswith(EOF_BLOCK) and blocks[-1][1] == b""
            head, body = _split(b"".join(p for _, p in blocks))
            assert head and head[0].startswith(b"@SQ")
            got[fn] = (head[:-1], sorted(body))
        recs[len(extra)] = got
    assert recs[0] == recs[1] and sum(len(b) for _, b in recs[1].values()) >= 20000 and "unmapped.bam" in recs[1]


def test_without_the_option_a_compressed_run_writes_the_bytes_it_wrote_before(example, plain):
    """one rank, --ordered: the file is the header's blocks and then every chunk's, each made by mi355x_bgzf_compress at level 3"""
    from mpibwa_amd import api
    d, prefix, fq = example
    head, body = plain
    lib = api.load_library()
    out = os.path.join(d, "host.gz")
    r = _run(1, BASE + ["--ordered", "-g", "-o", out, prefix] + fq, d)
    assert "device BGZF" not in r.stderr
    data = open(out, "rb").read()
    zhead, zbody = _split(b"".join(p for _, p in _bgzf_blocks(data)))
    assert zhead[:-1] == head[:-1] and zbody == body
    # the chunks: -K 1000000 closes a chunk when its bases exceed K / 2 per file
    names, bases, chunks = [], 0, [[]]
    with open(fq[0], "rb") as f:
        lines = f.read().split(b"\n")
    first_of_chunk = {}
    for k in range(0, len(lines) - 3, 4):
        name = lines[k][1:].split()[0]
        if name.endswith(b"/1"):
            name = name[:-2]
        if bases == 0:
            first_of_chunk[name] = True
        bases += len(lines[k + 1])
        if bases > 500000:
            bases = 0
    for ln in body:
        q = ln.split(b"\t", 1)[0]
        if q in first_of_chunk and chunks[-1] and chunks[-1][-1].split(b"\t", 1)[0] != q:
            chunks.append([])
        chunks[-1].append(ln)
    assert len(chunks) == 3

    def host(t):
        cap = lib.mi355x_bgzf_bound(len(t))
        buf = C.create_string_buffer(cap)
        n = lib.mi355x_bgzf_compress(t, len(t), 3, buf, cap)
        return buf.raw[:n]
    assert data == host(b"".join(zhead)) + b"".join(host(b"".join(c)) for c in chunks)
