"""mpibwa_gpu --bam on the GPU box: real BAM files.  On the example data, --bam and --bam --device-bgzf on one and two
ranks, and [-f] --bam --device-bgzf --by-chr (with discordant.bam when there is no -f): every file is well-formed BGZF that ends in the 28-byte empty block, its payload is the BAM
magic, the plain run's header text (up to @PG), the contigs of the index and records that decode (tests/bam_model.py) to the plain
run's records; every block behind the header holds whole records; the run reports what the device path encoded.  --bam together with
-b is a usage error, and a -b run without --bam writes what it wrote before: mi355x_bgzf_compress over the header and the chunks."""
import ctypes as C
import gzip
import os
import re
import subprocess
import tarfile

import pytest

import bam_model as bm

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


def _split(text):
    lines = text.splitlines(keepends=True)
    return [ln for ln in lines if ln.startswith(b"@")], [ln for ln in lines if not ln.startswith(b"@")]


@pytest.fixture(scope="module")
def example(tmp_path_factory, built):
    from mpibwa_amd import api
    api.load_library().mi355x_finalize()
    d = tmp_path_factory.mktemp("bamdrv")
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
    """the plain runs, one rank, chunks in input order: without and with -f"""
    d, prefix, fq = example
    out = {}
    for extra in ((), ("-f",)):
        path = os.path.join(d, "plain%d.sam" % len(extra))
        _run(1, BASE + list(extra) + ["--ordered", "-o", path, prefix] + fq, d)
        out[extra] = _split(open(path, "rb").read())
        assert len(out[extra][1]) >= 20000
    return out


def _contigs(head):
    out = []
    for ln in head:
        if ln.startswith(b"@SQ"):
            f = dict(x.split(b":", 1) for x in ln.rstrip(b"\n").split(b"\t")[1:])
            out.append((f[b"SN"], int(f[b"LN"])))
    return out


def _read_bam(path, head):
    """-> (blocks behind the header, decoded records as normalised SAM lines); the header is held against the plain run's"""
    data = open(path, "rb").read()
    blocks = bm.bgzf_blocks(data)
    assert data.endswith(EOF_BLOCK) and blocks[-1][1] == b"" and all(p for _, p in blocks[:-1])
    stream = b"".join(p for _, p in blocks)
    text, contigs, at = bm.decode_header(stream)
    zhead = text.splitlines(keepends=True)
    assert zhead[:-1] == head[:-1] and zhead[-1].startswith(b"@PG\tID:mpibwa_gpu") and b"\0" not in text
    assert contigs == _contigs(head) and len(contigs) >= 1
    hdr_blocks, seen = 0, 0
    while seen < at:
        seen += len(blocks[hdr_blocks][1])
        hdr_blocks += 1
    assert seen == at   # the header's blocks hold the header alone
    body = blocks[hdr_blocks:-1]
    names = [n for n, _ in contigs]
    lines = []
    for _, p in body:
        recs = bm.split_records(p)   # whole records: the block_size chain ends at the payload's end
        lines += [bm.decode_record(r, names) + b"\n" for r in recs]
    return body, lines


def _want(body):
    return sorted(bm.normalise(ln.rstrip(b"\n")) + b"\n" for ln in body)


@pytest.mark.parametrize("device,ranks", [(False, 1), (False, 2), (True, 1), (True, 2)])
def test_bam_files_hold_the_plain_runs_records(example, plain, device, ranks):
    d, prefix, fq = example
    head, body = plain[()]
    out = os.path.join(d, "out%d%d.bam" % (device, ranks))
    r = _run(ranks, BASE + ["--bam"] + (["--device-bgzf"] if device else []) + ["-o", out, prefix] + fq, d)
    blocks, lines = _read_bam(out, head)
    assert sorted(lines) == _want(body)
    assert os.path.getsize(out) < 0.6 * sum(len(ln) for ln in body)
    m = re.search(REPORT, r.stderr)
    assert bool(m) == device, r.stderr[-3000:]
    assert "device BGZF:" not in r.stderr
    if device:
        n_rec, n_host, n_sam, n_bam, n_blocks, n_out = (int(x) for x in m.groups())
        assert (n_rec, n_host, n_sam) == (len(body), 0, sum(len(ln) for ln in body))
        assert (n_bam, n_blocks, n_out) == (sum(len(p) for _, p in blocks), len(blocks), sum(len(b) for b, _ in blocks))


REPORT = r"device BAM: (\d+) records \((\d+) by the host encoder\), (\d+) bytes of SAM -> (\d+) bytes of BAM in (\d+) blocks -> (\d+) bytes"


@pytest.mark.parametrize("fixmate", [True, False])
def test_by_chromosome_files_are_complete_bams(example, plain, fixmate):
    """with -f: contigs and unmapped; without: also discordant.bam, whose records are the ones whose RNAME and RNEXT are two contigs"""
    d, prefix, fq = example
    head, body = plain[("-f",) if fixmate else ()]
    dd = os.path.join(d, "bychr%d" % fixmate)
    os.makedirs(dd)
    r = _run(2, BASE + (["-f"] if fixmate else []) + ["--bam", "--device-bgzf", "--by-chr", "-o", os.path.join(dd, "x.bam"), prefix] + fq, d)
    names = [n for n, _ in _contigs(head)]
    got, disc, files, all_blocks = [], [], sorted(os.listdir(dd)), []
    assert files == sorted([n.decode() + ".bam" for n in names] + ["unmapped.bam"] + ([] if fixmate else ["discordant.bam"]))
    for fn in files:
        blocks, lines = _read_bam(os.path.join(dd, fn), head)
        all_blocks += blocks
        if fn == "discordant.bam":
            disc = lines
            continue
        for ln in lines:
            assert ln.split(b"\t")[2] == (b"*" if fn == "unmapped.bam" else fn[:-4].encode())
        got += lines
    assert sorted(got) == _want(body)
    if not fixmate:
        def two_contigs(ln):
            f = ln.split(b"\t")
            return f[2] != b"*" and f[6] not in (b"=", b"*", f[2])
        assert sorted(disc) == sorted(ln for ln in _want(body) if two_contigs(ln))
    # the run's report equals what the files hold
    m = re.search(REPORT, r.stderr)
    assert m, r.stderr[-3000:]
    n_rec, n_host, n_sam, n_bam, n_blocks, n_out = (int(x) for x in m.groups())
    in_files = got + disc
    assert (n_rec, n_host) == (len(in_files), 0)
    assert (n_bam, n_blocks, n_out) == (sum(len(p) for _, p in all_blocks), len(all_blocks), sum(len(b) for b, _ in all_blocks))
    text_of = {bm.normalise(ln.rstrip(b"\n")) + b"\n": len(ln) for ln in body}
    assert n_sam == sum(text_of[ln] for ln in in_files)


def test_bam_with_b_is_a_usage_error_and_b_alone_writes_what_it_wrote(example, plain):
    from mpibwa_amd import api
    d, prefix, fq = example
    head, body = plain[()]
    for other in ("-b", "-g"):
        bad = os.path.join(d, "never.bam")
        r = _run(1, BASE + ["--bam", other, "-o", bad, prefix] + fq, d, ok=False)
        assert r.returncode != 0 and "usage:" in r.stderr and "--bam" in r.stderr and not os.path.exists(bad)
    lib = api.load_library()
    out = os.path.join(d, "host_b.bam")
    r = _run(1, BASE + ["--ordered", "-b", "-o", out, prefix] + fq, d)
    assert "device BAM" not in r.stderr
    data = open(out, "rb").read()
    zhead, zbody = _split(b"".join(p for _, p in bm.bgzf_blocks(data)))
    assert zhead[:-1] == head[:-1] and zbody == body and data.endswith(EOF_BLOCK)
    # the chunks: -K 1000000 closes a chunk when its bases exceed K / 2 per file (tests/test_gpu_bgzf_driver.py)
    bases, first_of_chunk, chunks = 0, set(), [[]]
    with open(fq[0], "rb") as f:
        lines = f.read().split(b"\n")
    for k in range(0, len(lines) - 3, 4):
        name = lines[k][1:].split()[0]
        if name.endswith(b"/1"):
            name = name[:-2]
        if bases == 0:
            first_of_chunk.add(name)
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
    assert data == host(b"".join(zhead)) + b"".join(host(b"".join(c)) for c in chunks) + EOF_BLOCK
