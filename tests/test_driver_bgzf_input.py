"""mpibwa_gpu on BGZF-compressed FASTQ (driver/mpibwa_gpu.c: bgzf_table, read_text): a compressed file is its text, so the chunk table
that --dry-run prints for the bgzipped files is the one for the plain files, line for line, for any number of ranks and any -K, in the
single-end, lockstep and trimmed modes.  The blocks hold 700 bytes of text each, so records straddle blocks and the ranks' byte slices
start in the middle of blocks.  CPU only: --dry-run inflates on the cores whatever --device-inflate says."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_in_cases as cases
from test_driver import EXE, mpiexec

pytestmark = pytest.mark.skipif(mpiexec() is None, reason="no mpiexec in this container")


def _run(ranks, args, cwd):
    env = dict(os.environ)
    env.pop("LD_LIBRARY_PATH", None)
    return subprocess.run([mpiexec(), "-n", str(ranks), EXE, "mem", "--dry-run"] + args, capture_output=True, text=True, timeout=300, env=env, cwd=cwd)


def _table(ranks, args, cwd):
    r = _run(ranks, args, cwd)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()


def _bgzip(path, text, size=700):
    with open(path, "wb") as f:
        f.write(cases.blocks(text, size) + cases.EOF_BLOCK)
    return path


@pytest.fixture(scope="module")
def files(built, tmp_path_factory):
    if not os.path.exists(EXE):
        pytest.skip("mpibwa_gpu not built (no MPI installation)")
    d = tmp_path_factory.mktemp("bgzf_in")
    rng = np.random.default_rng(12)
    n = 1200

    def fastq(lens, tag):
        out = []
        for i, ln in enumerate(lens):
            seq = bytes(rng.choice(list(b"ACGT"), ln).tolist())
            qual = bytes([64]) + bytes(rng.choice(list(b"@+IJ#"), ln - 1).tolist())     # quality lines that start with '@'
            out.append(b"@q%05d/%d\n%s\n+\n%s\n" % (i, tag, seq, qual))
        return b"".join(out)
    even = [100] * n
    texts = {"R1": fastq(even, 1), "R2": fastq(even, 2),
             "T1": fastq([int(x) for x in rng.integers(30, 160, n)], 1), "T2": fastq([int(x) for x in rng.integers(30, 160, n)], 2)[:-1]}
    assert len(texts["R1"]) == len(texts["R2"]) and len(texts["T1"]) != len(texts["T2"])
    paths = {}
    for name, text in texts.items():
        plain = str(d / (name + ".fastq"))
        with open(plain, "wb") as f:
            f.write(text)
        paths[name] = (plain, _bgzip(str(d / (name + ".fastq.gz")), text))
    return str(d), paths, texts


@pytest.mark.parametrize("mode,names", [("se", ["R1"]), ("pe", ["R1", "R2"]), ("pe_trim", ["T1", "T2"])])
def test_the_chunk_table_is_that_of_the_plain_files(files, mode, names):
    d, paths, _ = files
    for K in (20_000, 7_000):
        for ranks in (1, 2, 3):
            want = _table(ranks, ["-K", str(K), "PREFIX_UNUSED"] + [paths[x][0] for x in names], d)
            assert want[0].split()[1] == mode and len(want) > 6
            got = _table(ranks, ["-K", str(K), "--device-inflate", "PREFIX_UNUSED"] + [paths[x][1] for x in names], d)
            assert got == want, (mode, K, ranks)


def test_r1_compressed_with_r2_plain_and_more_ranks_than_blocks(files):
    d, paths, texts = files
    want = _table(2, ["-K", "30000", "PREFIX_UNUSED", paths["R1"][0], paths["R2"][0]], d)
    assert _table(2, ["-K", "30000", "PREFIX_UNUSED", paths["R1"][1], paths["R2"][0]], d) == want
    assert _table(2, ["-K", "30000", "PREFIX_UNUSED", paths["R1"][0], paths["R2"][1]], d) == want
    # one block of text and the EOF block on three ranks: two slices hold no block start
    small = texts["R1"][:213 * 40]
    plain, packed = os.path.join(d, "small.fastq"), os.path.join(d, "small.fastq.gz")
    with open(plain, "wb") as f:
        f.write(small)
    _bgzip(packed, small, size=65280)
    assert _table(3, ["-K", "2000", "PREFIX_UNUSED", packed], d) == _table(3, ["-K", "2000", "PREFIX_UNUSED", plain], d)


def test_plain_gzip_is_refused_with_one_line_that_names_the_file(files):
    d, paths, texts = files
    path = os.path.join(d, "plain_gzip.fastq.gz")
    with gzip.open(path, "wb") as g:
        g.write(texts["R1"])
    r = _run(2, ["-K", "30000", "PREFIX_UNUSED", path], d)
    assert r.returncode != 0
    lines = [ln for ln in r.stderr.splitlines() if "[mpibwa_gpu]" in ln]
    assert len(lines) == 1 and path in lines[0] and "bgzip" in lines[0] and "unpack" in lines[0]


def test_a_damaged_block_ends_the_run_and_names_its_offset(files):
    d, paths, _ = files
    data = bytearray(open(paths["R1"][1], "rb").read())
    off = [o for o, _ in cases.split(bytes(data))][7]
    data[off + 30] ^= 0xff
    path = os.path.join(d, "damaged.fastq.gz")
    with open(path, "wb") as f:
        f.write(data)
    r = _run(1, ["-K", "30000", "PREFIX_UNUSED", path], d)
    assert r.returncode != 0 and ("byte %d " % off) in r.stderr
