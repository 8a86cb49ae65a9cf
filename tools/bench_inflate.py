"""The device inflate against zlib on the cores -> profiles/inflate_dev.json (or --out FILE).

  python tools/bench_inflate.py [--mb 200] [--rounds 5] [--threads 16] [--e2e [pairs]] [--out FILE]

Stage rate: one chunk's worth of FASTQ text — the example reads of tests/golden/mpibwa_examples REPEATED with fresh names until they
are --mb megabytes — as BGZF blocks of zlib level 6 (mi355x_bgzf_compress: 65 280 bytes of text per block, cut at line ends).
mi355x_bgzf_inflate_dev and mi355x_bgzf_inflate (--threads host threads: MPIBWA_SAMPOST_THREADS) take turns, --rounds times after one
warm-up call each; per call: wall seconds, GB/s of text, and the CPU-seconds of this process (time.process_time: all threads).  The
yardstick is zlib on the cores.  A measurement needs an MI355X; without one the device call ends the process.

--e2e: also the program, as tools/e2e_driver.py runs it (`mpiexec -n 1 mpibwa_gpu mem -K 100000000 --in-flight 8` on 2 x pairs reads of
SURVEY §8d's workload, 2 000 000 pairs = six chunks): plain FASTQ, the same files bgzipped (level 6) through the host path, and
through --device-inflate; per leg the driver's own chunk-loop clock, the process's wall time and the CPU-seconds of the whole run
(user + system of mpiexec and its children: index load, fq_open's scan and the chunk loop), and whether the sorted records are the
plain leg's.  It builds the 3.1 Gbp synthetic reference first.

Not measured here: several ranks, a long run, the kernel's own duration per piece."""
import ctypes as C
import gzip
import json
import os
import hashlib
import platform
import re
import resource
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def chunk_text(mb):
    with gzip.open(os.path.join(ROOT, "tests", "golden", "mpibwa_examples", "HCC1187C_R1_10K.fastq.gz"), "rb") as g:
        lines = g.read().split(b"\n")
    reads = [(lines[k].split()[0], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]
    out, size, rep = [], 0, 0
    while size < mb << 20:
        for name, seq, qual in reads:
            out.append(b"%s.%d 1:N:0:1\n%s\n+\n%s\n" % (name, rep, seq, qual))
            size += len(out[-1])
        rep += 1
    return b"".join(out)


def driver_legs(lib, pairs):
    """plain, bgzipped through the host path, bgzipped through --device-inflate: one rank, eight chunks in flight"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mpibwa_amd import bigindex
    from test_driver import EXE, mpiexec
    wd = os.environ.get("MPIBWA_BENCH_DIR", "/tmp/mpibwa_bench")
    os.makedirs(wd, exist_ok=True)
    idx = bigindex.make_or_get(wd, genome_mbp=3100, seed=38, log=lambda *a: print(*a, file=sys.stderr, flush=True), model="grch38like", repeat_frac=0.05)
    fq = [os.path.join(wd, "inf_R1.fastq"), os.path.join(wd, "inf_R2.fastq")]
    with open(fq[0], "wb") as f1, open(fq[1], "wb") as f2:
        for part in range(0, pairs, 250_000):
            for name, a, b in idx.simulate_pairs(min(250_000, pairs - part), seed=900 + part):
                nm = ("@p%d_%s" % (part, name)).encode()
                f1.write(nm + b"/1\n" + a + b"\n+\n" + b"I" * len(a) + b"\n")
                f2.write(nm + b"/2\n" + b + b"\n+\n" + b"I" * len(b) + b"\n")
    gz, sizes = [], []
    for path in fq:
        text = open(path, "rb").read()
        cap = lib.mi355x_bgzf_bound(len(text))
        z = C.create_string_buffer(cap)
        n = lib.mi355x_bgzf_compress(text, len(text), 6, z, cap)
        with open(path + ".gz", "wb") as f:
            f.write(z.raw[:n])
        gz.append(path + ".gz")
        sizes.append((len(text), n))
        del z, text
    cores = int(lib.mi355x_host_cpus())
    lib.mi355x_finalize()          # the driver process brings its own copy of the index onto the GPU
    env = dict(os.environ)
    env.pop("LD_LIBRARY_PATH", None)
    out, legs, want = os.path.join(wd, "inf_drv.sam"), [], None
    for name, extra, files in (("plain FASTQ", [], fq), ("bgzipped, host path", [], gz), ("bgzipped, --device-inflate", ["--device-inflate"], gz)):
        u0, t0 = resource.getrusage(resource.RUSAGE_CHILDREN), time.time()
        r = subprocess.run([mpiexec(), "-n", "1", EXE, "mem", "-t", str(cores), "-K", "100000000", "--in-flight", "8"] + extra + ["-o", out, idx.prefix] + files,
                           capture_output=True, text=True, env=env, timeout=1500)
        wall, u1 = time.time() - t0, resource.getrusage(resource.RUSAGE_CHILDREN)
        m = re.search(r"chunk loop: (\d+) reads in (\d+) chunks.* ([\d.]+) s = ([\d.]+) Mreads/s", r.stderr)
        if r.returncode != 0 or not m:
            print(r.stderr[-3000:], file=sys.stderr)
            raise SystemExit("driver failed")
        lines = sorted(ln for ln in open(out, "rb").read().splitlines(keepends=True) if not ln.startswith(b"@"))
        md5 = hashlib.md5(b"".join(lines)).hexdigest()
        want = want or md5
        rep = re.search(r"BGZF input: .*", r.stderr)
        legs.append({"leg": name, "args": extra, "reads": int(m.group(1)), "chunks": int(m.group(2)), "chunk_loop_s": float(m.group(3)), "Mreads_per_s": float(m.group(4)),
                     "process_wall_s": round(wall, 2), "cpu_s_user_plus_system_whole_run": round(u1.ru_utime - u0.ru_utime + u1.ru_stime - u0.ru_stime, 2),
                     "records": len(lines), "same_records_as_plain": md5 == want, "report": rep.group(0) if rep else None})
        print(legs[-1], file=sys.stderr, flush=True)
    return {"pairs": pairs, "fastq_bytes_and_bgzf_bytes": sizes, "in_flight": 8, "ranks": 1, "legs": legs}


def main():
    args = sys.argv[1:]
    mb = int(args[args.index("--mb") + 1]) if "--mb" in args else 200
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 5
    threads = int(args[args.index("--threads") + 1]) if "--threads" in args else 16
    os.environ["MPIBWA_SAMPOST_THREADS"] = str(threads)
    from mpibwa_amd import api
    lib = api.load_library()
    text = chunk_text(mb)
    cap = lib.mi355x_bgzf_bound(len(text))
    z = C.create_string_buffer(cap)
    n_z = lib.mi355x_bgzf_compress(text, len(text), 6, z, cap)
    assert n_z > 0
    data = z.raw[:n_z]
    del z
    out = C.create_string_buffer(len(text))
    legs = {
        "device": lambda: lib.mi355x_bgzf_inflate_dev(data, len(data), out, len(text)),
        "host_zlib": lambda: lib.mi355x_bgzf_inflate(data, len(data), out, len(text)),
    }
    res = {"box": platform.node(), "cores": int(lib.mi355x_host_cpus()), "host_threads": threads, "text_bytes": len(text), "compressed_bytes": len(data),
           "text": "example reads as FASTQ, repeated with fresh names to a chunk's size; BGZF blocks of zlib level 6", "rounds": rounds, "legs": {}}
    for name, f in legs.items():   # warm-up: buffers, streams, threads, code objects; and the result itself
        assert f() == len(text) and out.raw == text, name
    times = {k: [] for k in legs}
    for _ in range(rounds):        # alternating
        for name, f in legs.items():
            c0, t0 = time.process_time(), time.perf_counter()
            n = f()
            times[name].append((time.perf_counter() - t0, time.process_time() - c0))
            assert n == len(text)
    for name in legs:
        wall = [w for w, _ in times[name]]
        cpu = [c for _, c in times[name]]
        res["legs"][name] = {"wall_s": [round(w, 4) for w in wall], "wall_s_median": round(statistics.median(wall), 4),
                             "GB_per_s_of_text_median": round(len(text) / statistics.median(wall) / 1e9, 3),
                             "GB_per_s_of_text_best": round(len(text) / min(wall) / 1e9, 3),
                             "process_cpu_s_per_call_median": round(statistics.median(cpu), 3)}
    c = (C.c_uint64 * 4)()
    lib.mi355x_bgzf_inflate_dev_counts(c)
    res["device_counts"] = {"blocks": c[0], "failed": c[1], "bytes_in": c[2], "bytes_out": c[3]}
    if "--e2e" in args:
        k = args.index("--e2e")
        res["driver_legs"] = driver_legs(lib, int(args[k + 1]) if k + 1 < len(args) and args[k + 1].isdigit() else 2_000_000)
    else:
        res["driver_legs"] = "not measured"
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "inflate_dev.json")
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
