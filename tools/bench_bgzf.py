"""The device BGZF path against the host path -> profiles/bgzf_dev.json (or --out FILE).

  python tools/bench_bgzf.py [--mb 270] [--rounds 5] [--e2e [pairs]] [--out FILE]

Stage rate: a SAM text of a chunk's size — the example reads of tests/golden/mpibwa_examples laid out as records with their real
qualities (the recipe of tests/test_gpu_bgzf.py), REPEATED with fresh names and positions until it is --mb megabytes (270: a chunk of
667 k reads); it is not the aligner's own output.  mi355x_bgzf_compress_dev and mi355x_bgzf_compress at levels 1 and 3 (its own
threads: the machine's cores, MPIBWA_SAMPOST_THREADS) take turns, --rounds times after one warm-up round each; per call: wall seconds,
GB/s of text, compressed / text, and the CPU-seconds of this process (time.process_time: all threads).  A measurement needs an
MI355X; without one the device call ends the process.

--e2e: also tools/e2e_driver.py with E2E_P="8,8:-g,8:-g --device-bgzf,8:-f -b,8:-f -b --device-bgzf" (wall time and file sizes per
leg); it builds the 3.1 Gbp synthetic reference first, which takes far longer than the legs."""
import ctypes as C
import gzip
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mpibwa_amd import api  # noqa: E402


def chunk_text(mb, seed=9):
    import numpy as np
    rng = np.random.default_rng(seed)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "mpibwa_examples", "HCC1187C_R1_10K.fastq.gz"), "rb") as g:
        lines = g.read().split(b"\n")
    reads = [(lines[k][1:].split()[0], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 3, 4)]
    out, size, rep = [], 0, 0
    while size < mb << 20:
        pos = rng.integers(1, 50_000_000, len(reads))
        for k, (name, seq, qual) in enumerate(reads):
            out.append(b"%s.%d\t%d\tchr%d\t%d\t60\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:%d\tMD:Z:%d\tAS:i:%d\tXS:i:%d\n" % (
                name, rep, 99 if k % 2 else 147, 1 + k % 22, pos[k], len(seq), pos[k] + 250, 350, seq, qual, k % 3, len(seq), len(seq) - k % 7, k % 40))
            size += len(out[-1])
        rep += 1
    return b"".join(out)


def main():
    args = sys.argv[1:]
    mb = int(args[args.index("--mb") + 1]) if "--mb" in args else 270
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 5
    lib = api.load_library()
    text = chunk_text(mb)
    cap = lib.mi355x_bgzf_bound(len(text))
    out = C.create_string_buffer(cap)
    legs = {
        "device": lambda: lib.mi355x_bgzf_compress_dev(text, len(text), out, cap),
        "host_level_1": lambda: lib.mi355x_bgzf_compress(text, len(text), 1, out, cap),
        "host_level_3": lambda: lib.mi355x_bgzf_compress(text, len(text), 3, out, cap),
    }
    res = {"box": platform.node(), "cores": int(lib.mi355x_host_cpus()), "text_bytes": len(text),
           "text": "example reads (real qualities) as SAM-like records, repeated to a chunk's size", "rounds": rounds, "legs": {}}
    sizes = {}
    for name, f in legs.items():   # warm-up: buffers, streams, threads, code objects
        sizes[name] = f()
        assert sizes[name] > 0
    times = {k: [] for k in legs}
    for _ in range(rounds):        # alternating
        for name, f in legs.items():
            c0, t0 = time.process_time(), time.perf_counter()
            n = f()
            times[name].append((time.perf_counter() - t0, time.process_time() - c0))
            assert n == sizes[name]
    for name in legs:
        wall = [w for w, _ in times[name]]
        cpu = [c for _, c in times[name]]
        res["legs"][name] = {"compressed_bytes": sizes[name], "compressed_over_text": round(sizes[name] / len(text), 4),
                             "wall_s": [round(w, 4) for w in wall], "wall_s_median": round(statistics.median(wall), 4),
                             "GB_per_s_of_text_median": round(len(text) / statistics.median(wall) / 1e9, 3),
                             "GB_per_s_of_text_best": round(len(text) / min(wall) / 1e9, 3),
                             "process_cpu_s_per_call_median": round(statistics.median(cpu), 3)}
    c = (C.c_uint64 * 4)()
    lib.mi355x_bgzf_dev_counts(c)
    res["device_counts"] = {"blocks": c[0], "stored": c[1], "bytes_in": c[2], "bytes_out": c[3]}
    if "--e2e" in args:
        k = args.index("--e2e")
        pairs = args[k + 1] if k + 1 < len(args) and args[k + 1].isdigit() else "2000000"
        lib.mi355x_finalize()
        env = dict(os.environ, E2E_P="8,8:-g,8:-g --device-bgzf,8:-f -b,8:-f -b --device-bgzf")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "e2e_driver.py"), pairs], check=True, env=env, stdout=subprocess.PIPE, text=True)
        res["driver_legs"] = json.loads(r.stdout.strip().splitlines()[-1])   # (its last line is its result)
    else:
        res["driver_legs"] = "not measured"
    out = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "bgzf_dev.json")
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
