"""The device BAM path against the host path and against the device BGZF path on the same text -> profiles/bam_dev.json
(or --out FILE).

  python tools/bench_bam.py [--mb 270] [--rounds 5] [--e2e [pairs]] [--out FILE]

The text is tools/bench_bgzf.py's: the example reads with their real qualities laid out as SAM records on chr1 .. chr22 and repeated
to a chunk's size; it is not the aligner's own output.  Three legs take turns, --rounds times after one warm-up round each:
mi355x_bam_compress_dev, mi355x_bam_compress at level 3 (its own threads: MPIBWA_SAMPOST_THREADS, default the machine's cores), and
mi355x_bgzf_compress_dev on the same text — the difference between the first and the third is what the encoder passes cost or save
(BAM has fewer bytes to deflate, but denser ones).  Per call: wall seconds, GB/s of SAM text, output bytes over text bytes, and the
CPU-seconds of this process (all threads).  A measurement needs an MI355X; without one the device call ends the process.

--e2e: also tools/e2e_driver.py with E2E_P="8,8:-b --device-bgzf,8:--bam --device-bgzf,8:--bam" (wall time and file sizes per leg: plain
SAM, the reference's -b from the device deflate, real BAM from the device, real BAM on the cores); it builds the 3.1 Gbp synthetic
reference first, which takes far longer than the legs."""
import ctypes as C
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mpibwa_amd import abi, api  # noqa: E402
from bench_bgzf import chunk_text  # noqa: E402


def contigs():
    names = [b"chr%d" % k for k in range(1, 23)]
    anns = (abi.bntann1_t * len(names))()
    for i, n in enumerate(names):
        anns[i].name = n
        anns[i].anno = b""
        anns[i].len = 60_000_000
    bns = abi.bntseq_t()
    bns.n_seqs = len(names)
    bns.anns = anns
    return bns, anns


def main():
    args = sys.argv[1:]
    mb = int(args[args.index("--mb") + 1]) if "--mb" in args else 270
    rounds = int(args[args.index("--rounds") + 1]) if "--rounds" in args else 5
    lib = api.load_library()
    text = chunk_text(mb)
    bns, _keep = contigs()
    cap = lib.mi355x_bgzf_bound(max(lib.mi355x_bam_bound(len(text)), len(text)))
    out = C.create_string_buffer(cap)
    legs = {
        "bam_device": lambda: lib.mi355x_bam_compress_dev(text, len(text), C.byref(bns), out, cap),
        "bam_host_level_3": lambda: lib.mi355x_bam_compress(text, len(text), C.byref(bns), 3, out, cap),
        "bgzf_device_same_text": lambda: lib.mi355x_bgzf_compress_dev(text, len(text), out, cap),
    }
    res = {"box": platform.node(), "cores": int(lib.mi355x_host_cpus()), "text_bytes": len(text),
           "text": "example reads (real qualities) as SAM-like records, repeated to a chunk's size", "rounds": rounds, "legs": {}}
    sizes = {}
    for name, f in legs.items():   # warm-up: buffers, streams, threads, code objects
        sizes[name] = f()
        assert sizes[name] > 0, (name, sizes[name])
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
        res["legs"][name] = {"output_bytes": sizes[name], "output_over_text": round(sizes[name] / len(text), 4),
                             "wall_s": [round(w, 4) for w in wall], "wall_s_median": round(statistics.median(wall), 4),
                             "GB_per_s_of_text_median": round(len(text) / statistics.median(wall) / 1e9, 3),
                             "GB_per_s_of_text_best": round(len(text) / min(wall) / 1e9, 3),
                             "process_cpu_s_per_call_median": round(statistics.median(cpu), 3)}
    c = (C.c_uint64 * 6)()
    lib.mi355x_bam_dev_counts(c)
    res["bam_device_counts"] = dict(zip(("records", "records_by_the_host_encoder", "sam_bytes", "bam_bytes", "blocks", "compressed_bytes"), list(c)))
    if "--e2e" in args:
        k = args.index("--e2e")
        pairs = args[k + 1] if k + 1 < len(args) and args[k + 1].isdigit() else "2000000"
        lib.mi355x_finalize()
        env = dict(os.environ, E2E_P="8,8:-b --device-bgzf,8:--bam --device-bgzf,8:--bam")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "e2e_driver.py"), pairs], check=True, env=env, stdout=subprocess.PIPE, text=True)
        res["driver_legs"] = json.loads(r.stdout.strip().splitlines()[-1])   # (its last line is its result)
    else:
        res["driver_legs"] = "not measured"
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "bam_dev.json")
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
