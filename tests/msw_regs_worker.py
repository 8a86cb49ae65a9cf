"""Worker of tests/test_gpu_msw_regs.py: a process of its own, so that what launch_msw reads from the environment once per process
(MPIBWA_MSW_REGS) can differ from the test session's.
usage: msw_regs_worker.py <index prefix> <out.npz> <reads.json: [(name, seq1, seq2)] of the two-length chunk>
Writes Engine.matesw's records of every family and option set of tests/msw_regs_cases.py (key "<family>/<option set>") and the SAM of
the two-length chunk (key "sam", bytes) to out.npz; prints RESULT <json>."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msw_cases as mc  # noqa: E402
import msw_regs_cases as rc  # noqa: E402
from mpibwa_amd import abi, api  # noqa: E402

prefix, out, reads_json = sys.argv[1], sys.argv[2], sys.argv[3]
eng = api.Engine(prefix, device=0)
res = {}
for family, name in rc.all_cases():
    cs = rc.cases(family, name)
    res["%s/%s" % (family, name)] = eng.matesw(mc.set_opt(eng.opt(), name), *cs.matesw_args())[0]
with open(reads_json) as f:
    reads = [(n, a.encode(), b.encode()) for n, a, b in json.load(f)]
sam = b"".join(eng.process(eng.opt(flag=abi.MEM_F_PE), reads))
res["sam"] = np.frombuffer(sam, dtype=np.uint8)
np.savez(out, **res)
print("RESULT " + json.dumps(dict(regs_env=os.environ.get("MPIBWA_MSW_REGS"), n_msw=int(eng.stats()["n_msw"]), sam_bytes=len(sam))), flush=True)
