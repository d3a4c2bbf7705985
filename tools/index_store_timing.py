#!/usr/bin/env python3
"""What saving an index costs (sg_index_store_reference, index_store.inc / index_store.cpp): at 1 M and 10 M synthetic strings
(synth.make_dict, built on the device) the index is saved to a temporary directory
  - with the device encoder: one warm-up call, then the median of five — the kernels and the position scan, the staging copies
    (host CSR to the device, the encoded bytes back), building and writing the header, and the whole call with the file writes;
  - with the host encoder (device = -1): one warm-up call, then the median of three — the encoder, the header, the whole call.
The per-phase seconds come from the library (sg_debug_index_store_times); the whole call is also timed from Python around it.
The files of the two encoders are compared byte for byte.  Writes profiles/index_store_timing.json and prints it.  GPU box only."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:
    import torch  # noqa: F401  (first, so libamdhip64 is shared with torch)
except Exception:
    pass

from suggest_amd import IndexDescription, NGramIndex, _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_store_timing.json"))
args = ap.parse_args()


def timed_save(ix, hd, dl, device):
    out = (C.c_double * 4)()
    t0 = time.perf_counter()
    ix.save(hd, dl, device=device)
    wall = time.perf_counter() - t0
    _lib.check(_lib.lib().sg_debug_index_store_times(out))
    return dict(encode=out[0], staging=out[1], header=out[2], call=out[3], wall=wall)


def median_of(runs):
    return {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0]}


record = {"tool": "tools/index_store_timing.py", "sizes": []}
for n in args.sizes:
    blob, offs = synth.make_dict(n, seed=1)
    t0 = time.perf_counter()
    ix = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), device=args.device, upload=False, build="device")
    build_s = time.perf_counter() - t0
    st = ix.stats()
    with tempfile.TemporaryDirectory() as tmp:
        dev, host = (os.path.join(tmp, "d.hd"), os.path.join(tmp, "d.dl")), (os.path.join(tmp, "h.hd"), os.path.join(tmp, "h.dl"))
        timed_save(ix, dev[0], dev[1], args.device)                       # warm-up: code objects, first allocations
        dev_runs = [timed_save(ix, dev[0], dev[1], args.device) for _ in range(5)]
        timed_save(ix, host[0], host[1], -1)
        host_runs = [timed_save(ix, host[0], host[1], -1) for _ in range(3)]
        same = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(dev, host))
        row = {"strings": n, "build_device_s": round(build_s, 3), "lists": st["n_lists"], "postings": st["n_postings"], "postings_raw": st["n_postings_raw"],
               "dl_bytes": os.path.getsize(dev[1]), "hd_bytes": os.path.getsize(dev[0]), "files_identical": same,
               "device": median_of(dev_runs), "host": median_of(host_runs),
               "device_encode_runs_s": [round(r["encode"], 4) for r in dev_runs], "host_encode_runs_s": [round(r["encode"], 4) for r in host_runs]}
        row["host_encode_over_device_encode_plus_staging"] = round(row["host"]["encode"] / max(row["device"]["encode"] + row["device"]["staging"], 1e-9), 2)
    record["sizes"].append(row)
    ix.close()
    print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
