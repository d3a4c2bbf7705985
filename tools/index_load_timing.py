#!/usr/bin/env python3
"""What opening a saved index costs (sg_index_load_reference_ex, index_load.inc / ref_index_reader.cpp): at 1 M and 10 M
synthetic strings (synth.make_dict, built on the device, saved with the device encoder to a temporary directory) the files are
loaded, without an upload,
  - with the device decoder: one warm-up load, then the median of five;
  - with the host reader (device = -1, the reader as it was before the device route existed): one warm-up load, then the median
    of three.
The per-phase milliseconds come from the library (sg_debug_index_load_times): reading the files, parsing the header and interning
the terms, host-to-device copies, the kernels (the host decoders on the host route), device-to-host copies, assembly, the whole
call; the call is also timed from Python around it.  The digests of the two routes are compared.  Writes
profiles/index_load_timing.json and prints it.  GPU box only."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_load_timing.json"))
args = ap.parse_args()

PHASES = ("read_ms", "parse_ms", "h2d_ms", "decode_ms", "d2h_ms", "assemble_ms", "call_ms")
DESC = IndexDescription(**synth.DESCRIPTION)


def timed_load(hd, dl, decode_device):
    out = (C.c_double * 7)()
    t0 = time.perf_counter()
    ix = NGramIndex.from_reference_files(hd, dl, DESC, upload=False, decode_device=decode_device)
    wall = (time.perf_counter() - t0) * 1e3
    _lib.check(_lib.lib().sg_debug_index_load_times(out, 7))
    row = dict(zip(PHASES, out), wall_ms=wall)
    digest = ix.digest()
    ix.close()
    return row, digest


def median_of(runs):
    return {k: round(statistics.median(r[k] for r in runs), 2) for k in runs[0]}


record = {"tool": "tools/index_load_timing.py", "sizes": []}
for n in args.sizes:
    blob, offs = synth.make_dict(n, seed=1)
    ix = NGramIndex(blob=blob, offs=offs, description=DESC, device=args.device, upload=False, build="device")
    st = ix.stats()
    with tempfile.TemporaryDirectory() as tmp:
        hd, dl = os.path.join(tmp, "d.hd"), os.path.join(tmp, "d.dl")
        ix.save(hd, dl, device=args.device)
        ix.close()
        timed_load(hd, dl, args.device)                                   # warm-up: code objects, first allocations, the page cache
        dev = [timed_load(hd, dl, args.device) for _ in range(5)]
        timed_load(hd, dl, -1)
        host = [timed_load(hd, dl, -1) for _ in range(3)]
        row = {"strings": n, "lists": st["n_lists"], "postings": st["n_postings"], "postings_raw": st["n_postings_raw"],
               "dl_bytes": os.path.getsize(dl), "hd_bytes": os.path.getsize(hd),
               "digests_identical": len({d for _, d in dev + host}) == 1,
               "device": median_of([r for r, _ in dev]), "host": median_of([r for r, _ in host]),
               "device_call_runs_ms": [round(r["call_ms"], 2) for r, _ in dev], "host_call_runs_ms": [round(r["call_ms"], 2) for r, _ in host]}
        row["host_call_over_device_call"] = round(row["host"]["call_ms"] / max(row["device"]["call_ms"], 1e-9), 2)
        row["host_decode_assemble_over_device_h2d_decode_d2h_assemble"] = round(
            (row["host"]["decode_ms"] + row["host"]["assemble_ms"]) /
            max(sum(row["device"][k] for k in ("h2d_ms", "decode_ms", "d2h_ms", "assemble_ms")), 1e-9), 2)
    record["sizes"].append(row)
    print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
