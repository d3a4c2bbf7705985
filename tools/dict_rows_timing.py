#!/usr/bin/env python3
"""What returning result rows as strings costs (sg_dictionary, suggest_amd/csrc/dict_rows.inc): the synthetic
dictionary and query batch of bench.py's headline config (synth.make_dict / make_queries, jaccard 0.5), at k = 10 and 100.  Per k,
one warm-up and the median of `--reps` runs:
  (a) search_ms        sg_suggest_batch_device alone, device-resident buffers                          device events
  (b) materialise_ms   sg_dictionary_rows_device alone, on the rows (a) left                           device events
  (c) fused_host_ms    sg_suggest_batch_strings, host buffers                                          host clock
  (d) today_host_ms    sg_suggest_batch, then sg_dictionary_rows on a HOST-resident handle — the       host clock
                       plain loop on one thread, which is today's route; of it, host_loop_ms: the loop alone
and text_bytes, the bytes of the strings.  The text of (b), (c) and (d) is compared.  No pass mark: the figures are the result.
Writes profiles/dict_rows_timing.json and prints it.  GPU box only."""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from suggest_amd import IndexDescription, NGramIndex, _lib, synth
from suggest_amd.dictionary import DeviceDictionary
from suggest_amd.metric import resolve

ap = argparse.ArgumentParser()
ap.add_argument("--dict-size", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=65536)
ap.add_argument("--topk", type=int, nargs="+", default=[10, 100])
ap.add_argument("--metric", default="jaccard")
ap.add_argument("--similarity", type=float, default=0.5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dict_rows_timing.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/dict_rows_timing.py measures on a GPU: none is visible")
dev = torch.device("cuda", args.device)
torch.cuda.set_device(dev)
stream = torch.cuda.current_stream()


def timed(fn, reps=args.reps):
    """median milliseconds between two device events around fn(), after one warm-up"""
    fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def timed_host(fn, reps=args.reps):
    """median milliseconds of a host clock around fn(), which returns synchronised, after one warm-up"""
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


desc = IndexDescription(**synth.DESCRIPTION)
t0 = time.perf_counter()
blob, offs = synth.make_dict(args.dict_size, seed=1)
qb, qo = synth.make_queries(args.queries, blob, offs, seed=2)
n_q = len(qo) - 1
code = resolve(args.metric).code
ix = NGramIndex(blob=blob, offs=offs, description=desc, device=args.device, build="device")
on_device = DeviceDictionary(blob=blob, offs=offs, device=args.device)
on_host = DeviceDictionary(blob=blob, offs=offs, device=-1)
d_q = torch.from_numpy(qb).to(dev)
d_o = torch.from_numpy(qo.view(np.int64)).to(dev)
L = _lib.lib()
record = {"tool": "tools/dict_rows_timing.py", "date": datetime.date.today().isoformat(), "gpu": torch.cuda.get_device_name(dev),
          "host_cpus": os.cpu_count(), "dict_size": args.dict_size, "dict_bytes": on_device.bytes, "queries": n_q, "metric": args.metric,
          "similarity": args.similarity, "reps": args.reps, "setup_s": round(time.perf_counter() - t0, 1), "rows": []}

for k in args.topk:
    slots = n_q * k
    d_ids = torch.zeros((n_q, k), dtype=torch.int32, device=dev)
    d_sc = torch.zeros((n_q, k), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(n_q, dtype=torch.int32, device=dev)

    def search():
        ix.suggest_batch_device(d_q.data_ptr(), d_o.data_ptr(), n_q, args.metric, args.similarity, k, d_ids.data_ptr(), d_sc.data_ptr(),
                                d_cnt.data_ptr(), stream.cuda_stream)
    search_ms = timed(search)                                                   # (a)
    cap = slots * on_device.max_len
    d_text = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_toffs = torch.zeros(slots + 1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(2, dtype=torch.int64, device=dev)

    def materialise():
        on_device.rows_device(d_ids.data_ptr(), d_cnt.data_ptr(), None, n_q, k, slots, d_text.data_ptr(), cap, d_toffs.data_ptr(),
                              d_info.data_ptr(), stream.cuda_stream)
    materialise_ms = timed(materialise)                                         # (b)
    text_bytes, outside = (int(x) for x in d_info.cpu().numpy())
    assert outside == 0
    b_text = d_text[:text_bytes].cpu().numpy()
    b_toffs = d_toffs.cpu().numpy().view(np.uint64)

    ids, sc, cnt = np.zeros((n_q, k), dtype=np.uint32), np.zeros((n_q, k), dtype=np.float64), np.zeros(n_q, dtype=np.uint32)
    text, toffs, needed = np.zeros(text_bytes + 1, dtype=np.uint8), np.zeros(slots + 1, dtype=np.uint64), C.c_uint64()

    def fused():
        with ix._use() as h, on_device._use() as dh:
            _lib.check(L.sg_suggest_batch_strings(h, qb.ctypes.data, qo.ctypes.data, n_q, code, args.similarity, k, ids.ctypes.data, sc.ctypes.data,
                                                  cnt.ctypes.data, dh, text.ctypes.data, text_bytes, toffs.ctypes.data, C.byref(needed)))
    fused_ms = timed_host(fused)                                                # (c)
    same_c = needed.value == text_bytes and np.array_equal(toffs, b_toffs) and np.array_equal(text[:text_bytes], b_text)
    text[:] = 0

    def plain():
        with ix._use() as h:
            _lib.check(L.sg_suggest_batch(h, qb.ctypes.data, qo.ctypes.data, n_q, code, args.similarity, k, ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data))

    def loop():
        with on_host._use() as dh:
            _lib.check(L.sg_dictionary_rows(dh, ids.ctypes.data, cnt.ctypes.data, None, n_q, k, slots, text.ctypes.data, text_bytes, toffs.ctypes.data,
                                            C.byref(needed)))

    def today():
        plain()
        loop()
    today_ms = timed_host(today)                                                # (d)
    loop_ms = timed_host(loop)
    same_d = needed.value == text_bytes and np.array_equal(toffs, b_toffs) and np.array_equal(text[:text_bytes], b_text)
    row = {"k": k, "search_ms": round(search_ms, 4), "materialise_ms": round(materialise_ms, 4), "fused_host_ms": round(fused_ms, 4),
           "today_host_ms": round(today_ms, 4), "host_loop_ms": round(loop_ms, 4), "text_bytes": text_bytes, "entries": int(cnt[cnt < 0xFFFFFFF0].sum()),
           "materialise_over_search": round(materialise_ms / max(search_ms, 1e-9), 4), "fused_minus_search_ms": round(fused_ms - search_ms, 4),
           "materialise_above_host_loop": bool(materialise_ms > loop_ms), "fused_text_equal": bool(same_c), "host_text_equal": bool(same_d)}
    record["rows"].append(row)
    print(json.dumps(row), flush=True)
    del d_text

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
print(json.dumps(record))
