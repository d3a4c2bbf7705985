#!/usr/bin/env python3
"""What ranking result rows by edit distance costs (suggest_amd/csrc/edit_rank.inc): on the synthetic dictionary and
query batch of bench.py's headline config (synth.make_dict / make_queries, jaccard 0.5) and on tests/golden/cars.dict with its own
lines as queries, at k_candidates = 16 / 64 / 256 and k = 10.  Per k_candidates, one warm-up and the median of `--reps` runs:
  search_ms          sg_suggest_batch_device alone (k = k_candidates), device-resident buffers              device events
  distance_ms        sg_edit_rows_device alone, on the rows the search left                                  device events
  rerank_ms          sg_edit_rerank_device (distances + the stable re-rank) less distance_ms                 device events
  edit_host_ms       sg_suggest_batch_edit, host buffers                                                     host clock
  plain_host_ms      sg_suggest_batch with k = k_candidates, host buffers                                    host clock
and edit_over_search = (distance_ms + rerank_ms) / search_ms, the ratio to report.  No pass mark: the figures are the result.
Writes profiles/edit_rank_timing.json and prints it.  GPU box only."""
import argparse
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

from suggest_amd import IndexDescription, NGramIndex, synth
from suggest_amd.dictionary import DeviceDictionary, edit_config
from suggest_amd.index import pack_strings

ap = argparse.ArgumentParser()
ap.add_argument("--dict-size", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=65536)
ap.add_argument("--candidates", type=int, nargs="+", default=[16, 64, 256])
ap.add_argument("--topk", type=int, default=10)
ap.add_argument("--metric", default="jaccard")
ap.add_argument("--similarity", type=float, default=0.5)
ap.add_argument("--mode", default="osa")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_rank_timing.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/edit_rank_timing.py measures on a GPU: none is visible")
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


def measure(name, ix, dd, qb, qo, similarity):
    n_q = len(qo) - 1
    d_q = torch.from_numpy(qb).to(dev)
    d_o = torch.from_numpy(qo.view(np.int64)).to(dev)
    cfg = edit_config(args.mode, True, None)
    rows = []
    for kc in args.candidates:
        slots = n_q * kc
        d_ids = torch.zeros((n_q, kc), dtype=torch.int32, device=dev)
        d_sc = torch.zeros((n_q, kc), dtype=torch.float64, device=dev)
        d_cnt = torch.zeros(n_q, dtype=torch.int32, device=dev)
        d_dist = torch.zeros(slots, dtype=torch.int32, device=dev)
        d_info = torch.zeros(2, dtype=torch.int64, device=dev)

        def search():
            ix.suggest_batch_device(d_q.data_ptr(), d_o.data_ptr(), n_q, args.metric, similarity, kc, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(),
                                    stream.cuda_stream)

        def distance():
            dd.edit_rows_device(cfg, d_q.data_ptr(), d_o.data_ptr(), d_ids.data_ptr(), d_cnt.data_ptr(), None, n_q, kc, slots, d_dist.data_ptr(),
                                d_info.data_ptr(), stream.cuda_stream)

        def both():             # (a second run finds the rows ranked already: the same launches, the same work)
            dd.edit_rerank_device(cfg, d_q.data_ptr(), d_o.data_ptr(), d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), None, n_q, kc, slots, kc,
                                  d_dist.data_ptr(), d_info.data_ptr(), stream.cuda_stream)
        search_ms = timed(search)
        distance_ms = timed(distance)
        entries = int(d_cnt.cpu().numpy().view(np.uint32).clip(0, kc)[d_cnt.cpu().numpy().view(np.uint32) < 0xFFFFFFF0].sum())
        both_ms = timed(both)
        k = min(args.topk, kc)
        edit_host_ms = timed_host(lambda: ix.suggest_batch_edit(dd, None, args.metric, similarity, kc, k, mode=args.mode, blob=qb, offs=qo))
        plain_host_ms = timed_host(lambda: ix.suggest_batch(None, args.metric, similarity, kc, blob=qb, offs=qo))
        row = {"dictionary": name, "k_candidates": kc, "k": k, "entries": entries, "search_ms": round(search_ms, 4), "distance_ms": round(distance_ms, 4),
               "rerank_ms": round(both_ms - distance_ms, 4), "edit_over_search": round(both_ms / max(search_ms, 1e-9), 4),
               "edit_host_ms": round(edit_host_ms, 4), "plain_host_ms": round(plain_host_ms, 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


record = {"tool": "tools/edit_rank_timing.py", "date": datetime.date.today().isoformat(), "gpu": torch.cuda.get_device_name(dev), "host_cpus": os.cpu_count(),
          "queries": args.queries, "metric": args.metric, "similarity": args.similarity, "cars_similarity": 0.3, "mode": args.mode, "reps": args.reps,
          "rows": []}

with open(os.path.join(ROOT, "tests", "golden", "cars.dict"), "rb") as f:
    cars = [l[:-1] if l.endswith(b"\r") else l for l in f.read().split(b"\n") if l]
cars_desc = IndexDescription(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("russian", "english", "numbers", "$"))
rng = np.random.RandomState(1)
cq = [cars[int(i)] for i in rng.randint(0, len(cars), args.queries)]
cqb, cqo = pack_strings(cq)
cix = NGramIndex(cars, cars_desc, device=args.device)
record["rows"] += measure("cars.dict", cix, DeviceDictionary(cars, device=args.device), cqb, cqo, record["cars_similarity"])
cix.close()

if args.dict_size:
    t0 = time.perf_counter()
    blob, offs = synth.make_dict(args.dict_size, seed=1)
    qb, qo = synth.make_queries(args.queries, blob, offs, seed=2)
    ix = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), device=args.device, build="device")
    dd = DeviceDictionary(blob=blob, offs=offs, device=args.device)
    record["dict_size"], record["dict_bytes"], record["setup_s"] = args.dict_size, dd.bytes, round(time.perf_counter() - t0, 1)
    record["rows"] += measure("synthetic", ix, dd, qb, qo, args.similarity)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
print(json.dumps(record))
