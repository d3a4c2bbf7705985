#!/usr/bin/env python3
"""What the complete search by edit distance costs (suggest_amd/csrc/edit_search.inc): on tests/golden/cars.dict with
its own lines, one and two edits applied, as queries, and on the synthetic dictionary of bench.py's headline config (synth.make_dict)
with its own strings edited the same way; max_distance 1 and 2, k = 10, Levenshtein, folded.  Per (dictionary, max_distance), one
warm-up and the median of `--reps` runs:
  search_ms        sg_edit_search_device, device-resident buffers                                            device events
  survive_share    the share of (query, document) pairs that pass the two bounds, counted on the host from the index's arrays
                   over the first `--share-queries` queries
  exhaustive_ms    the parent's only complete route: sg_edit_rows_device over rows that list every docID, on the first
                   `--exhaustive-queries` queries where n_q * n_docs slots fit (--exhaustive-slots), beside search_ms on the same
                   queries (search_sub_ms)                                                                    device events
  candidates_ms    sg_suggest_batch_edit with 64 candidates, k = 64, the same max_distance, host buffers     host clock
  missed           matches the candidate route did not return: the sum of the complete search's histograms less its entries
No pass mark: the figures are the result.  Writes profiles/edit_search_timing.json and prints it.  GPU box only."""
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
ap.add_argument("--max-distance", type=int, nargs="+", default=[1, 2])
ap.add_argument("--topk", type=int, default=10)
ap.add_argument("--candidates", type=int, default=64)
ap.add_argument("--share-queries", type=int, default=256)
ap.add_argument("--exhaustive-queries", type=int, default=4096)
ap.add_argument("--exhaustive-slots", type=int, default=1 << 28)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_search_timing.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/edit_search_timing.py measures on a GPU: none is visible")
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
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def edited(lines, n, seed):
    """n of the lines with one and two edits applied (insert, delete, substitute, transpose; ASCII letters)"""
    rng = np.random.RandomState(seed)
    out = []
    for j, i in enumerate(rng.randint(0, len(lines), n)):
        s = bytearray(lines[int(i)])
        for _ in range(1 + j % 2):
            op, p = int(rng.randint(0, 4)), int(rng.randint(0, max(1, len(s))))
            c = 97 + int(rng.randint(0, 26))
            if op == 0 and s:
                del s[p]
            elif op == 1:
                s.insert(p, c)
            elif op == 2 and s:
                s[p] = c
            elif len(s) > 1:
                p = min(p, len(s) - 2)
                s[p], s[p + 1] = s[p + 1], s[p]
        out.append(bytes(s))
    return out


def popcount64(x):
    x = x - ((x >> np.uint64(1)) & np.uint64(0x5555555555555555))
    x = (x & np.uint64(0x3333333333333333)) + ((x >> np.uint64(2)) & np.uint64(0x3333333333333333))
    x = (x + (x >> np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    return (x * np.uint64(0x0101010101010101)) >> np.uint64(56)


def survive_share(ei, queries, md):
    """the filter of edit_search.inc restated over the index's own arrays (valid UTF-8 queries; folded by str.lower where that
    yields one rune)"""
    runes, sig = ei.array("runes").astype(np.int64), ei.array("sig")
    kept = 0
    for q in queries:
        rs = [ord(ch.lower()) if len(ch.lower()) == 1 else ord(ch) for ch in q.decode("utf-8", "replace")]
        sq = np.uint64(0)
        for r in rs:
            sq |= np.uint64(1) << np.uint64(((r * 0x9E3779B1) & 0xFFFFFFFF) >> 26)
        ok = (np.abs(runes - len(rs)) <= md) & (popcount64(sq & ~sig) <= md) & (popcount64(sig & ~sq) <= md)
        kept += int(ok.sum())
    return kept / max(1, len(queries) * runes.size)


def measure(name, ix, dd, queries, similarity):
    ei = dd.edit_index(fold_case=True)
    qb, qo = pack_strings(queries)
    n_q, k = len(queries), args.topk
    d_q = torch.from_numpy(qb).to(dev)
    d_o = torch.from_numpy(qo.view(np.int64)).to(dev)
    d_ids, d_dist = torch.zeros(n_q * k, dtype=torch.int32, device=dev), torch.zeros(n_q * k, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(n_q, dtype=torch.int32, device=dev)
    rows = []
    for md in args.max_distance:
        d_hist = torch.zeros(n_q * (md + 1), dtype=torch.int32, device=dev)
        cfg = ei.config(md)

        def search(n=n_q):
            ei.search_device(cfg, d_q.data_ptr(), d_o.data_ptr(), n, k, d_ids.data_ptr(), d_dist.data_ptr(), d_cnt.data_ptr(), d_hist.data_ptr(), stream.cuda_stream)
        search_ms = timed(search)
        hist = d_hist.cpu().numpy().view(np.uint32).astype(np.int64)
        matches = int(hist.sum())
        row = {"dictionary": name, "n_docs": dd.n_docs, "queries": n_q, "max_distance": md, "k": k, "search_ms": round(search_ms, 3), "matches": matches,
               "survive_share": round(survive_share(ei, queries[:args.share_queries], md), 6), "share_queries": min(n_q, args.share_queries)}
        n_ex = min(n_q, args.exhaustive_queries, args.exhaustive_slots // max(1, dd.n_docs))
        if n_ex:
            x_ids = torch.arange(dd.n_docs, dtype=torch.int32, device=dev).repeat(n_ex)
            x_cnt = torch.full((n_ex,), dd.n_docs, dtype=torch.int32, device=dev)
            x_dist = torch.zeros(n_ex * dd.n_docs, dtype=torch.int32, device=dev)
            x_info = torch.zeros(2, dtype=torch.int64, device=dev)
            ecfg = edit_config("levenshtein", True, None)
            row["exhaustive_queries"] = n_ex
            row["exhaustive_ms"] = round(timed(lambda: dd.edit_rows_device(ecfg, d_q.data_ptr(), d_o.data_ptr(), x_ids.data_ptr(), x_cnt.data_ptr(), None, n_ex,
                                                                           dd.n_docs, n_ex * dd.n_docs, x_dist.data_ptr(), x_info.data_ptr(), stream.cuda_stream)), 3)
            row["search_sub_ms"] = round(timed(lambda: search(n_ex)), 3)
            del x_ids, x_dist
        if ix is not None:
            kc = args.candidates
            res = {}

            def cand():
                res["r"] = ix.suggest_batch_edit(dd, None, "jaccard", similarity, kc, kc, mode="levenshtein", max_distance=md, blob=qb, offs=qo)
            row["candidates_ms"] = round(timed_host(cand), 3)
            c = res["r"][3].astype(np.int64)
            row["candidates"], row["similarity"] = kc, similarity
            row["missed"] = matches - int(c[c < 0xFFFFFFF0].sum())
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


record = {"tool": "tools/edit_search_timing.py", "date": datetime.date.today().isoformat(), "gpu": torch.cuda.get_device_name(dev), "host_cpus": os.cpu_count(),
          "mode": "levenshtein", "fold_case": True, "reps": args.reps, "rows": []}

with open(os.path.join(ROOT, "tests", "golden", "cars.dict"), "rb") as f:
    cars = [l[:-1] if l.endswith(b"\r") else l for l in f.read().split(b"\n") if l]
cix = NGramIndex(cars, IndexDescription(ngram_size=3, wrap=("$", "$"), pad="$", alphabet=("russian", "english", "numbers", "$")), device=args.device)
record["rows"] += measure("cars.dict", cix, DeviceDictionary(cars, device=args.device), edited(cars, args.queries, 1), 0.3)
cix.close()

if args.dict_size:
    t0 = time.perf_counter()
    blob, offs = synth.make_dict(args.dict_size, seed=1)
    o = offs.astype(np.int64)
    raw = blob.tobytes()
    pick = np.random.RandomState(3).randint(0, args.dict_size, 4 * args.queries)
    pool = [raw[o[i]:o[i + 1]] for i in pick]
    ix = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), device=args.device, build="device")
    dd = DeviceDictionary(blob=blob, offs=offs, device=args.device)
    record["dict_size"], record["dict_bytes"], record["setup_s"] = args.dict_size, dd.bytes, round(time.perf_counter() - t0, 1)
    record["rows"] += measure("synthetic", ix, dd, edited(pool, args.queries, 2), 0.5)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
print(json.dumps(record))
