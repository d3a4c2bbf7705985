#!/usr/bin/env python3
"""What searching a dictionary sharded by docID range costs on ONE GPU (sg_sharded, suggest_amd/csrc/shard_merge.inc): the
synthetic dictionary and query batch of bench.py's headline config (synth.make_dict / make_queries, jaccard 0.5) cut into
W = 1, 2, 4, 8 shards, at k = 10 and 100.  Per (W, k), device-resident buffers, device events, one warm-up and the median of
`--reps` runs:
  - sharded_ms        sg_sharded_suggest_batch_device: W searches and the merge launch on one stream
  - searches_sum_ms   the W shards' own sg_suggest_batch_device calls, each timed alone, summed
  - merge_kernel_ms   the merge launch alone, on the rows those calls left (sg_debug_shard_merge / sg_debug_shard_merge_time)
  - unsharded_ms      sg_suggest_batch_device on the unsharded index
  - torch_merge_ms    the existing route on the same rows on the GPU: distributed.merge_topk (two torch.sort over [n, W * k])
and the ratios merge_kernel / searches_sum, torch_merge / merge_kernel, sharded / unsharded.  The merged rows of the kernel, of
merge_topk and of the sharded call are compared.
  - host_ms           sg_sharded_suggest_batch, host buffers: a host clock around the call, which returns synchronised; one
                      warm-up, the median of `--reps` runs (host_runs_ms: each of them), on a handle with one lane (devices
                      (0,), key "1") and on one with two (devices (0, 0), key "2").  host_rows: a SHA-256 of the rows, to hold
                      two builds of the library against each other; host_rows_equal_sharded_call: against the device-resident call's.
--host-only measures the host-buffer call alone (an A/B of two builds under SG_LIB_NAME, a process each).
Writes profiles/shard_merge_timing.json and prints it.  GPU box only."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from suggest_amd import IndexDescription, NGramIndex, ShardedIndex, _lib, synth
from suggest_amd.distributed import merge_topk, shard_bounds
from suggest_amd.metric import resolve
from suggest_amd.sharded import shard_merge

ap = argparse.ArgumentParser()
ap.add_argument("--dict-size", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=65536)
ap.add_argument("--shards", type=int, nargs="+", default=[1, 2, 4, 8])
ap.add_argument("--topk", type=int, nargs="+", default=[10, 100])
ap.add_argument("--metric", default="jaccard")
ap.add_argument("--similarity", type=float, default=0.5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--host-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_merge_timing.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/shard_timing.py measures on a GPU: none is visible")
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
    """milliseconds of a host clock around fn(), which returns synchronised, after one warm-up: (median, every run)"""
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), out


def host_handles(W):
    """W shards built on the GPU behind a handle with one lane and behind one with two"""
    return {str(n): ShardedIndex(blob=blob, offs=offs, description=desc, n_shards=W, devices=(args.device,) * n, build="device") for n in (1, 2)}


def host_call(sh, k):
    """-> (median ms, runs, rows) of sg_sharded_suggest_batch"""
    ids, sc, cnt = np.empty((n_q, k), dtype=np.uint32), np.empty((n_q, k), dtype=np.float64), np.empty(n_q, dtype=np.uint32)
    for x in (ids, sc, cnt):
        x.fill(0)           # (the pages are there before the first call)
    code = resolve(args.metric).code
    with sh._use() as h:
        ms, runs = timed_host(lambda: _lib.check(_lib.lib().sg_sharded_suggest_batch(h, qb.ctypes.data, qo.ctypes.data, n_q, code, args.similarity, k,
                                                                                     ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data)))
    return ms, runs, (ids, sc, cnt)


def write_record():
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


def host_cells(handles, k):
    row, rows = {"host_ms": {}, "host_runs_ms": {}, "host_rows": {}}, None
    for key, sh in handles.items():
        ms, runs, rows = host_call(sh, k)
        row["host_ms"][key] = round(ms, 4)
        row["host_runs_ms"][key] = [round(x, 4) for x in runs]
        row["host_rows"][key] = hashlib.sha256(b"".join(x.tobytes() for x in rows)).hexdigest()
    return row, rows


desc = IndexDescription(**synth.DESCRIPTION)
t0 = time.perf_counter()
blob, offs = synth.make_dict(args.dict_size, seed=1)
qb, qo = synth.make_queries(args.queries, blob, offs, seed=2)
n_q = len(qo) - 1
d_q = torch.from_numpy(qb).to(dev)
d_o = torch.from_numpy(qo.view(np.int64)).to(dev)
record = {"tool": "tools/shard_timing.py", "dict_size": args.dict_size, "queries": n_q, "metric": args.metric, "similarity": args.similarity,
          "reps": args.reps, "gpu": torch.cuda.get_device_name(dev), "setup_s": round(time.perf_counter() - t0, 1), "rows": []}


def rows_for(k):
    return (torch.zeros((n_q, k), dtype=torch.int32, device=dev), torch.zeros((n_q, k), dtype=torch.float64, device=dev),
            torch.zeros(n_q, dtype=torch.int32, device=dev))


def search(ix, out, k):
    ix.suggest_batch_device(d_q.data_ptr(), d_o.data_ptr(), n_q, args.metric, args.similarity, k, out[0].data_ptr(), out[1].data_ptr(),
                            out[2].data_ptr(), stream.cuda_stream)


if args.host_only:
    for W in args.shards:
        handles = host_handles(W)
        for k in args.topk:
            row = dict({"shards": W, "k": k}, **host_cells(handles, k)[0])
            record["rows"].append(row)
            print(json.dumps(row), flush=True)
        for x in handles.values():
            x.close()
    write_record()
    sys.exit(0)

full = NGramIndex(blob=blob, offs=offs, description=desc, device=args.device, build="device")
S = full.stats()["n_segments"]
unsharded = {}
for k in args.topk:
    out = rows_for(k)
    unsharded[k] = (timed(lambda: search(full, out, k)), out)

for W in args.shards:
    shards, los = [], []
    for s in range(W):
        lo, hi = shard_bounds(args.dict_size, W, s)
        shards.append(NGramIndex(blob=blob[int(offs[lo]):int(offs[hi])], offs=(offs[lo:hi + 1] - offs[lo]).astype(np.uint64), description=desc,
                                 device=args.device, build="device", min_segments=S))
        los.append(lo)
    sh = ShardedIndex.adopt(shards, los)
    handles = host_handles(W)
    for k in args.topk:
        un_ms, un_rows = unsharded[k]
        per = [rows_for(k) for _ in range(W)]
        searches = [timed(lambda s=s: search(shards[s], per[s], k)) for s in range(W)]
        out = rows_for(k)
        sharded_ms = timed(lambda: search(sh, out, k))
        # the rows the shards left: the kernel alone (host arrays through the direct hook), and merge_topk on the GPU
        ids = torch.stack([p[0] for p in per]); sc = torch.stack([p[1] for p in per]); cnt = torch.stack([p[2] for p in per])
        h_ids, h_sc, h_cnt = ids.cpu().numpy().view(np.uint32), sc.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)
        kernel_ms, ms = [], C.c_double()
        for _ in range(args.reps + 1):
            k_rows = shard_merge(h_ids, h_sc, h_cnt, los, device=args.device)
            _lib.check(_lib.lib().sg_debug_shard_merge_time(C.byref(ms)))
            kernel_ms.append(ms.value)
        kernel_ms = statistics.median(kernel_ms[1:])
        g_ids = (ids.to(torch.int64) & 0xFFFFFFFF) + torch.tensor(los, dtype=torch.int64, device=dev)[:, None, None]
        g_cnt = cnt.to(torch.int64) & 0xFFFFFFFF
        t_rows = [None]

        def torch_route():
            t_rows[0] = merge_topk(g_ids, sc, g_cnt, k)
        torch_ms = timed(torch_route)
        t_ids, t_sc, t_cnt = (x.cpu().numpy() for x in t_rows[0])
        s_ids, s_sc, s_cnt = out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint32)
        u_ids, u_sc, u_cnt = un_rows[0].cpu().numpy().view(np.uint32), un_rows[1].cpu().numpy(), un_rows[2].cpu().numpy().view(np.uint32)
        valid = (np.arange(k)[None, :] < np.minimum(s_cnt, k)[:, None]) & (s_cnt < 0xFFFFFFF0)[:, None]
        row = {"shards": W, "k": k,
               "sharded_ms": round(sharded_ms, 4), "searches_sum_ms": round(sum(searches), 4), "searches_ms": [round(x, 4) for x in searches],
               "merge_kernel_ms": round(kernel_ms, 4), "unsharded_ms": round(un_ms, 4), "torch_merge_ms": round(torch_ms, 4),
               "merge_bytes_read": W * n_q * (k * 12 + 4), "merge_bytes_written": n_q * (k * 12 + 4),
               "merge_kernel_over_searches_sum": round(kernel_ms / max(sum(searches), 1e-9), 4),
               "torch_merge_over_merge_kernel": round(torch_ms / max(kernel_ms, 1e-9), 2),
               "sharded_over_unsharded": round(sharded_ms / max(un_ms, 1e-9), 3),
               "kernel_rows_equal_sharded_call": bool(np.array_equal(k_rows[0], s_ids) and np.array_equal(k_rows[1].view(np.uint64), s_sc.view(np.uint64)) and np.array_equal(k_rows[2], s_cnt)),
               "kernel_rows_equal_merge_topk": bool(np.array_equal(t_cnt.astype(np.uint32), s_cnt) and np.array_equal(t_ids.astype(np.uint32)[valid], s_ids[valid])
                                                    and np.array_equal(t_sc.view(np.uint64)[valid], s_sc.view(np.uint64)[valid])),
               "sharded_rows_equal_unsharded": bool(np.array_equal(u_cnt, s_cnt) and np.array_equal(u_ids[valid], s_ids[valid])
                                                    and np.array_equal(u_sc.view(np.uint64)[valid], s_sc.view(np.uint64)[valid]))}
        host, h_rows = host_cells(handles, k)
        row.update(host)
        row["host_rows_equal_sharded_call"] = bool(np.array_equal(h_rows[0], s_ids) and np.array_equal(h_rows[1].view(np.uint64), s_sc.view(np.uint64))
                                                   and np.array_equal(h_rows[2], s_cnt))
        record["rows"].append(row)
        print(json.dumps(row), flush=True)
        del ids, sc, cnt, g_ids, g_cnt, t_rows, per, out
        torch.cuda.empty_cache()
    sh.close()
    for x in shards + list(handles.values()):
        x.close()

write_record()
