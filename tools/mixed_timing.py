#!/usr/bin/env python3
"""What a mixed batch costs (sg_suggest_batch_mixed, suggest_amd/csrc/mixed_batch.inc): 65 536 queries of the
synthetic dictionaries (synth.make_dict / make_queries) spread evenly over 1, 2, 8 and 64 configs — mixes of the BASELINE ones
(jaccard 0.5 k 10, cosine 0.4 k 20, dice 0.5 k 10 and neighbours of them in similarity and k).  Per (dictionary, configs), one
warm-up and the median of `--reps` runs, the two sides alternating:
  1. mixed_device      sg_suggest_batch_mixed_device on device-resident buffers, split by events on its stream
                       (sg_debug_mixed_timing / sg_debug_mixed_times): count (with the one wait for the group sizes), permute,
                       gather, the groups' launches, scatter — the call's own four steps apart from the launches, so that a slow
                       group launch is not blamed on them; own_ms is their sum
  2. mixed_host_ms     sg_suggest_batch_mixed on host buffers, a host clock around the call
     regroup_host_ms   what a caller had to do before this call existed: regroup the queries by config on the host (numpy),
                       call sg_suggest_batch once per config, put the rows back in caller order — against the library named by
                       --parent-lib (a build of the parent commit, loaded into the same process beside the current one; without
                       it, the current library), split into regroup_ms (host work) and calls_ms
                       rows_equal: the two routes' rows, bit for bit
  3. --load: tests/cpp/mixed_load (256 blocking single-query callers, 1 / 2 / 8 keys) with sg_coalesce_mixed off and on, a process
     each, alternating: q/s, batches taken, queries per batch
Writes profiles/mixed_batch_timing.json and prints it.  GPU box only."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from suggest_amd import IndexDescription, NGramIndex, _lib, synth
from suggest_amd.index import _c_desc, mixed_table
from suggest_amd.metric import resolve

ap = argparse.ArgumentParser()
ap.add_argument("--dict-sizes", type=int, nargs="+", default=[1_000_000, 10_000_000])
ap.add_argument("--queries", type=int, default=65536)
ap.add_argument("--configs", type=int, nargs="+", default=[1, 2, 8, 64])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--parent-lib", default=None, help="file name, beside the library, of a build of the parent commit")
ap.add_argument("--load", action="store_true", help="also run the single-query load generator (item 3)")
ap.add_argument("--load-dict", type=int, default=1_000_000)
ap.add_argument("--load-seconds", type=float, default=3.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_batch_timing.json"))
args = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("tools/mixed_timing.py measures on a GPU: none is visible")
dev = torch.device("cuda", args.device)
torch.cuda.set_device(dev)
stream = torch.cuda.Stream(device=dev)
L = _lib.lib()


def config_mix(n):
    """n distinct configs: the BASELINE three, then neighbours of them in similarity and k"""
    base = (("jaccard", 0.5, 10), ("cosine", 0.4, 20), ("dice", 0.5, 10))
    out = []
    for g in range(n):
        m, s, k = base[g % 3]
        step = g // 3
        out.append(dict(metric=m, similarity=round(s + 0.01 * (step % 11), 2), k=k + (step // 11) * 5))
    assert len({(c["metric"], c["similarity"], c["k"]) for c in out}) == n
    return out


def parent_library():
    """the parent commit's build beside the current one, in this process (its own handle type: raw ctypes calls)"""
    if not args.parent_lib:
        return None
    P = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), args.parent_lib))
    vp, u32, i32, dbl = C.c_void_p, C.c_uint32, C.c_int, C.c_double
    P.sg_index_build_device.argtypes = [vp, vp, u32, C.POINTER(_lib.SgDesc), i32, C.POINTER(vp)]
    P.sg_index_upload.argtypes = [vp, i32]
    P.sg_suggest_batch.argtypes = [vp, vp, vp, u32, i32, dbl, u32, vp, vp, vp]
    P.sg_index_release.argtypes = [vp]
    P.sg_index_release.restype = None
    P.sg_last_error.restype = C.c_char_p
    assert not hasattr(P, "sg_suggest_batch_mixed"), "--parent-lib names a build that has the mixed call"
    return P


def regroup_route(call, qb, qo, configs, config_of):
    """-> (rows, regroup seconds, calls seconds): the host regroups, `call` answers one config's queries, the rows go back"""
    t0 = time.perf_counter()
    order = np.argsort(config_of, kind="stable")
    lens = (qo[1:] - qo[:-1]).astype(np.int64)
    glens = lens[order]
    goffs = np.concatenate([[0], np.cumsum(glens)]).astype(np.uint64)
    src = np.repeat(qo[:-1].astype(np.int64)[order] - goffs[:-1].astype(np.int64), glens) + np.arange(int(goffs[-1]))
    gblob = qb[src]
    start = np.concatenate([[0], np.cumsum(np.bincount(config_of, minlength=len(configs)))])
    ks = np.array([c["k"] for c in configs], dtype=np.int64)
    row_offs = np.concatenate([[0], np.cumsum(ks[config_of])])
    ids, sc, cnt = np.zeros(int(row_offs[-1]), np.uint32), np.zeros(int(row_offs[-1]), np.float64), np.zeros(len(config_of), np.uint32)
    t_regroup = time.perf_counter() - t0
    t_calls = 0.0
    for g, c in enumerate(configs):
        lo, hi = int(start[g]), int(start[g + 1])
        if lo == hi:
            continue
        t1 = time.perf_counter()
        o = np.ascontiguousarray(goffs[lo:hi + 1] - goffs[lo])
        b = gblob[int(goffs[lo]):int(goffs[hi])]
        gi, gs, gc = call(b, o, hi - lo, c)
        t_calls += time.perf_counter() - t1
        t1 = time.perf_counter()
        members = order[lo:hi]
        at = (row_offs[members][:, None] + np.arange(c["k"])[None, :]).ravel()
        ids[at], sc[at], cnt[members] = gi.ravel(), gs.ravel(), gc
        t_regroup += time.perf_counter() - t1
    return (ids, sc, cnt), t_regroup, t_calls


def measure(n_docs):
    t0 = time.perf_counter()
    blob, offs = synth.make_dict(n_docs, seed=1)
    qb, qo = synth.make_queries(args.queries, blob, offs, seed=2)
    n_q = len(qo) - 1
    desc = IndexDescription(**synth.DESCRIPTION)
    ix = NGramIndex(blob=blob, offs=offs, description=desc, device=args.device, build="device")
    P = parent_library()
    ph = C.c_void_p()
    if P:
        cd = _c_desc(desc)
        assert P.sg_index_build_device(blob.ctypes.data, offs.ctypes.data, n_docs, C.byref(cd), args.device, C.byref(ph)) == 0, P.sg_last_error()
        assert P.sg_index_upload(ph, args.device) == 0, P.sg_last_error()

    def plain_call(b, o, n, c):
        gi, gs, gc = np.zeros((n, c["k"]), np.uint32), np.zeros((n, c["k"]), np.float64), np.zeros(n, np.uint32)
        code = resolve(c["metric"]).code
        if P:
            assert P.sg_suggest_batch(ph, b.ctypes.data, o.ctypes.data, n, code, c["similarity"], c["k"], gi.ctypes.data, gs.ctypes.data, gc.ctypes.data) == 0, P.sg_last_error()
        else:
            with ix._use() as h:
                _lib.check(L.sg_suggest_batch(h, b.ctypes.data, o.ctypes.data, n, code, c["similarity"], c["k"], gi.ctypes.data, gs.ctypes.data, gc.ctypes.data))
        return gi, gs, gc

    d_q = torch.from_numpy(qb).to(dev)
    d_o = torch.from_numpy(qo.view(np.int64)).to(dev)
    rows = []
    setup_s = round(time.perf_counter() - t0, 1)
    for n_cfg in args.configs:
        configs = config_mix(n_cfg)
        config_of = (np.arange(n_q) % n_cfg).astype(np.uint32)
        np.random.RandomState(5).shuffle(config_of)
        table = mixed_table(configs)
        total = int(np.array([c["k"] for c in configs], dtype=np.int64)[config_of].sum())
        d_cfg = torch.from_numpy(config_of.view(np.int32)).to(dev)
        d_ids = torch.zeros(total, dtype=torch.int32, device=dev)
        d_sc = torch.zeros(total, dtype=torch.float64, device=dev)
        d_cnt = torch.zeros(n_q, dtype=torch.int32, device=dev)
        d_ro = torch.zeros(n_q + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        steps, host_ms, regroup_ms, calls_ms = [], [], [], []
        ms = (C.c_double * 5)()
        mixed_rows = other_rows = None
        _lib.check(L.sg_debug_mixed_timing(1))
        try:
            for rep in range(args.reps + 1):           # (rep 0: the warm-up)
                ix.suggest_batch_mixed_device(d_q.data_ptr(), d_o.data_ptr(), n_q, table, d_cfg.data_ptr(), total, d_ids.data_ptr(), d_sc.data_ptr(),
                                              d_cnt.data_ptr(), d_ro.data_ptr(), stream=stream.cuda_stream)
                stream.synchronize()
                _lib.check(L.sg_debug_mixed_times(ms))
                other_rows, t_regroup, t_calls = regroup_route(plain_call, qb, qo, configs, config_of)
                t1 = time.perf_counter()
                mixed_rows = ix.suggest_batch_mixed(blob=qb, offs=qo, configs=table, config_of=config_of)
                t_host = time.perf_counter() - t1
                if rep:
                    steps.append(list(ms)); host_ms.append(t_host * 1e3); regroup_ms.append(t_regroup * 1e3); calls_ms.append(t_calls * 1e3)
        finally:
            _lib.check(L.sg_debug_mixed_timing(0))
        med = [statistics.median(s[i] for s in steps) for i in range(5)]
        dev_rows = (d_ids.cpu().numpy().view(np.uint32), d_sc.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32))
        same = lambda a, b: bool(all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)))      # noqa: E731
        row = {"dict_size": n_docs, "configs": n_cfg, "queries": n_q, "row_slots": total,
               "mixed_device": {"count_ms": round(med[0], 4), "permute_ms": round(med[1], 4), "gather_ms": round(med[2], 4), "groups_ms": round(med[3], 4),
                                "scatter_ms": round(med[4], 4), "own_ms": round(med[0] + med[1] + med[2] + med[4], 4), "total_ms": round(sum(med), 4)},
               "mixed_host_ms": round(statistics.median(host_ms), 4), "mixed_host_runs_ms": [round(x, 3) for x in host_ms],
               "regroup_host_ms": round(statistics.median(r + c for r, c in zip(regroup_ms, calls_ms)), 4),
               "regroup_host_runs_ms": [round(r + c, 3) for r, c in zip(regroup_ms, calls_ms)],
               "regroup_ms": round(statistics.median(regroup_ms), 4), "calls_ms": round(statistics.median(calls_ms), 4),
               "regroup_library": args.parent_lib or "current",
               "rows_equal": same(mixed_rows[:3], other_rows), "device_rows_equal_host": same(dev_rows, mixed_rows[:3])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if P:
        P.sg_index_release(ph)
    ix.close()
    return setup_s, rows


record = {"tool": "tools/mixed_timing.py", "queries": args.queries, "reps": args.reps, "gpu": torch.cuda.get_device_name(dev), "rows": [], "setup_s": {}}
for n in args.dict_sizes:
    s, rows = measure(n)
    record["setup_s"][str(n)] = s
    record["rows"] += rows

if args.load:
    binary = os.path.join(ROOT, "tests", "cpp", "_build", "mixed_load")
    record["load"] = []
    for keys in (1, 2, 8):
        for rep in range(2):
            for mixed in (0, 1):                      # (alternating; a fresh process each: the GPU is opened by one at a time)
                r = subprocess.run([binary, str(args.load_dict), "256", str(args.load_seconds), str(keys), str(mixed)], capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit("mixed_load failed: " + r.stdout + r.stderr)
                line = json.loads(r.stdout.strip().splitlines()[-1])
                record["load"].append(line)
                print(json.dumps(line), flush=True)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
