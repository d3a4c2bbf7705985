#!/usr/bin/env python3
"""What writing a language model in the reference's formats costs (lm_store.inc / lm_store.cpp).  At a 1 M-token and a 4 M-token
generated corpus (Zipf words over a vocabulary of a twentieth of the tokens, sentences of 6 .. 21 words), order 3, the model is
built on the device (LanguageModel.from_corpus) and then
  (a) saved as <k>-gm files with the device writer and with the host writer — one warm-up call each, then the median of five;
      the seconds per phase come from the library (sg_debug_lm_store_times: staging, kernels, copy-back, file writes), the
      whole call is timed around it, and the two writers' files are compared byte for byte;
  (b) corpus to <k>-gm files: from_corpus + save_ngrams (device writer) against sg_lm_build_google on the same text, wall
      clock, once each after the warm-ups of (a).  The host builder is a std::map per order on one thread: it is timed on the
      first quarter of the lines first, and on the whole text only if that took under 30 s; the device route is timed on the
      same text as the host route;
  (c) save(mph=True) against save(mph=False), median of five each: the difference is mph_build and the write of its section.
Writes the record (default profiles/lm_store_timing.json) and prints it.  GPU box only."""
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
import numpy as np

try:
    import torch  # noqa: F401  (first, so libamdhip64 is shared with torch)
except Exception:
    pass

from suggest_amd import _lib
from suggest_amd.spell import LanguageModel

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, nargs="+", default=[1_000_000, 4_000_000])
ap.add_argument("--order", type=int, default=3)
ap.add_argument("--device", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_store_timing.json"))
args = ap.parse_args()

ALPHA, SEPS = ("english", "numbers"), ("\n",)
PHASES = ("staging", "kernels", "copy_back", "file_write")


def corpus_lines(tokens, seed=7):
    rnd = np.random.RandomState(seed)
    vocab = max(tokens // 20, 1000)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    words = np.array(["".join(letters[rnd.randint(0, 26, size=int(n))]) + "x%d" % i for i, n in enumerate(rnd.randint(1, 9, size=vocab))])
    ids = (rnd.zipf(1.2, size=tokens) - 1) % vocab
    lines, at = [], 0
    while at < tokens:
        n = int(rnd.randint(6, 22))
        lines.append(" ".join(words[ids[at:at + n]]).encode())
        at += n
    return lines


def render(ls):
    return b"\n".join(ls) + b"\n"


def timed_ngrams(lm, directory, device):
    out = (C.c_double * 4)()
    t0 = time.perf_counter()
    lm.save_ngrams(directory, device=device)
    wall = time.perf_counter() - t0
    _lib.check(_lib.lib().sg_debug_lm_store_times(out))
    r = dict(zip(PHASES, (float(x) for x in out)))
    r["device_part"] = r["staging"] + r["kernels"] + r["copy_back"]
    r["wall"] = wall
    return r


def median_of(runs):
    return {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0]}


def files(directory):
    return [open(os.path.join(directory, "%d-gm" % k), "rb").read() for k in range(1, args.order + 1)]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


record = {"tool": "tools/lm_store_timing.py", "order": args.order, "sizes": []}
for tokens in args.tokens:
    lines = corpus_lines(tokens)
    text = render(lines)
    LanguageModel.from_corpus(text, args.order, "<S>", "</S>", ALPHA, SEPS, id_order="count", device=args.device).close()   # warm-up
    build_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        lm = LanguageModel.from_corpus(text, args.order, "<S>", "</S>", ALPHA, SEPS, id_order="count", device=args.device)
        build_s.append(time.perf_counter() - t0)
        if len(build_s) < 3:
            lm.close()
    row = {"tokens": int(sum(ln.count(b" ") + 1 for ln in lines)), "text_bytes": len(text), "words": len(lm),
           "entries": [len(lm.level(i)[1]) for i in range(args.order)], "from_corpus_s": round(statistics.median(build_s), 4)}
    with tempfile.TemporaryDirectory() as tmp:
        dev, host = (os.path.join(tmp, n) for n in ("dev", "host"))
        for d in (dev, host):
            os.mkdir(d)
        # (a)
        timed_ngrams(lm, dev, args.device)
        dev_runs = [timed_ngrams(lm, dev, args.device) for _ in range(5)]
        timed_ngrams(lm, host, -1)
        host_runs = [timed_ngrams(lm, host, -1) for _ in range(5)]
        want = files(host)
        row.update(gm_bytes=[len(f) for f in want], files_identical=files(dev) == want,
                   device=median_of(dev_runs), host=median_of(host_runs),
                   device_wall_runs_s=[round(r["wall"], 4) for r in dev_runs], host_wall_runs_s=[round(r["wall"], 4) for r in host_runs],
                   device_kernels_runs_s=[round(r["kernels"], 4) for r in dev_runs])
        row["host_wall_over_device_wall"] = round(row["host"]["wall"] / max(row["device"]["wall"], 1e-9), 2)
        # (c)
        paths = os.path.join(tmp, "m.lm"), os.path.join(tmp, "m.cdb")
        lm.save(*paths, mph=True)
        with_mph = statistics.median(timed(lambda: lm.save(*paths, mph=True)) for _ in range(5))
        lm_bytes = os.path.getsize(paths[0])
        without = statistics.median(timed(lambda: lm.save(*paths, mph=False)) for _ in range(5))
        row["save_binary"] = {"with_mph_s": round(with_mph, 4), "without_mph_s": round(without, 4), "mph_s": round(with_mph - without, 4),
                              "mph_share": round((with_mph - without) / max(with_mph, 1e-9), 3), "lm_bytes_with_mph": lm_bytes}
        lm.close()
        # (b)
        quarter = render(lines[:len(lines) // 4])

        def host_route(t):
            d = tempfile.mkdtemp(dir=tmp)
            return timed(lambda: LanguageModel.build_files(t, d, args.order, "<S>", "</S>", ALPHA, SEPS))

        def device_route(t):
            d = tempfile.mkdtemp(dir=tmp)

            def run():
                m = LanguageModel.from_corpus(t, args.order, "<S>", "</S>", ALPHA, SEPS, id_order="lines", device=args.device)
                m.save_ngrams(d, device=args.device)
                m.close()
            return timed(run)

        device_route(quarter)
        b = {"quarter_tokens": int(sum(ln.count(b" ") + 1 for ln in lines[:len(lines) // 4])), "quarter_device_route_s": round(device_route(quarter), 4),
             "quarter_host_route_s": round(host_route(quarter), 3)}
        if b["quarter_host_route_s"] < 30.0:
            b.update(device_route_s=round(device_route(text), 4), host_route_s=round(host_route(text), 3))
            b["host_over_device"] = round(b["host_route_s"] / b["device_route_s"], 1)
        else:
            b.update(device_route_s=None, host_route_s=None, note="host route timed on the first quarter of the lines only")
            b["host_over_device"] = round(b["quarter_host_route_s"] / b["quarter_device_route_s"], 1)
        row["corpus_to_files"] = b
    record["sizes"].append(row)
    print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
    f.write("\n")
