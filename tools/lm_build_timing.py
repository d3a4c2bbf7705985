#!/usr/bin/env python3
"""Language-model build time (lm_build.inc): a text rendered from the corpus sample of BASELINE config 5's generator
(tools/make_synthetic_lm.py: Zipf words, sentences of 6..21 words; the sample's sentences, one per line, markers dropped), built
  - on the device: sg_lm_build_device, wall clock with the upload of the text and the copy-down of the levels — one warm-up
    call, then the median of five;
  - by the file route it replaces: sg_lm_build_google into a temporary directory + sg_lm_load_google_ex, wall clock, once.
    It is timed on the first quarter of the lines first; only if that took under 30 s is the whole text timed as well
    (the route is a tree of std::map per order on one thread).  The device is timed on the same prefix for the ratio.
Prints one JSON line.  GPU box only.  For the kernel split: `rocprofv3 --kernel-trace --stats -- python tools/lm_build_timing.py --skip-host`."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

try:
    import torch  # noqa: F401  (first, so libamdhip64 is shared with torch)
except Exception:
    pass

import make_synthetic_lm
from suggest_amd.spell import LanguageModel

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=4_600_000, help="corpus tokens to generate (the sample is its first 4 M positions)")
ap.add_argument("--vocab", type=int, default=200_000)
ap.add_argument("--order", type=int, default=3)
ap.add_argument("--skip-host", action="store_true")
args = ap.parse_args()

ALPHA, SEPS = ("english",), ("\n",)
with tempfile.TemporaryDirectory() as tmp:                     # (only the corpus sample is kept, not the files)
    info = make_synthetic_lm.make(tmp, tokens=args.tokens, vocab=args.vocab, verbose=False)
T, words = info["corpus_sample"], info["word_list"]
markers = (info["start_id"], info["end_id"])
lines, cur = [], []
for i in T.tolist():
    if i == markers[1]:
        lines.append(b" ".join(cur)); cur = []
    elif i != markers[0]:
        cur.append(words[i])


def render(ls):
    return b"\n".join(ls) + b"\n"


def time_device(text):
    LanguageModel.from_corpus(text, args.order, "<S>", "</S>", ALPHA, SEPS, id_order="count").close()      # warm-up
    runs = []
    for _ in range(5):
        t0 = time.perf_counter()
        m = LanguageModel.from_corpus(text, args.order, "<S>", "</S>", ALPHA, SEPS, id_order="count")
        runs.append(time.perf_counter() - t0)
        n_words = len(m)
        m.close()
    return statistics.median(runs), runs, n_words


def time_host(text):
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        LanguageModel.build_files(text, d, args.order, "<S>", "</S>", ALPHA, SEPS)
        t1 = time.perf_counter()
        m = LanguageModel(d, args.order, "<S>", "</S>", ALPHA, id_order="count")
        t2 = time.perf_counter()
        m.close()
    return t2 - t0, t1 - t0, t2 - t1


def tokens_of(ls):
    return int(sum(x.count(b" ") + 1 for x in ls))


full, quarter = render(lines), render(lines[:len(lines) // 4])
out = {"order": args.order, "lines": len(lines), "tokens": tokens_of(lines), "text_bytes": len(full)}
med, runs, n_words = time_device(full)
out.update(words=n_words, device_s=round(med, 4), device_runs_s=[round(x, 4) for x in runs], device_tokens_per_s=round(out["tokens"] / med))
if not args.skip_host:
    q_tokens = tokens_of(lines[:len(lines) // 4])
    q_med, q_runs, _ = time_device(quarter)
    h_all, h_build, h_load = time_host(quarter)
    out.update(prefix_tokens=q_tokens, prefix_device_s=round(q_med, 4), prefix_host_s=round(h_all, 3), prefix_host_build_s=round(h_build, 3),
               prefix_host_load_s=round(h_load, 3), prefix_ratio=round(h_all / q_med, 1))
    if h_all < 30.0:
        h_all, h_build, h_load = time_host(full)
        out.update(host_s=round(h_all, 3), host_build_s=round(h_build, 3), host_load_s=round(h_load, 3), ratio=round(h_all / med, 1))
    else:
        out.update(host_s=None, note="host route timed on the first quarter of the lines only")
print(json.dumps(out))
