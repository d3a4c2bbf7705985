#!/usr/bin/env python3
"""Sentence scoring throughput (lm_score.inc): BASELINE config 5's synthetic model (tools/make_synthetic_lm.py, 50 M tokens,
~1 M words, order 3) and 65 536 sentences of its corpus sample, scored
  - on the device, text resident in HBM (sg_lm_score_text_batch_device: tokenise + lookups + windows), timed with events
    after a warm-up;
  - on the device from host buffers (sg_lm_score_text_batch, copies included), wall clock;
  - by the host loop over sg_lm_score_word_ids (one call per sentence, ids mapped beforehand), the baseline.
GPU box only.  For the kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/lm_score_timing.py`."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import make_synthetic_lm
from suggest_amd import _lib
from suggest_amd.index import pack_strings
from suggest_amd.spell import LanguageModel

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=50_000_000)
ap.add_argument("--sentences", type=int, default=65536)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

d = tempfile.mkdtemp()
info = make_synthetic_lm.make(d, tokens=args.tokens, vocab=1_000_000 if args.tokens >= 20_000_000 else max(1000, args.tokens // 40), verbose=False)
lm = LanguageModel(binary=os.path.join(d, "synth.lm"), dictionary=os.path.join(d, "synth.cdb"))
T, words = info["corpus_sample"], info["word_list"]
starts = np.nonzero(T == info["start_id"])[0]
ends = np.nonzero(T == info["end_id"])[0]
sent_ids = []
for s in starts:                                               # the corpus's own sentences, markers dropped
    e = ends[np.searchsorted(ends, s)] if np.searchsorted(ends, s) < len(ends) else None
    if e is None:
        break
    sent_ids.append(T[s + 1:e])
    if len(sent_ids) == args.sentences:
        break
lines = [b" ".join(words[int(i)] for i in x) for x in sent_ids]
n = len(lines)
windows = int(sum(len(x) + 3 - lm.order for x in sent_ids))
blob, offs = pack_strings(lines)
print("model: %d words, %d tokens; %d sentences, %d windows, %.1f MB of text" % (len(lm), info["tokens"], n, windows, len(blob) / 1e6))

# ---- device-resident text path, events
d_blob = torch.from_numpy(blob).cuda()
d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
d_sc = torch.zeros(n, dtype=torch.float64, device="cuda")
d_w = torch.zeros(n, dtype=torch.int32, device="cuda")
d_u = torch.zeros(n, dtype=torch.int32, device="cuda")
st = torch.cuda.Stream()


def dev_call():
    lm.score_text_batch_device(d_blob.data_ptr(), d_offs.data_ptr(), n, len(blob), d_sc.data_ptr(), d_w.data_ptr(), d_u.data_ptr(),
                               stream=st.cuda_stream)


for _ in range(5):
    dev_call()
st.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(st)
for _ in range(args.reps):
    dev_call()
e1.record(st)
e1.synchronize()
t_dev = e0.elapsed_time(e1) / 1e3 / args.reps

# ---- host buffers in and out
scores, w, u = lm.score_text_batch(blob=blob, offs=offs)
t0 = time.perf_counter()
for _ in range(5):
    lm.score_text_batch(blob=blob, offs=offs)
t_hostbuf = (time.perf_counter() - t0) / 5

# ---- the host loop (the baseline): one sg_lm_score_word_ids per sentence, ids mapped beforehand
L = _lib.lib()
arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in sent_ids]
t0 = time.perf_counter()
host = np.array([L.sg_lm_score_word_ids(lm._h, a.ctypes.data, len(a)) for a in arrs])
t_host = time.perf_counter() - t0

dev_rows = d_sc.cpu().numpy()
agree = np.abs(dev_rows - host) <= 1e-12 * np.maximum(1.0, np.abs(host))
print("device, text in HBM (events, %d reps): %.3f ms per batch = %.2f M sentences/s, %.1f M windows/s" % (args.reps, t_dev * 1e3, n / t_dev / 1e6, windows / t_dev / 1e6))
print("device, host buffers (wall clock):     %.3f ms per batch = %.2f M sentences/s, %.1f M windows/s" % (t_hostbuf * 1e3, n / t_hostbuf / 1e6, windows / t_hostbuf / 1e6))
print("host loop sg_lm_score_word_ids:        %.3f ms per batch = %.3f M sentences/s, %.2f M windows/s (one thread)" % (t_host * 1e3, n / t_host / 1e6, windows / t_host / 1e6))
print("device / host loop: %.0fx; rows within 1e-12 of the host: %d / %d; bit-identical: %d" % (t_host / t_dev, int(agree.sum()), n, int((dev_rows == host).sum())))
