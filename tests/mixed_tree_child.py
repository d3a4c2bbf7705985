"""The program tests/test_gpu_mixed_tree.py starts: the single-query coalescer with the mixed switch on, under whatever
SG_COALESCE_TREE the environment holds (a process switch, read once — hence a process of its own).  The SAME 258 threads, whose
thread-local waiters outlive their requests, go through three takes behind the hold:
  A  one key               -> one plain take (with the tree: every sleeper but the leaves gets two children);
  B  258 keys (k = 1 + i)  -> a mixed take of SG_MAX_MIXED_CONFIGS keys; the two requests whose keys come 257th and 258th go back to
                              the queue and are answered by a second mixed take, while their callers must stay asleep — a wake-up
                              through a child pointer left over from A would return them early, count untouched;
  C  one key again         -> a plain take after the mixed ones.
Every caller's row is the plain batch call's, and the counters say which takes were made.  Prints one JSON line; exit status 0."""
import ctypes as C
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import CARS_DESC, GOLDEN  # noqa: E402  (puts the repository on sys.path, imports torch before the library)

import numpy as np  # noqa: E402

N = 258
UNTOUCHED = 0xABCDEF01
SPECIAL = 0xFFFFFFF0


def main():
    from suggest_amd import IndexDescription, NGramIndex, _lib
    from suggest_amd.metric import resolve
    with open(os.path.join(GOLDEN, "cars.dict"), "rb") as f:
        docs = [ln.rstrip(b"\r") for ln in f.read().split(b"\n") if ln]
    ix = NGramIndex(docs, IndexDescription(**CARS_DESC))
    L = _lib.lib()
    jaccard = resolve("jaccard").code
    rng = np.random.RandomState(5)
    queries = [bytes(docs[int(i)]) + b"q" for i in rng.randint(0, len(docs), N)]

    def stats():
        out = (C.c_uint64 * 4)()
        with ix._use() as h:
            _lib.check(L.sg_debug_coalesce_stats(h, out))
        return [int(x) for x in out]

    def hold(on):
        with ix._use() as h:
            _lib.check(L.sg_debug_coalesce_hold(h, 1 if on else 0))

    rounds = [lambda i: 10, lambda i: 1 + i, lambda i: 10]          # the k of caller i: the key, everything else equal
    go = [threading.Event() for _ in rounds]
    done = threading.Barrier(N + 1)
    results = [[None] * N for _ in rounds]
    errors = []

    def caller(i):
        for r, k_of in enumerate(rounds):
            go[r].wait()
            try:
                k, q = k_of(i), queries[i]
                ids, sc, cnt = np.zeros(k, np.uint32), np.zeros(k, np.float64), C.c_uint32(UNTOUCHED)
                with ix._use() as h:
                    _lib.check(L.sg_suggest_one(h, q, len(q), jaccard, 0.5, k, ids.ctypes.data, sc.ctypes.data, C.addressof(cnt)))
                results[r][i] = (ids, sc, int(cnt.value))
            except Exception as e:      # noqa: BLE001
                errors.append((r, i, repr(e)))
            done.wait(120)

    ix.coalesce_mixed(True)
    threads = [threading.Thread(target=caller, args=(i,), daemon=True) for i in range(N)]
    for t in threads:
        t.start()
    took = []
    for r in range(len(rounds)):
        before = stats()
        hold(True)
        try:
            go[r].set()
            deadline = time.monotonic() + 60
            while stats()[0] < N and time.monotonic() < deadline:
                time.sleep(0.002)
            held = stats()
        finally:
            hold(False)                  # (release before the index goes, whatever happened)
        done.wait(120)
        assert held[0] == N and held[1:] == before[1:], (r, before, held)
        after = stats()
        assert after[0] == 0, after
        took.append([a - b for a, b in zip(after[1:], before[1:])])
    for t in threads:
        t.join(60)
    assert not errors, errors[:5]
    # takes, of them mixed, launches: A and C one plain take; B 256 keys, then the two that went back to the queue
    assert took == [[1, 0, 1], [2, 2, N], [1, 0, 1]], took
    plain = {}
    for r, k_of in enumerate(rounds):
        for i in range(N):
            k = k_of(i)
            if (k, i) not in plain:
                pi, ps, pc = ix.suggest_batch([queries[i]], "jaccard", 0.5, k)
                plain[(k, i)] = (pi[0], ps[0], int(pc[0]))
            pi, ps, pc = plain[(k, i)]
            ids, sc, cnt = results[r][i]
            assert cnt == pc, (r, i, hex(cnt), pc)
            n = 0 if pc >= SPECIAL else min(pc, k)
            assert np.array_equal(ids[:n], pi[:n]) and np.array_equal(sc[:n].view(np.uint64), ps[:n].view(np.uint64)), (r, i)
    ix.close()
    print(json.dumps({"tree": os.environ.get("SG_COALESCE_TREE", "0"), "took": took}))


if __name__ == "__main__":
    main()
