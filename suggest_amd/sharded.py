"""ShardedIndex: a dictionary sharded by docID range behind one handle (sg_sharded, include/suggest_hip.h).

For dictionaries past one NGramIndex's limits (2^29 documents per upload, 2^26 per device build, one GPU's HBM per replica):
W shards on one GPU or several, one call searches all of them, and a HIP kernel merges the per-shard top-k rows on the
device under the reference's order (score desc, docID asc).  Rows come back with dictionary-wide docIDs.  One process, no
torch.distributed (suggest_amd/distributed.py::DocShardedIndex is the one-process-per-shard form).

The merged rows equal the unsharded index's for dictionaries without documents that repeat a term.  With such documents the
primary entries are the same, but the reference's secondary duplicate rows depend on relative list lengths,
which differ inside a shard: they can differ from the unsharded index's.
"""
import contextlib
import ctypes as C
import threading

import numpy as np

from . import _lib
from .index import IndexDescription, _c_desc, pack_strings
from .metric import resolve


class ShardedIndex:
    def __init__(self, docs=None, offs=None, description=None, n_shards=1, devices=(0,), build="host", blob=None, _handle=None):
        """docs: a list of str / bytes, or a uint8 blob together with `offs` (blob= names the blob outright).  Shard s goes to
        devices[s % len(devices)]; build="device" builds every shard on its own GPU (sg_sharded_build)."""
        self._hlock = threading.Lock()
        self.description = description or IndexDescription()
        if _handle is not None:
            self._h = _handle
            return
        if build not in ("host", "device"):
            raise ValueError("build must be 'host' or 'device'")
        if blob is None and offs is not None:
            blob = docs
        if blob is None:
            blob, offs = pack_strings(docs)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        desc = _c_desc(self.description)
        h = C.c_void_p()
        _lib.check(_lib.lib().sg_sharded_build(blob.ctypes.data if blob.size else None, offs.ctypes.data, len(offs) - 1, C.byref(desc),
                                               int(n_shards), devs, len(devices), 0 if build == "device" else -1, C.byref(h)))
        self._h = h

    @classmethod
    def adopt(cls, indexes, doc_lo):
        """Shards that are already built and uploaded (NGramIndex objects; sg_sharded_adopt retains their handles): doc_lo[s] =
        the dictionary docID of shard s's document 0."""
        arr = (C.c_void_p * len(indexes))()
        lo = np.ascontiguousarray(doc_lo, dtype=np.uint64)
        if len(lo) != len(indexes):
            raise ValueError("one doc_lo per shard")
        h = C.c_void_p()
        with contextlib.ExitStack() as st:
            for i, ix in enumerate(indexes):
                arr[i] = st.enter_context(ix._use())
            _lib.check(_lib.lib().sg_sharded_adopt(arr, lo.ctypes.data, len(indexes), C.byref(h)))
        return cls(description=indexes[0].description if indexes else None, _handle=h)

    @contextlib.contextmanager
    def _use(self):
        """The handle, retained for the duration of a C call (as NGramIndex._use)."""
        L = _lib.lib()
        with self._hlock:
            h = self._h
            if not h:
                raise ValueError("sharded index is closed")
            L.sg_sharded_retain(h)
        try:
            yield h
        finally:
            L.sg_sharded_release(h)

    def close(self):
        lock = getattr(self, "_hlock", None)
        if lock is None:
            return
        with lock:
            h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().sg_sharded_release(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shards(self):
        """-> [(doc_lo, device)] of the shards that stand, in docID order (sg_sharded_shards)"""
        lo = (C.c_uint64 * _lib.SG_MAX_SHARDS)()
        dev = (C.c_int * _lib.SG_MAX_SHARDS)()
        with self._use() as h:
            n = _lib.lib().sg_sharded_shards(h, lo, dev, _lib.SG_MAX_SHARDS)
        return [(int(lo[i]), int(dev[i])) for i in range(n)]

    def suggest_batch(self, queries=None, metric="jaccard", similarity=0.5, k=10, blob=None, offs=None):
        """-> (ids[n_q,k] u32 dictionary docIDs, scores[n_q,k] f64, counts[n_q] u32); row i best first (sg_sharded_suggest_batch)"""
        if blob is None:
            blob, offs = pack_strings(queries)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n_q = len(offs) - 1
        ids = np.zeros((n_q, k), dtype=np.uint32)
        sc = np.zeros((n_q, k), dtype=np.float64)
        cnt = np.zeros(n_q, dtype=np.uint32)
        code = resolve(metric).code
        if code is None:
            raise ValueError("a sharded search takes the metrics with a device twin (jaccard, cosine, dice, exact, overlap)")
        with self._use() as h:
            _lib.check(_lib.lib().sg_sharded_suggest_batch(h, blob.ctypes.data if blob.size else None, offs.ctypes.data, n_q, code,
                                                           float(similarity), int(k), ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data))
        return ids, sc, cnt

    def suggest_batch_device(self, d_blob, d_offs, n_q, metric, similarity, k, d_ids, d_scores, d_counts, stream=0):
        """Device-resident buffers (raw pointers; torch tensors' data_ptr()), asynchronous on `stream`; every shard has to be
        resident on the device that owns them (sg_sharded_suggest_batch_device)."""
        with self._use() as h:
            _lib.check(_lib.lib().sg_sharded_suggest_batch_device(h, d_blob, d_offs, int(n_q), resolve(metric).code, float(similarity),
                                                                  int(k), d_ids, d_scores, d_counts, stream))

    def autocomplete_batch(self, queries=None, limit=10, blob=None, offs=None):
        """-> (ids[n_q,limit] u32, counts[n_q] u32): the `limit` smallest dictionary docIDs (sg_sharded_autocomplete_batch)"""
        if blob is None:
            blob, offs = pack_strings(queries)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n_q = len(offs) - 1
        ids = np.zeros((n_q, limit), dtype=np.uint32)
        cnt = np.zeros(n_q, dtype=np.uint32)
        with self._use() as h:
            _lib.check(_lib.lib().sg_sharded_autocomplete_batch(h, blob.ctypes.data if blob.size else None, offs.ctypes.data, n_q, int(limit),
                                                                ids.ctypes.data, cnt.ctypes.data))
        return ids, cnt


def shard_merge(ids, scores, counts, doc_lo, k=None, autocomplete=False, device=0):
    """Test hook (sg_debug_shard_merge): the merge kernel alone on host arrays — ids [W, n, k] u32 local docIDs, scores [W, n, k]
    f64 (None with autocomplete), counts [W, n] u32, doc_lo [W] u64 -> (ids [n, k] u32, scores [n, k] f64 or None, counts [n] u32)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    doc_lo = np.ascontiguousarray(doc_lo, dtype=np.uint64)
    W, n, kk = ids.shape
    k = kk if k is None else int(k)
    assert k == kk and counts.shape == (W, n) and doc_lo.shape == (W,)
    o_ids = np.zeros((n, k), dtype=np.uint32)
    o_cnt = np.zeros(n, dtype=np.uint32)
    if autocomplete:
        sc = o_sc = None
    else:
        sc = np.ascontiguousarray(scores, dtype=np.float64)
        assert sc.shape == ids.shape
        o_sc = np.zeros((n, k), dtype=np.float64)
    _lib.check(_lib.lib().sg_debug_shard_merge(int(device), ids.ctypes.data, None if sc is None else sc.ctypes.data, counts.ctypes.data,
                                               doc_lo.ctypes.data, W, n, k, 1 if autocomplete else 0, o_ids.ctypes.data,
                                               None if o_sc is None else o_sc.ctypes.data, o_cnt.ctypes.data))
    return o_ids, o_sc, o_cnt
