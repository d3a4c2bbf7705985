"""DeviceDictionary: the reference's dictionary.Dictionary (docID -> string, docID = line number) behind sg_dictionary
(include/suggest_hip.h) — in the HBM of one GPU, where the rows of any search become strings without a
Python loop per slot, or host-resident (device=-1: no GPU needed, the plain host loop).
"""
import contextlib
import ctypes as C
import os
import threading

import numpy as np

from . import _lib
from .index import _enc, pack_strings


def text_guess(dictionary, slots):
    """A first text capacity for `slots` slots: twice the dictionary's mean string, never above slots * max_len (which always
    suffices).  A call that needs more says how much and is repeated once."""
    n = max(1, dictionary.n_docs)
    mean = -(-dictionary.bytes // n)
    return int(min(slots * dictionary.max_len, max(1 << 16, 2 * slots * mean)))


def split_text(text, text_offs):
    """(text, text_offs) -> list[bytes], one per slot"""
    b = text.tobytes()
    o = text_offs.tolist()
    return [b[o[i]:o[i + 1]] for i in range(len(o) - 1)]


EDIT_MODES = {"levenshtein": _lib.SG_EDIT_LEVENSHTEIN, "osa": _lib.SG_EDIT_OSA}


def edit_config(mode="levenshtein", fold_case=True, max_distance=None):
    """sg_edit_config: mode "levenshtein" or "osa" (adjacent transpositions at cost 1), max_distance None: no bound"""
    if mode not in EDIT_MODES and mode not in EDIT_MODES.values():
        raise ValueError("unknown edit mode %r" % (mode,))
    return _lib.SgEditConfig(EDIT_MODES.get(mode, mode), 1 if fold_case else 0, _lib.SG_EDIT_NONE if max_distance is None else int(max_distance), 0)


class DeviceDictionary:
    def __init__(self, lines=None, blob=None, offs=None, device=0, _handle=None):
        """`lines`: a list of str / bytes in docID order, or (blob, offs) as pack_strings returns them (sg_dictionary_upload).
        device < 0: a host-resident handle."""
        self._hlock = threading.Lock()
        if _handle is None:
            if blob is None:
                blob, offs = pack_strings(lines)
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
            offs = np.ascontiguousarray(offs, dtype=np.uint64)
            _handle = C.c_void_p()
            _lib.check(_lib.lib().sg_dictionary_upload(blob.ctypes.data if blob.size else None, offs.ctypes.data, len(offs) - 1, int(device),
                                                       C.byref(_handle)))
        self._h = _handle
        L = _lib.lib()
        self.n_docs, self.bytes, self.max_len = int(L.sg_dictionary_size(_handle)), int(L.sg_dictionary_bytes(_handle)), int(L.sg_dictionary_max_len(_handle))
        self.device = int(L.sg_dictionary_device(_handle))

    @classmethod
    def from_cdb(cls, path, device=0):
        """dictionary.OpenCDBDictionary: the <name>.cdb of BuildCDBDictionary / store_cdb_dictionary (sg_dictionary_open_cdb)"""
        h = C.c_void_p()
        _lib.check(_lib.lib().sg_dictionary_open_cdb(_enc(os.fspath(path)), int(device), C.byref(h)))
        return cls(_handle=h)

    def __len__(self):
        return self.n_docs

    @contextlib.contextmanager
    def _use(self):
        """The handle, retained for the duration of a C call (a concurrent close() only drops its own reference)."""
        L = _lib.lib()
        with self._hlock:
            h = self._h
            if not h:
                raise ValueError("dictionary is closed")
            L.sg_dictionary_retain(h)
        try:
            yield h
        finally:
            L.sg_dictionary_release(h)

    def close(self):
        lock = getattr(self, "_hlock", None)
        if lock is None:
            return
        with lock:
            h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().sg_dictionary_release(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self, ids, counts, row_offs=None, text_cap=None):
        """The strings of id rows (sg_dictionary_rows) -> (text u8, text_offs[slots + 1] u64): slot s holds
        text[text_offs[s] : text_offs[s + 1]].  ids [n_rows, row] with counts [n_rows]; or flat ids with ragged
        row_offs [n_rows + 1] as suggest_batch_mixed returns them.  Slots past a row's count, of a flagged row (SG_COUNT_*) or
        of no row are empty.  An id outside the dictionary raises."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        n_rows = counts.size
        if row_offs is None:
            row = ids.shape[1] if ids.ndim == 2 else (ids.size // n_rows if n_rows else 0)
            ro = None
        else:
            row = 0
            row_offs = np.ascontiguousarray(row_offs, dtype=np.uint64)
            ro = row_offs.ctypes.data
        slots = ids.size
        text_offs = np.zeros(slots + 1, dtype=np.uint64)
        cap = text_guess(self, slots) if text_cap is None else int(text_cap)
        needed = C.c_uint64()
        L = _lib.lib()
        while True:
            text = np.zeros(cap, dtype=np.uint8)
            with self._use() as h:
                rc = L.sg_dictionary_rows(h, ids.ctypes.data if slots else None, counts.ctypes.data if n_rows else None, ro, n_rows, int(row), slots,
                                          text.ctypes.data if cap else None, cap, text_offs.ctypes.data, C.byref(needed))
            if rc < 0 and text_cap is None and needed.value > cap and int(text_offs[slots]) == needed.value:
                cap = int(needed.value)        # (the text was too small: the call says how much it takes)
                continue
            _lib.check(rc)
            return text[:needed.value], text_offs

    def rows_device(self, d_ids, d_counts, d_row_offs, n_rows, row, slots, d_text, text_cap, d_text_offs, d_info, stream=0):
        """sg_dictionary_rows_device: raw device pointers (torch tensors' data_ptr(); d_row_offs None: rows of `row` slots),
        asynchronous on `stream`.  d_text_offs: slots + 1 u64; d_info: 2 u64 — the bytes needed, the entries outside."""
        with self._use() as h:
            _lib.check(_lib.lib().sg_dictionary_rows_device(h, d_ids, d_counts, d_row_offs, int(n_rows), int(row), int(slots), d_text, int(text_cap),
                                                            d_text_offs, d_info, stream))

    @staticmethod
    def _edit_rows(queries, ids, counts, row_offs, blob, offs):
        if blob is None:
            blob, offs = pack_strings(queries)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        n_rows = counts.size
        if len(offs) - 1 != n_rows:
            raise ValueError("one query per row: %d queries, %d rows" % (len(offs) - 1, n_rows))
        if row_offs is None:
            row = ids.shape[1] if ids.ndim == 2 else (ids.size // n_rows if n_rows else 0)
        else:
            row = 0
            row_offs = np.ascontiguousarray(row_offs, dtype=np.uint64)
        return blob, offs, counts, n_rows, int(row), row_offs

    def edit_distances(self, queries, ids, counts, row_offs=None, mode="levenshtein", fold_case=True, blob=None, offs=None):
        """sg_edit_rows -> distances (u32, shaped as ids): the edit distance between row i's query and each of its entries, over
        runes; 0xFFFFFFFF where a slot holds no entry.  Geometry as rows().  An id outside the dictionary raises."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        blob, offs, counts, n_rows, row, row_offs = self._edit_rows(queries, ids, counts, row_offs, blob, offs)
        dist = np.zeros(ids.shape, dtype=np.uint32)
        cfg = edit_config(mode, fold_case, None)
        with self._use() as h:
            _lib.check(_lib.lib().sg_edit_rows(h, C.byref(cfg), blob.ctypes.data if blob.size else None, offs.ctypes.data, ids.ctypes.data if ids.size else None,
                                               counts.ctypes.data if n_rows else None, None if row_offs is None else row_offs.ctypes.data, n_rows, row,
                                               ids.size, dist.ctypes.data if ids.size else None))
        return dist

    def edit_rerank(self, queries, ids, counts, scores=None, row_offs=None, k_out=None, mode="levenshtein", fold_case=True, max_distance=None, blob=None,
                    offs=None):
        """sg_edit_rerank -> (ids, scores or None, distances, counts), copies: every row stably re-ranked by (distance ascending, the
        order it had), entries above max_distance removed, at most k_out kept (None: the row), tails zeroed.  The exact top-k by
        edit distance among the row's entries — not over the whole dictionary."""
        ids = np.array(ids, dtype=np.uint32, order="C")
        blob, offs, counts, n_rows, row, row_offs = self._edit_rows(queries, ids, counts, row_offs, blob, offs)
        counts = counts.copy()
        if scores is not None:
            scores = np.array(scores, dtype=np.float64, order="C")
        dist = np.zeros(ids.shape, dtype=np.uint32)
        if k_out is None:
            k_out = max(1, row if row_offs is None else ids.size)
        cfg = edit_config(mode, fold_case, max_distance)
        with self._use() as h:
            _lib.check(_lib.lib().sg_edit_rerank(h, C.byref(cfg), blob.ctypes.data if blob.size else None, offs.ctypes.data, ids.ctypes.data if ids.size else None,
                                                 None if scores is None else scores.ctypes.data, counts.ctypes.data if n_rows else None,
                                                 None if row_offs is None else row_offs.ctypes.data, n_rows, row, ids.size, int(k_out),
                                                 dist.ctypes.data if ids.size else None))
        return ids, scores, dist, counts

    def edit_rows_device(self, config, d_q, d_q_offs, d_ids, d_counts, d_row_offs, n_rows, row, slots, d_dist, d_info, stream=0):
        """sg_edit_rows_device: raw device pointers, asynchronous on `stream`.  d_dist: slots u32; d_info: 2 u64."""
        with self._use() as h:
            _lib.check(_lib.lib().sg_edit_rows_device(h, C.byref(config), d_q, d_q_offs, d_ids, d_counts, d_row_offs, int(n_rows), int(row), int(slots), d_dist,
                                                      d_info, stream))

    def edit_rerank_device(self, config, d_q, d_q_offs, d_ids, d_scores, d_counts, d_row_offs, n_rows, row, slots, k_out, d_dist, d_info, stream=0):
        """sg_edit_rerank_device: as edit_rows_device, and the rows re-ranked in place (d_scores None: autocomplete rows)"""
        with self._use() as h:
            _lib.check(_lib.lib().sg_edit_rerank_device(h, C.byref(config), d_q, d_q_offs, d_ids, d_scores, d_counts, d_row_offs, int(n_rows), int(row),
                                                        int(slots), int(k_out), d_dist, d_info, stream))

    def edit_index(self, fold_case=True):
        """sg_edit_index_create -> EditIndex: the search structure for a complete search of this dictionary by edit distance"""
        return EditIndex(self, fold_case)

    def get(self, doc_id):
        """Dictionary.Get"""
        if not 0 <= int(doc_id) < self.n_docs:
            raise KeyError(doc_id)
        text, _ = self.rows(np.array([[doc_id]], dtype=np.uint32), np.array([1], dtype=np.uint32), text_cap=max(1, self.max_len))
        return text.tobytes()


class EditIndex:
    """sg_edit_index: a rune count and a 64-bit rune signature per string of a DeviceDictionary, and over them the
    complete search by edit distance — every string within max_distance edits of a query, the k nearest returned, ties by docID.
    Nothing is missed: no q-gram index proposes the candidates."""

    def __init__(self, dictionary, fold_case=True):
        self._hlock = threading.Lock()
        self.dictionary = dictionary
        self.fold_case = bool(fold_case)
        h = C.c_void_p()
        with dictionary._use() as dh:
            _lib.check(_lib.lib().sg_edit_index_create(dh, 1 if fold_case else 0, C.byref(h)))
        self._h = h
        self.n_docs, self.device = dictionary.n_docs, dictionary.device

    @contextlib.contextmanager
    def _use(self):
        L = _lib.lib()
        with self._hlock:
            h = self._h
            if not h:
                raise ValueError("edit index is closed")
            L.sg_edit_index_retain(h)
        try:
            yield h
        finally:
            L.sg_edit_index_release(h)

    def close(self):
        lock = getattr(self, "_hlock", None)
        if lock is None:
            return
        with lock:
            h, self._h = getattr(self, "_h", None), None
        if h:
            _lib.lib().sg_edit_index_release(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def config(self, max_distance, transpositions=False):
        return _lib.SgEditConfig(_lib.SG_EDIT_OSA if transpositions else _lib.SG_EDIT_LEVENSHTEIN, 1 if self.fold_case else 0, int(max_distance), 0)

    def array(self, which):
        """Test hook (sg_debug_edit_index_array): "runes" (u32 per string) or "sig" (u64 per string), as they lie in memory"""
        sel, dt = {"runes": (0, np.uint32), "sig": (1, np.uint64)}[which]
        n = C.c_uint64()
        with self._use() as h:
            _lib.check(_lib.lib().sg_debug_edit_index_array(h, sel, None, 0, C.byref(n)))
            out = np.zeros(n.value // np.dtype(dt).itemsize, dtype=dt)
            if out.size:
                _lib.check(_lib.lib().sg_debug_edit_index_array(h, sel, out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    def search(self, queries, k, max_distance, transpositions=False, blob=None, offs=None):
        """sg_edit_search -> (ids [n_q, k], dist [n_q, k], counts [n_q], hist [n_q, max_distance + 1]), all u32.  Row i: the
        min(k, hist[i].sum()) strings nearest to query i by (distance, docID); counts[i] = SG_COUNT_TOO_LONG for a query of more
        than 64 runes.  hist[i][t]: the strings at distance exactly t."""
        if blob is None:
            blob, offs = pack_strings(queries)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n_q, k = len(offs) - 1, int(k)
        cfg = self.config(max_distance, transpositions)
        ids = np.zeros((n_q, max(k, 0)), dtype=np.uint32)
        dist = np.zeros((n_q, max(k, 0)), dtype=np.uint32)
        counts = np.zeros(n_q, dtype=np.uint32)
        hist = np.zeros((n_q, min(int(max_distance), _lib.SG_EDIT_SEARCH_MAX_DISTANCE) + 1), dtype=np.uint32)
        with self._use() as h:
            _lib.check(_lib.lib().sg_edit_search(h, C.byref(cfg), blob.ctypes.data if blob.size else None, offs.ctypes.data, n_q, k,
                                                 ids.ctypes.data, dist.ctypes.data, counts.ctypes.data, hist.ctypes.data))
        return ids, dist, counts, hist

    def search_device(self, config, d_q, d_q_offs, n_q, k, d_ids, d_dist, d_counts, d_hist=None, stream=0):
        """sg_edit_search_device: raw device pointers (torch tensors' data_ptr()), asynchronous on `stream`.  d_ids, d_dist: n_q * k
        u32; d_counts: n_q u32; d_hist: n_q * (max_distance + 1) u32 or None."""
        with self._use() as h:
            _lib.check(_lib.lib().sg_edit_search_device(h, C.byref(config), d_q, d_q_offs, int(n_q), int(k), d_ids, d_dist, d_counts, d_hist, stream))

    def search_strings(self, queries, k, max_distance, transpositions=False):
        """The rows as strings -> (values: a list[bytes] per query, dist, counts, hist).  The search and the dictionary's
        materialise step (sg_dictionary_rows_device) run back to back on one stream over device-resident rows; needs torch and a
        device-resident dictionary."""
        import torch
        blob, offs = pack_strings(queries)
        n_q, k = len(offs) - 1, int(k)
        dev = torch.device("cuda", self.device)
        bins = int(max_distance) + 1
        slots = n_q * k
        text_cap = max(1, slots * self.dictionary.max_len)

        def on_dev(a, view):
            return torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).to(dev)
        d_q = on_dev(blob if blob.size else np.zeros(1, dtype=np.uint8), np.uint8)
        d_qo = on_dev(offs, np.int64)
        d_ids, d_dist = torch.zeros(max(slots, 1), dtype=torch.int32, device=dev), torch.zeros(max(slots, 1), dtype=torch.int32, device=dev)
        d_cnt, d_hist = torch.zeros(max(n_q, 1), dtype=torch.int32, device=dev), torch.zeros(max(n_q * bins, 1), dtype=torch.int32, device=dev)
        d_text, d_to = torch.zeros(text_cap, dtype=torch.uint8, device=dev), torch.zeros(slots + 1, dtype=torch.int64, device=dev)
        d_info = torch.zeros(2, dtype=torch.int64, device=dev)
        st = torch.cuda.current_stream(dev)
        st.synchronize()
        self.search_device(self.config(max_distance, transpositions), d_q.data_ptr(), d_qo.data_ptr(), n_q, k, d_ids.data_ptr(), d_dist.data_ptr(),
                           d_cnt.data_ptr(), d_hist.data_ptr(), stream=st.cuda_stream)
        self.dictionary.rows_device(d_ids.data_ptr(), d_cnt.data_ptr(), None, n_q, k, slots, d_text.data_ptr(), text_cap, d_to.data_ptr(), d_info.data_ptr(),
                                    stream=st.cuda_stream)
        st.synchronize()
        counts = d_cnt.cpu().numpy().view(np.uint32)[:n_q]
        values = split_text(d_text.cpu().numpy(), d_to.cpu().numpy().view(np.uint64))
        rows = [values[i * k:i * k + (0 if counts[i] >= 0xFFFFFFF0 else int(counts[i]))] for i in range(n_q)]
        return (rows, d_dist.cpu().numpy().view(np.uint32)[:slots].reshape(n_q, k), counts,
                d_hist.cpu().numpy().view(np.uint32)[:n_q * bins].reshape(n_q, bins))
