"""suggest.Service — the reference's public API (pkg/suggest/service.go:20-173) over the MI355X engine.

Same method names, argument meaning and error behaviour as the Go type, plus additive *Batch methods
(the GPU earns its keep on batches).  Dictionaries stay host side (docID -> string, line order), as in
pkg/dictionary/memory_dictionary.go — unless the service is made with device_dictionary=True: then every dictionary is also
held in HBM (DeviceDictionary) and the batch methods take their strings from there, one blob per call instead of a list
lookup per slot.  Both settings return equal results.
"""
import json
import os
import threading

from .dictionary import DeviceDictionary
from .index import IndexDescription, NGramIndex
from . import _lib
from .metric import resolve


class ResultItem:
    """pkg/suggest/service.go:12-17; distance: the edit distance to the query where a search re-ranked by it, else None"""
    __slots__ = ("score", "value", "distance")

    def __init__(self, score, value, distance=None):
        self.score, self.value, self.distance = score, value, distance

    def __repr__(self):
        if self.distance is None:
            return "ResultItem(score=%r, value=%r)" % (self.score, self.value)
        return "ResultItem(score=%r, value=%r, distance=%r)" % (self.score, self.value, self.distance)

    def __eq__(self, o):
        return isinstance(o, ResultItem) and (self.score, self.value, self.distance) == (o.score, o.value, o.distance)


class EditDistance:
    """A second ranking stage for SearchConfig(rerank=...): `candidates` per query by the q-gram metric, of those the top_k nearest
    by edit distance over runes (transpositions: optimal string alignment instead of Levenshtein; max_distance None: no bound).
    The exact top-k by edit distance AMONG THE CANDIDATES THE Q-GRAM SEARCH RETURNED, not over the whole dictionary.  Needs a
    Service(device_dictionary=True) and a metric with a device twin."""

    def __init__(self, candidates=64, transpositions=False, fold_case=True, max_distance=None):
        if candidates <= 0:
            raise ValueError("candidates should be greater or equal to 1")
        if max_distance is not None and not 0 <= max_distance <= 0xFFFFFFFF:
            raise ValueError("max_distance should be in 0 .. 2^32 - 1, or None")
        self.candidates, self.transpositions, self.fold_case, self.max_distance = int(candidates), bool(transpositions), bool(fold_case), max_distance

    @property
    def mode(self):
        return "osa" if self.transpositions else "levenshtein"

    def key(self):
        return (self.candidates, self.transpositions, self.fold_case, self.max_distance)


class SearchConfig:
    """NewSearchConfig — pkg/suggest/search.go:18-35 (same validation, same messages); rerank: an EditDistance, or None"""

    def __init__(self, query, top_k, metric, similarity, rerank=None):
        if top_k <= 0:
            raise ValueError("topK should be greater or equal to 1")
        if similarity <= 0 or similarity > 1:
            raise ValueError("similarity shouble be in (0.0, 1.0]")
        if rerank is not None and top_k > rerank.candidates:
            raise ValueError("topK should not be above the candidates of the re-rank")
        self.query, self.top_k, self.metric, self.similarity = query, int(top_k), resolve(metric), float(similarity)
        self.rerank = rerank


def read_dictionary(path):
    """OpenRAMDictionary — pkg/dictionary/helpers.go:25-48 (bufio.Scanner lines; docID = line number)"""
    with open(path, "rb") as f:
        data = f.read()
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in lines]


def read_cdb_dictionary(path):
    """OpenCDBDictionary (pkg/dictionary/helpers.go:14-22, cdb_dictionary.go): D. J. Bernstein's constant database
    written by BuildCDBDictionary (helpers.go:52-100) with key = docID as 4-byte little endian, value = the string.
    Records start at byte 2048 and run to the first hash table; returned in docID order."""
    import struct
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 2048:
        raise IOError("failed to open cdb dictionary file: %s" % path)
    tables = [struct.unpack_from("<II", data, 8 * i) for i in range(256)]
    end = min([pos for pos, n in tables if n] or [len(data)])            # (an empty table carries no position)
    out = {}
    pos = 2048
    while pos < end:
        klen, dlen = struct.unpack_from("<II", data, pos)
        key = data[pos + 8:pos + 8 + klen]
        out[struct.unpack("<I", key)[0] if klen == 4 else None] = data[pos + 8 + klen:pos + 8 + klen + dlen]
        pos += 8 + klen + dlen
    n = len(out)
    return [out.get(i, b"") for i in range(n)]


def read_configs(path):
    """ReadConfigs — pkg/suggest/config.go:84-112 (paths relative to the config file)"""
    with open(path, encoding="utf-8") as f:
        raw = json.load(f)
    base = os.path.dirname(os.path.abspath(path))
    out = []
    for d in raw:
        desc = IndexDescription.from_json(d)
        if desc.source and not os.path.isabs(desc.source):
            desc.source = os.path.join(base, desc.source)
        if desc.output and not os.path.isabs(desc.output):
            desc.output = os.path.join(base, desc.output)
        out.append(desc)
    return out


class Service:
    def __init__(self, device=0, device_dictionary=False):
        self._lock = threading.RLock()
        self._indexes = {}
        self._dictionaries = {}
        self._device_dictionaries = {}
        self.device = device
        self.device_dictionary = bool(device_dictionary)

    # -- AddIndexByDescription / AddRunTimeIndex / AddIndex (service.go:35-91) --
    def add_index_by_description(self, description):
        if description.driver == "RAM":
            return self.add_run_time_index(description)
        return self.add_on_disc_index(description)

    def add_on_disc_index(self, description):
        """AddOnDiscIndex (service.go:61-75): <output>/<name>.cdb dictionary + <name>.hd/.dl built by the reference's
        indexer; the posting lists are decoded once and kept as CSR in HBM."""
        base = os.path.join(description.output, description.name)
        dictionary = read_cdb_dictionary(base + ".cdb")
        index = NGramIndex.from_reference_files(base + ".hd", base + ".dl", description, device=self.device)
        on_device = DeviceDictionary.from_cdb(base + ".cdb", self.device) if self.device_dictionary else None
        return self._install(description.name, index, dictionary, on_device)

    def add_run_time_index(self, description):
        if not description.source or not os.path.exists(description.source):
            raise IOError("failed to create RAMDriver builder: open %s: no such file" % description.source)
        return self.add_index(description.name, read_dictionary(description.source), description)

    def add_index(self, name, dictionary, description):
        """dictionary: sequence of str/bytes, docID = position (dictionary.NewInMemoryDictionary)"""
        index = NGramIndex(dictionary, description, device=self.device)
        return self._install(name, index, dictionary)

    def _install(self, name, index, dictionary, on_device=None):
        dictionary = list(dictionary)
        if self.device_dictionary and on_device is None:
            on_device = DeviceDictionary(dictionary, device=self.device)
        with self._lock:                       # service.go:85-88
            old = self._indexes.get(name)
            old_dict = self._device_dictionaries.pop(name, None)
            self._indexes[name] = index
            self._dictionaries[name] = dictionary
            if on_device is not None:
                self._device_dictionaries[name] = on_device
        if old is not None:
            old.close()                        # handle is reference counted on the C side
        if old_dict is not None:
            old_dict.close()
        return None

    def get_dictionaries(self):
        with self._lock:
            return list(self._dictionaries)

    def _lookup(self, name):
        with self._lock:
            index, dictionary = self._indexes.get(name), self._dictionaries.get(name)
        if index is None or dictionary is None:
            raise KeyError("given dictionary %s is not exists" % name)   # service.go:111-113
        return index, dictionary

    def _lookup_device(self, name):
        with self._lock:
            return self._device_dictionaries.get(name)

    @staticmethod
    def _slot_values(text, text_offs, first, n):
        """the strings of slots first .. first + n of a (text, text_offs) pair"""
        o = text_offs[first:first + n + 1].tolist()
        b = text[o[0]:o[-1]].tobytes() if n else b""
        return [b[o[t] - o[0]:o[t + 1] - o[0]].decode("utf-8", "replace") for t in range(n)]

    @staticmethod
    def _value(dictionary, doc_id):
        v = dictionary[doc_id] if 0 <= doc_id < len(dictionary) else ""
        return v.decode("utf-8", "replace") if isinstance(v, (bytes, bytearray)) else v

    # -- Suggest / Autocomplete (service.go:105-173) --
    def _suggest_edit(self, dict_name, queries, top_k, metric, similarity, rerank):
        """rows of ResultItem with a distance (None for a query the plain call flags): search and rank on the device"""
        index, dictionary = self._lookup(dict_name)
        on_device = self._lookup_device(dict_name)
        if on_device is None:
            raise ValueError("a re-rank by edit distance needs Service(device_dictionary=True)")
        if resolve(metric).code is None:
            raise ValueError("a re-rank by edit distance takes the metrics with a device twin")
        ids, sc, dist, cnt = index.suggest_batch_edit(on_device, queries, metric, similarity, rerank.candidates, top_k, mode=rerank.mode,
                                                      fold_case=rerank.fold_case, max_distance=rerank.max_distance)
        out = []
        for i in range(len(queries)):
            c = int(cnt[i])
            if c >= _lib.SG_COUNT_TOO_LONG:
                out.append(None)
                continue
            out.append([ResultItem(float(sc[i, j]), self._value(dictionary, int(ids[i, j])), int(dist[i, j])) for j in range(c)])
        return out, cnt

    def suggest(self, dict_name, config):
        if getattr(config, "rerank", None) is not None:
            rows, cnt = self._suggest_edit(dict_name, [config.query], config.top_k, config.metric, config.similarity, config.rerank)
            if rows[0] is None:
                if int(cnt[0]) == _lib.SG_COUNT_TOO_LONG:
                    raise ValueError("query has more than %d n-grams" % _lib.SG_MAX_QUERY_TERMS)
                raise RuntimeError("query window is empty: the reference panics or dead-locks here (suggester.go:62)")
            return rows[0]
        index, dictionary = self._lookup(dict_name)
        cands = index.suggest(config.query, config.similarity, config.metric, config.top_k)
        return [ResultItem(score, self._value(dictionary, doc)) for doc, score in cands]

    def autocomplete(self, dict_name, query, limit):
        index, dictionary = self._lookup(dict_name)
        return [ResultItem(0, self._value(dictionary, doc)) for doc in index.autocomplete(query, limit)]

    # -- additive batch API --
    def suggest_batch(self, dict_name, queries, top_k, metric, similarity, rerank=None):
        SearchConfig("", top_k, metric, similarity, rerank)
        if rerank is not None:
            return self._suggest_edit(dict_name, list(queries), top_k, metric, similarity, rerank)[0]
        index, dictionary = self._lookup(dict_name)
        on_device = self._lookup_device(dict_name)
        if on_device is not None and resolve(metric).code is not None:
            ids, sc, cnt, text, text_offs = index.suggest_batch_strings(on_device, queries, metric, similarity, top_k)
            out = []
            for i in range(len(queries)):
                c = int(cnt[i])
                if c >= _lib.SG_COUNT_TOO_LONG:
                    out.append(None)
                    continue
                values = self._slot_values(text, text_offs, i * top_k, c)
                out.append([ResultItem(float(sc[i, j]), values[j]) for j in range(c)])
            return out
        ids, sc, cnt = index.suggest_batch(queries, metric, similarity, top_k)
        out = []
        for i in range(len(queries)):
            c = int(cnt[i])
            if c >= _lib.SG_COUNT_TOO_LONG:
                out.append(None)
                continue
            out.append([ResultItem(float(sc[i, j]), self._value(dictionary, int(ids[i, j]))) for j in range(c)])
        return out

    def suggest_many(self, dict_name, configs):
        """Service.Suggest for a list of SearchConfig — each with its own query, metric, similarity and topK — as ONE mixed batch
        (NGramIndex.suggest_batch_mixed): -> a list of [ResultItem] in the order of `configs`, None for a query the reference
        does not answer either (as suggest_batch).  Equal (metric, similarity, topK) share a table entry; more than 256 distinct
        ones go in several calls."""
        index, dictionary = self._lookup(dict_name)
        if any(getattr(c, "rerank", None) is not None for c in configs):
            raise ValueError("suggest_many does not re-rank: use suggest or suggest_batch for a SearchConfig with rerank=")
        out = [None] * len(configs)
        todo = list(range(len(configs)))
        while todo:
            table, number, taken, rest = [], {}, [], []
            for i in todo:
                c = configs[i]
                if c.metric.code is None:
                    raise ValueError("suggest_many takes the metrics with a device twin (jaccard, cosine, dice, exact, overlap)")
                key = (c.metric.code, c.similarity, c.top_k)
                if key not in number:
                    if len(table) == _lib.SG_MAX_MIXED_CONFIGS:
                        rest.append(i)
                        continue
                    number[key] = len(table)
                    table.append(key)
                taken.append(i)
            ids, sc, cnt, row_offs = index.suggest_batch_mixed([configs[i].query for i in taken], table, [number[(configs[i].metric.code, configs[i].similarity, configs[i].top_k)] for i in taken])
            on_device = self._lookup_device(dict_name)
            if on_device is not None:          # the generic step behind the mixed call: the ragged rows' strings in one blob
                text, text_offs = on_device.rows(ids, cnt, row_offs)
                for j, i in enumerate(taken):
                    c = int(cnt[j])
                    if c >= _lib.SG_COUNT_TOO_LONG:
                        continue
                    r = int(row_offs[j])
                    values = self._slot_values(text, text_offs, r, c)
                    out[i] = [ResultItem(float(sc[r + t]), values[t]) for t in range(c)]
                todo = rest
                continue
            for j, i in enumerate(taken):
                c = int(cnt[j])
                if c >= _lib.SG_COUNT_TOO_LONG:
                    continue
                r = int(row_offs[j])
                out[i] = [ResultItem(float(sc[r + t]), self._value(dictionary, int(ids[r + t]))) for t in range(c)]
            todo = rest
        return out

    # Go-style aliases so reference call sites read the same
    AddIndexByDescription = add_index_by_description
    AddRunTimeIndex = add_run_time_index
    AddOnDiscIndex = add_on_disc_index
    AddIndex = add_index
    GetDictionaries = get_dictionaries
    Suggest = suggest
    Autocomplete = autocomplete
