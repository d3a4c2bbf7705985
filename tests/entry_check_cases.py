"""What every search entry point of the C API answers to bad arguments: the table test_gpu_entry_checks.py and its CPU twin in
test_capi_cpu.py share.

An entry point opens with the same checks in the same order — null index, index not uploaded, k, similarity, metric (the last two
for a fuzzy search only), then the pointers it needs — and answers each with a return code and one exact sg_last_error() text
(include/suggest_hip.h; the texts mirror the reference's, "shouble" included).  A refused call writes nothing to its output
arrays.  ENTRIES names, per entry point, which of these it has; Call builds one call through ctypes from named arguments."""
import ctypes as C

import numpy as np

SG_E_INVALID, SG_E_NOT_UPLOADED = -1, -3
SG_JACCARD = 0
K = 4
SENTINEL = 0xC3

MSG_NULL_INDEX = "null index"
MSG_NULL_HANDLE = "null handle"
MSG_NOT_UPLOADED = "index not uploaded: call sg_index_upload first"
MSG_K_ZERO = "topK should be greater or equal to 1"
MSG_K_BIG = "topK above SG_MAX_TOPK"
MSG_SIMILARITY = "similarity shouble be in (0.0, 1.0]"
MSG_METRIC = "unknown metric"
MSG_NULL = "null argument"
MSG_NULL_DICT = "null dictionary"


class Buffers:
    """One query and the output arrays of one call, filled with a sentinel: untouched() says whether a call left them alone."""

    def __init__(self, query=b"nissan"):
        self.q = np.frombuffer(query, dtype=np.uint8).copy()
        self.offs = np.array([0, len(query)], dtype=np.uint64)
        self.out = {"ids": np.empty(2 * K, np.uint32), "scores": np.empty(2 * K, np.float64), "counts": np.empty(2, np.uint32),
                    "aux": np.empty(2 * K, np.uint32), "text": np.empty(256, np.uint8), "text_offs": np.empty(2 * K + 1, np.uint64),
                    "needed": np.empty(1, np.uint64)}
        self.ticket = C.c_void_p()
        self.reset()

    def reset(self):
        for a in self.out.values():
            a.view(np.uint8)[:] = SENTINEL
        self.ticket.value = None

    def untouched(self):
        return self.ticket.value is None and all((a.view(np.uint8) == SENTINEL).all() for a in self.out.values())

    def ptr(self, name):
        if name == "q":
            return self.q.ctypes.data
        if name == "offs":
            return self.offs.ctypes.data
        if name == "ticket":
            return C.addressof(self.ticket)
        return self.out[name].ctypes.data


class Entry:
    """One entry point.  args: its parameters after the handle, in order — "k" / "similarity" / "metric" take the case's value, a
    name of Buffers.ptr its pointer (null in the case that names it), ("lit", v) the value v, "n_q" one query, "len" the query's
    length, "lm" / "dict" / "tables" the handle the caller holds.  required: the pointers whose absence it refuses, with the text."""

    def __init__(self, name, args, required, fuzzy, handle="index", has_metric=None, device_buffers=False):
        self.name, self.args, self.required, self.fuzzy, self.handle = name, args, required, fuzzy, handle
        self.has_metric = fuzzy if has_metric is None else has_metric
        self.device_buffers = device_buffers      # its arrays would be read as device memory: never called with values that pass

    def call(self, L, handle, bufs, handles, k=K, similarity=0.5, metric=SG_JACCARD, null=None):
        """L: raw_lib().  -> (return code, sg_last_error())"""
        def addr(h):
            return C.c_void_p(h.value if isinstance(h, C.c_void_p) else h)

        argv = [addr(handle)]
        for a in self.args:
            if isinstance(a, tuple):
                argv.append(a[1])
            elif a == "k":
                argv.append(C.c_uint32(k))
            elif a == "similarity":
                argv.append(C.c_double(similarity))
            elif a == "metric":
                argv.append(C.c_int(metric))
            elif a == "n_q":
                argv.append(C.c_uint32(1))
            elif a == "len":
                argv.append(C.c_uint32(len(bufs.q)))
            elif a == null:
                argv.append(None)
            elif a in ("lm", "dict", "tables"):
                argv.append(addr(handles.get(a)))
            else:
                argv.append(C.c_void_p(bufs.ptr(a)))
        rc = getattr(L, self.name)(*argv)
        return rc, L.sg_last_error().decode()


def raw_lib():
    """The library without declared argument types: Entry.call passes every argument as the C type the header gives it, so a null
    goes where the binding's own declarations would refuse one."""
    from suggest_amd import _lib
    _lib.lib()
    L = C.CDLL(_lib.LIB_PATH)
    L.sg_last_error.restype = C.c_char_p
    return L


_ROWS = ["ids", "scores", "counts"]
_FUZZY = ["q", "offs", "n_q", "metric", "similarity", "k"] + _ROWS
_FUZZY_REQ = [(p, MSG_NULL) for p in ["offs"] + _ROWS]
_PREFIX_REQ = [(p, MSG_NULL) for p in ("offs", "ids", "counts")]
_STRINGS = ["dict", "text", ("lit", C.c_uint64(256)), "text_offs", "needed"]
_STRINGS_REQ = [("dict", MSG_NULL_DICT), ("text_offs", MSG_NULL)]
_STREAM = ("lit", None)
_DOC0, _REPLICA0 = ("lit", C.c_uint32(0)), ("lit", C.c_uint32(0))

ENTRIES = [
    Entry("sg_suggest_batch", _FUZZY, _FUZZY_REQ, True),
    Entry("sg_autocomplete_batch", ["q", "offs", "n_q", "k", "ids", "counts"], _PREFIX_REQ, False),
    Entry("sg_suggest_batch_device", _FUZZY + [_STREAM], [], True, device_buffers=True),
    Entry("sg_autocomplete_batch_device", ["q", "offs", "n_q", "k", "ids", "counts", _STREAM], [], False, device_buffers=True),
    Entry("sg_suggest_batch_multi", _FUZZY, _FUZZY_REQ, True),
    Entry("sg_autocomplete_batch_multi", ["q", "offs", "n_q", "k", "ids", "counts"], _PREFIX_REQ, False),
    Entry("sg_autocomplete_batch_from", ["q", "offs", "n_q", _DOC0, "k", "ids", "counts"], _PREFIX_REQ, False),
    Entry("sg_suggest_batch_from", ["q", "offs", "n_q", "metric", "similarity", ("lit", None), _DOC0, "k", "ids", "scores", "aux", "counts"],
          _FUZZY_REQ, True),
    Entry("sg_suggest_batch_tables", ["q", "offs", "n_q", "tables", "k"] + _ROWS, _FUZZY_REQ + [("tables", MSG_NULL)], False),
    Entry("sg_suggest_batch_strings", _FUZZY + _STRINGS, _FUZZY_REQ + _STRINGS_REQ, True),
    Entry("sg_autocomplete_batch_strings", ["q", "offs", "n_q", "k", "ids", "counts"] + _STRINGS, _PREFIX_REQ + _STRINGS_REQ, False),
    Entry("sg_suggest_submit", _FUZZY + ["ticket"], _FUZZY_REQ + [("ticket", MSG_NULL)], True),
    Entry("sg_suggest_submit_on", [_REPLICA0] + _FUZZY + ["ticket"], _FUZZY_REQ + [("ticket", MSG_NULL)], True),
    Entry("sg_autocomplete_submit", ["q", "offs", "n_q", _DOC0, "k", "ids", "counts", "ticket"], _PREFIX_REQ + [("ticket", MSG_NULL)], False),
    Entry("sg_suggest_one", ["q", "len", "metric", "similarity", "k"] + _ROWS, [(p, MSG_NULL) for p in ["q"] + _ROWS], True),
    Entry("sg_autocomplete_one", ["q", "len", "k", "ids", "counts"], [(p, MSG_NULL) for p in ("q", "ids", "counts")], False),
    Entry("sg_autocomplete_one_from", ["q", "len", _DOC0, "k", "ids", "counts"], [(p, MSG_NULL) for p in ("q", "ids", "counts")], False),
    Entry("sg_sharded_suggest_batch", _FUZZY, _FUZZY_REQ, True, handle="sharded"),
    Entry("sg_sharded_autocomplete_batch", ["q", "offs", "n_q", "k", "ids", "counts"], _PREFIX_REQ, False, handle="sharded"),
    Entry("sg_sharded_suggest_batch_device", _FUZZY + [_STREAM], _FUZZY_REQ, True, handle="sharded", device_buffers=True),
    # Predict: Cosine always, so a similarity and no metric; its rows are [n_q][top_k + 1] ids and [n_q] counts
    Entry("sg_spell_predict_batch", ["lm", "q", "offs", "n_q", "k", "similarity", "ids", "counts"],
          [(p, MSG_NULL) for p in ("lm", "offs", "ids", "counts")], True, has_metric=False),
]


def value_cases(entry, max_topk):
    """-> [(keyword arguments of Entry.call, return code, message)]: the values an uploaded index's entry point refuses"""
    cases = [(dict(k=0), SG_E_INVALID, MSG_K_ZERO), (dict(k=max_topk + 1), SG_E_INVALID, MSG_K_BIG)]
    if entry.fuzzy:
        cases += [(dict(similarity=0.0), SG_E_INVALID, MSG_SIMILARITY), (dict(similarity=1.5), SG_E_INVALID, MSG_SIMILARITY)]
    if entry.has_metric:
        cases += [(dict(metric=99), SG_E_INVALID, MSG_METRIC)]
    return cases


def pointer_cases(entry):
    return [(dict(null=p), SG_E_INVALID, msg) for p, msg in entry.required]


def order_cases(entry, max_topk):
    """A bad value together with a null pointer: the value's message wins, for every value case and every required pointer — the
    values are checked before the pointers."""
    return [(dict(kw, null=p), rc, msg) for kw, rc, msg in value_cases(entry, max_topk) for p, _ in entry.required]


def null_handle_message(entry):
    return MSG_NULL_HANDLE if entry.handle == "sharded" else MSG_NULL_INDEX
