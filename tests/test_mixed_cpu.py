"""CPU-only checks of the mixed batch's entry points (sg_suggest_batch_mixed and its device twin; include/suggest_hip.h): what they
refuse before they look at a device, the bindings above them, and the Go shim's argument counts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import CARS_DESC, ROOT

NEW = ("sg_suggest_batch_mixed", "sg_suggest_batch_mixed_device", "sg_coalesce_mixed", "sg_debug_mixed_last", "sg_debug_coalesce_hold",
       "sg_debug_coalesce_stats")


@pytest.fixture(scope="module")
def host_index(cars_lines):
    from suggest_amd import IndexDescription, NGramIndex
    d = IndexDescription(ngram_size=CARS_DESC["ngram_size"], wrap=CARS_DESC["wrap"], pad=CARS_DESC["pad"], alphabet=CARS_DESC["alphabet"])
    return NGramIndex(cars_lines[:200], d, upload=False)


def _call(ix, route, queries, configs, config_of, rows_cap=None, null=None):
    """the C entry point itself -> (rc, message); `null`: the name of one pointer argument passed as NULL"""
    from suggest_amd import _lib
    from suggest_amd.index import mixed_table, pack_strings
    L = _lib.lib()
    blob, offs = pack_strings(queries)
    n_q = len(queries)
    table = mixed_table(configs) if not isinstance(configs, C.Array) else configs
    cfg_of = np.asarray(config_of, dtype=np.uint32)
    rows = sum(int(table[int(g)].k) for g in cfg_of if int(g) < len(table))
    cap = rows if rows_cap is None else rows_cap
    ids = np.zeros(max(rows, 1), dtype=np.uint32)
    sc = np.zeros(max(rows, 1), dtype=np.float64)
    cnt = np.zeros(max(n_q, 1), dtype=np.uint32)
    ro = np.zeros(n_q + 1, dtype=np.uint64)
    args = dict(q=blob.ctypes.data, offs=offs.ctypes.data, configs=table, config_of=cfg_of.ctypes.data, ids=ids.ctypes.data, scores=sc.ctypes.data,
                counts=cnt.ctypes.data, row_offs=ro.ctypes.data)
    if null:
        args[null] = None
    if route == "host":
        rc = L.sg_suggest_batch_mixed(ix._h, args["q"], args["offs"], n_q, args["configs"], len(table), args["config_of"], cap,
                                      args["ids"], args["scores"], args["counts"], args["row_offs"])
    else:       # (host addresses stand in for device ones: everything here is refused before a pointer is followed)
        rc = L.sg_suggest_batch_mixed_device(ix._h, args["q"], args["offs"], n_q, args["configs"], len(table), args["config_of"], cap,
                                             args["ids"], args["scores"], args["counts"], args["row_offs"], None)
    return rc, L.sg_last_error().decode()


FUZZY = ("jaccard", 0.5, 10)
QUERIES = ["nissan", "toyota", "bmw"]


@pytest.mark.parametrize("route", ["host", "device"])
def test_the_table_is_checked_before_the_index(host_index, route):
    from suggest_amd import _lib
    assert _call(host_index, route, QUERIES, [], [0, 0, 0]) == (-1, "mixed batch: n_configs outside 1 .. SG_MAX_MIXED_CONFIGS")
    assert _call(host_index, route, QUERIES, [FUZZY] * 257, [0, 0, 0]) == (-1, "mixed batch: n_configs outside 1 .. SG_MAX_MIXED_CONFIGS")
    assert _call(host_index, route, QUERIES, [FUZZY, dict(metric=5, similarity=0.5, k=3)], [0, 1, 0]) == (-1, "unknown metric")
    assert _call(host_index, route, QUERIES, [FUZZY, dict(metric=-1, similarity=0.5, k=3)], [0, 1, 0]) == (-1, "unknown metric")
    assert _call(host_index, route, QUERIES, [dict(metric="cosine", similarity=0.5, k=3, first_doc=1)], [0, 0, 0]) == (-1, "mixed batch: first_doc with a fuzzy config")
    # k = 0, a similarity outside (0, 1]: the plain call's checks and messages (search.go:18-35), for fuzzy and autocomplete entries
    assert _call(host_index, route, QUERIES, [FUZZY, ("dice", 0.5, 0)], [0, 0, 0]) == (-1, "topK should be greater or equal to 1")
    assert _call(host_index, route, QUERIES, [dict(autocomplete=1, k=0)], [0, 0, 0]) == (-1, "topK should be greater or equal to 1")
    assert _call(host_index, route, QUERIES, [("dice", 0.0, 5)], [0, 0, 0]) == (-1, "similarity shouble be in (0.0, 1.0]")
    assert _call(host_index, route, QUERIES, [("dice", 0.5, _lib.SG_MAX_TOPK + 1)], [0, 0, 0]) == (-1, "topK above SG_MAX_TOPK")
    assert _call(host_index, route, QUERIES, [_lib.SgSearchConfig(0, 2, 0.5, 5, 0)], [0, 0, 0]) == (-1, "mixed batch: autocomplete is 0 or 1")
    # an autocomplete entry ignores metric and similarity and may page: it passes the table's checks (and meets the missing upload)
    assert _call(host_index, route, QUERIES, [dict(autocomplete=1, k=5, first_doc=7, metric=9, similarity=-1.0)], [0, 0, 0])[0] == -3


@pytest.mark.parametrize("route", ["host", "device"])
def test_null_pointers_are_refused(host_index, route):
    from suggest_amd import _lib
    for name in ("offs", "configs", "config_of", "ids", "scores", "counts", "row_offs"):
        assert _call(host_index, route, QUERIES, [FUZZY], [0, 0, 0], null=name) == (-1, "null argument"), name
    L = _lib.lib()
    assert L.sg_suggest_batch_mixed(None, None, None, 0, None, 0, None, 0, None, None, None, None) == -1
    assert L.sg_last_error() == b"null index"
    assert L.sg_suggest_batch_mixed_device(None, None, None, 0, None, 0, None, 0, None, None, None, None, None) == -1
    assert L.sg_coalesce_mixed(None, 1) == -1 and L.sg_debug_coalesce_hold(None, 1) == -1 and L.sg_debug_coalesce_stats(None, None) == -1
    assert L.sg_debug_mixed_last(None, 0, None, 1) == -1


def test_the_host_route_checks_config_numbers_and_rows_cap(host_index):
    table = [FUZZY, ("cosine", 0.4, 3)]
    assert _call(host_index, "host", QUERIES, table, [0, 1, 2]) == (-1, "mixed batch: config_of holds a number outside the table")
    assert _call(host_index, "host", QUERIES, table, [0, 1, 0xFFFFFFFF]) == (-1, "mixed batch: config_of holds a number outside the table")
    assert _call(host_index, "host", QUERIES, table, [0, 1, 0], rows_cap=22) == (-1, "mixed batch: rows_cap is below the sum of the queries' k")
    # everything in order: only the upload is missing
    rc, msg = _call(host_index, "host", QUERIES, table, [0, 1, 0], rows_cap=23)
    assert (rc, msg) == (-3, "index not uploaded: call sg_index_upload first")
    assert _call(host_index, "device", QUERIES, table, [0, 1, 0])[0] == -3
    # no queries: nothing to do, row_offs = [0] — on the host route even without an upload
    assert _call(host_index, "host", [], table, [])[0] == 0


def test_switches_and_hooks_need_an_uploaded_index(host_index):
    from suggest_amd import _lib
    L = _lib.lib()
    assert L.sg_coalesce_mixed(host_index._h, 1) == -3
    assert L.sg_debug_coalesce_hold(host_index._h, 1) == -3
    assert L.sg_debug_coalesce_stats(host_index._h, (C.c_uint64 * 4)()) == -3
    perm = (C.c_uint32 * 4)()
    start = (C.c_uint32 * 2)()
    assert L.sg_debug_mixed_last(perm, 4, start, 1) == -1
    assert b"no mixed call" in L.sg_last_error()
    out = (C.c_double * 5)()
    assert L.sg_debug_mixed_times(out) == 0 and list(out) == [0.0] * 5 and L.sg_debug_mixed_times(None) == -1


def test_python_bindings(host_index):
    from suggest_amd import SearchConfig, Service, _lib
    from suggest_amd.index import mixed_table
    assert set(NEW) <= set(_lib.EXPORTS) and all(hasattr(_lib.lib(), n) for n in NEW)
    assert C.sizeof(_lib.SgSearchConfig) == 24 and _lib.SG_MAX_MIXED_CONFIGS == 256
    t = mixed_table([("cosine", 0.25, 7), dict(autocomplete=1, k=5, first_doc=3), _lib.SgSearchConfig(4, 0, 1.0, 2, 0)])
    assert [(c.metric, c.autocomplete, c.similarity, c.k, c.first_doc) for c in t] == [(1, 0, 0.25, 7, 0), (0, 1, 0.0, 5, 3), (4, 0, 1.0, 2, 0)]
    with pytest.raises(ValueError):
        host_index.suggest_batch_mixed(QUERIES, [FUZZY], [0, 0])                  # one config number per query
    with pytest.raises(_lib.SuggestHipError) as e:
        host_index.suggest_batch_mixed(QUERIES, [FUZZY], [0, 1, 0])
    assert e.value.code == -1
    with pytest.raises(_lib.SuggestHipError) as e:
        host_index.suggest_batch_mixed(QUERIES, [FUZZY], [0, 0, 0])
    assert e.value.code == -3
    with pytest.raises(_lib.SuggestHipError) as e:
        host_index.coalesce_mixed(True)
    assert e.value.code == -3
    ids, sc, cnt, ro = host_index.suggest_batch_mixed([], [FUZZY], [])
    assert ids.size == 0 and sc.size == 0 and cnt.size == 0 and ro.tolist() == [0]
    with pytest.raises(KeyError):
        Service().suggest_many("cars", [SearchConfig("x", 3, "cosine", 0.5)])


def test_go_shim_arity_matches_the_header():
    """go/suggesthip/suggesthip.go has never met a Go compiler: SuggestMany's call passes as many arguments as the header declares"""
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    for fn in ("sg_suggest_batch_mixed",):
        decl = re.search(r"int %s\(([^;]*)\);" % fn, header).group(1)
        call = re.search(r"C\.%s\(([^\n]*)\)\n" % fn, go)
        assert call, fn
        depth, n = 0, 1
        for ch in call.group(1):
            depth += ch in "([{"
            depth -= ch in ")]}"
            n += ch == "," and depth == 0
        assert n == decl.count(",") + 1 == 12, fn
    assert "func (i *Index) SuggestMany(reqs []ManyConfig) ([][]suggest.Candidate, []uint32, error)" in go
    fields = re.search(r"C\.sg_search_config\{([^}]*)\}", go).group(1)
    assert [f.split(":")[0].strip() for f in fields.split(",")] == ["metric", "autocomplete", "similarity", "k", "first_doc"]


def test_cpp_mirror_checks_before_the_device():
    import subprocess
    cpp = os.path.join(ROOT, "tests", "cpp")
    binary = os.path.join(cpp, "_build", "suggest_many_test")
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", cpp, "-f", "mixed.mk", "_build/suggest_many_test"], check=True, capture_output=True)
    r = subprocess.run([binary, "--cpu", os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
