"""CPU-only checks of the product's host side: the C-ABI library loads and exports every declared symbol,
the host tokenizer and CSR builder agree with the oracle and with the reference's index files."""
import os
import re

import numpy as np
import pytest

import oracle
import refindex
from conftest import CARS_DESC, WORDS_DESC, GOLDEN, ROOT


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(ngram_size=d["ngram_size"], wrap=d["wrap"], pad=d["pad"], alphabet=d["alphabet"])


def test_library_exports_every_declared_symbol():
    from suggest_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h")).read()
    declared = set(re.findall(r"\b(sg_[a-z_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    assert {"sg_debug_index_build_table_bits", "sg_debug_index_build_report"} <= declared
    # the builder's table hook takes 0 (the default) and 4 .. 20
    import ctypes as C
    try:
        assert [L.sg_debug_index_build_table_bits(b) for b in (3, 4, 20, 21, 0)] == [-1, 0, 0, -1, 0]
    finally:
        L.sg_debug_index_build_table_bits(0)
    assert L.sg_debug_index_build_report((C.c_uint32 * 4)()) == 0 and L.sg_debug_index_build_report(None) == -1
    from suggest_amd.index import build_report, build_table_bits
    with build_table_bits(4):
        pass
    with pytest.raises(_lib.SuggestHipError):
        with build_table_bits(21):
            pass
    assert list(build_report()) == ["passes", "log2_table", "terms", "long_docs"]


def test_product_does_not_touch_the_oracle():
    # the product path must not import, link, include or call anything under oracle/
    pat = re.compile(r"import\s+oracle|from\s+oracle|liboracle|oracle/|suggest_oracle|or_suggest|or_index")
    for dirpath, _, files in os.walk(os.path.join(ROOT, "suggest_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".inc")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert not pat.search(text), (f, pat.search(text).group(0))


def test_search_without_upload_fails_loudly(cars_lines):
    from suggest_amd import NGramIndex, _lib
    ix = NGramIndex(cars_lines[:100], _desc(CARS_DESC), upload=False)
    with pytest.raises(_lib.SuggestHipError) as e:
        ix.suggest_batch(["nissan"], "jaccard", 0.5, 5)
    assert e.value.code == -3


def test_search_entry_points_refuse_a_missing_or_unuploaded_index(cars_lines):
    """The CPU twin of test_gpu_entry_checks.py: every search entry point answers a null index with SG_E_INVALID, and an index that
    was never uploaded with SG_E_NOT_UPLOADED — before it looks at k, the similarity, the metric or a pointer — and writes nothing.
    (A sharded handle only adopts uploaded shards: its entry points have the null case alone here.)"""
    import entry_check_cases as ec
    from suggest_amd import NGramIndex
    ix = NGramIndex(cars_lines[:100], _desc(CARS_DESC), upload=False)
    L, bufs = ec.raw_lib(), ec.Buffers()
    for entry in ec.ENTRIES:
        for kw in (dict(), dict(k=0)):
            bufs.reset()
            rc, msg = entry.call(L, None, bufs, {}, **kw)
            assert (rc, msg) == (ec.SG_E_INVALID, ec.null_handle_message(entry)), (entry.name, kw)
            assert bufs.untouched(), (entry.name, kw)
        if entry.handle != "index":
            continue
        bad = [dict(), dict(k=0), dict(similarity=1.5), dict(metric=99)] + [dict(null=p) for p, _ in entry.required]
        for kw in bad:
            bufs.reset()
            with ix._use() as h:
                rc, msg = entry.call(L, h, bufs, {}, **kw)
            assert (rc, msg) == (ec.SG_E_NOT_UPLOADED, ec.MSG_NOT_UPLOADED), (entry.name, kw)
            assert bufs.untouched(), (entry.name, kw)
    ix.close()


def test_argument_validation(cars_lines):
    from suggest_amd import NGramIndex, IndexDescription, SearchConfig, _lib
    with pytest.raises(ValueError):
        SearchConfig("x", 0, "cosine", 0.5)          # search.go:20-22
    with pytest.raises(ValueError):
        SearchConfig("x", 1, "cosine", 0.0)          # search.go:24-26
    with pytest.raises(ValueError):
        SearchConfig("x", 1, "cosine", 1.5)
    with pytest.raises(_lib.SuggestHipError):
        NGramIndex(cars_lines[:10], IndexDescription(ngram_size=9), upload=False)


def test_host_tokenizer_matches_oracle(cars_lines, words_lines):
    from suggest_amd import NGramIndex
    for lines, desc in ((cars_lines, CARS_DESC), (words_lines[::50], WORDS_DESC)):
        ix = NGramIndex(lines[:50], _desc(desc), upload=False)
        ora = oracle.OracleIndex(lines[:50], **desc)
        probes = list(lines[::17]) + [b"", b" ", b"a", b"  x y  ", "Ёжик в тумане".encode(), b"\xff\xfeabc", "İi".encode(),
                                      b"NISSAN TITAN", b"lalala", "жи".encode()]
        for p in probes:
            for ac in (False, True):
                assert ix.tokenize(p, ac) == ora.tokenize(p, ac), (p, ac)


def test_cars_csr_matches_reference_files(cars_lines, golden_dir):
    """Host CSR == db/cars.{hd,dl} written by the reference (after de-duplicating a doc's repeated terms,
    which the CSR keeps as a multiplicity side table): same keys, raw lengths, postings."""
    from suggest_amd import NGramIndex
    ix = NGramIndex(cars_lines, _desc(CARS_DESC), upload=False)
    n_idx, ref = refindex.read_index(os.path.join(golden_dir, "db", "cars.hd"), os.path.join(golden_dir, "db", "cars.dl"))
    mine = ix.lists()
    st = ix.stats()
    assert st["n_segments"] == n_idx and st["n_lists"] == len(ref) and st["n_postings_raw"] == sum(v[0] for v in ref.values())
    assert set(mine) == set(ref)
    for key, (raw_len, post) in ref.items():
        assert mine[key] == (raw_len, sorted(set(post))), key


def test_words_csr_matches_oracle(words_lines):
    from suggest_amd import NGramIndex
    ix = NGramIndex(words_lines, _desc(WORDS_DESC), upload=False)
    ora = oracle.OracleIndex(words_lines, **WORDS_DESC).lists()
    mine = ix.lists()
    assert set(mine) == set(ora)
    assert all(mine[k] == (ora[k][0], ora[k][1]) for k in ora)


def test_threaded_host_build_equals_the_sequential_one(words_lines, cars_lines, monkeypatch):
    """build_host_index splits the docs into contiguous blocks, one thread each: term numbering (first occurrence over
    ascending docIDs), list layout and the repeated-term table must not depend on the number of blocks, nor on whether
    the blocks count into their own or into one shared set of cursors."""
    from suggest_amd import NGramIndex
    for lines, desc in ((words_lines, WORDS_DESC), (cars_lines + ["", "aaaaaa", "Škoda škoda"] * 1500, CARS_DESC)):
        got = {}
        for thr, shared in (("1", False), ("2", False), ("5", False), ("32", False), ("7", True)):
            monkeypatch.setenv("SG_BUILD_THREADS", thr)
            if shared:
                monkeypatch.setenv("SG_BUILD_SHARED_COUNTERS", "1")
            else:
                monkeypatch.delenv("SG_BUILD_SHARED_COUNTERS", raising=False)
            ix = NGramIndex(lines, _desc(desc), upload=False)
            got[(thr, shared)] = (ix.digest(), ix.stats())
            ix.close()
        first = got[("1", False)]
        assert all(v == first for v in got.values()), got


def test_algorithmic_bytes_matches_oracle_definition():
    from suggest_amd import NGramIndex, IndexDescription, synth
    blob, offs = synth.make_dict(20000, seed=1)
    qb, qo = synth.make_queries(64, blob, offs, seed=2)
    ix = NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), upload=False)
    ora = oracle.OracleIndex(blob=blob, offs=offs, **synth.DESCRIPTION)
    qs = synth.unpack(qb, qo)
    for metric, alpha, k in (("jaccard", 0.5, 10), ("cosine", 0.4, 20)):
        assert ix.algorithmic_bytes(qb, qo, metric, alpha, k) == sum(ora.algorithmic_bytes(q, metric, alpha, k) for q in qs)


def test_reference_built_files_load_into_the_same_csr(cars_lines, golden_dir):
    """sg_index_load_reference: the gob header + VB / skip-VB lists of db/cars.{hd,dl} give exactly the CSR
    that building from cars.dict gives (keys, raw lengths, postings), and match the independent Python decoder."""
    from suggest_amd import NGramIndex
    hd, dl = os.path.join(golden_dir, "db", "cars.hd"), os.path.join(golden_dir, "db", "cars.dl")
    loaded = NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), upload=False)
    built = NGramIndex(cars_lines, _desc(CARS_DESC), upload=False)
    a, b = loaded.lists(), built.lists()
    assert a == b
    sa, sb = loaded.stats(), built.stats()
    for key in ("n_docs", "n_segments", "n_terms", "n_lists", "n_postings", "n_postings_raw", "posting_bytes"):
        assert sa[key] == sb[key], key
    n_idx, ref = refindex.read_index(hd, dl)
    assert {k: (v[0], sorted(set(v[1]))) for k, v in ref.items()} == a


def test_reference_built_roaring_lists_load(golden_dir):
    """db/words_subset.{hd,dl} (subset of the reference's words index, bytes verbatim) holds all three codecs incl. 40
    roaring bitmaps; the C++ loader must agree with the Python decoder list by list."""
    from suggest_amd import NGramIndex
    hd, dl = os.path.join(golden_dir, "db", "words_subset.hd"), os.path.join(golden_dir, "db", "words_subset.dl")
    loaded = NGramIndex.from_reference_files(hd, dl, _desc(WORDS_DESC), upload=False).lists()
    n_idx, ref = refindex.read_index(hd, dl)
    assert sum(1 for v in ref.values() if v[0] > 256) == 40
    assert {k: (v[0], sorted(set(v[1]))) for k, v in ref.items()} == loaded


def test_loader_rejects_bad_inputs(golden_dir, tmp_path):
    from suggest_amd import NGramIndex, IndexDescription, _lib
    hd, dl = os.path.join(golden_dir, "db", "cars.hd"), os.path.join(golden_dir, "db", "cars.dl")
    with pytest.raises(_lib.SuggestHipError):
        NGramIndex.from_reference_files(hd + ".nope", dl, _desc(CARS_DESC), upload=False)
    with pytest.raises(_lib.SuggestHipError):      # alphabet that cannot express the stored terms
        NGramIndex.from_reference_files(hd, dl, IndexDescription(alphabet=("numbers",), pad="#"), upload=False)
    bad = tmp_path / "bad.hd"
    bad.write_bytes(open(hd, "rb").read()[:1000])
    with pytest.raises(_lib.SuggestHipError):
        NGramIndex.from_reference_files(str(bad), dl, _desc(CARS_DESC), upload=False)


def test_cdb_dictionary_matches_the_source_lines(cars_lines, golden_dir):
    from suggest_amd.service import read_cdb_dictionary
    assert read_cdb_dictionary(os.path.join(golden_dir, "db", "cars.cdb")) == cars_lines


def test_stream_shapes_are_pinned():
    """[r6] The stream workgroup a launch starts from (capi.inc pipe_shape_model) for the sixteen launches it was measured on —
    1 M ... 16 M synthetic strings (q = 3, 19.99 n-grams per document, SG_T_FLOOR 8) under Jaccard >= 0.5 and Cosine >= 0.4, each
    with the three shapes side by side on one resident index (profiles/r06final_shape_by_size.txt,
    r06final_shape_auto_by_size.txt) — and the 25 M-string index of the wide-descriptor test.  0 / 1 / 2 = 2 / 4 / 8 wavefronts on
    2^11 / 2^12 / 2^13 counters; the expected query volumes are the ones the GPU box printed (SG_VERBOSE)."""
    import ctypes as C
    from suggest_amd import _lib
    L = _lib.lib()
    JACCARD, COSINE = 0, 1

    def shape(est, metric, alpha, terms=19.99, floor=8):
        out = C.c_int32(-1)
        _lib.check(L.sg_debug_pipe_shape(float(est), float(terms), floor, metric, float(alpha), C.byref(out)))
        return out.value

    est = {1: 2316, 2: 4448, 4: 8711, 6: 12975, 8: 17240, 10: 21500, 13: 27950, 16: 34299, 25: 53484}    # million strings -> chunks
    fastest = {   # (million strings, metric): the shape with the shortest call in the sweeps
        (1, JACCARD): 0, (2, JACCARD): 0, (4, JACCARD): 1, (6, JACCARD): 1, (8, JACCARD): 1, (10, JACCARD): 1, (13, JACCARD): 2, (16, JACCARD): 2,
        (25, JACCARD): 2,
        (1, COSINE): 0, (2, COSINE): 1, (4, COSINE): 1, (6, COSINE): 2, (8, COSINE): 2, (10, COSINE): 2, (13, COSINE): 2, (16, COSINE): 2,
    }
    for (m, metric), want in fastest.items():
        assert shape(est[m], metric, 0.5 if metric == JACCARD else 0.4) == want, (m, metric)
    # a similarity that skips nothing streams every list: the heavier shape earlier; a high one the lighter shape later
    assert shape(est[10], JACCARD, 0.2) == 2 and shape(est[16], JACCARD, 0.8) == 1
    assert L.sg_debug_pipe_shape(1000.0, 20.0, 8, 7, 0.5, C.byref(C.c_int32())) != 0       # (a tabulated metric has no model: the index's own choice)


def test_tuner_choices_are_pinned(cars_lines, words_lines):
    """[r5] The auto-tuner's choices (counter words, filter table, pipeline) for the dictionaries they were measured on — rounds 2-3
    shipped the wrong filter table for three regimes unnoticed.  The statistics of the large synthetic dictionaries are the ones
    the GPU box printed (SG_VERBOSE: expected query volume / longest term, in 16-byte chunks of u32 postings); the reference's own
    dictionaries and a 200 k synthetic one are built here and their statistics recomputed."""
    import ctypes as C
    from suggest_amd import NGramIndex, IndexDescription, synth, _lib
    L = _lib.lib()

    def choice(est, longest):
        out = (C.c_int32 * 6)()
        _lib.check(L.sg_debug_tune_choice(float(est), float(longest), out))
        return {"log2_cnt": out[0], "level": out[1], "pipe": out[2], "stream": tuple(out[3:6])}

    BIG, MID, SMALL = (8, 13, 8192), (4, 12, 4096), (2, 11, 2048)
    measured = {   # dictionary: (expected query volume, longest term) -> what every sweep since round 4 found best (DESIGN.md §4 knobs)
        # stream = (wavefronts, log2 counters, descriptor bytes) of a stream workgroup (profiles/r05zj_*: 60 k ... 4 M strings)
        "headline 10M q=3": ((21500, 2520), dict(log2_cnt=11, level=4, pipe=1, stream=BIG)),
        "families 10M q=3": ((21536, 2527), dict(log2_cnt=11, level=4, pipe=1, stream=BIG)),
        "4M q=3": ((9264, 1090), dict(log2_cnt=11, level=4, pipe=1, stream=MID)),
        "2M q=3": ((4632, 545), dict(log2_cnt=11, level=4, pipe=1, stream=SMALL)),
        "cfg2 1M q=3": ((2316, 272), dict(log2_cnt=11, level=4, pipe=1, stream=SMALL)),
        "60k q=3": ((311, 32), dict(log2_cnt=11, level=4, pipe=1, stream=SMALL)),
        "cfg4 10M q=2": ((826904, 78375), dict(log2_cnt=11, level=4, pipe=0, stream=BIG)),
        "skewed 10M q=3": ((583089, 443397), dict(log2_cnt=12, level=4, pipe=0, stream=BIG)),
        "cfg5 vocabulary": ((1219, 397), dict(log2_cnt=11, level=2, pipe=0, stream=SMALL)),
        "cars": ((790, 390), dict(log2_cnt=11, level=2, pipe=0, stream=SMALL)),
        "words": ((5280, 3639), dict(log2_cnt=11, level=2, pipe=0, stream=SMALL)),
    }
    for name, ((est, longest), want) in measured.items():
        assert choice(est, longest) == want, name

    def built(ix):
        st, out = (C.c_double * 2)(), (C.c_int32 * 6)()
        with ix._use() as h:
            _lib.check(L.sg_debug_tune_index(h, st, out))
        return (st[0], st[1]), {"log2_cnt": out[0], "level": out[1], "pipe": out[2], "stream": tuple(out[3:6])}

    (est, longest), got = built(NGramIndex(cars_lines, _desc(CARS_DESC), upload=False))
    assert 600 < est < 1000 and 300 < longest < 500 and got == measured["cars"][1], (est, longest, got)
    (est, longest), got = built(NGramIndex(words_lines, _desc(WORDS_DESC), upload=False))
    assert 4000 < est < 6500 and 3000 < longest < 4200 and got == measured["words"][1], (est, longest, got)
    blob, offs = synth.make_dict(200000, seed=1)      # uniform strings: the longest term a tenth of a query's volume, like the headline
    (est, longest), got = built(NGramIndex(blob=blob, offs=offs, description=IndexDescription(**synth.DESCRIPTION), upload=False))
    assert 450 < est < 800 and longest < 0.25 * est and got == dict(log2_cnt=11, level=4, pipe=1, stream=SMALL), (est, longest, got)


def _rows_layout(n_q, k, split, reorder):
    import ctypes as C
    from suggest_amd import _lib
    out = (C.c_uint64 * 16)()
    _lib.check(_lib.lib().sg_debug_rows_layout(n_q, k, split, reorder, out))
    return dict(zip(("s", "id", "split", "items", "slot", "part_n", "part_s", "part_id", "ord", "ord_ctl", "bytes",
                     "slot_cap", "item_cap", "ord_blocks", "max_parts", "ctl_words"), (int(x) for x in out)))


def _assert_carved(regions, total):
    """regions: name -> (offset, bytes, alignment).  Every region aligned, inside the block, no two overlapping."""
    live = sorted((off, off + size, name) for name, (off, size, align) in regions.items() if size)
    for name, (off, size, align) in regions.items():
        assert off % align == 0, (name, off, align)
        assert off + size <= total, (name, off, size, total)
    for (_, e0, a), (b1, _, b) in zip(live, live[1:]):
        assert e0 <= b1, ("overlap", a, b)


def test_scratch_rows_layout_is_disjoint_and_sized():
    """The SCRATCH_ROWS block as launch() carves it (capi.inc rows_layout): the HBM top-k rows (k > SG_K_LDS = 64) or the
    split-query queue — a 64-byte control head, items, slot words, the parts' counts, score rows and id rows, slot_cap x
    SG_MAX_PARTS x k entries — then the ordered list of the queries and its control words (+ block histograms on the direct
    path).  Regions pairwise disjoint, aligned for their widest access, inside the block's size."""
    for n_q in (1, 2, 63, 1000, 4096, 8191, 8192, 65536, 131073, 1 << 21):
        for k in (1, 64, 65, 65536):
            for split in (0, 1):
                for reorder in (0, 1, 2):
                    L = _rows_layout(n_q, k, split, reorder)
                    ctx = (n_q, k, split, reorder)
                    reg = {}
                    if k > 64:
                        assert L["split"] == L["items"] == 0 and L["slot_cap"] == 0, ctx
                        reg["s"] = (L["s"], n_q * k * 8, 8)
                        reg["id"] = (L["id"], n_q * k * 4, 4)
                    elif split:
                        P, sc, ic = L["max_parts"], L["slot_cap"], L["item_cap"]
                        assert P == 32 and 1 <= sc <= n_q and sc * P * k * 12 <= 1 << 30, ctx
                        assert ic == min(max(n_q * 4, 4096), 262144), ctx
                        reg["split"] = (L["split"], 64, 16)
                        reg["items"] = (L["items"], ic * 16, 16)
                        reg["slot"] = (L["slot"], sc * 8, 8)
                        reg["part_n"] = (L["part_n"], sc * P * 4, 4)
                        reg["part_s"] = (L["part_s"], sc * P * k * 8, 8)
                        reg["part_id"] = (L["part_id"], sc * P * k * 4, 4)
                    else:
                        assert L["bytes"] == 0 or reorder, ctx
                    if reorder:
                        blocks = (n_q + 1023) // 1024
                        assert L["ord_blocks"] == blocks, ctx
                        reg["ord"] = (L["ord"], n_q * 4, 4)
                        # control words, then (direct path) a 1024-byte histogram per block of the ordering launch
                        reg["ord_ctl"] = (L["ord_ctl"], L["ctl_words"] * 4 + (blocks * 1024 if reorder == 2 else 0), 16)
                    else:
                        assert L["ord"] == L["ord_ctl"] == 0, ctx
                    assert L["bytes"] % 16 == 0, ctx
                    _assert_carved(reg, L["bytes"])
                    # nothing but these regions: the block ends within 16 bytes (+ alignment) of the last one
                    if reg:
                        assert L["bytes"] - max(o + s for o, s, _ in reg.values()) < 16, ctx


def test_scratch_pipe_layout_is_disjoint_and_sized():
    """The SCRATCH_PIPE block (capi.inc pipe_layout): fb_n / ovf_n, then a piece's records (256-byte aligned), verify records,
    overflow blocks, candidate counts, and the batch's list of the queries handed back — n_q + 1 words, whatever the piece."""
    import ctypes as C
    from suggest_amd import _lib
    for n_q in (1, 2, 63, 1000, 65535, 65536, 65537, 1 << 21):
        for cand_cap in (1, 2, 16, 64, 512, 4096):
            out = (C.c_uint64 * 12)()
            _lib.check(_lib.lib().sg_debug_pipe_layout(n_q, cand_cap, out))
            rec, vrec, ovf, cand_n, fb_list, total, piece, vrec_words, ovf_cap, rec_stride, ovf_words, piece_max = (int(x) for x in out)
            ctx = (n_q, cand_cap)
            assert piece == min(n_q, piece_max) and ovf_cap == max(piece // 8, 64), ctx
            assert vrec_words >= 32 and vrec_words % 32 == 0, ctx          # whole 128-byte lines
            reg = {"counters": (0, 8, 4), "rec": (rec, piece * rec_stride * 4, 256), "vrec": (vrec, piece * vrec_words * 4, 16),
                   "ovf": (ovf, ovf_cap * ovf_words * 4, 16), "cand_n": (cand_n, piece * 4, 16), "fb_list": (fb_list, (n_q + 1) * 4, 16)}
            assert total % 16 == 0, ctx
            _assert_carved(reg, total)


# ---- the device block of a host-buffer call (csrc/host_call.inc: the regions a call declares) ----

IO_IN, IO_OUT, IO_BOTH = 1, 2, 3
IO_KINDS = {0: "search", 1: "strings", 2: "mixed", 3: "predict", 4: "dict_rows", 5: "edit_rows", 6: "edit_rerank", 7: "lm_text", 8: "lm_ids"}


def _io_layout(kind, n, k, flags, blob, rows):
    import ctypes as C
    from suggest_amd import _lib
    out = (C.c_uint64 * 45)()
    _lib.check(_lib.lib().sg_debug_io_layout(kind, n, k, flags, blob, rows, out))
    v = [int(x) for x in out]
    assert 1 <= v[0] <= 10
    return dict(out_hi=v[1], in_lo=v[2], in_hi=v[3], total=v[4], regions=[tuple(v[5 + 4 * i:9 + 4 * i]) for i in range(v[0])])


def _up(x, a):
    return (x + a - 1) // a * a


def _search_rule(n_q, slots, scores, aux, blob, text=False, sel=False):
    """The block of a search-shaped call as it has lain since the first host-buffer path: the rule, stated here."""
    at, reg = 0, {}

    def take(name, size, align):
        nonlocal at
        reg[name] = _up(at, align)
        at = reg[name] + size
    take("scores", slots * 8 if scores else 0, 16)
    take("ids", slots * 4, 4)
    take("counts", n_q * 4, 4)
    take("aux", slots * 4 if aux else 0, 4)
    if text:
        take("text_offs", (slots + 1) * 8 + 16, 8)            # (+ the step's two info words)
    out_end = at
    take("offs", (n_q + 1) * 8, 16)
    take("blob", blob, 8)
    if sel:
        take("sel", n_q * 4, 4)
    return reg, out_end, at, at + 16


def test_host_call_block_layout():
    """Every kind of host-buffer call over a small grid: the regions pairwise disjoint and aligned as declared; the one range
    copied back holds exactly the out and both-ways regions, the one range copied in exactly the in and both-ways regions; 16
    bytes follow the last region.  The search-shaped kinds lie where the rule above puts them."""
    for kind in IO_KINDS:
        for n in (1, 3, 1000):
            for k in (1, 7, 64, 100):
                for flags in range(8):
                    for blob in ((0, 20) if kind == 8 else (0, 5)):     # (word ids: 4 bytes each)
                        for rows in (n * k, n * k + 3, max(n * k - 1, 1)):
                            L = _io_layout(kind, n, k, flags, blob, rows)
                            ctx = (IO_KINDS[kind], n, k, flags, blob, rows)
                            R = L["regions"]
                            _assert_carved({i: (off, size, align) for i, (off, size, align, d) in enumerate(R)}, L["total"])
                            assert all(d in (IO_IN, IO_OUT, IO_BOTH) for _, _, _, d in R), ctx
                            last = max(off + size for off, size, _, _ in R)
                            assert L["total"] >= last + 16 and L["in_hi"] == last, ctx
                            for off, size, _, d in R:
                                if not size:
                                    continue
                                assert (off + size <= L["out_hi"]) == bool(d & IO_OUT), (ctx, off, size, d)
                                assert (L["in_lo"] <= off and off + size <= L["in_hi"]) == bool(d & IO_IN), (ctx, off, size, d)
                                if d == IO_OUT:
                                    assert off + size <= L["in_lo"], ctx
                                if d == IO_IN:
                                    assert off >= L["out_hi"], ctx
                            if kind > 3:
                                continue
                            # ---- today's kinds: equality with the rule ----
                            scores, aux = bool(flags & 1), bool(flags & 2)
                            if kind == 0:
                                want = _search_rule(n, n * k, scores, aux, blob)
                                names = ["scores", "ids", "counts", "aux", "offs", "blob"]
                            elif kind == 1:
                                want = _search_rule(n, n * k, scores, False, blob, text=True)
                                names = ["scores", "ids", "counts", "aux", "offs", "blob", "text_offs"]
                            elif kind == 2:
                                want = _search_rule(n, rows, True, False, blob, sel=True)
                                names = ["scores", "ids", "counts", "aux", "offs", "blob", "sel"]
                            else:
                                want = _search_rule(n, n * (k + 1), False, False, blob)
                                names = ["scores", "ids", "counts", "aux", "offs", "blob"]
                            reg, out_end, end, total = want
                            got = {name: R[i][0] for i, name in enumerate(names)}
                            assert got == {name: reg[name] for name in names}, (ctx, got, reg)
                            if kind == 1:                       # the info words: the 16 bytes behind the text offsets
                                assert R[7][:2] == (reg["text_offs"] + (n * k + 1) * 8, 16), ctx
                            assert (L["out_hi"], L["in_lo"], L["in_hi"], L["total"]) == (out_end, reg["offs"], end, total), ctx


# ---- the knob table (csrc/knobs.inc) ----

INT32_MAX = 2**31 - 1
# name: (lowest, highest, default, routes).  Pinned here so that a changed range or default is a decision, not an accident.
KNOB_TABLE = {
    "SG_LOG2_CNT": (9, 14, 11, "ET"), "SG_T_FLOOR": (2, 64, 8, "ET"), "SG_FILTER_LEVEL": (0, 7, 4, "ET"), "SG_TIGHTEN": (0, 2, 2, "ET"),
    "SG_ROOMY": (0, 2, 2, "ET"), "SG_ORDER": (0, INT32_MAX, 1, "ET"), "SG_PRETOK": (0, INT32_MAX, 2048, "ET"),
    "SG_SPLIT_CHUNKS": (0, INT32_MAX, 65536, "ET"), "SG_PARTS_CNT_BONUS": (0, 3, 2, "ET"), "SG_G8": (0, 2, 0, "E"), "SG_PIPE": (0, 2, 2, "ET"),
    "SG_PIPE_NW": (2, 8, 8, "ET"), "SG_PIPE_LOG2_CNT": (9, 13, 13, "ET"), "SG_PIPE_DT_BYTES": (1024, 32768, 8192, "ET"),
    "SG_PIPE_SHAPE_AUTO": (1, 1, 1, "T"), "SG_PIPE_SHAPE_BIAS": (-2, 0, 0, "T"), "SG_PIPE_SUB": (3, 5, 4, "ET"),
    "SG_PIPE_CAND_CAP": (1, 4096, 64, "ET"), "SG_PIPE_WIDE": (0, 1, 0, "ET"), "SG_PLAN2": (0, 1, 1, "ET"),
}
SHAPE_KNOBS = ("SG_PIPE_NW", "SG_PIPE_LOG2_CNT", "SG_PIPE_DT_BYTES")
TUNER_KNOBS = ("SG_LOG2_CNT", "SG_FILTER_LEVEL") + SHAPE_KNOBS
PROCESS_SWITCHES = {"SG_HOST_THREADS", "SG_COALESCE_LANES", "SG_COALESCE_SPIN_US", "SG_COALESCE_TREE", "SG_BUILD_THREADS",
                    "SG_BUILD_SHARED_COUNTERS", "SG_NO_LONG_QUERIES", "SG_VERBOSE", "SG_DEBUG_SKIP"}


def _knobs(ix=None):
    from suggest_amd.index import knobs
    return {r["name"]: r for r in knobs(ix)}


def _tune_index(ix):
    """sg_debug_tune_index: what the first upload does to the knobs, without a GPU -> (rc, out[6], message)"""
    import ctypes as C
    from suggest_amd import _lib
    st, out = (C.c_double * 2)(), (C.c_int32 * 6)()
    with ix._use() as h:
        rc = _lib.lib().sg_debug_tune_index(h, st, out)
    return rc, list(out), _lib.lib().sg_last_error().decode()


def _tune(ix, name, value):
    from suggest_amd import _lib
    with ix._use() as h:
        rc = _lib.lib().sg_index_tune(h, name.encode(), int(value))
    return rc, _lib.lib().sg_last_error().decode()


@pytest.fixture
def no_knobs_in_env(monkeypatch):
    for name in KNOB_TABLE:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_knob_table_is_the_pinned_one():
    rows = _knobs()
    assert {n: (r["lo"], r["hi"], r["default"], "E" * r["env"] + "T" * r["tune"]) for n, r in rows.items()} == KNOB_TABLE
    assert tuple(n for n, r in rows.items() if r["pins_shape"]) == SHAPE_KNOBS
    assert {n for n, r in rows.items() if r["tuner"]} == set(TUNER_KNOBS)
    assert [n for n, r in rows.items() if r["pow2"]] == ["SG_PIPE_NW"]
    assert all(r["value"] == r["default"] and not r["explicit"] for r in rows.values())


def test_environment_and_tune_accept_and_reject_alike(cars_lines, no_knobs_in_env):
    """Every row at and just outside the ends of its range (SG_PIPE_NW: also between its powers of two; the environment: also text
    that is no integer): both routes take a value or refuse it with SG_E_INVALID alike, a value taken is the index's afterwards, a
    refused one leaves the index untuned, and a row that one route does not serve is refused there in so many words."""
    from suggest_amd import NGramIndex
    monkeypatch, desc, docs = no_knobs_in_env, _desc(CARS_DESC), cars_lines[:100]
    for name, row in _knobs().items():
        values = [v for v in (row["lo"] - 1, row["lo"], row["hi"], row["hi"] + 1) if -2**31 <= v <= INT32_MAX]
        values += [3, 6] if row["pow2"] else []
        for v in values + ["abc", "4x"]:
            legal = isinstance(v, int) and row["lo"] <= v <= row["hi"] and not (row["pow2"] and v & (v - 1))
            ix = NGramIndex(docs, desc, upload=False)
            monkeypatch.setenv(name, str(v))
            rc, _, msg = _tune_index(ix)
            assert (rc == 0) == (legal and row["env"]), (name, v, rc, msg)
            if rc == 0:
                got = _knobs(ix)[name]
                assert got["value"] == v and got["explicit"], (name, v, got)
            else:
                assert rc == -1 and name in msg, (name, v, rc, msg)
                assert ("not from the environment" in msg) == (not row["env"]), (name, v, msg)
                assert str(v) in msg or not row["env"], (name, v, msg)
                assert _tune_index(ix)[0] == -1, (name, v, "a refused value must leave the index untuned")
                monkeypatch.delenv(name)
                assert _tune_index(ix)[0] == 0 and not _knobs(ix)[name]["explicit"], (name, v, "nothing of the refused attempt may stay")
            monkeypatch.delenv(name, raising=False)
            ix.close()
            if not isinstance(v, int):
                continue
            ix = NGramIndex(docs, desc, upload=False)
            rc, msg = _tune(ix, name, v)
            assert (rc == 0) == (legal and row["tune"]), (name, v, rc, msg)
            if rc == 0:
                got = _knobs(ix)[name]
                assert got["value"] == v and got["explicit"], (name, v, got)
            else:
                assert rc == -1 and name in msg, (name, v, rc, msg)
                assert ("not set through sg_index_tune" in msg) == (not row["tune"]), (name, v, msg)
                assert not _knobs(ix)[name]["explicit"], (name, v)
            ix.close()
    ix = NGramIndex(docs, desc, upload=False)
    assert _tune(ix, "SG_NO_SUCH_KNOB", 1)[0] == -1
    monkeypatch.setenv("SG_T_FLOOR", "")            # an empty variable counts as not set
    assert _tune_index(ix)[0] == 0 and not _knobs(ix)["SG_T_FLOOR"]["explicit"]


def test_explicit_knobs_beat_the_tuner(cars_lines, no_knobs_in_env):
    """cars: the tuner chooses filter level 2, 2^11 counters and the smallest stream workgroup (test_tuner_choices_are_pinned).  A knob
    set before the first upload — through sg_index_tune or the environment — is still there after it; the others are the tuner's."""
    from suggest_amd import NGramIndex
    monkeypatch, desc = no_knobs_in_env, _desc(CARS_DESC)
    rc, out, _ = _tune_index(NGramIndex(cars_lines, desc, upload=False))
    assert rc == 0 and out == [11, 2, 0, 2, 11, 2048]
    ix = NGramIndex(cars_lines, desc, upload=False).tune(SG_FILTER_LEVEL=4, SG_LOG2_CNT=12)
    rc, out, _ = _tune_index(ix)
    assert rc == 0 and out == [12, 4, 0, 2, 11, 2048], out
    rows = _knobs(ix)
    assert rows["SG_FILTER_LEVEL"]["explicit"] and rows["SG_LOG2_CNT"]["explicit"] and not rows["SG_PIPE_NW"]["explicit"]
    assert rows["SG_PIPE_SHAPE_AUTO"]["value"] == 1            # (the tuner's stream workgroup pins nothing)
    ix = NGramIndex(cars_lines, desc, upload=False).tune(SG_PIPE_NW=8)
    rc, out, _ = _tune_index(ix)
    assert rc == 0 and out == [11, 2, 0, 8, 11, 2048], out
    monkeypatch.setenv("SG_FILTER_LEVEL", "4")
    monkeypatch.setenv("SG_LOG2_CNT", "12")
    rc, out, _ = _tune_index(NGramIndex(cars_lines, desc, upload=False))
    assert rc == 0 and out == [12, 4, 0, 2, 11, 2048], out


def test_shape_knobs_pin_the_stream_workgroup_and_auto_hands_it_back(cars_lines, no_knobs_in_env):
    from suggest_amd import NGramIndex
    monkeypatch, desc, docs = no_knobs_in_env, _desc(CARS_DESC), cars_lines[:100]
    for name, value in zip(SHAPE_KNOBS, (4, 12, 4096)):
        ix = NGramIndex(docs, desc, upload=False)
        assert _knobs(ix)["SG_PIPE_SHAPE_AUTO"]["value"] == 1
        ix.tune(**{name: value})
        assert _knobs(ix)["SG_PIPE_SHAPE_AUTO"]["value"] == 0, name
        assert _tune_index(ix)[0] == 0 and _knobs(ix)["SG_PIPE_SHAPE_AUTO"]["value"] == 0, name     # (the first upload keeps it)
        ix.tune(SG_PIPE_SHAPE_AUTO=1)
        assert _knobs(ix)["SG_PIPE_SHAPE_AUTO"]["value"] == 1 and _knobs(ix)[name]["value"] == value, name
        ix = NGramIndex(docs, desc, upload=False)
        monkeypatch.setenv(name, str(value))
        assert _tune_index(ix)[0] == 0 and _knobs(ix)["SG_PIPE_SHAPE_AUTO"]["value"] == 0, name
        monkeypatch.delenv(name)
    ix = NGramIndex(docs, desc, upload=False).tune(SG_T_FLOOR=4, SG_PIPE_SUB=3, SG_PIPE=1)      # (any other knob pins nothing)
    assert _tune_index(ix)[0] == 0 and _knobs(ix)["SG_PIPE_SHAPE_AUTO"]["value"] == 1


def test_the_prose_names_what_the_table_names():
    """The sg_index_tune comment of the header and DESIGN.md §4c name every row of the table, and every SG_* name in them is a row or
    one of the process-wide switches."""
    header = open(os.path.join(ROOT, "include", "suggest_hip.h")).read()
    decl = header.index("int sg_index_tune(")
    comment = header[header.rindex("/*", 0, decl):decl]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4c."):design.index("### 4d.")]
    rows = set(_knobs())
    for where, text in (("suggest_hip.h", comment), ("DESIGN.md §4c", section)):
        named = set(re.findall(r"SG_[A-Z0-9_]+", text))
        assert rows <= named, (where, rows - named)
        assert named <= rows | PROCESS_SWITCHES, (where, named - rows - PROCESS_SWITCHES)
    for name, row in _knobs().items():         # the table's line of each row carries its range and default
        line = next(l for l in section.splitlines() if l.startswith("| `%s` |" % name))
        cells = [c.strip() for c in line.split("|")]
        lo, hi = ("2", "8") if row["pow2"] else (str(row["lo"]).replace("-", "−"), "2^31−1" if row["hi"] == INT32_MAX else str(row["hi"]))
        assert cells[2].startswith(lo) and cells[2].endswith(hi) and cells[3] == str(row["default"]), (name, cells)
        assert cells[4] == " ".join(("E",) * row["env"] + ("T",) * row["tune"]) and cells[5] == "P" * row["pins_shape"] and cells[6] == "A" * row["tuner"], (name, cells)


def test_the_fuzzer_draws_legal_knob_values():
    """tools/fuzz_parity.py sets its knobs through the environment: every SG_* name it can draw is a row that the environment serves,
    every value inside the row's range (an illegal one would now fail the trial's upload).  Other keys are the fuzzer's own."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    rows = _knobs()

    def check(name, value, ctx):
        if not name.startswith("SG_"):
            return
        row = rows.get(name)
        assert row is not None and row["env"], (ctx, name)
        v = int(value)
        assert str(v) == value and row["lo"] <= v <= row["hi"] and not (row["pow2"] and v & (v - 1)), (ctx, name, value)

    for name, choices in fz.KNOBS:
        for value in choices:
            check(name, value, "KNOBS")
    trials = 0
    for seed in list(range(1, 301)) + [300004, 700812, 610200998, 77700102924]:
        t = fz.make_trial(seed)
        if t is None:
            continue
        trials += 1
        for name, value in t["env"].items():
            check(name, value, seed)
    assert trials > 200
