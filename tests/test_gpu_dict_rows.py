"""Result rows as strings from a dictionary held in HBM (sg_dictionary; suggest_amd/csrc/dict_rows.inc).  Every text
the device gives is compared byte for byte with tests/dict_rows_ref.py, the numpy restatement of the step's rules, computed from the
same id rows; the searches' rows themselves are compared with the plain calls' bit for bit."""
import os
import subprocess
import threading

import numpy as np
import pytest

import dict_rows_ref as ref
from conftest import CARS_DESC, GOLDEN, ROOT

pytestmark = pytest.mark.gpu

GUARD = 64
CARS_CDB = os.path.join(GOLDEN, "db", "cars.cdb")


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(**d)


@pytest.fixture(scope="module")
def torch():
    import torch  # (before the library: both must resolve the same libamdhip64, suggest_amd/_lib.py)
    return torch


@pytest.fixture(scope="module")
def step(torch):
    from suggest_amd.dictionary import DeviceDictionary
    lines = ref.step_lines()
    blob, offs = ref.pack(lines)
    return dict(lines=lines, blob=blob, offs=offs, dd=DeviceDictionary(lines, device=0))


@pytest.fixture(scope="module")
def cars(torch, cars_lines):
    from suggest_amd import NGramIndex
    from suggest_amd.dictionary import DeviceDictionary
    lines = [l.encode("utf-8") if isinstance(l, str) else bytes(l) for l in cars_lines]
    blob, offs = ref.pack(lines)
    ix = NGramIndex(cars_lines, _desc(CARS_DESC))
    yield dict(lines=lines, blob=blob, offs=offs, ix=ix, dd=DeviceDictionary(lines, device=0), cdb=DeviceDictionary.from_cdb(CARS_CDB, 0))
    ix.close()


def _to_dev(torch, a, dtype):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(a.view(view).copy()).to("cuda:0")


def _device_step(torch, dd, ids, counts, row=0, row_offs=None, slots=None, text_cap=0, fill=0xEE):
    """sg_dictionary_rows_device on tensors -> (text[text_cap] u8, the GUARD bytes behind it, text_offs u64, info [2])"""
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    slots = ids.size if slots is None else slots
    d_ids, d_cnt = _to_dev(torch, ids, None), _to_dev(torch, counts, None)
    d_ro = None if row_offs is None else _to_dev(torch, np.asarray(row_offs, dtype=np.uint64), None)
    d_text = torch.full((text_cap + GUARD,), fill, dtype=torch.uint8, device="cuda:0")
    d_toffs = torch.full((slots + 1,), -1, dtype=torch.int64, device="cuda:0")
    d_info = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    dd.rows_device(d_ids.data_ptr(), d_cnt.data_ptr(), None if d_ro is None else d_ro.data_ptr(), len(counts), row, slots,
                   d_text.data_ptr(), text_cap, d_toffs.data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    text = d_text.cpu().numpy()
    return text[:text_cap], text[text_cap:], d_toffs.cpu().numpy().view(np.uint64), d_info.cpu().numpy().view(np.uint64)


# ---- 1: the step on synthetic rows ----
@pytest.mark.parametrize("name,n_rows,row,v", ref.step_cases(), ids=[c[0] for c in ref.step_cases()])
def test_step_on_synthetic_rows(torch, step, name, n_rows, row, v):
    from suggest_amd import _lib
    ids, counts = ref.step_rows(n_rows, row, v, len(step["lines"]))
    want = ref.materialise(ids, counts, step["blob"], step["offs"], row=row)
    with _lib.poisoned(1):
        text, guard, toffs, info = _device_step(torch, step["dd"], ids, counts, row=row, text_cap=want[2])
        host_text, host_toffs = step["dd"].rows(ids, counts)              # the host-buffer route over the same handle
    assert info.tolist() == [want[2], 0]
    ref.check(text, toffs, want)
    assert np.all(guard == 0xEE)
    ref.check(host_text, host_toffs, want)


# ---- 2: text_cap = needed, needed - 1, 0 ----
@pytest.mark.parametrize("n_rows,row,v", [(257, 5, 0), (1, 65536, 3)])
def test_text_cap(torch, step, n_rows, row, v):
    from suggest_amd import _lib
    ids, counts = ref.step_rows(n_rows, row, v, len(step["lines"]))
    want = ref.materialise(ids, counts, step["blob"], step["offs"], row=row)
    needed = want[2]
    assert needed > 0
    for cap in (needed, needed - 1, 0):
        with _lib.poisoned(1):
            text, guard, toffs, info = _device_step(torch, step["dd"], ids, counts, row=row, text_cap=cap)
        assert info.tolist() == [needed, 0], cap                          # reported, never overrun
        assert np.array_equal(toffs, want[1]), cap                        # complete whatever the cap
        assert np.all(guard == 0xEE), cap
        # a string that would end past the cap is not written at all; every other one is there
        expect = np.full(cap, 0xEE, dtype=np.uint8)
        ends = want[1][1:]
        last = int(np.searchsorted(ends, cap, side="right"))              # slots [0, last) end at or before the cap
        n = int(want[1][last])
        expect[:n] = want[0][:n]
        assert np.array_equal(text, expect), cap
        if cap < needed:
            with pytest.raises(_lib.SuggestHipError) as e:
                step["dd"].rows(ids, counts, text_cap=cap)
            assert e.value.code == -1 and "text buffer too small" in str(e.value)
    host_text, host_toffs = step["dd"].rows(ids, counts, text_cap=needed)
    ref.check(host_text, host_toffs, want)


# ---- 2b: the host-buffer route's result regions under the poison ----
def test_host_rows_under_the_poison(torch, step):
    """sg_dictionary_rows on a device handle is a host-buffer call like every other: its text offsets are a result region of the
    shared path, poisoned (and counted) while sg_debug_poison is on.  Fixed rows (3 x 4, counts 0 / 2 / 4) and ragged rows: text
    and offsets equal the restatement's and the unpoisoned call's under both pattern families."""
    from suggest_amd import _lib
    n_docs = len(step["lines"])
    rng = np.random.default_rng(7)
    fixed_ids = rng.integers(0, n_docs, size=(3, 4), dtype=np.uint32)
    fixed_cnt = np.array([0, 2, 4], dtype=np.uint32)
    ragged_offs = np.array([0, 0, 3, 4, 9], dtype=np.uint64)                 # rows of 0, 3, 1 and 5 slots, 2 slots of no row behind them
    ragged_ids = rng.integers(0, n_docs, size=11, dtype=np.uint32)
    ragged_cnt = np.array([0, 2, 1, 5], dtype=np.uint32)
    cases = [(fixed_ids, fixed_cnt, None, ref.materialise(fixed_ids, fixed_cnt, step["blob"], step["offs"], row=4)),
             (ragged_ids, ragged_cnt, ragged_offs, ref.materialise(ragged_ids, ragged_cnt, step["blob"], step["offs"], row_offs=ragged_offs))]
    for ids, counts, row_offs, want in cases:
        assert want[2] > 0 and want[3] == 0
        plain = step["dd"].rows(ids, counts, row_offs=row_offs)
        ref.check(plain[0], plain[1], want)
        for family in (1, 2):
            _lib.poison_stats()
            with _lib.poisoned(family):
                text, toffs = step["dd"].rows(ids, counts, row_offs=row_offs)
                st = _lib.poison_stats()
            ref.check(text, toffs, want)
            assert np.array_equal(toffs, plain[1]) and np.array_equal(text[:want[2]], plain[0][:want[2]])
            out_bytes = st["out_ids"] + st["out_scores"] + st["out_counts"]
            print("family %d, %s rows: %s" % (family, "fixed" if row_offs is None else "ragged", st))
            assert out_bytes >= (ids.size + 1) * 8, st                       # the text offsets at least


# ---- 3: ragged geometry from a real mixed call ----
MIXED = [dict(metric="jaccard", similarity=0.5, k=10), dict(metric="cosine", similarity=0.4, k=1), dict(metric="dice", similarity=0.3, k=300),
         dict(metric="overlap", similarity=0.6, k=65), dict(autocomplete=1, k=7)]


def test_ragged_rows_of_a_mixed_device_call(torch, cars):
    from suggest_amd import _lib
    from suggest_amd.index import pack_strings
    rng = np.random.RandomState(3)
    queries = [cars["lines"][int(i)][:int(rng.randint(3, 40))].decode("utf-8", "ignore").encode("utf-8") for i in rng.randint(0, len(cars["lines"]), 200)]
    config_of = rng.randint(0, len(MIXED), len(queries)).astype(np.uint32)
    qb, qo = pack_strings(queries)
    rows = int(sum(MIXED[int(g)]["k"] for g in config_of))
    cap = rows + 37                                                        # slots = rows_cap > the sum of the k: spare slots
    d_blob, d_offs, d_cfg = _to_dev(torch, qb, None), _to_dev(torch, qo, None), _to_dev(torch, config_of, None)
    with _lib.poisoned(1):
        d_ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda:0")
        d_sc = torch.zeros((cap,), dtype=torch.float64, device="cuda:0")
        d_cnt = torch.full((len(queries),), -1, dtype=torch.int32, device="cuda:0")
        d_ro = torch.full((len(queries) + 1,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        cars["ix"].suggest_batch_mixed_device(d_blob.data_ptr(), d_offs.data_ptr(), len(queries), MIXED, d_cfg.data_ptr(), cap, d_ids.data_ptr(),
                                              d_sc.data_ptr(), d_cnt.data_ptr(), d_ro.data_ptr())
        ids = d_ids.cpu().numpy().view(np.uint32)
        counts = d_cnt.cpu().numpy().view(np.uint32)
        ro = d_ro.cpu().numpy().view(np.uint64)
        assert int(ro[-1]) == rows and int(counts[counts < ref.COUNT_FLAG_MIN].sum()) > 500
        want = ref.materialise(ids, counts, cars["blob"], cars["offs"], row_offs=ro, slots=cap)
        d_text = torch.full((want[2] + GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_toffs = torch.full((cap + 1,), -1, dtype=torch.int64, device="cuda:0")
        d_info = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        cars["dd"].rows_device(d_ids.data_ptr(), d_cnt.data_ptr(), d_ro.data_ptr(), len(queries), 0, cap, d_text.data_ptr(), want[2],
                               d_toffs.data_ptr(), d_info.data_ptr())
        torch.cuda.synchronize()
    text = d_text.cpu().numpy()
    toffs = d_toffs.cpu().numpy().view(np.uint64)
    assert d_info.cpu().numpy().tolist() == [want[2], 0]
    ref.check(text[:want[2]], toffs, want)
    assert np.all(text[want[2]:] == 0xEE)
    assert np.all(toffs[rows:] == want[2])                                 # the spare slots have length 0
    host_text, host_toffs = cars["dd"].rows(ids[:rows], counts, ro)        # ... and the host-buffer route with the same geometry
    ref.check(host_text, host_toffs, ref.materialise(ids[:rows], counts, cars["blob"], cars["offs"], row_offs=ro))


# ---- 4: an id outside the dictionary ----
def test_an_id_outside_the_dictionary(torch, cars):
    from suggest_amd import _lib
    from suggest_amd.dictionary import DeviceDictionary
    n = len(cars["lines"])
    short = DeviceDictionary(cars["lines"][:-1], device=0)                 # one line shorter than the index
    short_blob, short_offs = ref.pack(cars["lines"][:-1])
    queries = [cars["lines"][n - 1], cars["lines"][n - 2], cars["lines"][0], cars["lines"][n - 1]]
    ids, sc, cnt = cars["ix"].suggest_batch(queries, "jaccard", 0.9, 4)
    assert int((ids[(np.arange(4)[None, :] < cnt[:, None])] == n - 1).sum()) >= 2
    want = ref.materialise(ids, cnt, short_blob, short_offs, row=4)
    assert want[3] >= 2
    text, guard, toffs, info = _device_step(torch, short, ids, cnt, row=4, text_cap=want[2])
    assert info.tolist() == [want[2], want[3]]
    ref.check(text, toffs, want)
    with pytest.raises(_lib.SuggestHipError) as e:
        short.rows(ids, cnt)
    assert e.value.code == -1 and "docID outside the dictionary" in str(e.value)
    with pytest.raises(_lib.SuggestHipError) as e:
        cars["ix"].suggest_batch_strings(short, queries, "jaccard", 0.9, 4)
    assert e.value.code == -1 and "docID outside the dictionary" in str(e.value)
    host_text, host_toffs = short.rows(ids[2:3], cnt[2:3])                 # the next call is right
    ref.check(host_text, host_toffs, ref.materialise(ids[2:3], cnt[2:3], short_blob, short_offs, row=4))
    short.close()


# ---- 5: 64-bit offsets ----
def test_text_past_4_gib(torch):
    from suggest_amd.dictionary import DeviceDictionary
    big = np.random.default_rng(9).integers(0, 256, size=65536, dtype=np.uint8)
    dd = DeviceDictionary([b"ab", big.tobytes()], device=0)
    slots = 70000
    total = slots * 65536                                                   # 4.6 GB
    d_ids = torch.ones((slots,), dtype=torch.int32, device="cuda:0")
    d_cnt = torch.ones((slots,), dtype=torch.int32, device="cuda:0")
    d_text = torch.empty((total + GUARD,), dtype=torch.uint8, device="cuda:0")
    d_text[total:] = 0xEE
    d_toffs = torch.full((slots + 1,), -1, dtype=torch.int64, device="cuda:0")
    d_info = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    dd.rows_device(d_ids.data_ptr(), d_cnt.data_ptr(), None, slots, 1, slots, d_text.data_ptr(), total, d_toffs.data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    assert d_info.cpu().numpy().tolist() == [total, 0]
    toffs = d_toffs.cpu().numpy()
    assert int(toffs[slots]) == total and np.array_equal(toffs, np.arange(slots + 1, dtype=np.int64) * 65536)
    want = torch.from_numpy(big).to("cuda:0")
    for s in np.unique(np.concatenate([[0, 65535, 65536, 65537, slots - 1], np.random.default_rng(1).integers(0, slots, 251)])).tolist():
        assert torch.equal(d_text[s * 65536:(s + 1) * 65536], want), s
    assert bool((d_text[total:] == 0xEE).all())
    del d_text
    dd.close()


# ---- 6: end to end on cars ----
def _lines_of(rows_text, lines):
    from suggest_amd.dictionary import split_text
    return split_text(*rows_text)


@pytest.mark.parametrize("which", ["dd", "cdb"])
def test_fused_calls_on_cars(torch, cars, reference_tests, which):
    from suggest_amd import _lib
    from suggest_amd.dictionary import split_text
    dd, ix, lines = cars[which], cars["ix"], cars["lines"]
    for metric, sim, k in (("cosine", 0.7, 5), ("jaccard", 0.5, 64)):
        plain = ix.suggest_batch(lines, metric, sim, k)
        with _lib.poisoned(1):
            ids, sc, cnt, text, toffs = ix.suggest_batch_strings(dd, lines, metric, sim, k)
            plain_p = ix.suggest_batch(lines, metric, sim, k)
        assert np.array_equal(cnt, plain[2]) and np.array_equal(ids, plain_p[0]) and np.array_equal(sc.view(np.uint64), plain_p[1].view(np.uint64))
        valid = np.arange(k)[None, :] < np.minimum(cnt, k)[:, None]
        assert np.array_equal(ids[valid], plain[0][valid]) and np.array_equal(sc.view(np.uint64)[valid], plain[1].view(np.uint64)[valid])
        ref.check(text, toffs, ref.materialise(ids, cnt, cars["blob"], cars["offs"], row=k))
        assert int(cnt.sum()) >= len(lines)
    plain = ix.autocomplete_batch(lines, 10)
    ids, cnt, text, toffs = ix.autocomplete_batch_strings(dd, lines, 10)
    assert np.array_equal(ids, plain[0]) and np.array_equal(cnt, plain[1])
    ref.check(text, toffs, ref.materialise(ids, cnt, cars["blob"], cars["offs"], row=10))
    t = reference_tests["service_cars"]                                    # service_test.go:35,53-59
    assert len(t["queries"]) == 5
    ids, sc, cnt, text, toffs = ix.suggest_batch_strings(dd, t["queries"], t["metric"], t["similarity"], t["topK"])
    got = split_text(text, toffs)
    for i, exp in enumerate(t["expected_values"]):
        assert [b.decode("utf-8") for b in got[i * t["topK"]:i * t["topK"] + int(cnt[i])]] == exp, t["queries"][i]
    # a text buffer that is too small: refused, with the size — and the rows are delivered all the same
    L = _lib.lib()
    from suggest_amd.index import pack_strings
    import ctypes as C
    qb, qo = pack_strings(t["queries"])
    k = t["topK"]
    ids2, sc2, cnt2 = np.zeros((5, k), dtype=np.uint32), np.zeros((5, k), dtype=np.float64), np.zeros(5, dtype=np.uint32)
    toffs2, small, needed = np.zeros(5 * k + 1, dtype=np.uint64), np.full(8 + GUARD, 0xEE, dtype=np.uint8), C.c_uint64()
    with ix._use() as h, dd._use() as dh:
        rc = L.sg_suggest_batch_strings(h, qb.ctypes.data, qo.ctypes.data, 5, 1, float(t["similarity"]), k, ids2.ctypes.data, sc2.ctypes.data, cnt2.ctypes.data,
                                        dh, small.ctypes.data, 8, toffs2.ctypes.data, C.byref(needed))
    assert rc == -1 and L.sg_last_error() == b"text buffer too small" and needed.value == int(toffs[-1])
    assert np.array_equal(ids2, ids) and np.array_equal(cnt2, cnt) and np.array_equal(sc2.view(np.uint64), sc.view(np.uint64)) and np.array_equal(toffs2, toffs)
    assert np.all(small == 0xEE)


def test_the_dictionary_must_be_on_the_index_device(torch, cars):
    from suggest_amd import _lib
    from suggest_amd.dictionary import DeviceDictionary
    host = DeviceDictionary(cars["lines"], device=-1)
    with pytest.raises(_lib.SuggestHipError) as e:
        cars["ix"].suggest_batch_strings(host, ["nissan"], "cosine", 0.5, 3)
    assert e.value.code == -2
    with pytest.raises(_lib.SuggestHipError) as e:
        DeviceDictionary([b"a"], device=4096)
    assert e.value.code == -1


# ---- 7: behind the other calls, through the generic step ----
def _host_lookup(ids, counts, lines, slots_per_row):
    out = []
    for i in range(len(counts)):
        c = int(counts[i])
        n = 0 if c >= ref.COUNT_FLAG_MIN else min(c, slots_per_row)
        out += [lines[int(d)] for d in ids[i, :n]] + [b""] * (slots_per_row - n)
    return out


def test_sharded_rows(torch, cars):
    from suggest_amd.dictionary import split_text
    from suggest_amd.sharded import ShardedIndex
    sh = ShardedIndex(cars["lines"], description=_desc(CARS_DESC), n_shards=3)
    queries = cars["lines"][::97] + [b"nisan", b"toyta corola"]
    ids, sc, cnt = sh.suggest_batch(queries, "jaccard", 0.4, 12)          # dictionary-wide ids
    assert int(ids.max()) > 2 * len(cars["lines"]) // 3
    assert split_text(*cars["dd"].rows(ids, cnt)) == _host_lookup(ids, cnt, cars["lines"], 12)
    sh.close()


def test_predict_rows(torch, tmp_path):
    import predict_shapes as ps
    from suggest_amd import LanguageModel, SpellChecker
    from suggest_amd.dictionary import DeviceDictionary, split_text
    m = ps.build(str(tmp_path), big_group=130, big_family=100)
    model = LanguageModel(m["directory"], ps.ORDER, alphabet=ps.ALPHA)
    sc = SpellChecker(model)
    words = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in model.words()]
    dd = DeviceDictionary(words, device=0)
    queries = ps.queries(m)[:400]
    ids, cnt = sc.predict_batch(queries, 7, 0.3)                          # rows of topK + 1, counts that may overshoot
    assert ids.shape[1] == 8 and int((cnt[cnt < ref.COUNT_FLAG_MIN] > 0).sum()) > 10
    assert split_text(*dd.rows(ids, cnt)) == _host_lookup(ids, cnt, words, 8)
    dd.close()


def test_tabulated_metric_rows(torch, cars):
    from suggest_amd.dictionary import split_text
    from suggest_amd.metric import Metric

    class Halfway(Metric):                                                  # a metric the device has no twin of
        def MinY(self, alpha, size): return max(1, size - 2)
        def MaxY(self, alpha, size): return size + 2
        def Threshold(self, alpha, a, b): return max(1, (a + b) // 3)
        def Distance(self, inter, a, b): return 1 - float(inter) / float(max(a, b))

    queries = cars["lines"][::211]
    ids, sc, cnt = cars["ix"].suggest_batch(queries, Halfway(), 0.5, 9)
    assert int(cnt[cnt < ref.COUNT_FLAG_MIN].sum()) > len(queries)
    assert split_text(*cars["dd"].rows(ids, cnt)) == _host_lookup(ids, cnt, cars["lines"], 9)


# ---- 8: the Service ----
def test_service_with_a_device_dictionary(torch, cars_lines, tmp_path):
    from suggest_amd import SearchConfig, Service
    from suggest_amd.index import IndexDescription
    plain, dev = Service(), Service(device_dictionary=True)
    for s in (plain, dev):
        s.AddIndex("cars", cars_lines, _desc(CARS_DESC))
    queries = list(cars_lines[::53]) + ["nisan", "", "toyta corola", "zzzzqqqq"]
    a, b = plain.suggest_batch("cars", queries, 7, "cosine", 0.4), dev.suggest_batch("cars", queries, 7, "cosine", 0.4)
    assert a == b and sum(len(r) for r in a if r) > len(queries)
    keys = [("jaccard", 0.5, 5), ("cosine", 0.4, 10), ("dice", 0.3, 65), ("exact", 1.0, 1)]
    configs = [SearchConfig(q, keys[i % 4][2], keys[i % 4][0], keys[i % 4][1]) for i, q in enumerate(queries)]
    assert plain.suggest_many("cars", configs) == dev.suggest_many("cars", configs)
    assert plain.Autocomplete("cars", "niss", 10) == dev.Autocomplete("cars", "niss", 10)
    # the DISC driver opens the .cdb through the library
    d = IndexDescription(name="cars", driver="DISC", output=os.path.join(GOLDEN, "db"), **CARS_DESC)
    disc = Service(device_dictionary=True)
    disc.AddIndexByDescription(d)
    assert disc.suggest_batch("cars", queries, 7, "cosine", 0.4) == a
    # three threads, one dictionary handle
    out, errors = [None] * 3, []

    def worker(i):
        try:
            for _ in range(3):
                out[i] = (dev.suggest_batch("cars", queries, 7, "cosine", 0.4), dev.suggest_many("cars", configs))
        except Exception as e:            # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=worker, args=(i,)) for i in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    want = (a, plain.suggest_many("cars", configs))
    assert all(o == want for o in out)


# ---- 9: the C++ mirror ----
def test_cpp_mirror_device_dictionary():
    binary = os.path.join(ROOT, "tests", "cpp", "_build", "dict_rows_test")
    if not os.path.exists(binary):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "dict_rows.mk"], check=True, capture_output=True)
    r = subprocess.run([binary, GOLDEN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
