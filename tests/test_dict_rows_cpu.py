"""CPU-only checks of result rows as strings (sg_dictionary, include/suggest_hip.h): the numpy restatement and its
checker, the host-resident handle — upload, the .cdb route, the plain host loop on the step's shapes — every refusal that needs no
GPU, and the bindings above them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dict_rows_ref as ref
from conftest import CARS_DESC, GOLDEN, ROOT

NEW = ("sg_dictionary_upload", "sg_dictionary_open_cdb", "sg_dictionary_retain", "sg_dictionary_release", "sg_dictionary_size", "sg_dictionary_bytes",
       "sg_dictionary_max_len", "sg_dictionary_device", "sg_dictionary_rows_device", "sg_dictionary_rows", "sg_suggest_batch_strings",
       "sg_autocomplete_batch_strings")
CARS_CDB = os.path.join(GOLDEN, "db", "cars.cdb")


@pytest.fixture(scope="module")
def lines():
    return ref.step_lines()


@pytest.fixture(scope="module")
def host_dict(lines):
    from suggest_amd.dictionary import DeviceDictionary
    return DeviceDictionary(lines, device=-1)


def _rows(d, ids, counts, row=0, row_offs=None, slots=None, text_cap=None, null=None):
    """sg_dictionary_rows itself -> (rc, message, text, text_offs, needed)"""
    from suggest_amd import _lib
    L = _lib.lib()
    ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    slots = ids.size if slots is None else slots
    ro = None if row_offs is None else np.ascontiguousarray(row_offs, dtype=np.uint64)
    cap = slots * d.max_len if text_cap is None else text_cap
    text = np.full(cap + 64, 0xEE, dtype=np.uint8)
    toffs = np.full(slots + 1, 0xEEEEEEEE, dtype=np.uint64)
    needed = C.c_uint64(0xEEEE)
    a = dict(ids=ids.ctypes.data, counts=counts.ctypes.data, text=text.ctypes.data, text_offs=toffs.ctypes.data, needed=C.byref(needed))
    if null:
        a[null] = None
    with d._use() as h:
        rc = L.sg_dictionary_rows(h, a["ids"], a["counts"], None if ro is None else ro.ctypes.data, len(counts), row, slots, a["text"], cap,
                                  a["text_offs"], a["needed"])
    assert np.all(text[cap:] == 0xEE), "bytes behind the text buffer were written"
    return rc, L.sg_last_error().decode(), text[:cap], toffs, int(needed.value)


def test_the_step_dictionary_is_as_the_issue_describes_it(lines):
    lens = [len(b) for b in lines]
    assert len(lines) == 203 and lens[197:] == [63, 64, 65, 255, 4096, 70001]
    assert set(lens[:197]) == set(range(41)) and lens[:41] != sorted(lens[:41])


def test_the_step_shapes_meet_every_residue_pair_and_every_count(lines):
    blob, offs = ref.pack(lines)
    seen, counts_seen, past_seen = set(), {}, set()
    for name, n_rows, row, v in ref.step_cases():
        ids, counts = ref.step_rows(n_rows, row, v, len(lines))
        for i in range(n_rows):
            counts_seen.setdefault((n_rows, row), set()).add(int(counts[i]))
            c = int(counts[i])
            n = 0 if c >= ref.COUNT_FLAG_MIN else min(c, row)
            past_seen |= set(int(x) for x in ids[i, n:][:3])
        text, toffs, needed, outside = ref.materialise(ids, counts, blob, offs, row=row)
        assert outside == 0
        flat = ids.reshape(-1)
        length = (toffs[1:] - toffs[:-1]).astype(np.int64)
        s = np.nonzero(length >= 1)[0]
        seen |= set(zip((offs[flat[s]] % 16).tolist(), (toffs[s] % 16).tolist()))
    assert len(seen) == 256, "the shapes miss %d of the 256 (source, destination) residues mod 16" % (256 - len(seen))
    for n_rows, row in ref.STEP_SHAPES:          # every shape's rows take all eight count values (equal values of a 1-slot row fold)
        assert counts_seen[(n_rows, row)] == set(ref.count_values(row)), (n_rows, row)
    assert past_seen >= {ref.POISON_ID, len(lines), 0xFFFFFFFF}


def test_the_checker_fails_on_a_wrong_result(lines):
    blob, offs = ref.pack(lines)
    ids, counts = ref.step_rows(257, 5, 0, len(lines))
    good = ref.materialise(ids, counts, blob, offs, row=5)
    ref.check(good[0].copy(), good[1].copy(), good)
    text = good[0].copy()
    text[len(text) // 2] ^= 1
    with pytest.raises(AssertionError):           # a corrupted blob
        ref.check(text, good[1], good)
    toffs = good[1].copy()
    toffs[100:] += 1
    with pytest.raises(AssertionError):           # a shifted offset
        ref.check(good[0], toffs, good)
    flagged = int(np.nonzero(counts >= ref.COUNT_FLAG_MIN)[0][0])
    toffs = good[1].copy()
    toffs[flagged * 5 + 1:] += 3                  # a string written into a flagged row
    text = np.insert(good[0], int(good[1][flagged * 5]), [65, 66, 67])
    with pytest.raises(AssertionError):
        ref.check(text, toffs, good)
    with pytest.raises(AssertionError):           # a text cut short
        ref.check(good[0][:-1], good[1], good)


def test_the_restatement_by_hand():
    blob, offs = ref.pack([b"alpha", b"", b"be", b"gamma!"])
    ids = np.array([[0, 3, 9], [2, 1, 0]], dtype=np.uint32)
    text, toffs, needed, outside = ref.materialise(ids, [2, 4], blob, offs, row=3)
    assert (text.tobytes(), toffs.tolist(), needed, outside) == (b"alphagamma!bealpha", [0, 5, 11, 11, 13, 13, 18], 18, 0)
    text, toffs, needed, outside = ref.materialise(ids, [3, 0xFFFFFFFD], blob, offs, row=3)
    assert (text.tobytes(), toffs.tolist(), needed, outside) == (b"alphagamma!", [0, 5, 11, 11, 11, 11, 11], 11, 1)
    # ragged: a row of 1, a flagged row of 2, a row of 2 that claims 5, a spare slot that belongs to no row
    text, toffs, needed, outside = ref.materialise(ids.reshape(-1), [1, 0xFFFFFFFE, 5], blob, offs, row_offs=[0, 1, 3, 5], slots=6)
    assert (text.tobytes(), toffs.tolist(), needed, outside) == (b"alphabe", [0, 5, 5, 5, 7, 7, 7], 7, 0)


@pytest.mark.parametrize("name,n_rows,row,v", ref.step_cases(), ids=[c[0] for c in ref.step_cases()])
def test_host_handle_equals_the_restatement(host_dict, lines, name, n_rows, row, v):
    blob, offs = ref.pack(lines)
    ids, counts = ref.step_rows(n_rows, row, v, len(lines))
    want = ref.materialise(ids, counts, blob, offs, row=row)
    rc, msg, text, toffs, needed = _rows(host_dict, ids, counts, row=row, text_cap=want[2])
    assert (rc, needed) == (0, want[2]), msg
    ref.check(text, toffs, want)


def test_host_handle_ragged_rows_and_spare_slots(host_dict, lines):
    blob, offs = ref.pack(lines)
    rng = np.random.default_rng(5)
    ks = [1, 7, 300, 2, 64, 1, 9]
    ro = np.concatenate([[0], np.cumsum(ks)]).astype(np.uint64)
    slots = int(ro[-1]) + 13
    ids = rng.integers(0, len(lines) - 2, size=slots, dtype=np.uint32)
    counts = np.array([1, 3, 300, 0xFFFFFFFF, 70, 0, 9], dtype=np.uint32)
    ids[int(ro[-1]):] = [ref.POISON_ID, len(lines), 0xFFFFFFFF] * 4 + [ref.POISON_ID]
    want = ref.materialise(ids, counts, blob, offs, row_offs=ro, slots=slots)
    rc, msg, text, toffs, needed = _rows(host_dict, ids, counts, row_offs=ro, slots=slots)
    assert (rc, needed) == (0, want[2]), msg
    ref.check(text, toffs, want)
    assert np.all(toffs[int(ro[-1]):] == want[2])


def test_text_cap_needed_and_below(host_dict, lines):
    blob, offs = ref.pack(lines)
    ids, counts = ref.step_rows(257, 5, 0, len(lines))
    want = ref.materialise(ids, counts, blob, offs, row=5)
    for cap in (want[2] - 1, 0):
        rc, msg, text, toffs, needed = _rows(host_dict, ids, counts, row=5, text_cap=cap)
        assert (rc, msg, needed) == (-1, "text buffer too small", want[2])
        assert np.array_equal(toffs, want[1])                    # complete: the caller sizes a retry from it
    rc, msg, text, toffs, needed = _rows(host_dict, ids, counts, row=5, text_cap=want[2])
    assert rc == 0
    ref.check(text, toffs, want)


def test_an_id_outside_the_dictionary_is_refused(lines):
    from suggest_amd.dictionary import DeviceDictionary
    short = DeviceDictionary(lines[:-1], device=-1)
    ids = np.array([[0, len(lines) - 1, 1]], dtype=np.uint32)
    rc, msg, _, toffs, needed = _rows(short, ids, [3], row=3)
    assert (rc, msg) == (-1, "docID outside the dictionary")
    assert toffs.tolist() == [0, len(lines[0]), len(lines[0]), len(lines[0]) + len(lines[1])] and needed == int(toffs[-1])
    rc, msg, text, toffs, needed = _rows(short, ids, [1], row=3)         # the next call is right; the id past the count is not looked at
    assert rc == 0 and text[:needed].tobytes() == lines[0]
    short.close()


def test_refusals_that_need_no_gpu(host_dict, lines):
    from suggest_amd import IndexDescription, NGramIndex, _lib
    L = _lib.lib()
    ids = np.zeros((2, 3), dtype=np.uint32)
    for name in ("ids", "counts", "text_offs", "text"):
        rc, msg = _rows(host_dict, ids, [1, 1], row=3, null=name)[:2]
        assert (rc, msg) == (-1, "null argument"), name
    assert _rows(host_dict, ids, [1, 1], row=3, null="needed")[0] == 0                 # (needed may be null)
    assert L.sg_dictionary_rows(None, None, None, None, 0, 0, 0, None, 0, None, None) == -1 and L.sg_last_error() == b"null dictionary"
    assert _rows(host_dict, ids, [1, 1], row=4)[:2] == (-1, "dictionary rows: slots is below n_rows * row")
    assert _rows(host_dict, ids.reshape(-1), [1, 1], row_offs=[0, 4, 3])[:2] == (-1, "row offsets must not decrease")
    # a host-resident handle given to a device call, or to a fused call
    with host_dict._use() as h:
        x = ids.ctypes.data            # (host addresses stand in for device ones: everything here is refused before a pointer is followed)
        assert L.sg_dictionary_rows_device(h, x, x, None, 2, 3, 6, x, 8, x, x, None) == -2                 # SG_E_UNSUPPORTED
        assert b"host-resident" in L.sg_last_error()
        assert L.sg_dictionary_rows_device(h, x, x, None, 2, 3, 6, x, 8, x, None, None) == -1
        assert L.sg_dictionary_rows_device(h, x, x, None, 2, 3, 6, x, 8, None, x, None) == -1
    assert L.sg_dictionary_rows_device(None, None, None, None, 0, 0, 0, None, 0, None, None, None) == -1
    # the fused calls check what the plain calls check, in their order: the upload first
    d = IndexDescription(ngram_size=CARS_DESC["ngram_size"], wrap=CARS_DESC["wrap"], pad=CARS_DESC["pad"], alphabet=CARS_DESC["alphabet"])
    ix = NGramIndex([b"nissan", b"toyota"], d, upload=False)
    with pytest.raises(_lib.SuggestHipError) as e:
        ix.suggest_batch_strings(host_dict, ["nisan"], "cosine", 0.5, 0)
    assert e.value.code == -3
    with pytest.raises(_lib.SuggestHipError) as e:
        ix.suggest_batch_strings(host_dict, ["nisan"], "cosine", 0.5, 3)
    assert e.value.code == -3
    with pytest.raises(_lib.SuggestHipError) as e:
        ix.autocomplete_batch_strings(host_dict, ["nis"], 3)
    assert e.value.code == -3
    assert L.sg_suggest_batch_strings(None, None, None, 0, 0, 0.5, 1, None, None, None, None, None, 0, None, None) == -1
    # upload: null pointers, offsets that decrease, a device that is not there is met only with a GPU
    out = C.c_void_p()
    offs = np.array([0, 3, 2], dtype=np.uint64)
    blob = np.zeros(4, dtype=np.uint8)
    assert L.sg_dictionary_upload(blob.ctypes.data, offs.ctypes.data, 2, -1, C.byref(out)) == -1 and L.sg_last_error() == b"document offsets must not decrease"
    assert L.sg_dictionary_upload(blob.ctypes.data, None, 2, -1, C.byref(out)) == -1
    assert L.sg_dictionary_upload(blob.ctypes.data, offs.ctypes.data, 2, -1, None) == -1
    assert L.sg_dictionary_open_cdb(None, -1, C.byref(out)) == -1
    assert (L.sg_dictionary_size(None), L.sg_dictionary_bytes(None), L.sg_dictionary_max_len(None), L.sg_dictionary_device(None)) == (0, 0, 0, -1)
    L.sg_dictionary_retain(None)
    L.sg_dictionary_release(None)


def test_offsets_that_start_anywhere_and_the_handle_figures(lines):
    from suggest_amd.dictionary import DeviceDictionary
    blob, offs = ref.pack(lines)
    d = DeviceDictionary(blob=np.concatenate([np.zeros(7, dtype=np.uint8), blob]), offs=offs + np.uint64(7), device=-1)
    assert (d.n_docs, d.bytes, d.max_len, d.device, len(d)) == (203, int(offs[-1]), 70001, -1, 203)
    assert d.get(202) == lines[202] and d.get(3) == lines[3]
    with pytest.raises(KeyError):
        d.get(203)
    empty = DeviceDictionary([], device=-1)
    assert (empty.n_docs, empty.bytes, empty.max_len) == (0, 0, 0)
    text, toffs = empty.rows(np.zeros((0, 4), dtype=np.uint32), np.zeros(0, dtype=np.uint32))
    assert text.size == 0 and toffs.tolist() == [0]


def test_cars_cdb_equals_the_dictionary_line_for_line(cars_lines):
    from suggest_amd.dictionary import DeviceDictionary, split_text
    from suggest_amd.service import read_cdb_dictionary
    d = DeviceDictionary.from_cdb(CARS_CDB, -1)
    n = len(cars_lines)
    assert d.n_docs == n
    text, toffs = d.rows(np.arange(n, dtype=np.uint32).reshape(1, n), [n])
    got = split_text(text, toffs)
    want = [l.encode("utf-8") if isinstance(l, str) else l for l in cars_lines]
    assert got == want and got == read_cdb_dictionary(CARS_CDB)


def test_a_stored_cdb_round_trips_and_broken_files_are_refused(tmp_path):
    from suggest_amd import _lib
    from suggest_amd.dictionary import DeviceDictionary, split_text
    from suggest_amd.index import store_cdb_dictionary
    words = [b"", b"a", b"", b"\xd0\x9d\xd0\xb8\xd0\xb2\xd0\xb0", b"x" * 300, b""]
    path = str(tmp_path / "w.cdb")
    store_cdb_dictionary(words, path)
    d = DeviceDictionary.from_cdb(path, -1)
    assert d.n_docs == 6 and split_text(*d.rows(np.arange(6, dtype=np.uint32).reshape(1, 6), [6])) == words
    data = open(path, "rb").read()
    cut = str(tmp_path / "cut.cdb")
    open(cut, "wb").write(data[:1000])
    with pytest.raises(_lib.SuggestHipError) as e:
        DeviceDictionary.from_cdb(cut, -1)
    assert e.value.code == -1 and "cdb dictionary is truncated" in str(e.value)
    cut2 = str(tmp_path / "cut2.cdb")
    open(cut2, "wb").write(data[:2048 + 20])              # the records end before the hash tables the header points to
    with pytest.raises(_lib.SuggestHipError) as e:
        DeviceDictionary.from_cdb(cut2, -1)
    assert "cdb dictionary is corrupted" in str(e.value)
    hole = bytearray(data)
    first = 2048                                            # record 0: klen 4, dlen 0, key 0 -> key 9
    assert hole[first:first + 12] == bytes([4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    hole[first + 8] = 9
    hp = str(tmp_path / "hole.cdb")
    open(hp, "wb").write(bytes(hole))
    with pytest.raises(_lib.SuggestHipError) as e:
        DeviceDictionary.from_cdb(hp, -1)
    assert "cdb dictionary has a hole in its ids" in str(e.value)
    with pytest.raises(_lib.SuggestHipError) as e:
        DeviceDictionary.from_cdb(str(tmp_path / "none.cdb"), -1)
    assert "failed to open cdb dictionary file" in str(e.value)


def test_python_bindings():
    from suggest_amd import Service, _lib
    assert set(NEW) <= set(_lib.EXPORTS) and all(hasattr(_lib.lib(), n) for n in NEW)
    s = Service(device=0, device_dictionary=True)
    assert s.device_dictionary and not Service().device_dictionary
    with pytest.raises(KeyError):
        s.suggest_batch("cars", ["x"], 3, "cosine", 0.5)


def test_go_shim_arity_matches_the_header():
    """go/suggesthip/suggesthip.go has never met a Go compiler: its calls pass as many arguments as the header declares"""
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    for fn, want in (("sg_dictionary_upload", 5), ("sg_dictionary_open_cdb", 3), ("sg_suggest_batch_strings", 15)):
        decl = re.search(r"int %s\(([^;]*)\);" % fn, header).group(1)
        call = re.search(r"C\.%s\(([^\n]*)\)\n" % fn, go)
        assert call, fn
        depth, n = 0, 1
        for ch in call.group(1):
            depth += ch in "([{"
            depth -= ch in ")]}"
            n += ch == "," and depth == 0
        assert n == decl.count(",") + 1 == want, fn
    assert "func (i *Index) SuggestStrings(dict *DeviceDictionary, queries []string, similarity float64, m metric.Metric, k int)" in go
    assert "func NewDeviceDictionary(lines []string, device int) (*DeviceDictionary, error)" in go


def test_cpp_mirror_device_dictionary_compiles_and_runs_on_the_host(tmp_path):
    src = tmp_path / "snippet.cpp"
    src.write_text('''
#include "suggest_hip.hpp"
#include <cstdio>
int main() {
  using namespace suggest;
  dictionary::DeviceDictionary d(std::vector<std::string>{"alpha", "", "be"}, -1);
  std::shared_ptr<dictionary::Dictionary> as_dictionary = std::make_shared<dictionary::DeviceDictionary>(d.Size() ? std::vector<std::string>{"x"} : std::vector<std::string>{}, -1);
  if (d.Size() != 3 || d.Get(0) != "alpha" || d.Get(1) != "" || d.Get(2) != "be" || as_dictionary->Get(0) != "x" || d.Device() != -1) return 1;
  try { d.Get(3); return 2; } catch (const Error&) {}
  const uint32_t ids[4] = {2, 0, 7, 1}, counts[2] = {2, 0xFFFFFFFDu};
  std::vector<uint64_t> offs;
  if (d.Rows(ids, counts, nullptr, 2, 2, 4, offs) != "bealpha" || offs != std::vector<uint64_t>{0, 2, 7, 7, 7}) return 3;
  std::puts("ok");
  return 0;
}
''')
    binary = tmp_path / "snippet"
    lib_dir = os.path.join(ROOT, "suggest_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(binary), "-L" + lib_dir,
                        "-lsuggest_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,%s/lib" % rocm, "-Wl,-rpath-link,%s/lib" % rocm], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(binary)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
