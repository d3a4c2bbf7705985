"""sg_index_store_reference with the host encoder (device = -1) and sg_dictionary_store_cdb: a built index saved as the
reference's <name>.hd / <name>.dl (Writer.Commit, pkg/index/indexer_writer.go:88-167; codec.go:17-51) and <name>.cdb
(helpers.go:52-95).  Held against the reference's own bytes under golden/db and the Python encoders of refindex.py and
index_store_shapes.py.  No GPU needed; tests/test_gpu_index_store.py runs the same checks on the device encoder."""
import os
import subprocess

import pytest

import refindex
from conftest import CARS_DESC, WORDS_DESC, ROOT
from index_store_shapes import check_saved, check_shapes, cpp_program, dropped_repeats_files, fixture_lists, type_prefix


def _desc(d):
    from suggest_amd import IndexDescription
    return IndexDescription(**d)


def _save(ix, tmp_path, name, device=-1):
    hd, dl = str(tmp_path / (name + ".hd")), str(tmp_path / (name + ".dl"))
    ix.save(hd, dl, device=device)
    return hd, dl


@pytest.fixture(scope="module")
def cars_index(cars_lines):
    from suggest_amd import NGramIndex
    return NGramIndex(cars_lines, _desc(CARS_DESC), upload=False)


@pytest.fixture(scope="module")
def words_index(words_lines):
    from suggest_amd import NGramIndex
    return NGramIndex(words_lines, _desc(WORDS_DESC), upload=False)


def test_cars_saved_equals_the_reference_files(cars_index, tmp_path, golden_dir):
    hd, dl = _save(cars_index, tmp_path, "cars")
    assert os.path.getsize(dl) == 154469
    want = fixture_lists(golden_dir, "cars")
    indices, terms = check_saved(hd, dl, want)                       # every list's bytes; positions tile the file
    assert indices == 52
    _, _, ref_terms = refindex.read_header(os.path.join(golden_dir, "db", "cars.hd"))
    assert {(t, i, s, n) for t, i, s, _, n in terms} == {(t, i, s, n) for t, i, s, _, n in ref_terms}
    assert len(terms) == 36285
    assert sum(1 for t in terms if t[4] <= 65) == 36276 and sum(1 for t in terms if 65 < t[4] <= 256) == 9
    assert sum(1 for raw, post in cars_index.lists().values() if raw > len(post)) == 147      # lists with repeats
    # the order is ours: segment ascending, then the order of sg_index_lists
    assert [t[1] for t in terms] == sorted(t[1] for t in terms)
    # the type definitions in front of the value message: emitted by the gob encoder, equal to the reference's 213 bytes
    prefix = type_prefix(open(os.path.join(golden_dir, "db", "cars.hd"), "rb").read())
    assert len(prefix) == 213
    assert type_prefix(open(hd, "rb").read()) == prefix


def test_words_saved_equals_the_reference_subset(words_index, tmp_path, golden_dir):
    hd, dl = _save(words_index, tmp_path, "words")
    want = fixture_lists(golden_dir, "words_subset")
    assert len(want) == 7311 and sum(1 for raw, _ in want.values() if raw > 256) == 40
    check_saved(hd, dl, want)


def test_round_trips(cars_index, words_index, tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    for name, ix, desc in (("cars", cars_index, CARS_DESC), ("words", words_index, WORDS_DESC)):
        hd, dl = _save(ix, tmp_path, name)
        back = NGramIndex.from_reference_files(hd, dl, _desc(desc), upload=False)
        assert back.lists() == ix.lists(), name
        assert back.stats()["n_segments"] == ix.stats()["n_segments"]
    # the reference's own files, loaded and saved again
    ref = NGramIndex.from_reference_files(os.path.join(golden_dir, "db", "cars.hd"), os.path.join(golden_dir, "db", "cars.dl"),
                                          _desc(CARS_DESC), upload=False)
    hd, dl = _save(ref, tmp_path, "cars_again")
    check_saved(hd, dl, fixture_lists(golden_dir, "cars"))
    assert NGramIndex.from_reference_files(hd, dl, _desc(CARS_DESC), upload=False).lists() == ref.lists()


def test_round_trip_keeps_the_raw_length_of_dropped_repeats(tmp_path, golden_dir):
    from suggest_amd import NGramIndex
    desc, hd, dl = dropped_repeats_files(tmp_path, golden_dir)
    ix = NGramIndex.from_reference_files(hd, dl, _desc(desc), upload=False)
    hd2, dl2 = _save(ix, tmp_path, "t2")
    assert any(raw > 256 and raw > len(post) for raw, post in ix.lists().values())
    assert NGramIndex.from_reference_files(hd2, dl2, _desc(desc), upload=False).lists() == ix.lists()
    _, a = refindex.read_index(hd, dl)
    _, b = refindex.read_index(hd2, dl2)
    assert {k: (v[0], sorted(set(v[1])) if v[0] > 256 else v[1]) for k, v in a.items()} == b


def test_yardstick_only_python_run_encoder_matches_the_fixture_and_the_stated_shapes(golden_dir):
    """Covers NONE of the library: it passes without the feature.  It checks the tests' own yardstick: it reproduces the 40 roaring lists of the reference's words index, and the shapes hold the
    containers the issue names (runs without an offset header, runs with one and a key gap, a bitmap, arrays only, the tie)"""
    import struct
    from index_store_shapes import edge_shapes, encode_roaring_runs
    for (_, _), (raw, data) in fixture_lists(golden_dir, "words_subset").items():
        if raw > 256:
            assert encode_roaring_runs(refindex.decode_roaring(data)) == data
    enc = {name: encode_roaring_runs(sorted(set(post))) for name, raw, post in edge_shapes() if raw > 256}
    cookie = lambda b: struct.unpack_from("<I", b, 0)[0]                                    # noqa: E731
    two = enc["roar_two_runs_no_offsets"]
    assert cookie(two) == 12347 | 1 << 16 and len(two) == 4 + 1 + 8 + 2 * (2 + 4) and two[4] == 3
    k4 = enc["roar_runs_keys_0_1_2_5"]
    assert cookie(k4) == 12347 | 3 << 16 and [struct.unpack_from("<H", k4, 5 + 4 * i)[0] for i in range(4)] == [0, 1, 2, 5]
    assert struct.unpack_from("<I", k4, 5 + 16)[0] == 5 + 16 + 16                          # the offset header is there
    assert cookie(enc["roar_bitmap_alternating"]) == 12346 and len(enc["roar_bitmap_alternating"]) == 8 + 4 + 4 + 8192
    assert cookie(enc["roar_sparse_arrays_5_keys"]) == 12346
    assert len(enc["roar_4096_and_4097"]) == 8 + 8 + 8 + 2 * 4096 + 8192
    tie = enc["roar_tie_5_6_7"]
    assert cookie(tie) == 12347 | 1 << 16 and tie[4] == 1 and tie[13:19] == struct.pack("<HHH", 1, 5, 2)
    for b in enc.values():
        assert refindex.decode_roaring(b) == sorted(set(refindex.decode_roaring(b)))
    for name, raw, post in edge_shapes():
        if raw > 256:
            assert refindex.decode_roaring(enc[name]) == sorted(set(post)), name


def test_edge_shapes_equal_the_python_encoders(tmp_path, golden_dir):
    check_shapes(tmp_path, golden_dir, -1)


def test_cdb_dictionary_equals_the_reference_file(cars_lines, tmp_path, golden_dir):
    import suggest_amd
    path = str(tmp_path / "cars.cdb")
    suggest_amd.store_cdb_dictionary(cars_lines, path)
    data = open(path, "rb").read()
    assert len(data) == 250607
    assert data == open(os.path.join(golden_dir, "db", "cars.cdb"), "rb").read()
    blob, offs = suggest_amd.pack_strings(cars_lines)
    suggest_amd.store_cdb_dictionary((blob, offs), path)             # the packed form
    assert open(path, "rb").read() == data
    suggest_amd.store_cdb_dictionary([], path)                       # an empty dictionary: the 2048-byte header alone
    assert open(path, "rb").read() == bytes(2048)


def test_unwritable_path_is_an_invalid_argument(cars_index, tmp_path):
    import ctypes as C
    import suggest_amd
    from suggest_amd import _lib
    missing = tmp_path / "no" / "such" / "dir"
    L = _lib.lib()
    rc = L.sg_index_store_reference(cars_index._h, str(missing / "x.hd").encode(), str(missing / "x.dl").encode(), -1)
    assert rc == -1                                                  # SG_E_INVALID
    assert b"x.dl" in L.sg_last_error() or b"x.hd" in L.sg_last_error()
    ok_dl = tmp_path / "ok.dl"
    assert L.sg_index_store_reference(cars_index._h, str(missing / "x.hd").encode(), str(ok_dl).encode(), -1) == -1
    assert b"x.hd" in L.sg_last_error()
    with pytest.raises(_lib.SuggestHipError) as e:
        cars_index.save(missing / "x.hd", missing / "x.dl", device=-1)
    assert e.value.code == -1
    with pytest.raises(_lib.SuggestHipError):
        suggest_amd.store_cdb_dictionary([b"a"], missing / "x.cdb")
    assert L.sg_index_store_reference(None, b"a", b"b", -1) == -1
    out = (C.c_double * 4)()
    assert L.sg_debug_index_store_times(out) == 0


def test_cpp_mirror_indexes_cars_on_the_host(tmp_path, golden_dir):
    """suggest::Index with the host builder and encoder; the files are loaded back with sg_index_load_reference.  NewFSBuilder is
    NOT exercised here: its Build() uploads to a GPU (tests/test_gpu_index_store.py runs the program without --cpu)."""
    r = subprocess.run([cpp_program(), "--cpu", golden_dir, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
    check_saved(str(tmp_path / "cars.hd"), str(tmp_path / "cars.dl"), fixture_lists(golden_dir, "cars"))


def test_go_shim_arities_match_the_header():
    """go/suggesthip/suggesthip.go has never met a Go compiler: the two new calls pass as many arguments as the header declares"""
    import re
    go = open(os.path.join(ROOT, "go", "suggesthip", "suggesthip.go"), encoding="utf-8").read()
    header = open(os.path.join(ROOT, "include", "suggest_hip.h"), encoding="utf-8").read()
    for fn in ("sg_index_store_reference", "sg_dictionary_store_cdb"):
        decl = re.search(r"int %s\(([^;]*)\);" % fn, header).group(1)
        call = re.search(r"C\.%s\(([^\n]*)\)\n" % fn, go)
        assert call, fn
        depth, n = 0, 1
        for ch in call.group(1):
            depth += ch in "([{"
            depth -= ch in ")]}"
            n += ch == "," and depth == 0
        assert n == decl.count(",") + 1, fn
    assert "func (i *Index) StoreReference(hdPath, dlPath string, device int) error" in go
    assert "func StoreCDBDictionary(" in go
